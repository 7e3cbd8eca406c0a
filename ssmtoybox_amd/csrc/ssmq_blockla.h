// The device code that the quadrature-weight, kernel-method, ML-II and predict kernels share (ssmq_weights.hip,
// ssmq_kernel_methods.hip, ssmq_ml2.hip, ssmq_predict.hip), in three parts:
//   block-cooperative linear algebra and the workgroup reduction - called by all threads of a workgroup, striding by the
//     actual block size; the routines that say so end with a barrier;
//   the staged RBF kernel matrix - rbf_stage is block-cooperative, rbf_exp / rbf_entry are per thread;
//   the Bayes-Sard polynomial basis (ipow, bs_basis_entry) - per thread.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ssmq {

// workgroup size: 256 threads per parameter row, 1024 for large point sets (N > 64: one row keeps a whole CU busy with
// L2-latency-bound loops, so it takes all the waves the CU can give); device code strides by the actual block size
#define kWgtBlock ((int)blockDim.x)

__device__ __forceinline__ void bsync() { __syncthreads(); }

// C (M x N, ldc) = op(A) op(B); op(A) is M x K, op(B) is K x N.  Block-cooperative; ends with a barrier.
__device__ inline void gemm(double *C, int ldc, const double *A, int lda, bool ta, const double *B, int ldb, bool tb, int M,
                     int N, int K) {
    for (int idx = threadIdx.x; idx < M * N; idx += kWgtBlock) {
        const int i = idx / N, j = idx % N;
        double s = 0.0;
        for (int k = 0; k < K; ++k) {
            const double a = ta ? A[k * lda + i] : A[i * lda + k];
            const double b = tb ? B[j * ldb + k] : B[k * ldb + j];
            s += a * b;
        }
        C[i * ldc + j] = s;
    }
    bsync();
}

// In-place right-looking Cholesky (lower) of the n x n matrix A; the strict upper triangle is left untouched.
// Returns false (to every thread) at the first non-positive pivot.
__device__ inline bool chol_block(double *A, int n, int *flag) {
    if (threadIdx.x == 0) *flag = 1;
    bsync();
    for (int k = 0; k < n; ++k) {
        if (threadIdx.x == 0) {
            const double p = A[k * n + k];
            if (!(p > 0.0)) *flag = 0;
            A[k * n + k] = sqrt(p);
        }
        bsync();
        if (*flag == 0) return false;
        const double r = 1.0 / A[k * n + k];
        for (int i = k + 1 + threadIdx.x; i < n; i += kWgtBlock) A[i * n + k] *= r;
        bsync();
        const int m = n - k - 1;
        for (int idx = threadIdx.x; idx < m * m; idx += kWgtBlock) {
            const int i = k + 1 + idx / m, j = k + 1 + idx % m;
            if (j <= i) A[i * n + j] -= A[i * n + k] * A[j * n + k];
        }
        bsync();
    }
    return true;
}

// X = (L L')^-1 for the lower factor L (n x n): each thread owns columns of X; forward then backward substitution.
__device__ inline void chol_inverse(const double *L, double *X, int n) {
    for (int c = threadIdx.x; c < n; c += kWgtBlock) {
        for (int i = 0; i < n; ++i) {
            double s = (i == c) ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= L[i * n + k] * X[k * n + c];   // X[k][c] = 0 for k < c
            X[i * n + c] = (i < c) ? 0.0 : s / L[i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double s = X[i * n + c];
            for (int k = i + 1; k < n; ++k) s -= L[k * n + i] * X[k * n + c];
            X[i * n + c] = s / L[i * n + i];
        }
    }
    bsync();
}

// X = A^-1 for a general n x n matrix by LU with partial pivoting (numpy.linalg.solve(V, I), bq/bqmod.py:954).
// A is destroyed.  Single-thread pivot search, block-parallel elimination; n is small (<= N).
__device__ inline bool lu_inverse(double *A, double *X, int n, int *piv, int *flag) {
    for (int idx = threadIdx.x; idx < n * n; idx += kWgtBlock) X[idx] = (idx / n == idx % n) ? 1.0 : 0.0;
    if (threadIdx.x == 0) *flag = 1;
    bsync();
    for (int k = 0; k < n; ++k) {
        if (threadIdx.x == 0) {
            int p = k;
            double best = fabs(A[k * n + k]);
            for (int i = k + 1; i < n; ++i)
                if (fabs(A[i * n + k]) > best) { best = fabs(A[i * n + k]); p = i; }
            *piv = p;
            if (best == 0.0) *flag = 0;
        }
        bsync();
        if (*flag == 0) return false;
        const int p = *piv;
        if (p != k) {
            for (int j = threadIdx.x; j < n; j += kWgtBlock) {
                double t = A[k * n + j]; A[k * n + j] = A[p * n + j]; A[p * n + j] = t;
                t = X[k * n + j]; X[k * n + j] = X[p * n + j]; X[p * n + j] = t;
            }
        }
        bsync();
        const double r = 1.0 / A[k * n + k];
        for (int i = k + 1 + threadIdx.x; i < n; i += kWgtBlock) A[i * n + k] *= r;
        bsync();
        const int m = n - k - 1;
        for (int idx = threadIdx.x; idx < m * n; idx += kWgtBlock) {
            const int i = k + 1 + idx / n, j = idx % n;
            const double l = A[i * n + k];
            if (j > k) A[i * n + j] -= l * A[k * n + j];
            X[i * n + j] -= l * X[k * n + j];
        }
        bsync();
    }
    // back substitution U X = Y, thread per column
    for (int c = threadIdx.x; c < n; c += kWgtBlock) {
        for (int i = n - 1; i >= 0; --i) {
            double s = X[i * n + c];
            for (int k = i + 1; k < n; ++k) s -= A[i * n + k] * X[k * n + c];
            X[i * n + c] = s / A[i * n + i];
        }
    }
    bsync();
    return true;
}

// X = (L L')^-1 Bm for the lower factor L (n x n) and a square right-hand side: thread per column, forward then backward
// substitution (scipy.linalg.cho_solve)
__device__ inline void chol_solve(const double *L, const double *Bm, double *X, int n) {
    for (int c = threadIdx.x; c < n; c += kWgtBlock) {
        for (int i = 0; i < n; ++i) {
            double s = Bm[i * n + c];
            for (int k = 0; k < i; ++k) s -= L[i * n + k] * X[k * n + c];
            X[i * n + c] = s / L[i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double s = X[i * n + c];
            for (int k = i + 1; k < n; ++k) s -= L[k * n + i] * X[k * n + c];
            X[i * n + c] = s / L[i * n + i];
        }
    }
    bsync();
}

// ---- large point sets (N > 64, 1024 threads) --------------------------------------------------------------------------
#define SSMQ_PKL(i, j) ((i) * ((i) + 1) / 2 + (j))   // packed lower triangle, j <= i

// Right-looking Cholesky of a packed lower triangle held in LDS (same subtraction order as chol_block: same factor).
// Two barriers per column: every thread forms the pivot's reciprocal root itself, and the trailing update walks rows and
// columns without an integer division per element.
__device__ inline bool chol_packed_lds(double *Lp, int n, int *flag) {
    if (threadIdx.x == 0) *flag = 1;
    bsync();
    for (int k = 0; k < n; ++k) {
        const double p = Lp[SSMQ_PKL(k, k)];
        if (!(p > 0.0)) return false;            // uniform: every thread reads the same pivot
        const double lkk = sqrt(p), r = 1.0 / lkk;
        bsync();                                 // everyone has read the pivot before it is overwritten
        if (threadIdx.x == 0) Lp[SSMQ_PKL(k, k)] = lkk;
        for (int i = k + 1 + threadIdx.x; i < n; i += kWgtBlock) Lp[SSMQ_PKL(i, k)] *= r;
        bsync();
        for (int i = k + 1 + (threadIdx.x >> 4); i < n; i += kWgtBlock >> 4) {
            const double lik = Lp[SSMQ_PKL(i, k)];
            for (int j = k + 1 + (threadIdx.x & 15); j <= i; j += 16) Lp[SSMQ_PKL(i, j)] -= lik * Lp[SSMQ_PKL(j, k)];
        }
        bsync();
    }
    return true;
}

// chol_inverse for a packed lower factor, into a packed lower triangle: column c's rows i >= c need only rows k >= c, so
// the arithmetic is chol_inverse's for the lower triangle, bit for bit.
__device__ inline void chol_inverse_packed(const double *Lp, double *Xp, int n) {
    for (int c = threadIdx.x; c < n; c += kWgtBlock) {
        for (int i = c; i < n; ++i) {
            double s = (i == c) ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= Lp[SSMQ_PKL(i, k)] * Xp[SSMQ_PKL(k, c)];
            Xp[SSMQ_PKL(i, c)] = s / Lp[SSMQ_PKL(i, i)];
        }
        for (int i = n - 1; i >= c; --i) {
            double s = Xp[SSMQ_PKL(i, c)];
            for (int k = i + 1; k < n; ++k) s -= Lp[SSMQ_PKL(k, i)] * Xp[SSMQ_PKL(k, c)];
            Xp[SSMQ_PKL(i, c)] = s / Lp[SSMQ_PKL(i, i)];
        }
    }
    bsync();
}

// Element (i, j), j <= i, of a lower triangle held densely (n x n, row-major) or packed
template <bool PACKED>
__device__ __forceinline__ auto tri_idx(int i, int j, int n) {
    if constexpr (PACKED) return SSMQ_PKL(i, j);
    else return (int64_t)i * n + j;
}
// ... and element (i, j) of the symmetric matrix whose lower triangle that is.  A macro, so that the two conditional loads stay
// in the caller's loop as written: wrapped in a function they become one load through a selected address before the loop is
// optimised, and the kernels come out longer.
#define SSMQ_SYM_LOWER(PACKED, X, i, j, n) \
    ((i) >= (j) ? (X)[ssmq::tri_idx<PACKED>(i, j, n)] : (X)[ssmq::tri_idx<PACKED>(j, i, n)])

// Factor A (its lower triangle, dense or packed) in place; false (to every thread) if A is not positive definite.  Then
// X = A^-1 from that factor into the lower triangle of X (the dense route fills the strict upper triangle as well): both
// routes form the lower triangle with the same arithmetic.  Two calls, because ML-II reads the factor's diagonal in between.
template <bool PACKED>
__device__ __forceinline__ bool chol_factor_tri(double *A, int n, int *flag) {
    return PACKED ? chol_packed_lds(A, n, flag) : chol_block(A, n, flag);
}
template <bool PACKED>
__device__ __forceinline__ void chol_inverse_tri(const double *L, double *X, int n) {
    if (PACKED) chol_inverse_packed(L, X, n);
    else chol_inverse(L, X, n);
}

// C (M x N, ldc) = op(A) op(B) through LDS tiles: 128 x 128 outputs per pass, 4 x 4 per thread (1024 threads), K in
// slabs of 16 whose loads are issued one slab ahead (registers) so that the L2 latency hides behind the arithmetic of
// the current slab; k ascends inside every output's sum exactly as in gemm(), so the result is bit-identical to it.
// tile: 2 * 16 * 132 doubles of LDS.
constexpr int kTileMN = 128, kTileK = 16, kTilePitch = kTileMN + 4;
__device__ inline void gemm_tiled(double *tile, double *C, int ldc, const double *A, int lda, bool ta, const double *B, int ldb,
                           bool tb, int M, int N, int K) {
    double *sA = tile, *sB = tile + kTileK * kTilePitch;     // sA[k][i], sB[k][j]
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 32 threads, each 4 x 4 outputs
    constexpr int kPer = kTileK * kTileMN / 1024;            // elements of either slab per thread (2)
    for (int i0 = 0; i0 < M; i0 += kTileMN)
        for (int j0 = 0; j0 < N; j0 += kTileMN) {
            double acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[r][q] = 0.0;
            double ra[kPer], rb[kPer];
            auto fetch = [&](int k0) {
#pragma unroll
                for (int u = 0; u < kPer; ++u) {
                    const int idx = threadIdx.x + u * kWgtBlock;
                    int kk, ii;                  // coalesced along the contiguous direction of each operand
                    if (ta) { kk = idx / kTileMN; ii = idx % kTileMN; } else { ii = idx / kTileK; kk = idx % kTileK; }
                    const int gi = i0 + ii, gk = k0 + kk;
                    ra[u] = (gi < M && gk < K) ? (ta ? A[gk * lda + gi] : A[gi * lda + gk]) : 0.0;
                    int kb, jj;
                    if (tb) { jj = idx / kTileK; kb = idx % kTileK; } else { kb = idx / kTileMN; jj = idx % kTileMN; }
                    const int gj = j0 + jj, gkb = k0 + kb;
                    rb[u] = (gj < N && gkb < K) ? (tb ? B[gj * ldb + gkb] : B[gkb * ldb + gj]) : 0.0;
                }
            };
            auto park = [&]() {
#pragma unroll
                for (int u = 0; u < kPer; ++u) {
                    const int idx = threadIdx.x + u * kWgtBlock;
                    int kk, ii;
                    if (ta) { kk = idx / kTileMN; ii = idx % kTileMN; } else { ii = idx / kTileK; kk = idx % kTileK; }
                    sA[kk * kTilePitch + ii] = ra[u];
                    int kb, jj;
                    if (tb) { jj = idx / kTileK; kb = idx % kTileK; } else { kb = idx / kTileMN; jj = idx % kTileMN; }
                    sB[kb * kTilePitch + jj] = rb[u];
                }
            };
            fetch(0);
            for (int k0 = 0; k0 < K; k0 += kTileK) {
                bsync();                         // the previous slab has been consumed
                park();
                bsync();
                if (k0 + kTileK < K) fetch(k0 + kTileK);
#pragma unroll
                for (int kk = 0; kk < kTileK; ++kk) {
                    double av[4], bv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) av[r] = sA[kk * kTilePitch + ty * 4 + r];
#pragma unroll
                    for (int q = 0; q < 4; ++q) bv[q] = sB[kk * kTilePitch + tx * 4 + q];
                    if (k0 + kk < K) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int q = 0; q < 4; ++q) acc[r][q] += av[r] * bv[q];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int gi = i0 + ty * 4 + r, gj = j0 + tx * 4 + q;
                    if (gi < M && gj < N) C[gi * ldc + gj] = acc[r][q];
                }
        }
    bsync();
}

// NV per-thread partial sums, the first n of them used -> their block sums in out[0 .. NV) (waves added in index order); ends with a barrier
template <int NV>
__device__ inline void block_sums(const double (&v)[NV], int n, double *red, double *out) {
    const int wave = threadIdx.x >> 6, nw = kWgtBlock >> 6;
#pragma unroll
    for (int p = 0; p < NV; ++p) {
        if (p < n) {
            double s = v[p];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if ((threadIdx.x & 63) == 0) red[wave * NV + p] = s;
        }
    }
    bsync();
    if ((int)threadIdx.x < n) {
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += red[w * NV + threadIdx.x];
        out[threadIdx.x] = s;
    }
    bsync();
}

// ---- the staged RBF kernel matrix (bq/bqkern.py:329-343 with utils.maha, utils.py:385-409) -----------------------------------
// zs = Lam^-1/2 x ([D][N], as x) and nrm[n] = |zs_n|^2 from the inverse length scales sil[D], which the caller's threads
// tid < D have just written to LDS: the barrier that publishes them is the first of the three here.
__device__ __forceinline__ void rbf_stage(const double *sil, const double *x, double *zs, double *nrm, int D, int N) {
    bsync();
    for (int idx = threadIdx.x; idx < D * N; idx += kWgtBlock) zs[idx] = sil[idx / N] * x[idx];
    bsync();
    for (int n = threadIdx.x; n < N; n += kWgtBlock) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) s += zs[d * N + n] * zs[d * N + n];
        nrm[n] = s;
    }
    bsync();
}
// exp(la - maha / 2) with maha as |a|^2 + |b|^2 - 2 a.b, la = 2 log(alpha): the entry formula on its own ...
__device__ __forceinline__ double rbf_exp(double la, double na, double nb, double dot) {
    return exp(la - 0.5 * ((na + nb) - 2.0 * dot));
}
// ... and entry (i, j) of the kernel matrix of the staged points
__device__ __forceinline__ double rbf_entry(double la, const double *zs, const double *nrm, int N, int D, int i, int j) {
    double dot = 0.0;
    for (int d = 0; d < D; ++d) dot += zs[d * N + i] * zs[d * N + j];
    return rbf_exp(la, nrm[i], nrm[j], dot);
}

// ---- polynomial basis of the Bayes-Sard model -------------------------------------------------------------------------------
__device__ inline double ipow(double x, int k) {
    double r = 1.0;
    for (int i = 0; i < k; ++i) r *= x;
    return r;
}

// Entry (n, q) of the Vandermonde matrix (utils.py:478-502) and of E[k(x, x_n) p_q(x)], the closed form of
// bq/bqmod.py:733-797; its `ell` is sqrt_inv_lam ** -2 = ell^2, reproduced as written there.  sil[d] = 1 / ell_d.
__device__ inline void bs_basis_entry(int D, int N, int NB, int n, int qb, const double *__restrict__ xi,
                               const int32_t *__restrict__ mulind, const double *sil, double &vand, double &kxpx) {
    double v = 1.0, kprod = 1.0;
    for (int d = 0; d < D; ++d) {
        const int al = mulind[d * NB + qb];
        const double x = xi[d * N + n];
        v *= ipow(x, al);
        const double sl = sil[d];
        const double el = 1.0 / (sl * sl);
        const double e1 = 1.0 + el * el;
        const double ea = el * pow(e1, -(1.0 + al) / 2.0) * exp(-(x * x) / (2.0 * e1));
        double eb = 0.0;
        const double xs = x / sqrt(e1);
        for (int m = 0; m <= al / 2; ++m) {
            // al! / (2^m m! (al - 2m)!)
            double num = 1.0, den = 1.0;
            for (int t = 2; t <= al; ++t) num *= t;
            for (int t = 0; t < m; ++t) den *= 2.0;
            for (int t = 2; t <= m; ++t) den *= t;
            for (int t = 2; t <= al - 2 * m; ++t) den *= t;
            eb += (num / den) * (ipow(el, 2 * m) * ipow(xs, al - 2 * m));
        }
        kprod *= ea * eb;
    }
    vand = v;
    kxpx = kprod;
}

}  // namespace ssmq
