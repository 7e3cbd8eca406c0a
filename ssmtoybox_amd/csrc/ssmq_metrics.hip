// Error statistics of a batch of filtered trajectories, reduced over the Monte-Carlo axis on the device.
//
// Reference: ssmtoybox/utils.py:18-38 (squared_error), :41-64 (mse_matrix), :66-120 (log_cred_ratio),
// :123-148 (neg_log_likelihood) as the studies aggregate them (research/tpq/tpq_base.py:154-172: RMSE averaged over
// simulations, MSE matrix per time step, log credibility ratio against the per-step MSE matrix).
//
// Layout: the filter outputs stay where ssmq_filter_forward_dev left them - planes [T][D][ld] / [T][D*D][ld], one
// trajectory per lane - so each thread streams its trajectory's D + D + D*D doubles of a time step with 512-B wave
// accesses and nothing is copied to the host except [T][NV] sums.  Reduction order is fixed (thread-serial over a
// strided slice, wave shuffle tree, LDS across waves, then a second kernel over the partials in index order): results
// are deterministic and independent of launch timing.  HBM-bound: algorithmic 8 (2 D + D^2) bytes per trajectory and
// step; the kernels move 8 (2 D + D (D + 1) / 2) - only the lower triangle of P is read (the Cholesky factor needs no
// more, as LAPACK 'L' under the filters) and only the lower triangle of the outer products is accumulated.
#include "ssmq_host.h"

namespace ssmq {
namespace {

// every input is read exactly once: non-temporal loads keep the stream out of the way of L2 (238 -> 210 us at D = 6)
#define SSMQ_MLOAD(src) __builtin_nontemporal_load(&(src))

constexpr int kMetBlock = 256;
constexpr int kMetPerThread = 8;       // trajectories each thread accumulates before the block reduction
constexpr int kMetMaxD = SSMQ_MAX_DIM;

__host__ __device__ constexpr int met_nv(int D) { return D + 2 + D * D + 2; }

// in-place lower Cholesky of a dense D x D matrix held in registers / scratch; false if not positive definite
template <int DT>
__device__ __forceinline__ bool chol_dense(double *A, int D) {
    const int n = DT > 0 ? DT : D;
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        double s = A[j * n + j];
        for (int k = 0; k < j; ++k) s -= A[j * n + k] * A[j * n + k];
        if (!(s > 0.0)) ok = false;
        const double l = sqrt(s), r = 1.0 / l;
        A[j * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double v = A[i * n + j];
            for (int k = 0; k < j; ++k) v -= A[i * n + k] * A[j * n + k];
            A[i * n + j] = v * r;
        }
    }
    return ok;
}

// |L^-1 dx|^2 = dx' (L L')^-1 dx
template <int DT>
__device__ __forceinline__ double whitened_norm2(const double *L, const double *dx, int D) {
    const int n = DT > 0 ? DT : D;
    double v[DT > 0 ? DT : kMetMaxD];
    double q = 0.0;
    for (int i = 0; i < n; ++i) {
        double s = dx[i];
        for (int k = 0; k < i; ++k) s -= L[i * n + k] * v[k];
        v[i] = s / L[i * n + i];
        q += v[i] * v[i];
    }
    return q;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// block-wide sums of NV per-thread values -> out[NV] (written by thread 0..NV-1); sh: [kMetBlock / 64][NV]
__device__ __forceinline__ void block_sums(const double *acc, int NV, double *sh, double *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int v = 0; v < NV; ++v) {
        const double s = wave_sum(acc[v]);
        if (lane == 0) sh[wave * NV + v] = s;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < NV; v += kMetBlock) {
        double s = 0.0;
        for (int w = 0; w < kMetBlock / 64; ++w) s += sh[w * NV + v];
        out[v] = s;
    }
}

struct MetArgs {
    const double *x, *fm, *fP;     // [T][D][ld], [T][D][ld], [T][D*D][ld]
    const int32_t *status;         // [ld] or null; nonzero = trajectory excluded (its filter failed)
    const double *mse;             // phase 2: [T][D*D] global MSE matrices (already regularised), device
    double *partial;               // [T][chunks][NV]
    uint8_t *left;                 // [T][chunks][kMetBlock]: bit r = the thread's r-th entry was left to the second pass
    int64_t B, ld;
    int32_t D, T, chunks;
};

// The streaming kernels decide once which entries they leave to the second pass (P not positive definite) and record it: one
// byte per thread and step, bit r for the thread's r-th entry, stored unconditionally (no initialisation pass).  k_indef_sums
// runs the same (block, thread, r) -> trajectory map and reads its own byte back.  It does not factor P again: a second
// factorisation - even the same routine, inlined into other code and contracted into other fused operations - can take the
// other side at a pivot of rounding size, and the entry would be added by both passes or by neither.
__device__ __forceinline__ void store_left(const MetArgs &a, int t, uint32_t left) {
    a.left[((int64_t)t * a.chunks + blockIdx.x) * kMetBlock + threadIdx.x] = (uint8_t)left;
}

// block-wide sums with a compile-time count (accumulators stay in registers)
template <int NV>
__device__ __forceinline__ void block_sums_fixed(const double (&acc)[NV], double *sh, double *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const double s = wave_sum(acc[v]);
        if (lane == 0) sh[wave * NV + v] = s;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < NV; v += kMetBlock) {
        double s = 0.0;
        for (int w = 0; w < kMetBlock / 64; ++w) s += sh[w * NV + v];
        out[v] = s;
    }
}

// |L^-1 dx|^2 with L packed lower
template <int D>
__device__ __forceinline__ double whitened_norm2_packed(const double (&L)[D * (D + 1) / 2], const double (&dx)[D]) {
    double v[D];
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double s = dx[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[SSMQ_PK(i, k)] * v[k];
        v[i] = s / L[SSMQ_PK(i, i)];
        q += v[i] * v[i];
    }
    return q;
}

// ---- item bodies: one (trajectory, step) entry, shared by the sums over the Monte-Carlo axis (k_error_sums, k_lcr_sums, their
// run-time-sized forms, k_indef_sums) and the per-trajectory scores (k_traj_scores) ---------------------------------------------
// negative log-likelihood (utils.py:143-148) for positive-definite P: log det = 2 sum log L_ii.  L: lower triangle of P on entry,
// its Cholesky factor on return.  The entry's term is added to `sum` (every item below adds in place: the sums keep the fused
// multiply-add they have always ended in); false, `sum` untouched, if P is not positive definite
template <int D>
__device__ __forceinline__ bool nll_item(double (&L)[D * (D + 1) / 2], const double (&dx)[D], double &sum) {
    if (!chol_packed<D>(L)) return false;
    double logdet = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) logdet += log(L[SSMQ_PK(i, i)]);
    const double q = whitened_norm2_packed<D>(L, dx);
    sum += 0.5 * (2.0 * logdet + q + D * 1.8378770664093453 /* log(2 pi) */);
    return true;
}

// ... run-time D, P dense (lower triangle filled)
__device__ __forceinline__ bool nll_item_dense(double *P, const double *dx, int D, double &sum) {
    if (!chol_dense<0>(P, D)) return false;
    double logdet = 0.0;
    for (int i = 0; i < D; ++i) logdet += log(P[i * D + i]);
    const double q = whitened_norm2<0>(P, dx, D);
    sum += 0.5 * (2.0 * logdet + q + D * 1.8378770664093453);
    return true;
}

// log credibility ratio (utils.py:113-120) from the two quadratic forms dx' P^-1 dx and dx' M^-1 dx
__device__ __forceinline__ void lcr_add(double qa, double qb, double &sum) { sum += 10.0 * (log10(qa) - log10(qb)); }

// ... for positive-definite P (L as in nll_item) against the factored MSE matrix M
template <int D>
__device__ __forceinline__ bool lcr_item(double (&L)[D * (D + 1) / 2], const double (&M)[D * (D + 1) / 2], const double (&dx)[D],
                                         double &sum) {
    if (!chol_packed<D>(L)) return false;              // the reference's SVD square root (utils.py:426-432): lcr_item_indef
    const double qa = whitened_norm2_packed<D>(L, dx), qb = whitened_norm2_packed<D>(M, dx);
    lcr_add(qa, qb, sum);
    return true;
}

__device__ __forceinline__ bool lcr_item_dense(double *P, const double *M, const double *dx, int D, double &sum) {
    if (!chol_dense<0>(P, D)) return false;
    const double qa = whitened_norm2<0>(P, dx, D), qb = whitened_norm2<0>(M, dx, D);
    lcr_add(qa, qb, sum);
    return true;
}

// phase 1 values per time step (output): se[D] | rmse | nll | mse[D*D] | n_ok | n_pd.
// Compile-time D: accumulators se[D], rmse, nll, lower triangle of the outer products, two counts - all in registers;
// the partial row is written in the packed order and expanded by k_reduce_partials.
template <int D>
__global__ __launch_bounds__(kMetBlock) void k_error_sums(MetArgs a) {
    constexpr int TRI = D * (D + 1) / 2, NA = D + 2 + TRI + 2;
    const int t = blockIdx.y;
    extern __shared__ double sh[];
    double acc[NA];
#pragma unroll
    for (int v = 0; v < NA; ++v) acc[v] = 0.0;
    const double *x = a.x + (int64_t)t * D * a.ld, *fm = a.fm + (int64_t)t * D * a.ld;
    const double *fP = a.fP + (int64_t)t * D * D * a.ld;
    // 32-bit lane index against wave-uniform plane pointers: loads take the (SGPR base + VGPR offset) form and no
    // 64-bit address is kept per plane
    const uint32_t base = blockIdx.x * (uint32_t)(kMetBlock * kMetPerThread) + threadIdx.x;
    uint32_t left = 0;
    for (int r = 0; r < kMetPerThread; ++r) {
        const uint32_t b = base + (uint32_t)r * kMetBlock;
        if ((int64_t)b >= a.B) break;
        if (a.status && a.status[b] != 0) continue;
        double dx[D], L[TRI];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) L[SSMQ_PK(i, j)] = SSMQ_MLOAD(fP[((int64_t)i * D + j) * a.ld + b]);
        double n2 = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            dx[d] = SSMQ_MLOAD(x[(int64_t)d * a.ld + b]) - SSMQ_MLOAD(fm[(int64_t)d * a.ld + b]);
            acc[d] += dx[d] * dx[d];
            n2 += dx[d] * dx[d];
        }
        acc[D] += sqrt(n2);
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) acc[D + 2 + SSMQ_PK(i, j)] += dx[i] * dx[j];
        acc[D + 2 + TRI] += 1.0;
        if (nll_item<D>(L, dx, acc[D + 1])) acc[D + 3 + TRI] += 1.0;
        else left |= 1u << r;
    }
    store_left(a, t, left);
    block_sums_fixed<NA>(acc, sh, a.partial + ((int64_t)t * a.chunks + blockIdx.x) * NA);
}

// run-time D (> 6): dense arrays in scratch, same packed partial row
__global__ __launch_bounds__(kMetBlock) void k_error_sums_generic(MetArgs a) {
    const int D = a.D, TRI = D * (D + 1) / 2, NA = D + 2 + TRI + 2;
    const int t = blockIdx.y;
    extern __shared__ double sh[];
    double acc[kMetMaxD + 2 + kMetMaxD * (kMetMaxD + 1) / 2 + 2];
    for (int v = 0; v < NA; ++v) acc[v] = 0.0;
    const double *x = a.x + (int64_t)t * D * a.ld, *fm = a.fm + (int64_t)t * D * a.ld;
    const double *fP = a.fP + (int64_t)t * D * D * a.ld;
    const int64_t base = (int64_t)blockIdx.x * kMetBlock * kMetPerThread;
    uint32_t left = 0;
    for (int r = 0; r < kMetPerThread; ++r) {
        const int64_t b = base + (int64_t)r * kMetBlock + threadIdx.x;
        if (b >= a.B) break;
        if (a.status && a.status[b] != 0) continue;
        double dx[kMetMaxD], P[kMetMaxD * kMetMaxD];
        double n2 = 0.0;
        for (int d = 0; d < D; ++d) {
            dx[d] = SSMQ_MLOAD(x[(int64_t)d * a.ld + b]) - SSMQ_MLOAD(fm[(int64_t)d * a.ld + b]);
            acc[d] += dx[d] * dx[d];
            n2 += dx[d] * dx[d];
        }
        acc[D] += sqrt(n2);
        for (int i = 0; i < D; ++i)
            for (int j = 0; j <= i; ++j) {
                acc[D + 2 + SSMQ_PK(i, j)] += dx[i] * dx[j];
                P[i * D + j] = fP[((int64_t)i * D + j) * a.ld + b];
            }
        acc[D + 2 + TRI] += 1.0;
        if (nll_item_dense(P, dx, D, acc[D + 1])) acc[D + 3 + TRI] += 1.0;
        else left |= 1u << r;
    }
    store_left(a, t, left);
    block_sums(acc, NA, sh, a.partial + ((int64_t)t * a.chunks + blockIdx.x) * NA);
}

// phase 2 values per time step: lcr | n counted | n left to the second pass (P not positive definite)
template <int D>
__global__ __launch_bounds__(kMetBlock) void k_lcr_sums(MetArgs a) {
    constexpr int TRI = D * (D + 1) / 2;
    const int t = blockIdx.y;
    extern __shared__ double sh[];
    double acc[3] = {0.0, 0.0, 0.0};
    const double *x = a.x + (int64_t)t * D * a.ld, *fm = a.fm + (int64_t)t * D * a.ld;
    const double *fP = a.fP + (int64_t)t * D * D * a.ld;
    // the step's MSE matrix is the same for every trajectory: wave-uniform loads, factored once per thread
    double M[TRI];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) M[SSMQ_PK(i, j)] = a.mse[(int64_t)t * D * D + i * D + j];
    const bool m_ok = chol_packed<D>(M);
    const uint32_t base = blockIdx.x * (uint32_t)(kMetBlock * kMetPerThread) + threadIdx.x;
    uint32_t left = 0;
    for (int r = 0; r < kMetPerThread && m_ok; ++r) {
        const uint32_t b = base + (uint32_t)r * kMetBlock;
        if ((int64_t)b >= a.B) break;
        if (a.status && a.status[b] != 0) continue;
        double dx[D], L[TRI];
#pragma unroll
        for (int d = 0; d < D; ++d) dx[d] = x[(int64_t)d * a.ld + b] - fm[(int64_t)d * a.ld + b];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) L[SSMQ_PK(i, j)] = SSMQ_MLOAD(fP[((int64_t)i * D + j) * a.ld + b]);
        if (!lcr_item<D>(L, M, dx, acc[0])) {   // left to k_indef_sums
            acc[2] += 1.0;
            left |= 1u << r;
            continue;
        }
        acc[1] += 1.0;
    }
    store_left(a, t, left);
    block_sums_fixed<3>(acc, sh, a.partial + ((int64_t)t * a.chunks + blockIdx.x) * 3);
}

__global__ __launch_bounds__(kMetBlock) void k_lcr_sums_generic(MetArgs a) {
    const int D = a.D;
    const int t = blockIdx.y;
    extern __shared__ double sh[];
    double acc[3] = {0.0, 0.0, 0.0};
    const double *x = a.x + (int64_t)t * D * a.ld, *fm = a.fm + (int64_t)t * D * a.ld;
    const double *fP = a.fP + (int64_t)t * D * D * a.ld;
    double M[kMetMaxD * kMetMaxD];
    for (int i = 0; i < D * D; ++i) M[i] = a.mse[(int64_t)t * D * D + i];
    const bool m_ok = chol_dense<0>(M, D);
    const int64_t base = (int64_t)blockIdx.x * kMetBlock * kMetPerThread;
    uint32_t left = 0;
    for (int r = 0; r < kMetPerThread && m_ok; ++r) {
        const int64_t b = base + (int64_t)r * kMetBlock + threadIdx.x;
        if (b >= a.B) break;
        if (a.status && a.status[b] != 0) continue;
        double dx[kMetMaxD], P[kMetMaxD * kMetMaxD];
        for (int d = 0; d < D; ++d) dx[d] = x[(int64_t)d * a.ld + b] - fm[(int64_t)d * a.ld + b];
        for (int i = 0; i < D; ++i)
            for (int j = 0; j <= i; ++j) P[i * D + j] = fP[((int64_t)i * D + j) * a.ld + b];
        if (!lcr_item_dense(P, M, dx, D, acc[0])) {
            acc[2] += 1.0;
            left |= 1u << r;
            continue;
        }
        acc[1] += 1.0;
    }
    store_left(a, t, left);
    block_sums(acc, 3, sh, a.partial + ((int64_t)t * a.chunks + blockIdx.x) * 3);
}

// ---- covariances that are not positive definite ----------------------------------------------------------------------
// The reference's metrics do not need a positive-definite P: neg_log_likelihood uses inv(P) and sign * logdet of
// slogdet (utils.py:143-148), log_cred_ratio's mat_sqrt falls back to u sqrt(s) of an SVD (utils.py:426-432), i.e. the
// quadratic form with |P| = U S U'.  The streaming kernels above go through the Cholesky factor and leave such entries
// out and record which (store_left); when the counts say that some were left out, this kernel makes a second pass that adds
// exactly the recorded entries' terms:
//   phase 1: 0.5 (sign log|det P| + dx' P^-1 dx + D log 2 pi) from an LU factorisation with partial pivoting of the
//            full matrix;  phase 2: 10 (log10 dx'|P|^-1 dx - log10 dx' M^-1 dx), |P| through a Jacobi
//            eigen-decomposition of the symmetric part (eigenvalues in absolute value).
// Rare path, run-time D, dense arrays in scratch; same deterministic two-level reduction.  partial row: term sum | count.
__device__ bool lu_solve_logdet(double *A, const double *rhs, double *z, int n, double *sign, double *logabs) {
    int perm_sign = 1;
    double la = 0.0;
    for (int i = 0; i < n; ++i) z[i] = rhs[i];
    for (int k = 0; k < n; ++k) {
        int p = k;
        double best = fabs(A[k * n + k]);
        for (int i = k + 1; i < n; ++i)
            if (fabs(A[i * n + k]) > best) { best = fabs(A[i * n + k]); p = i; }
        if (!(best > 0.0)) return false;           // singular (or NaN): numpy.linalg.inv raises
        if (p != k) {
            for (int j = 0; j < n; ++j) { const double t = A[k * n + j]; A[k * n + j] = A[p * n + j]; A[p * n + j] = t; }
            const double t = z[k]; z[k] = z[p]; z[p] = t;
            perm_sign = -perm_sign;
        }
        const double piv = A[k * n + k];
        if (piv < 0.0) perm_sign = -perm_sign;
        la += log(fabs(piv));
        for (int i = k + 1; i < n; ++i) {
            const double l = A[i * n + k] / piv;
            for (int j = k + 1; j < n; ++j) A[i * n + j] -= l * A[k * n + j];
            z[i] -= l * z[k];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        double s2 = z[i];
        for (int j = i + 1; j < n; ++j) s2 -= A[i * n + j] * z[j];
        z[i] = s2 / A[i * n + i];
    }
    *sign = (double)perm_sign;
    *logabs = la;
    return true;
}

// dx' |S|^-1 dx for the symmetric matrix S (destroyed): cyclic Jacobi rotations, V accumulates the eigenvectors
__device__ double abs_quadratic_form(double *S, double *V, const double *dx, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i) {
            diag += S[i * n + i] * S[i * n + i];
            for (int j = 0; j < i; ++j) off += S[i * n + j] * S[i * n + j];
        }
        if (!(off > 1e-32 * diag)) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = S[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (S[q * n + q] - S[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; ++k) {
                    const double skp = S[k * n + p], skq = S[k * n + q];
                    S[k * n + p] = c * skp - sn * skq;
                    S[k * n + q] = sn * skp + c * skq;
                }
                for (int k = 0; k < n; ++k) {
                    const double spk = S[p * n + k], sqk = S[q * n + k];
                    S[p * n + k] = c * spk - sn * sqk;
                    S[q * n + k] = sn * spk + c * sqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - sn * vkq;
                    V[k * n + q] = sn * vkp + c * vkq;
                }
            }
    }
    double q = 0.0;
    for (int i = 0; i < n; ++i) {
        double u = 0.0;
        for (int k = 0; k < n; ++k) u += V[k * n + i] * dx[k];
        q += u * u / fabs(S[i * n + i]);
    }
    return q;
}

// The two items for a P that is not positive definite.  P: the full matrix (destroyed); z, W: work space of D and D * D doubles.
// false: P is singular (numpy.linalg.inv raises there) and the entry has no term.
__device__ __forceinline__ bool nll_item_indef(double *P, const double *dx, double *z, int D, double &sum) {
    double sign, logabs;
    if (!lu_solve_logdet(P, dx, z, D, &sign, &logabs)) return false;
    double q = 0.0;
    for (int d = 0; d < D; ++d) q += dx[d] * z[d];
    sum += 0.5 * (sign * logabs + q + D * 1.8378770664093453);
    return true;
}

// qb: dx' M^-1 dx of the same entry
__device__ __forceinline__ void lcr_item_indef(double *P, double *W, const double *dx, double qb, int D, double &sum) {
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) W[i * D + j] = 0.5 * (P[i * D + j] + P[j * D + i]);
    const double qa = abs_quadratic_form(W, P, dx, D);
    lcr_add(qa, qb, sum);
}

__global__ __launch_bounds__(kMetBlock) void k_indef_sums(MetArgs a, int phase) {
    const int D = a.D;
    const int t = blockIdx.y;
    extern __shared__ double sh[];
    double acc[2] = {0.0, 0.0};
    const double *x = a.x + (int64_t)t * D * a.ld, *fm = a.fm + (int64_t)t * D * a.ld;
    const double *fP = a.fP + (int64_t)t * D * D * a.ld;
    double M[kMetMaxD * kMetMaxD];
    // bits set: the streaming kernel found the step's MSE matrix positive definite (it runs no entry otherwise) and this P not
    const uint32_t left = a.left[((int64_t)t * a.chunks + blockIdx.x) * kMetBlock + threadIdx.x];
    if (phase == 2 && left != 0) {
        for (int i = 0; i < D * D; ++i) M[i] = a.mse[(int64_t)t * D * D + i];
        chol_dense<0>(M, D);
    }
    const int64_t base = (int64_t)blockIdx.x * kMetBlock * kMetPerThread;
    for (int r = 0; r < kMetPerThread; ++r) {
        const int64_t b = base + (int64_t)r * kMetBlock + threadIdx.x;
        if (b >= a.B) break;
        if (!((left >> r) & 1u)) continue;          // the streaming kernel has counted it (or it is excluded)
        double dx[kMetMaxD], P[kMetMaxD * kMetMaxD], W[kMetMaxD * kMetMaxD], z[kMetMaxD];
        for (int d = 0; d < D; ++d) dx[d] = x[(int64_t)d * a.ld + b] - fm[(int64_t)d * a.ld + b];
        for (int i = 0; i < D * D; ++i) P[i] = fP[(int64_t)i * a.ld + b];
        if (phase == 1) {
            if (!nll_item_indef(P, dx, z, D, acc[0])) continue;
            acc[1] += 1.0;
        } else {
            lcr_item_indef(P, W, dx, whitened_norm2<0>(M, dx, D), D, acc[0]);
            acc[1] += 1.0;
        }
    }
    block_sums(acc, 2, sh, a.partial + ((int64_t)t * a.chunks + blockIdx.x) * 2);
}

// ---- per-trajectory scores -----------------------------------------------------------------------------------------------------
// What the reference's studies resample (utils.py:223-244 bootstrap_var on the time-averaged score of every trajectory): for
// trajectory b, over the steps k0 .. T - 1,
//   rows 0 .. D-1  sqrt(mean_k (x - m)_d^2)      (research/bsq/bsq_ungm.py:32)
//   row  D         mean_k ||x - m||              (research/tpq/tpq_base.py:154-160)
//   row  D + 1     mean_k negative log-likelihood
//   row  D + 2     mean_k log credibility ratio against mse[k]; NaN without mse
// One lane per trajectory, the same coalesced plane reads as k_error_sums, the item bodies above.  A P that is not positive
// definite takes the fallbacks of k_indef_sums in place (traj_items_indef); a singular P, or an MSE matrix that is not positive
// definite, leaves NaN in that row, as the sums leave such entries out.  Excluded trajectories and the lanes B .. ld-1: NaN.
struct ScoreArgs {
    const double *x, *fm, *fP;     // [T][D][ld], [T][D][ld], [T][D*D][ld]
    const int32_t *status;         // [ld] or null
    const double *mse;             // [T][D*D] (regularised), device, or null
    double *scores;                // [D + 3][ld]
    int64_t B, ld;
    int32_t D, T, k0;
};

// fP: the step's covariance planes; qb: dx' M^-1 dx (read only with want_lcr)
__device__ __noinline__ void traj_items_indef(const double *fP, int64_t ld, int64_t b, const double *dx, int D, bool want_lcr,
                                              double qb, double *nll, double *lcr) {       // both are added to
    double P[kMetMaxD * kMetMaxD], W[kMetMaxD * kMetMaxD], z[kMetMaxD];
    for (int i = 0; i < D * D; ++i) P[i] = fP[(int64_t)i * ld + b];
    double s_nll = *nll, s_lcr = *lcr;
    if (!nll_item_indef(P, dx, z, D, s_nll)) s_nll = __builtin_nan("");
    if (want_lcr) {
        for (int i = 0; i < D * D; ++i) P[i] = fP[(int64_t)i * ld + b];
        lcr_item_indef(P, W, dx, qb, D, s_lcr);
    }
    *nll = s_nll;
    *lcr = s_lcr;
}

template <int DT>
__global__ __launch_bounds__(kMetBlock) void k_traj_scores(ScoreArgs a) {
    constexpr int DM = DT > 0 ? DT : kMetMaxD, TRI = DM * (DM + 1) / 2;
    const int D = DT > 0 ? DT : a.D;
    const int64_t b = (int64_t)blockIdx.x * kMetBlock + threadIdx.x;
    if (b >= a.ld) return;
    const double nan = __builtin_nan("");
    if (b >= a.B || (a.status && a.status[b] != 0)) {
        for (int r = 0; r < D + 3; ++r) a.scores[(int64_t)r * a.ld + b] = nan;
        return;
    }
    double se[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) se[d] = 0.0;
    double rm = 0.0, nll = 0.0, lcr = a.mse ? 0.0 : nan;
    for (int t = a.k0; t < a.T; ++t) {
        const double *x = a.x + (int64_t)t * D * a.ld, *fm = a.fm + (int64_t)t * D * a.ld;
        const double *fP = a.fP + (int64_t)t * D * D * a.ld;
        double dx[DM], n2 = 0.0, qb = 0.0;
        bool pd, m_ok = false;
        if constexpr (DT > 0) {
            double L[TRI], L2[TRI], M[TRI];
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) L2[SSMQ_PK(i, j)] = L[SSMQ_PK(i, j)] = SSMQ_MLOAD(fP[((int64_t)i * DT + j) * a.ld + b]);
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                dx[d] = SSMQ_MLOAD(x[(int64_t)d * a.ld + b]) - SSMQ_MLOAD(fm[(int64_t)d * a.ld + b]);
                se[d] += dx[d] * dx[d];
                n2 += dx[d] * dx[d];
            }
            pd = nll_item<DT>(L, dx, nll);
            if (a.mse) {
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) M[SSMQ_PK(i, j)] = a.mse[(int64_t)t * DT * DT + i * DT + j];
                m_ok = chol_packed<DT>(M);
                if (m_ok && pd) lcr_item<DT>(L2, M, dx, lcr);
                if (m_ok && !pd) qb = whitened_norm2_packed<DT>(M, dx);
            }
        } else {
            double P[kMetMaxD * kMetMaxD], M[kMetMaxD * kMetMaxD];
            for (int d = 0; d < D; ++d) {
                dx[d] = SSMQ_MLOAD(x[(int64_t)d * a.ld + b]) - SSMQ_MLOAD(fm[(int64_t)d * a.ld + b]);
                se[d] += dx[d] * dx[d];
                n2 += dx[d] * dx[d];
            }
            for (int i = 0; i < D; ++i)
                for (int j = 0; j <= i; ++j) P[i * D + j] = fP[((int64_t)i * D + j) * a.ld + b];
            pd = nll_item_dense(P, dx, D, nll);
            if (a.mse) {
                for (int i = 0; i < D * D; ++i) M[i] = a.mse[(int64_t)t * D * D + i];
                m_ok = chol_dense<0>(M, D);
                if (m_ok && pd) {
                    for (int i = 0; i < D; ++i)
                        for (int j = 0; j <= i; ++j) P[i * D + j] = fP[((int64_t)i * D + j) * a.ld + b];
                    lcr_item_dense(P, M, dx, D, lcr);
                }
                if (m_ok && !pd) qb = whitened_norm2<0>(M, dx, D);
            }
        }
        rm += sqrt(n2);
        if (!pd) traj_items_indef(fP, a.ld, b, dx, D, m_ok, qb, &nll, &lcr);
        if (a.mse && !m_ok) lcr = nan;
    }
    const double steps = (double)(a.T - a.k0);
#pragma unroll
    for (int d = 0; d < DM; ++d)
        if (d < D) a.scores[(int64_t)d * a.ld + b] = sqrt(se[d] / steps);
    a.scores[(int64_t)D * a.ld + b] = rm / steps;
    a.scores[(int64_t)(D + 1) * a.ld + b] = nll / steps;
    a.scores[(int64_t)(D + 2) * a.ld + b] = lcr / steps;
}

// out[t][v] = sum over chunks, in chunk order.  D > 0: phase-1 rows, partials hold the outer products as a packed
// lower triangle (NA values per row) and the output row is the full layout of met_nv(D) values.
__global__ void k_reduce_partials(const double *partial, double *out, int chunks, int NV, int total, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int t = i / NV, v = i % NV;
    int NA = NV, src = v;
    if (D > 0) {
        const int TRI = D * (D + 1) / 2;
        NA = D + 2 + TRI + 2;
        if (v >= D + 2 && v < D + 2 + D * D) {
            const int r = (v - D - 2) / D, c = (v - D - 2) % D;
            src = D + 2 + (r >= c ? SSMQ_PK(r, c) : SSMQ_PK(c, r));
        } else if (v >= D + 2 + D * D) {
            src = v - D * D + TRI;
        }
    }
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += partial[((int64_t)t * chunks + c) * NA + src];
    out[i] = s;
}

template <int DT>
hipError_t launch_phase(const MetArgs &a, int phase, hipStream_t s) {
    const int D = DT > 0 ? DT : a.D;
    const int NV = phase == 1 ? met_nv(D) : 3;       // upper bound of the packed row
    const size_t lds = sizeof(double) * (kMetBlock / 64) * NV;
    dim3 grid((unsigned)a.chunks, (unsigned)a.T);
    if constexpr (DT > 0) {
        if (phase == 1)
            hipLaunchKernelGGL(k_error_sums<DT>, grid, dim3(kMetBlock), lds, s, a);
        else
            hipLaunchKernelGGL(k_lcr_sums<DT>, grid, dim3(kMetBlock), lds, s, a);
    } else {
        if (phase == 1)
            hipLaunchKernelGGL(k_error_sums_generic, grid, dim3(kMetBlock), lds, s, a);
        else
            hipLaunchKernelGGL(k_lcr_sums_generic, grid, dim3(kMetBlock), lds, s, a);
    }
    return hipGetLastError();
}

}  // namespace


// second pass over the entries whose covariance is not positive definite: d_out [T][2] = term sum | count
int launch_metrics_indef(int phase, int D, int64_t B, int64_t ld, int T, const double *x, const double *fm, const double *fP,
                         const int32_t *status, const double *mse, double *partial, uint8_t *left, double *out, hipStream_t s) {
    MetArgs a{x, fm, fP, status, mse, partial, left, B, ld, D, T, metrics_chunks(B)};
    hipLaunchKernelGGL(k_indef_sums, dim3((unsigned)a.chunks, (unsigned)T), dim3(kMetBlock), sizeof(double) * (kMetBlock / 64) * 2,
                       s, a, phase);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "k_indef_sums");
    hipLaunchKernelGGL(k_reduce_partials, dim3((T * 2 + 255) / 256), dim3(256), 0, s, partial, out, a.chunks, 2, T * 2, 0);
    return hip_fail(hipGetLastError(), "k_reduce_partials");
}

// d_scores [D + 3][ld]; mse: device [T][D*D] or null
int launch_traj_scores(int D, int64_t B, int64_t ld, int T, int k0, const double *x, const double *fm, const double *fP,
                       const int32_t *status, const double *mse, double *scores, hipStream_t s) {
    ScoreArgs a{x, fm, fP, status, mse, scores, B, ld, D, T, k0};
    const dim3 grid((unsigned)((ld + kMetBlock - 1) / kMetBlock)), block(kMetBlock);
    switch (D) {
        case 1: hipLaunchKernelGGL(k_traj_scores<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_traj_scores<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_traj_scores<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_traj_scores<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_traj_scores<5>, grid, block, 0, s, a); break;
        case 6: hipLaunchKernelGGL(k_traj_scores<6>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(k_traj_scores<0>, grid, block, 0, s, a); break;
    }
    return hip_fail(hipGetLastError(), "k_traj_scores");
}

int metrics_values_per_step(int D) { return met_nv(D); }

// d_out [T][NV] device; d_partial scratch of T * chunks * NV doubles (chunks from metrics_chunks); left: T * chunks *
// metrics_left_bytes() bytes, written by launch_metrics and read by launch_metrics_indef of the same phase
int metrics_left_bytes() { return kMetBlock; }

int metrics_chunks(int64_t B) { return (int)((B + (int64_t)kMetBlock * kMetPerThread - 1) / ((int64_t)kMetBlock * kMetPerThread)); }

int launch_metrics(int phase, int D, int64_t B, int64_t ld, int T, const double *x, const double *fm, const double *fP,
                   const int32_t *status, const double *mse, double *partial, uint8_t *left, double *out, hipStream_t s) {
    MetArgs a{x, fm, fP, status, mse, partial, left, B, ld, D, T, metrics_chunks(B)};
    hipError_t e;
    switch (D) {
        case 1: e = launch_phase<1>(a, phase, s); break;
        case 2: e = launch_phase<2>(a, phase, s); break;
        case 3: e = launch_phase<3>(a, phase, s); break;
        case 4: e = launch_phase<4>(a, phase, s); break;
        case 5: e = launch_phase<5>(a, phase, s); break;
        case 6: e = launch_phase<6>(a, phase, s); break;
        default: e = launch_phase<0>(a, phase, s); break;
    }
    if (e != hipSuccess) return hip_fail(e, phase == 1 ? "k_error_sums" : "k_lcr_sums");
    const int NV = phase == 1 ? met_nv(D) : 3, total = T * NV;
    hipLaunchKernelGGL(k_reduce_partials, dim3((total + 255) / 256), dim3(256), 0, s, partial, out, a.chunks, NV, total,
                       phase == 1 ? D : 0);
    return hip_fail(hipGetLastError(), "k_reduce_partials");
}

}  // namespace ssmq
