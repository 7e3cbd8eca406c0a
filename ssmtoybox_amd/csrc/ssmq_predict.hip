// ---- prediction: Model.predict of the GP, TP and Bayes-Sard models (bq/bqmod.py:454-493, 840-891, 1090-1130), batched ----------
//
// B independent fits, M test points each.  Two kernels, because the factorisation is per fit and the test points are not:
//   k_predict_fit   one 256-thread workgroup per fit, the front half of ml2_eval: K + jitter I at the NATURAL parameters
//                   (the arithmetic of k_rbf_factor), Cholesky, explicit inverse (N <= 64: dense in LDS, symmetrised as
//                   _cho_inv does; N <= 128: packed lower triangles, the lower triangle taken for the symmetric matrix), then
//                   A = iK Y, the TP scale (nu - 2 + y'iK y) / (nu - 2 + num_pts) and, for Bayes-Sard, V, Z = V'iK,
//                   (Z V)^-1 by Cholesky (no jitter on Z V here, unlike bq_weights) and A_bs = (Z V)^-1 V'.  Everything
//                   phase 2 needs goes to a per-fit workspace (PredCarve), the status flag too.
//   k_predict_test  one 256-thread workgroup per (fit, tile of up to 64 test points): lane l of every wave owns test point
//                   l of the tile, the four waves share the rows of each sum and add their parts in wave order.  The
//                   fit's packed iK is loaded into LDS once; the kx row of every lane is parked in LDS as kx[n][lane]
//                   (consecutive lanes, consecutive doubles: no bank conflict), iK is read as LDS broadcasts.
// A fit's arithmetic depends on nothing but its own data and (N, NB) - not on B, M or the position in the batch - so row b
// of a batch is bit-equal to a batch of one.
#include <algorithm>
#include "ssmq_weights_host.h"
#include "ssmq_blockla.h"

namespace ssmq {

constexpr int kPredBlock = 256, kPredWaves = kPredBlock / 64;

struct PredCarve {      // offsets (doubles) into one fit's workspace
    int64_t iK, A, scal, zs, nrm, V, Z, G, iG, Abs, end;
    __host__ __device__ PredCarve(int64_t D, int64_t N, int64_t E, int64_t NB) {
        int64_t w = 0;
        iK = w; w += N * (N + 1) / 2;   // packed lower triangle of sym((K + jitter I)^-1)
        A = w; w += N * E;              // iK Y
        scal = w; w += 2;               // [0]: TP variance scale (1 for the GP)
        zs = w; w += D * N;             // Lam^-1/2 x_obs
        nrm = w; w += N;                // |zs_n|^2
        V = w; w += N * NB;             // Vandermonde of x_obs (N x NB)
        Z = w; w += NB * N;             // V' iK
        G = w; w += NB * NB;            // Z V -> its Cholesky factor
        iG = w; w += NB * NB;           // (Z V)^-1
        Abs = w; w += NB * N;           // (Z V)^-1 V'
        end = w;
    }
};

struct PredArgs {
    int32_t D, N, E, NB, x_per_fit, test_per_fit, tile, tp_num_pts;
    int64_t B, M, ntiles;
    double jitter, nu;                  // nu = 0: no TP scale
    const double *x;                    // [D][N] or [B][D][N]
    const double *y;                    // [B][N][E]
    const double *par;                  // [B][1 + D], natural parameters
    const int32_t *mulind;              // [D][NB]
    const double *test;                 // [D][M] or [B][D][M]
    double *work;                       // [B] x PredCarve::end
    double *mean, *var;                 // [B][M][E], [B][M]
    int32_t *status;                    // [B]
};

template <bool PACKED>
__global__ __launch_bounds__(kPredBlock) void k_predict_fit(const PredArgs a) {
    extern __shared__ __align__(16) double lds[];
    __shared__ double s_sil[SSMQ_MAX_DIM];
    __shared__ int s_flag;
    const int D = a.D, N = a.N, E = a.E, NB = a.NB, tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t nn = PACKED ? (int64_t)N * (N + 1) / 2 : (int64_t)N * N;
    const PredCarve cv(D, N, E, NB);
    double *w = a.work + b * cv.end;
    double *Km = lds, *Xm = lds + nn;
    const double *x = a.x + (a.x_per_fit ? b * D * N : 0);
    const double *Y = a.y + b * N * E;
    const double *pr = a.par + b * (1 + D);
    double *zs = w + cv.zs, *nrm = w + cv.nrm;
    const double la = 2.0 * log(pr[0]);
    if (tid < D) s_sil[tid] = 1.0 / pr[1 + tid];
    rbf_stage(s_sil, x, zs, nrm, D, N);
    for (int idx = tid; idx < N * N; idx += kWgtBlock) {
        const int i = idx / N, j = idx % N;
        if (j > i) continue;
        Km[tri_idx<PACKED>(i, j, N)] = rbf_entry(la, zs, nrm, N, D, i, j) + (i == j ? a.jitter : 0.0);
    }
    bsync();
    if (!chol_factor_tri<PACKED>(Km, N, &s_flag)) {
        if (tid == 0) a.status[b] = 1;
        return;
    }
    chol_inverse_tri<PACKED>(Km, Xm, N);
    // S: the symmetric inverse as a packed lower triangle, in LDS for the products below and in the workspace for phase 2
    double *S = PACKED ? Xm : Km;
    if (!PACKED) {
        for (int idx = tid; idx < N * N; idx += kWgtBlock) {
            const int i = idx / N, j = idx % N;
            if (j <= i) S[SSMQ_PKL(i, j)] = 0.5 * (Xm[i * N + j] + Xm[j * N + i]);     // Km: the factor is no longer needed
        }
        bsync();
    }
    for (int idx = tid; idx < N * (N + 1) / 2; idx += kWgtBlock) w[cv.iK + idx] = S[idx];
    double *A = w + cv.A;
    for (int idx = tid; idx < N * E; idx += kWgtBlock) {
        const int i = idx / E, e = idx % E;
        double s = 0.0;
        for (int k = 0; k < N; ++k) s += SSMQ_SYM_LOWER(true, S, i, k, N) * Y[k * E + e];
        A[idx] = s;
    }
    bsync();
    if (tid == 0) {
        double scale = 1.0;
        if (a.nu != 0.0) {              // E = 1 (checked by the entry point)
            double s = 0.0;
            for (int i = 0; i < N; ++i) s += Y[i] * A[i];
            scale = (a.nu - 2.0 + s) / (a.nu - 2.0 + a.tp_num_pts);
        }
        w[cv.scal] = scale;
    }
    int st = 0;
    if (NB > 0) {
        double *V = w + cv.V, *Z = w + cv.Z, *G = w + cv.G, *iG = w + cv.iG, *Abs = w + cv.Abs;
        for (int idx = tid; idx < N * NB; idx += kWgtBlock) {
            const int n = idx / NB, q = idx % NB;
            double v = 1.0;
            for (int d = 0; d < D; ++d) v *= ipow(x[d * N + n], a.mulind[d * NB + q]);
            V[idx] = v;
        }
        bsync();
        for (int idx = tid; idx < NB * N; idx += kWgtBlock) {
            const int q = idx / N, n = idx % N;
            double s = 0.0;
            for (int k = 0; k < N; ++k) s += V[k * NB + q] * SSMQ_SYM_LOWER(true, S, k, n, N);
            Z[idx] = s;
        }
        bsync();
        // Z V; the reference factors it with cho_factor's lower=False, which reads the upper triangle: entry (i, j), j <= i,
        // of the factor's input is (Z V)(j, i)
        for (int idx = tid; idx < NB * NB; idx += kWgtBlock) {
            const int i = idx / NB, j = idx % NB;
            double s = 0.0;
            if (j <= i)
                for (int n = 0; n < N; ++n) s += Z[j * N + n] * V[n * NB + i];
            G[idx] = s;
        }
        bsync();
        if (chol_block(G, NB, &s_flag)) {
            chol_inverse(G, iG, NB);
            for (int idx = tid; idx < NB * N; idx += kWgtBlock) {
                const int q = idx / N, n = idx % N;
                double s = 0.0;
                for (int r = 0; r < NB; ++r) s += iG[q * NB + r] * V[n * NB + r];
                Abs[idx] = s;
            }
        } else {
            st = 2;
        }
    }
    if (tid == 0) a.status[b] = st;
}

// the four waves' parts of one per-lane sum, added in wave order (to every wave); red: kPredBlock doubles of LDS
__device__ __forceinline__ double pred_tile_sum(double v, double *red) {
    red[threadIdx.x] = v;
    bsync();
    const int lane = threadIdx.x & 63;
    double s = red[lane];
#pragma unroll
    for (int wv = 1; wv < kPredWaves; ++wv) s += red[wv * 64 + lane];
    bsync();
    return s;
}

__global__ __launch_bounds__(kPredBlock) void k_predict_test(const PredArgs a) {
    extern __shared__ __align__(16) double lds[];
    const int D = a.D, N = a.N, E = a.E, NB = a.NB, tile = a.tile, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x / a.ntiles, t = blockIdx.x % a.ntiles, M = a.M;
    const int64_t m = t * tile + lane;
    const bool mine = wave == 0 && lane < tile && m < M;
    double *mean = a.mean + (b * M + m) * E, *var = a.var + b * M + m;
    if (a.status[b] != 0) {                 // uniform: the fit has no factorisation
        if (mine) {
            for (int e = 0; e < E; ++e) mean[e] = __builtin_nan("");
            *var = __builtin_nan("");
        }
        return;
    }
    const PredCarve cv(D, N, E, NB);
    const double *__restrict__ w = a.work + b * cv.end;
    const int npk = N * (N + 1) / 2;
    double *iK = lds, *kx = iK + npk, *bv = kx + (int64_t)N * tile, *red = bv + (int64_t)NB * tile;
    for (int idx = tid; idx < npk; idx += kPredBlock) iK[idx] = w[cv.iK + idx];
    // lanes past the tile or past M work on the last test point and store nothing
    const int64_t mc = m < M ? m : M - 1;
    const int kl = lane < tile ? lane : tile - 1;       // their LDS column: a duplicate of the tile's last
    const double *xt = a.test + (a.test_per_fit ? b * D * M : 0);
    const double *pr = a.par + b * (1 + D);
    const double *zs = w + cv.zs, *nrm = w + cv.nrm;
    const double la = 2.0 * log(pr[0]);
    // kx as RBFGauss.eval forms it (k_rbf_eval): exp(2 log alpha - (|a|^2 + |b|^2 - 2 a.b) / 2)
    double z[SSMQ_MAX_DIM];
    double na = 0.0;
#pragma unroll
    for (int d = 0; d < SSMQ_MAX_DIM; ++d) {
        z[d] = 0.0;
        if (d < D) {
            z[d] = (1.0 / pr[1 + d]) * xt[d * M + mc];
            na += z[d] * z[d];
        }
    }
    if (lane < tile) {
        for (int n = wave; n < N; n += kPredWaves) {
            double dot = 0.0;
#pragma unroll
            for (int d = 0; d < SSMQ_MAX_DIM; ++d)
                if (d < D) dot += z[d] * zs[d * N + n];
            kx[n * tile + lane] = rbf_exp(la, na, nrm[n], dot);
        }
    }
    bsync();
    // kx iK kx' over the packed triangle: row i gives kx_i (2 sum_{j < i} iK_ij kx_j + iK_ii kx_i)
    double acc = 0.0;
    for (int i = wave; i < N; i += kPredWaves) {
        const double *row = iK + SSMQ_PKL(i, 0);
        double s = 0.0;
        for (int j = 0; j < i; ++j) s += row[j] * kx[j * tile + kl];
        const double ki = kx[i * tile + kl];
        acc += ki * (2.0 * s + row[i] * ki);
    }
    const double quad = pred_tile_sum(acc, red);
    double v = exp(la) - quad;              // kxx = eval(test, test, diag=True) = exp(2 log alpha - 0)
    if (NB > 0) {
        // b = Z kx' - vx', var += b' (Z V)^-1 b, and kx <- kx - b' A_bs in place for the mean
        const double *Z = w + cv.Z, *iG = w + cv.iG, *Abs = w + cv.Abs;
        for (int q = wave; q < NB; q += kPredWaves) {
            double s = 0.0;
            for (int n = 0; n < N; ++n) s += Z[q * N + n] * kx[n * tile + kl];
            double vx = 1.0;
            for (int d = 0; d < D; ++d) vx *= ipow(xt[d * M + mc], a.mulind[d * NB + q]);
            if (lane < tile) bv[q * tile + lane] = s - vx;
        }
        bsync();
        double bq = 0.0;
        for (int q = wave; q < NB; q += kPredWaves) {
            double s = 0.0;
            for (int r = 0; r < NB; ++r) s += iG[q * NB + r] * bv[r * tile + kl];
            bq += bv[q * tile + kl] * s;
        }
        v += pred_tile_sum(bq, red);
        for (int n = wave; n < N; n += kPredWaves) {
            double s = 0.0;
            for (int q = 0; q < NB; ++q) s += bv[q * tile + kl] * Abs[q * N + n];
            if (lane < tile) kx[n * tile + lane] -= s;
        }
        bsync();
    }
    v *= w[cv.scal];
    const double *A = w + cv.A;
    double me[kFitMaxE];
#pragma unroll
    for (int e = 0; e < kFitMaxE; ++e) me[e] = 0.0;
    for (int n = wave; n < N; n += kPredWaves) {
        const double k = kx[n * tile + kl];
#pragma unroll
        for (int e = 0; e < kFitMaxE; ++e)
            if (e < E) me[e] += k * A[n * E + e];
    }
#pragma unroll
    for (int e = 0; e < kFitMaxE; ++e) {
        if (e < E) {                        // uniform
            const double s = pred_tile_sum(me[e], red);
            if (mine) mean[e] = s;
        }
    }
    if (mine) *var = v;
}

static size_t pred_test_lds(int N, int NB, int tile) {
    return sizeof(double) * ((size_t)N * (N + 1) / 2 + (size_t)(N + NB) * tile + kPredBlock);
}

}  // namespace ssmq

extern "C" int ssmq_gp_predict_batch(int D, int N, int E, int64_t B, const double *x_obs, int x_per_fit, const double *fcn_obs,
                                     double jitter, double nu, int tp_num_pts, const double *par, const int32_t *mulind, int NB,
                                     int64_t M, const double *test, int test_per_fit, double *mean, double *var,
                                     int32_t *status) {
    using namespace ssmq;
    const bool ok = M >= 1 && NB >= 0 && (NB == 0 || mulind) && (nu == 0.0 || (E == 1 && NB == 0 && tp_num_pts >= 1)) &&
                    jitter >= 0.0 && (B <= 0 || (x_obs && fcn_obs && par && test && mean && var && status));
    int rc = fit_check("gp_predict_batch", D, N, E, B, nu, ok, NB <= N && M <= INT32_MAX, ", num_basis <= N, M <= 2^31 - 1");
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    const bool packed = N > 64;
    const size_t cap = 160 * 1024 - 1024;
    static thread_local unsigned attr_epoch = 0;
    if ((rc = set_max_dynamic_lds(attr_epoch, {(const void *)k_predict_fit<true>, (const void *)k_predict_fit<false>,
                                               (const void *)k_predict_test}, cap)))
        return rc;
    // the widest tile whose LDS fits: 64 lanes but for Bayes-Sard with many basis functions on many points
    int tile = 64;
    while (tile > 8 && pred_test_lds(N, NB, tile) > cap) tile >>= 1;
    const size_t fit_lds = sizeof(double) * 2 * (packed ? (size_t)N * (N + 1) / 2 : (size_t)N * N);
    const PredCarve cv(D, N, E, NB);
    const int64_t ntiles = (M + tile - 1) / tile;
    // rows per chunk: workspace and results of a chunk within 512 MiB, its grid within 2^31 - 1 workgroups
    const size_t per_fit = sizeof(double) * ((size_t)cv.end + (size_t)M * (E + 1));
    int64_t cb = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20) / per_fit));
    cb = std::min<int64_t>(std::min<int64_t>(cb, B), std::max<int64_t>(1, (int64_t)INT32_MAX / ntiles));
    const size_t nx = (size_t)D * N * (x_per_fit ? B : 1), ny = (size_t)B * N * E, np = (size_t)B * (1 + D);
    const size_t nt = (size_t)D * M * (test_per_fit ? B : 1);
    DBuf dx, dy, dp, dt, dmi, dw, dm, dv, dst;
    if ((rc = dx.alloc(sizeof(double) * nx)) || (rc = dy.alloc(sizeof(double) * ny)) || (rc = dp.alloc(sizeof(double) * np)) ||
        (rc = dt.alloc(sizeof(double) * nt)) || (rc = dmi.alloc(sizeof(int32_t) * (size_t)D * NB)) ||
        (rc = dw.alloc(sizeof(double) * (size_t)cv.end * cb)) || (rc = dm.alloc(sizeof(double) * (size_t)cb * M * E)) ||
        (rc = dv.alloc(sizeof(double) * (size_t)cb * M)) || (rc = dst.alloc(sizeof(int32_t) * cb)))
        return rc;
    SSMQ_HIP(hipMemcpyAsync(dx.p, x_obs, sizeof(double) * nx, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dy.p, fcn_obs, sizeof(double) * ny, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dp.p, par, sizeof(double) * np, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dt.p, test, sizeof(double) * nt, hipMemcpyHostToDevice, s));
    if (NB > 0) SSMQ_HIP(hipMemcpyAsync(dmi.p, mulind, sizeof(int32_t) * (size_t)D * NB, hipMemcpyHostToDevice, s));
    PredArgs a{};
    a.D = D; a.N = N; a.E = E; a.NB = NB; a.x_per_fit = x_per_fit ? 1 : 0; a.test_per_fit = test_per_fit ? 1 : 0;
    a.tile = tile; a.tp_num_pts = tp_num_pts; a.M = M; a.ntiles = ntiles; a.jitter = jitter; a.nu = nu;
    a.mulind = (const int32_t *)dmi.p; a.work = dw.d(); a.mean = dm.d(); a.var = dv.d(); a.status = (int32_t *)dst.p;
    for (int64_t b0 = 0; b0 < B; b0 += cb) {
        const int64_t nb = std::min<int64_t>(cb, B - b0);
        a.B = nb;
        a.x = dx.d() + (x_per_fit ? b0 * D * N : 0);
        a.y = dy.d() + b0 * N * E;
        a.par = dp.d() + b0 * (1 + D);
        a.test = dt.d() + (test_per_fit ? b0 * D * M : 0);
        if (packed) hipLaunchKernelGGL(k_predict_fit<true>, dim3((unsigned)nb), dim3(kPredBlock), fit_lds, s, a);
        else hipLaunchKernelGGL(k_predict_fit<false>, dim3((unsigned)nb), dim3(kPredBlock), fit_lds, s, a);
        if ((rc = hip_fail(hipGetLastError(), "k_predict_fit"))) return rc;
        hipLaunchKernelGGL(k_predict_test, dim3((unsigned)(nb * ntiles)), dim3(kPredBlock), pred_test_lds(N, NB, tile), s, a);
        if ((rc = hip_fail(hipGetLastError(), "k_predict_test"))) return rc;
        SSMQ_HIP(hipMemcpyAsync(mean + b0 * M * E, dm.p, sizeof(double) * nb * M * E, hipMemcpyDeviceToHost, s));
        SSMQ_HIP(hipMemcpyAsync(var + b0 * M, dv.p, sizeof(double) * nb * M, hipMemcpyDeviceToHost, s));
        SSMQ_HIP(hipMemcpyAsync(status + b0, dst.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, s));
        SSMQ_HIP(hipStreamSynchronize(s));      // the next chunk reuses the workspace and the result buffers
    }
    for (int64_t b = 0; b < B; ++b)
        if (status[b]) return (int)std::min<int64_t>(b + 1, INT32_MAX);
    return SSMQ_OK;
}
