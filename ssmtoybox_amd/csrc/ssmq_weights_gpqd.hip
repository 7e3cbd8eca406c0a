// Quadrature weights of GP quadrature with derivative observations (research/gpqd/gpqd_base.py: GaussianProcessDerModel.bq_weights
// with RBFGaussDer), once per parameter change: one workgroup, the joint kernel matrix of M = N + Nd D observations - the integrand's
// values at all N points and its D partial derivatives at the Nd points of which_der - LDS-resident (91 x 91 doubles at most).
// The RBF front half is the shared one of ssmq_blockla.h (rbf_stage / rbf_entry, chol_block, chol_inverse, gemm).  All length-scale
// matrices are diagonal, so every derivative expectation is a closed form in lam_k = ell_k^2 on top of q and Q of the plain kernel:
//   joint kernel, observation (n, k) = d/dx_k at point n, d_k(a, b) = (x_a - x_b)_k / lam_k:
//     K[i, (j, k)] = Kff[i, j] d_k(i, j),   K[(i, k), (j, l)] = Kff[i, j] (delta_kl / lam_k - d_k(i, j) d_l(i, j))
//   expectations under N(0, I), scaling = False:
//     qd[(n, k)]          = -q_n x_nk / (1 + lam_k)
//     Rd[a, (n, k)]       = q_n delta_ak / (1 + lam_k) + (x_na / (1 + lam_a)) qd[(n, k)]
//     Qfd[i, (n, k)]      = Q[n, i] (eta_nk + eta_ik - x_nk / lam_k),                       eta_nk = x_nk / (lam_k (2 + lam_k))
//     Qdd[(i, k), (j, l)] = Q[i, j] ((x_ik / lam_k - mu_k) (x_jl / lam_l - mu_l) + delta_kl / (lam_k (2 + lam_k))),  mu = eta_i + eta_j
//   weights: iK = sym((K + jitter I)^-1), wm = q~ iK, Wc = sym(iK Q~ iK), Wcc = R~ iK, model_var = alpha^2 (1 - tr(Q~ iK)),
//     integral_var = alpha^2 det(2 Lam^-1 + I)^-1/2 - wm q~.
// Every expectation takes the subset as it is - the reference's bq_weights passes which_der to exp_x_dkx alone and fails on a proper
// subset.  Not a hot path: one launch of 256 threads.
#include "ssmq_weights_host.h"
#include "ssmq_blockla.h"

namespace ssmq {

struct GpqdWgtArgs {
    int D, N, Nd, M, scaling;
    double jitter;
    const double *xi, *par;        // [D][N], [1 + D]
    const int32_t *wd;             // [Nd]
    double *work;
    double *wm, *Wc, *Wcc, *mv, *iv, *K, *L, *iK, *q, *Q, *R;
    int32_t *status;
};

static size_t gpqd_work_doubles(int D, int N, int M) { return (size_t)D * N + 2 * (size_t)N + 2 * (size_t)N * N + 2 * (size_t)M * M + 64; }

static __device__ double block_sum256(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    bsync();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    bsync();
    double s = 0.0;
    for (int w = 0; w < kWgtBlock / 64; ++w) s += red[w];
    bsync();
    return s;
}

__global__ __launch_bounds__(256) void k_weights_gpqd(const GpqdWgtArgs a) {
    extern __shared__ double A[];          // [M][M]: the joint kernel matrix, then its factor
    __shared__ double s_sil[SSMQ_MAX_DIM], s_red[16];
    __shared__ int s_flag;
    const int D = a.D, N = a.N, M = a.M, tid = threadIdx.x;
    double *w = a.work;
    double *zs = w; w += D * N;
    double *nrm = w; w += N;
    double *qf = w; w += N;
    double *Kff = w; w += N * N;
    double *Qff = w; w += N * N;
    double *X = w; w += M * M;
    double *T = w;
    const double alpha = a.par[0];
    if (tid < D) s_sil[tid] = 1.0 / a.par[1 + tid];
    rbf_stage(s_sil, a.xi, zs, nrm, D, N);
    const double la = a.scaling ? 2.0 * log(alpha) : 0.0;
    for (int idx = tid; idx < N * N; idx += kWgtBlock) Kff[idx] = rbf_entry(la, zs, nrm, N, D, idx / N, idx % N);
    bsync();
#define GQ_X(d, n) a.xi[(d) * N + (n)]
#define GQ_IL(d) (s_sil[d] * s_sil[d])
    // observation r: point and derivative direction (-1: the value)
#define GQ_PT(r) ((r) < N ? (r) : a.wd[((r) - N) / D])
#define GQ_DIR(r) ((r) < N ? -1 : ((r) - N) % D)
    for (int idx = tid; idx < M * M; idx += kWgtBlock) {
        const int r = idx / M, c = idx % M;
        const int pr = GQ_PT(r), pc = GQ_PT(c), kr = GQ_DIR(r), kc = GQ_DIR(c);
        const double kff = Kff[pr * N + pc];
        double v;
        if (kr < 0 && kc < 0) {
            v = kff;
        } else if (kr < 0) {
            v = kff * (GQ_IL(kc) * (GQ_X(kc, pr) - GQ_X(kc, pc)));
        } else if (kc < 0) {
            v = kff * (GQ_IL(kr) * (GQ_X(kr, pc) - GQ_X(kr, pr)));
        } else {
            const double dr = GQ_IL(kr) * (GQ_X(kr, pr) - GQ_X(kr, pc)), dc = GQ_IL(kc) * (GQ_X(kc, pr) - GQ_X(kc, pc));
            v = kff * ((kr == kc ? GQ_IL(kr) : 0.0) - dr * dc);
        }
        a.K[idx] = v;
        A[idx] = v + (r == c ? a.jitter : 0.0);
    }
    bsync();
    const bool pd = chol_block(A, M, &s_flag);
    if (tid == 0) *a.status = pd ? 0 : 1;
    if (!pd) {
        const double nan = __builtin_nan("");
        for (int idx = tid; idx < M * M; idx += kWgtBlock) { a.L[idx] = nan; a.iK[idx] = nan; a.Wc[idx] = nan; a.Q[idx] = nan; }
        for (int idx = tid; idx < D * M; idx += kWgtBlock) { a.Wcc[idx] = nan; a.R[idx] = nan; }
        for (int idx = tid; idx < M; idx += kWgtBlock) { a.wm[idx] = nan; a.q[idx] = nan; }
        if (tid == 0) { *a.mv = nan; *a.iv = nan; }
        return;
    }
    for (int idx = tid; idx < M * M; idx += kWgtBlock) a.L[idx] = (idx % M <= idx / M) ? A[idx] : 0.0;
    chol_inverse(A, X, M);
    for (int idx = tid; idx < M * M; idx += kWgtBlock) {
        const int i = idx / M, j = idx % M;
        a.iK[idx] = 0.5 * (X[i * M + j] + X[j * M + i]);
    }
    // ---- expectations of the plain kernel (as k_weights forms them), then the derivative ones ---------------------------------
    double cq = 1.0, cQ = 1.0, ck = 1.0;
    for (int d = 0; d < D; ++d) {
        const double il = GQ_IL(d);
        cq *= il + 1.0;
        cQ *= il + il + 1.0;
        ck *= 2.0 * il + 1.0;
    }
    cq = 1.0 / sqrt(cq);
    cQ = 1.0 / sqrt(cQ);
    const double kbar = alpha * alpha * (1.0 / sqrt(ck));
    for (int n = tid; n < N; n += kWgtBlock) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) {
            const double lam = 1.0 / GQ_IL(d), x = GQ_X(d, n);
            s += x * ((1.0 / (lam + 1.0)) * x);
        }
        qf[n] = cq * exp(-0.5 * s);
    }
    for (int idx = tid; idx < N * N; idx += kWgtBlock) {
        const int i = idx / N, j = idx % N;
        double m2i = 0.0, m2j = 0.0, mij = 0.0, ni = 0.0, nj = 0.0;
        for (int d = 0; d < D; ++d) {
            const double il = GQ_IL(d);
            const double v = 1.0 / (il + il + 1.0);
            const double yi = il * GQ_X(d, i), yj = -(il * GQ_X(d, j));
            m2i += (yi * v) * yi;
            m2j += (yj * v) * yj;
            mij += (yi * v) * yj;
            ni += il * GQ_X(d, i) * GQ_X(d, i);
            nj += il * GQ_X(d, j) * GQ_X(d, j);
        }
        const double mh = (m2i + m2j) - 2.0 * mij;
        Qff[idx] = cQ * exp(((0.0 - 0.5 * ni) + (0.0 - 0.5 * nj)) + 0.5 * mh);
    }
    bsync();
#define GQ_LAM(d) (1.0 / GQ_IL(d))
#define GQ_ETA(d, n) (GQ_X(d, n) / (GQ_LAM(d) * (2.0 + GQ_LAM(d))))
    for (int r = tid; r < M; r += kWgtBlock) {
        const int p = GQ_PT(r), k = GQ_DIR(r);
        a.q[r] = k < 0 ? qf[p] : -(qf[p] * GQ_X(k, p) / (1.0 + GQ_LAM(k)));
    }
    for (int idx = tid; idx < D * M; idx += kWgtBlock) {
        const int d = idx / M, r = idx % M;
        const int p = GQ_PT(r), k = GQ_DIR(r);
        const double mu = GQ_X(d, p) / (1.0 + GQ_LAM(d));
        a.R[idx] = k < 0 ? qf[p] * mu : (d == k ? qf[p] / (1.0 + GQ_LAM(k)) : 0.0) + mu * -(qf[p] * GQ_X(k, p) / (1.0 + GQ_LAM(k)));
    }
    for (int idx = tid; idx < M * M; idx += kWgtBlock) {
        const int r = idx / M, c = idx % M;
        const int pr = GQ_PT(r), pc = GQ_PT(c), kr = GQ_DIR(r), kc = GQ_DIR(c);
        const double qq = Qff[pr * N + pc];
        double v;
        if (kr < 0 && kc < 0) {
            v = qq;
        } else if (kr < 0) {
            v = qq * ((GQ_ETA(kc, pc) + GQ_ETA(kc, pr)) - GQ_X(kc, pc) * GQ_IL(kc));
        } else if (kc < 0) {
            v = qq * ((GQ_ETA(kr, pr) + GQ_ETA(kr, pc)) - GQ_X(kr, pr) * GQ_IL(kr));
        } else {
            const double t1 = GQ_X(kr, pr) * GQ_IL(kr) - (GQ_ETA(kr, pr) + GQ_ETA(kr, pc));
            const double t2 = GQ_X(kc, pc) * GQ_IL(kc) - (GQ_ETA(kc, pr) + GQ_ETA(kc, pc));
            v = qq * (t1 * t2 + (kr == kc ? 1.0 / (GQ_LAM(kr) * (2.0 + GQ_LAM(kr))) : 0.0));
        }
        a.Q[idx] = v;
    }
    bsync();
    // ---- weights ---------------------------------------------------------------------------------------------------------------
    gemm(a.wm, M, a.q, M, false, a.iK, M, false, 1, M, M);          // wm = q~ iK
    gemm(a.Wcc, M, a.R, M, false, a.iK, M, false, D, M, M);         // Wcc = R~ iK
    gemm(T, M, a.iK, M, false, a.Q, M, false, M, M, M);             // T = iK Q~
    gemm(X, M, T, M, false, a.iK, M, false, M, M, M);               // X = iK Q~ iK
    for (int idx = tid; idx < M * M; idx += kWgtBlock) {
        const int i = idx / M, j = idx % M;
        a.Wc[idx] = 0.5 * (X[i * M + j] + X[j * M + i]);
    }
    double tr = 0.0, qw = 0.0;
    for (int idx = tid; idx < M * M; idx += kWgtBlock) tr += a.Q[idx] * a.iK[(idx % M) * M + idx / M];
    for (int r = tid; r < M; r += kWgtBlock) qw += a.wm[r] * a.q[r];
    tr = block_sum256(tr, s_red);
    qw = block_sum256(qw, s_red);
    if (tid == 0) {
        *a.mv = alpha * alpha * (1.0 - tr);
        *a.iv = kbar - qw;
    }
#undef GQ_X
#undef GQ_IL
#undef GQ_PT
#undef GQ_DIR
#undef GQ_LAM
#undef GQ_ETA
}

}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_weights_gpqd(int D, int N, const double *xi, const double *par, int Nd, const int32_t *which_der, double jitter,
                                 int scaling, double *wm, double *Wc, double *Wcc, double *model_var, double *integral_var,
                                 double *K_out, double *L_out, double *iK_out, double *q_out, double *Q_out, double *R_out) {
    if (!xi || !par || Nd < 0 || (Nd > 0 && !which_der)) {
        set_error("ssmq_weights_gpqd: bad argument");
        return SSMQ_E_ARG;
    }
    if (D < 1 || D > SSMQ_USER_MAX_D || N < 2 || N > 2 * D + 1 || Nd > N) {
        set_error("ssmq_weights_gpqd: supported are D <= 6, 2 <= N <= 2 D + 1 points and at most N derivative points");
        return SSMQ_E_UNSUPPORTED;
    }
    for (int j = 0; j < Nd; ++j)
        if (which_der[j] < 0 || which_der[j] >= N || (j > 0 && which_der[j] <= which_der[j - 1])) {
            set_error("ssmq_weights_gpqd: which_der must be strictly increasing indices into the points");
            return SSMQ_E_ARG;
        }
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t s = stream();
    const int M = N + Nd * D;
    const size_t mm = (size_t)M * M, sizes[] = {(size_t)D * N, (size_t)1 + D, (size_t)(Nd + 1) / 2 + 1, gpqd_work_doubles(D, N, M),
                                                (size_t)M, mm, (size_t)D * M, 1, 1, mm, mm, mm, (size_t)M, mm, (size_t)D * M, 1};
    constexpr int kParts = sizeof(sizes) / sizeof(sizes[0]);
    size_t total = 0;
    for (size_t n : sizes) total += (n * sizeof(double) + 255) / 256 * 256;
    DBuf arena;
    if ((rc = arena.alloc(total))) return rc;
    double *part[kParts];
    {
        char *base = (char *)arena.p;
        for (int i = 0; i < kParts; ++i) {
            part[i] = (double *)base;
            base += (sizes[i] * sizeof(double) + 255) / 256 * 256;
        }
    }
    SSMQ_HIP(hipMemcpyAsync(part[0], xi, sizeof(double) * D * N, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(part[1], par, sizeof(double) * (1 + D), hipMemcpyHostToDevice, s));
    if (Nd > 0) SSMQ_HIP(hipMemcpyAsync(part[2], which_der, sizeof(int32_t) * Nd, hipMemcpyHostToDevice, s));
    GpqdWgtArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.N = N; a.Nd = Nd; a.M = M; a.scaling = scaling ? 1 : 0; a.jitter = jitter;
    a.xi = part[0]; a.par = part[1]; a.wd = (const int32_t *)part[2]; a.work = part[3];
    a.wm = part[4]; a.Wc = part[5]; a.Wcc = part[6]; a.mv = part[7]; a.iv = part[8]; a.K = part[9]; a.L = part[10]; a.iK = part[11];
    a.q = part[12]; a.Q = part[13]; a.R = part[14]; a.status = (int32_t *)part[15];
    const size_t lds = sizeof(double) * mm;
    static thread_local unsigned attr_epoch = ~0u;
    if ((rc = set_max_dynamic_lds(attr_epoch, {(const void *)k_weights_gpqd}, sizeof(double) * 91 * 91))) return rc;
    hipLaunchKernelGGL(k_weights_gpqd, dim3(1), dim3(256), lds, s, a);
    if ((rc = hip_fail(hipGetLastError(), "k_weights_gpqd"))) return rc;
#define SSMQ_D2H(host, idx, count) \
    if (host) SSMQ_HIP(hipMemcpyAsync(host, part[idx], sizeof(double) * (count), hipMemcpyDeviceToHost, s));
    SSMQ_D2H(wm, 4, (size_t)M)
    SSMQ_D2H(Wc, 5, mm)
    SSMQ_D2H(Wcc, 6, (size_t)D * M)
    SSMQ_D2H(model_var, 7, 1)
    SSMQ_D2H(integral_var, 8, 1)
    SSMQ_D2H(K_out, 9, mm)
    SSMQ_D2H(L_out, 10, mm)
    SSMQ_D2H(iK_out, 11, mm)
    SSMQ_D2H(q_out, 12, (size_t)M)
    SSMQ_D2H(Q_out, 13, mm)
    SSMQ_D2H(R_out, 14, (size_t)D * M)
#undef SSMQ_D2H
    int32_t st = 0;
    SSMQ_HIP(hipMemcpyAsync(&st, part[15], sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    return st ? 1 : SSMQ_OK;
}
