// ---- type-II maximum likelihood (ML-II) of the RBF kernel's parameters ----------------------------------------------------
//
//   GaussianProcessModel.neg_log_marginal_likelihood     bq/bqmod.py:537-596
//   StudentTProcessModel.neg_log_marginal_likelihood     bq/bqmod.py:1191-1245
//   RBFGauss.der_par                                     bq/bqkern.py:426-436
//   Model.optimize (scipy.optimize.minimize, BFGS, jac)  bq/bqmod.py:250-285
//
// One workgroup per row b (a parameter point, or a whole fit).  At log-parameters [log alpha, log ell_1 .. log ell_D]:
//   K = alpha^2 exp(-maha(Lam^-1/2 x) / 2) + jitter (the N x N jitter matrix), L = chol(K), X = K^-1, A = X Y  (Y: N x E)
//   GP value  E sum log diag L + (sum Y o A + E N log 2 pi) / 2
//   TP value  (nu + N) / 2 sum_e log(1 + y_e'a_e / (nu - 2)) + E (sum log diag L + const)
//   gradient  g_p = 1/2 sum_ij W_ij dK_p(i, j),  W = E X - A diag(s) A',  s_e = 1 (GP) or (nu + N) / (nu + y_e'a_e - 2) (TP)
// dK_p is der_par's: K WITHOUT the jitter, d/d alpha = 2 K / alpha (with respect to alpha itself, not log alpha - the
// reference's quirk, kept: the first gradient entry is the true derivative divided by alpha) and d/d log ell_d =
// (x_di - x_dj)^2 / ell_d^2 K.  The sum runs over the lower triangle once (W and dK are symmetric), so no N x N x P array is
// formed.  N <= 64: K / its factor and X dense in LDS (chol_block, chol_inverse as k_weights); N <= 128: packed lower
// triangles (chol_packed_lds and its packed twin below), 2 x 66 KiB at N = 128.  Both routes read the lower triangle of X,
// which the two inverses form with the same arithmetic.
// ML-II: one lane of the workgroup runs the row's BFGS state machine (ssmq_bfgs.h, analytic-gradient mode) in LDS, the
// workgroup evaluates the objective at its pending point, until the state machine ends - one launch for all fits, no
// grid-wide synchronisation.  A point where K is not positive definite is a value of +inf with a NaN gradient there (the
// reference raises LinAlgError out of minimize): the line search backs off from it.
#include <algorithm>
#include "ssmq_weights_host.h"
#include "ssmq_blockla.h"
#include "ssmq_bfgs.h"

namespace ssmq {

constexpr int kMl2PM = SSMQ_MAX_DIM + 1, kMl2Block = 256;

struct Ml2Args {
    int32_t D, N, E, x_per_fit, optimise, maxiter;
    int64_t B;
    double gtol, nu, tp_const;          // nu = 0: GP
    const double *x;                    // [D][N], or [B][D][N] (x_per_fit)
    const double *y;                    // [B][N][E]
    const double *jit;                  // [N][N]
    const double *lp;                   // [B][P]: evaluation points / start points (log-parameters)
    double *fun, *jac, *xout, *hess_inv;  // [B], [B][P], [B][P] (optimise), [B][P][P] (optimise)
    int32_t *status, *nit, *nfev;       // [B]; nit / nfev: optimise only
};

struct Ml2Shared {
    double sil[SSMQ_MAX_DIM], red[(kMl2Block / 64) * kMl2PM], sums[kMl2PM], yda[kFitMaxE], scale[kFitMaxE];
    double f, g[kMl2PM], lp[kMl2PM];
    int flag, done, nfev;
};

// value and gradient at the log-parameters sh.lp -> sh.f, sh.g (every thread may read them after the call); false: K is
// not positive definite (sh.f = NaN, sh.g = NaN).  lds: the dynamic LDS of the launch (see ml2_lds_bytes).
template <bool PACKED>
__device__ bool ml2_eval(const Ml2Args &a, int64_t b, Ml2Shared &sh, double *lds) {
    const int D = a.D, N = a.N, E = a.E, P = D + 1, tid = threadIdx.x;
    const int64_t nn = PACKED ? (int64_t)N * (N + 1) / 2 : (int64_t)N * N;
    double *Km = lds, *Xm = lds + nn, *zs = Xm + nn, *nrm = zs + D * N;
    double *AY = PACKED ? Km : nrm + N;      // packed: A = X Y over the factor, which is no longer needed by then
    const double *x = a.x + (a.x_per_fit ? b * D * N : 0);
    const double *Y = a.y + b * N * E;
    const double alpha = exp(sh.lp[0]);
    const double la = 2.0 * log(alpha);
    if (tid < D) sh.sil[tid] = 1.0 / exp(sh.lp[1 + tid]);
    rbf_stage(sh.sil, x, zs, nrm, D, N);
    // K + jitter, lower triangle (bq/bqkern.py:329-343: exp(2 log alpha - maha / 2), maha as |a|^2 + |b|^2 - 2 a.b).  The
    // reference factors with cho_factor's default lower=False, which reads the upper triangle of K + jitter: entry (i, j),
    // j <= i, takes the jitter's (j, i), so a jitter that is not symmetric (a per-point nugget, a triangle) counts as there.
    for (int idx = tid; idx < N * N; idx += kWgtBlock) {
        const int i = idx / N, j = idx % N;
        if (j > i) continue;
        Km[tri_idx<PACKED>(i, j, N)] = rbf_entry(la, zs, nrm, N, D, i, j) + a.jit[(int64_t)j * N + i];
    }
    bsync();
    if (!chol_factor_tri<PACKED>(Km, N, &sh.flag)) {
        if (tid == 0) {
            sh.f = __builtin_nan("");
            for (int p = 0; p < P; ++p) sh.g[p] = __builtin_nan("");
        }
        bsync();
        return false;
    }
    // half log det: sum log diag L
    {
        double v[1] = {0.0};
        for (int i = tid; i < N; i += kWgtBlock) v[0] += log(Km[tri_idx<PACKED>(i, i, N)]);
        block_sums<1>(v, 1, sh.red, sh.sums);
    }
    const double hld = sh.sums[0];
    chol_inverse_tri<PACKED>(Km, Xm, N);
    // A = X Y (N x E)
    for (int idx = tid; idx < N * E; idx += kWgtBlock) {
        const int i = idx / E, e = idx % E;
        double s = 0.0;
        for (int k = 0; k < N; ++k) s += SSMQ_SYM_LOWER(PACKED, Xm, i, k, N) * Y[k * E + e];
        AY[idx] = s;
    }
    bsync();
    const bool tp = a.nu != 0.0;
    if (tid < E) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += Y[i * E + tid] * AY[i * E + tid];
        sh.yda[tid] = s;
        sh.scale[tid] = tp ? (a.nu + N) / (a.nu + s - 2.0) : 1.0;
    }
    bsync();
    if (tid == 0) {
        double f;
        if (tp) {
            double ls = 0.0;
            for (int e = 0; e < E; ++e) ls += log(1.0 + sh.yda[e] / (a.nu - 2.0));
            f = 0.5 * (a.nu + N) * ls + E * (hld + a.tp_const);
        } else {
            double ya = 0.0;
            for (int e = 0; e < E; ++e) ya += sh.yda[e];
            f = E * hld + 0.5 * (ya + E * N * log(2.0 * M_PI));
        }
        sh.f = f;
    }
    // gradient: 1/2 sum_ij W_ij dK_p(i, j) over the lower triangle (off-diagonal entries twice)
    double acc[kMl2PM];
#pragma unroll
    for (int p = 0; p < kMl2PM; ++p) acc[p] = 0.0;
    const double da = 2.0 / alpha;
    for (int idx = tid; idx < N * N; idx += kWgtBlock) {
        const int i = idx / N, j = idx % N;
        if (j > i) continue;
        double w = E * Xm[tri_idx<PACKED>(i, j, N)];
        for (int e = 0; e < E; ++e) w -= sh.scale[e] * AY[i * E + e] * AY[j * E + e];
        const double c = (i == j ? 1.0 : 2.0) * w * rbf_entry(la, zs, nrm, N, D, i, j);
        acc[0] += c * da;
#pragma unroll
        for (int d = 0; d < SSMQ_MAX_DIM; ++d) {
            if (d < D) {
                const double dz = zs[d * N + i] - zs[d * N + j];
                acc[1 + d] += c * (dz * dz);
            }
        }
    }
    block_sums<kMl2PM>(acc, P, sh.red, sh.sums);
    if (tid < P) sh.g[tid] = 0.5 * sh.sums[tid];
    bsync();
    return true;
}

template <bool PACKED>
__global__ __launch_bounds__(kMl2Block) void k_ml2(const Ml2Args a) {
    extern __shared__ __align__(16) double lds[];
    __shared__ Ml2Shared sh;
    __shared__ __align__(16) char run_bytes[sizeof(ssmq_bfgs::RunT<kMl2PM>)];     // (no constructor runs on __shared__)
    ssmq_bfgs::RunT<kMl2PM> &run = *reinterpret_cast<ssmq_bfgs::RunT<kMl2PM> *>(run_bytes);
    const int64_t b = blockIdx.x;
    const int P = a.D + 1, tid = threadIdx.x;
    if (tid == 0) {
        if (a.optimise) ssmq_bfgs::bfgs_start(run, P, a.lp + b * P);
        sh.nfev = 0;
        sh.done = 0;
    }
    bsync();
    // one call site of the objective for both modes: a fit's fun / jac are bit for bit the evaluation mode's at its x
    while (!sh.done) {
        if (tid < P) sh.lp[tid] = a.optimise ? run.xt[tid] : a.lp[b * P + tid];
        bsync();
        const bool ok = ml2_eval<PACKED>(a, b, sh, lds);
        if (tid == 0) {
            ++sh.nfev;
            if (a.optimise) {
                const double f = ok ? sh.f : __builtin_huge_val();
                ssmq_bfgs::bfgs_advance_jac(run, P, f, sh.g, a.gtol, a.maxiter);
                sh.done = run.phase == ssmq_bfgs::PH_DONE;
            } else {
                sh.done = ok ? 1 : 2;
            }
        }
        bsync();
    }
    if (!a.optimise) {
        if (tid == 0) {
            a.fun[b] = sh.f;
            a.status[b] = sh.done == 1 ? 0 : 1;
        }
        if (tid < P) a.jac[b * P + tid] = sh.g[tid];
        return;
    }
    if (tid < P) {
        a.xout[b * P + tid] = run.x[tid];
        a.jac[b * P + tid] = run.g[tid];
    }
    for (int i = tid; i < P * P; i += kWgtBlock) a.hess_inv[b * P * P + i] = run.H[i];
    if (tid == 0) {
        a.fun[b] = run.old_fval;
        a.status[b] = run.status;
        a.nit[b] = run.k;
        a.nfev[b] = sh.nfev;
    }
}

static size_t ml2_lds_bytes(int D, int N, int E, bool packed) {
    const size_t nn = packed ? (size_t)N * (N + 1) / 2 : (size_t)N * N;
    return sizeof(double) * (2 * nn + (size_t)D * N + N + (packed ? 0 : (size_t)N * E));
}

// the TP's constant N / 2 log((nu - 2) pi) - log Gamma((nu + N) / 2) + log Gamma(nu / 2), formed as the reference forms it:
// the log of Gamma itself (np.log(gamma(.)))
static double ml2_tp_const(double nu, int N) {
    return (N / 2.0) * std::log((nu - 2.0) * M_PI) - std::log(std::tgamma((nu + N) / 2.0)) + std::log(std::tgamma(nu / 2.0));
}

// Host arrays in and out; synchronous.  Returns the first row whose K is not positive definite + 1 (evaluation), else 0.
static int ml2_impl(Ml2Args a, const double *x, const double *y, const double *jit, const double *lp, double *fun, double *jac,
                    double *xout, double *hess_inv, int32_t *status, int32_t *nit, int32_t *nfev) {
    const int D = a.D, N = a.N, E = a.E, P = D + 1;
    const int64_t B = a.B;
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    const bool packed = N > 64;
    const size_t lds = ml2_lds_bytes(D, N, E, packed);
    static thread_local unsigned attr_epoch = 0;
    const size_t cap = 160 * 1024 - 8192;            // static __shared__ of k_ml2: Ml2Shared + the BFGS state, < 8 KiB
    if ((rc = set_max_dynamic_lds(attr_epoch, {(const void *)k_ml2<true>, (const void *)k_ml2<false>}, cap))) return rc;
    const size_t nx = (size_t)D * N * (a.x_per_fit ? B : 1), ny = (size_t)B * N * E, nn = (size_t)N * N, np = (size_t)B * P;
    DBuf dx, dy, dj, dl, dfun, djac, dxo, dh, dst, dit, dfe;
    if ((rc = dx.alloc(sizeof(double) * nx)) || (rc = dy.alloc(sizeof(double) * ny)) || (rc = dj.alloc(sizeof(double) * nn)) ||
        (rc = dl.alloc(sizeof(double) * np)) || (rc = dfun.alloc(sizeof(double) * B)) || (rc = djac.alloc(sizeof(double) * np)) ||
        (rc = dst.alloc(sizeof(int32_t) * B)))
        return rc;
    if (a.optimise && ((rc = dxo.alloc(sizeof(double) * np)) || (rc = dh.alloc(sizeof(double) * np * P)) ||
                       (rc = dit.alloc(sizeof(int32_t) * B)) || (rc = dfe.alloc(sizeof(int32_t) * B))))
        return rc;
    SSMQ_HIP(hipMemcpyAsync(dx.p, x, sizeof(double) * nx, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dy.p, y, sizeof(double) * ny, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dj.p, jit, sizeof(double) * nn, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dl.p, lp, sizeof(double) * np, hipMemcpyHostToDevice, s));
    a.x = dx.d(); a.y = dy.d(); a.jit = dj.d(); a.lp = dl.d();
    a.fun = dfun.d(); a.jac = djac.d(); a.status = (int32_t *)dst.p;
    a.xout = a.optimise ? dxo.d() : nullptr;
    a.hess_inv = a.optimise ? dh.d() : nullptr;
    a.nit = a.optimise ? (int32_t *)dit.p : nullptr;
    a.nfev = a.optimise ? (int32_t *)dfe.p : nullptr;
    if (packed) hipLaunchKernelGGL(k_ml2<true>, dim3((unsigned)B), dim3(kMl2Block), lds, s, a);
    else hipLaunchKernelGGL(k_ml2<false>, dim3((unsigned)B), dim3(kMl2Block), lds, s, a);
    if ((rc = hip_fail(hipGetLastError(), "k_ml2"))) return rc;
    SSMQ_HIP(hipMemcpyAsync(fun, dfun.p, sizeof(double) * B, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipMemcpyAsync(jac, djac.p, sizeof(double) * np, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipMemcpyAsync(status, dst.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
    if (a.optimise) {
        SSMQ_HIP(hipMemcpyAsync(xout, dxo.p, sizeof(double) * np, hipMemcpyDeviceToHost, s));
        if (hess_inv) SSMQ_HIP(hipMemcpyAsync(hess_inv, dh.p, sizeof(double) * np * P, hipMemcpyDeviceToHost, s));
        if (nit) SSMQ_HIP(hipMemcpyAsync(nit, dit.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
        if (nfev) SSMQ_HIP(hipMemcpyAsync(nfev, dfe.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
    }
    SSMQ_HIP(hipStreamSynchronize(s));
    if (a.optimise) return SSMQ_OK;
    for (int64_t b = 0; b < B; ++b)
        if (status[b]) return (int)std::min<int64_t>(b + 1, INT32_MAX);
    return SSMQ_OK;
}

}  // namespace ssmq

extern "C" int ssmq_gp_nlml_batch(int D, int N, int E, int64_t B, const double *x_obs, int x_per_fit, const double *fcn_obs,
                                  const double *jitter, double nu, const double *log_par, double *nlml, double *grad,
                                  int32_t *status) {
    using namespace ssmq;
    int rc = fit_check("gp_nlml_batch", D, N, E, B, nu, B == 0 || (x_obs && fcn_obs && jitter && log_par));
    if (rc) return rc;
    if (B > 0 && (!nlml || !grad || !status)) {
        set_error("gp_nlml_batch: bad argument");
        return SSMQ_E_ARG;
    }
    Ml2Args a{};
    a.D = D; a.N = N; a.E = E; a.B = B; a.x_per_fit = x_per_fit ? 1 : 0; a.optimise = 0;
    a.nu = nu; a.tp_const = nu != 0.0 ? ml2_tp_const(nu, N) : 0.0;
    return ml2_impl(a, x_obs, fcn_obs, jitter, log_par, nlml, grad, nullptr, nullptr, status, nullptr, nullptr);
}

extern "C" int ssmq_gp_ml2_batch(int D, int N, int E, int64_t B, const double *x_obs, int x_per_fit, const double *fcn_obs,
                                 const double *jitter, double nu, double gtol, int maxiter, const double *log_par_0,
                                 double *x, double *fun, double *jac, double *hess_inv, int32_t *status, int32_t *nit,
                                 int32_t *nfev) {
    using namespace ssmq;
    int rc = fit_check("gp_ml2_batch", D, N, E, B, nu, B == 0 || (x_obs && fcn_obs && jitter && log_par_0));
    if (rc) return rc;
    if (B > 0 && (!x || !fun || !jac || !status)) {
        set_error("gp_ml2_batch: bad argument");
        return SSMQ_E_ARG;
    }
    Ml2Args a{};
    a.D = D; a.N = N; a.E = E; a.B = B; a.x_per_fit = x_per_fit ? 1 : 0; a.optimise = 1;
    a.gtol = gtol; a.maxiter = maxiter < 0 ? 200 * (D + 1) : maxiter;
    a.nu = nu; a.tp_const = nu != 0.0 ? ml2_tp_const(nu, N) : 0.0;
    return ml2_impl(a, x_obs, fcn_obs, jitter, log_par_0, fun, jac, x, hess_inv, status, nit, nfev);
}
