// Taylor-GPQD moment transform (mtran.py:668-701: TaylorGPQDTransform - the transform of ExtendedKalmanGPQD, ssinf.py:1302-1319):
// the linearisation of the extended Kalman filter read as single-point Gaussian-process quadrature with derivative observations
// and an RBF kernel (scale alpha, length-scales ell, Lam = diag(ell^2)).  With f = f(mean), J = f(mean, dx=True), P = cov:
//   wm = det(Lam^-1 P + I)^-1/2,  wc = det(2 Lam^-1 P + I)^-1/2,  Wc = Lam/2 (Lam/2 + P)^-1 P,
//   model_var = alpha^2 - alpha^2 wc (1 + tr(Wc Lam^-1)),  integ_var = alpha^2 wc - wm^2,
//   mean_f = wm f,  cov_f = wc (f f' + J Wc J') - mean_f mean_f' + model_var (the scalar on EVERY entry, mtran.py:699),
//   cov_fx = J P (Lam + P)^-1 Lam   - (E, D), the convention of include/ssmq.h; the reference returns the transpose.
// One trajectory per lane, element planes in and out, time argument, state index and broadcast placement of the Jacobian and the
// cov_add / cov_scale / ccov_scale hooks exactly as k_linearize (ssmq_linear.hip): the same 8 (D + D^2 + E + E^2 + E D) bytes per
// trajectory.  On top of its arithmetic: the Cholesky factors of Lam + P and Lam / 2 + P, whose pivots give both determinants
// (det(Lam^-1 P + I) = det(Lam + P) / det Lam), E triangular solve pairs for the cross-covariance and D for Wc - O(D^3) operations
// on registers.  Wc and the damping are formed as Lam (..)^-1 P, never as P - P (..)^-1 P or Lam - Lam (..)^-1 Lam: with long
// length-scales those differences cancel.  The symmetric P is read once, through its lower triangle.
// A pivot that is not positive (P not positive semi-definite) gives status 1 and NaN outputs.
#include "ssmq_device.h"
#include "ssmq_host.h"
#include "ssmq_math.h"
#include "ssmq_taylor_gpqd_kernel.h"   // TaylorGpqdArgs, chol_lower, chol_solve_vec; the user models' kernel k_taylor_gpqd_fn<>

// (the run-time-size instantiation <0, 0> cannot unroll the triangular loops of the factorisation: no warning for that)
#pragma clang diagnostic ignored "-Wpass-failed"

namespace ssmq {

// DT, ET > 0: the transform's dimensions at compile time (everything in registers: the shapes of the models that have a
// Jacobian); 0: run-time sizes, private arrays of the maximal size (scratch memory - the fallback, as k_linearize<0, 0>)
template <int DT, int ET>
__global__ __launch_bounds__(256) void k_taylor_gpqd(const TaylorGpqdArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    constexpr int DM = DT > 0 ? DT : SSMQ_MAX_DIM, EM = ET > 0 ? ET : SSMQ_MAX_DIM;
    const int D = DT > 0 ? DT : a.D, E = ET > 0 ? ET : a.E, din = a.din;
    const int64_t ld = a.ld;
    double x[DM], xs[kMaxIntegrandIn], o[SSMQ_MAX_DIM];
    double Js[EM * DM], J[EM * DM], C[EM * DM];
    double P[DM * DM], L[DM * DM], X[DM * DM], lam[DM], ri[DM], col[DM];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = a.mean[d * ld + b];
    // the lower triangle of P, mirrored
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double v = a.cov[(int64_t)(i * D + j) * ld + b];
            P[i * D + j] = v;
            P[j * D + i] = v;
        }
#pragma unroll
    for (int k = 0; k < kMaxIntegrandIn; ++k) {
        if (DT > 0) {                    // static register indices: a select chain over the DT candidates
            const int src = a.fp.n_idx > 0 ? (k < a.fp.n_idx ? a.fp.idx[k] : 0) : (k < D ? k : 0);
            double v = x[0];
#pragma unroll
            for (int q = 1; q < DM; ++q) v = (src == q) ? x[q] : v;
            xs[k] = k < DM ? v : 0.0;
        } else {
            const int src = a.fp.n_idx > 0 ? (k < a.fp.n_idx ? a.fp.idx[k] : 0) : (k < D ? k : 0);
            xs[k] = x[src];
        }
    }
    const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
    for (int e = 0; e < SSMQ_MAX_DIM; ++e) o[e] = 0.0;
    eval_integrand(a.fid, xs, t, a.fp, o);
    // the model's Jacobian with the compile-time pitch DM, then placed into the columns of the full state - every index static at the
    // compile-time shapes (a pitch of din, known only at run time, would put Js into scratch memory)
#pragma unroll
    for (int i = 0; i < EM * DM; ++i) Js[i] = 0.0;
    jac_integrand(a.fid, xs, t, a.fp, Js, DM);
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double v = 0.0;
            if (a.fp.n_idx > 0) {
#pragma unroll
                for (int k = 0; k < DM; ++k) v = (k < din && a.fp.idx[k] == d) ? Js[e * DM + k] : v;
            } else if (a.bcast) {
                v = Js[e * DM];
            } else {
                v = d < din ? Js[e * DM + d] : 0.0;
            }
            J[e * D + d] = v;
        }
    bool ok = true;
    double ell_prod = 1.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        lam[d] = a.ell[d] * a.ell[d];
        ell_prod *= a.ell[d];
    }
    // C = J P (E x D)
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += J[e * D + k] * P[k * D + d];
            C[e * D + d] = s;
        }
    // Lam + P = L L':  wm = sqrt(det Lam / det(Lam + P)),  cov_fx = C (Lam + P)^-1 Lam  (row e: one solve with the symmetric matrix)
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i * D + j] = P[i * D + j] + (i == j ? lam[i] : 0.0);
    const double wm = div_nr(ell_prod, chol_lower(L, ri, D, ok));
#pragma unroll
    for (int e = 0; e < E; ++e) {
#pragma unroll
        for (int d = 0; d < D; ++d) col[d] = C[e * D + d];
        chol_solve_vec(L, ri, col, D);
#pragma unroll
        for (int d = 0; d < D; ++d) a.cov_fx[(int64_t)(e * D + d) * ld + b] = col[d] * lam[d] * a.ccov_scale;      // (NaN below if a pivot fails)
    }
    // Lam / 2 + P = L L':  wc = sqrt(det(Lam / 2) / det(Lam / 2 + P)),  X = (Lam / 2 + P)^-1 P column by column,  Wc = Lam / 2 X
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i * D + j] = P[i * D + j] + (i == j ? 0.5 * lam[i] : 0.0);
    double half_prod = ell_prod;
#pragma unroll
    for (int d = 0; d < D; ++d) half_prod *= 0.70710678118654752440;
    const double wc = div_nr(half_prod, chol_lower(L, ri, D, ok));
    double tr = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
#pragma unroll
        for (int d = 0; d < D; ++d) col[d] = P[d * D + c];
        chol_solve_vec(L, ri, col, D);
        tr += 0.5 * col[c];                          // tr(Wc Lam^-1) = tr(X) / 2
#pragma unroll
        for (int d = 0; d < D; ++d) X[d * D + c] = 0.5 * lam[d] * col[d];
    }
    const double a2 = a.alpha * a.alpha;
    const double model_var = a2 - a2 * wc * (1.0 + tr), integ_var = a2 * wc - wm * wm;
    const double nan = __builtin_nan("");
    // C <- J Wc (E x D)
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += J[e * D + k] * X[k * D + d];
            C[e * D + d] = s;
        }
#pragma unroll
    for (int e = 0; e < E; ++e) a.mean_f[e * ld + b] = ok ? wm * o[e] : nan;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            double s = o[e] * o[e2];
#pragma unroll
            for (int d = 0; d < D; ++d) s += C[e * D + d] * J[e2 * D + d];
            s = wc * s - (wm * o[e]) * (wm * o[e2]) + model_var;
            s *= a.cov_scale;
            if (a.cov_add) s += a.cov_add[e * E + e2];
            a.cov_f[(int64_t)(e * E + e2) * ld + b] = ok ? s : nan;
        }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < E * D; ++i) a.cov_fx[(int64_t)i * ld + b] = nan;
    }
    if (a.model_var) a.model_var[b] = ok ? model_var : nan;
    if (a.integ_var) a.integ_var[b] = ok ? integ_var : nan;
    a.status[b] = ok ? 0 : 1;
}

int refuse_taylor_gpqd(const char *what) {
    set_error(std::string("the Taylor-GPQD transform (k_taylor_gpqd) has neither points nor weights: not implemented for ") + what);
    return SSMQ_E_UNSUPPORTED;
}

// D, E: the transform's; din: the integrand's own input count (ssmq_api_transform.hip: check_integrand, FInfo); alpha, ell and the
// optional variance planes come from the handle
int launch_taylor_gpqd(const ssmq_transform *h, int din, const ssmq_integrand *f, const FPar &fp, int64_t B, int64_t ld,
                       const double *d_mean, const double *d_cov, const double *d_time, int time_stride, double *d_mean_f,
                       double *d_cov_f, double *d_cov_fx, int32_t *d_status, const double *d_cov_add, double cov_scale,
                       double ccov_scale, hipStream_t s, const char **name, bool dry_run) {
    const int D = h->D, E = h->E;
    const bool user = is_user_integrand(f);      // its kernel is compiled for it (rtc_launch_taylor_gpqd makes the checks of that route)
    if (!user && !integrand_has_jacobian(f->id)) {
        set_error("Taylor-GPQD: this model has no Jacobian (its dyn_fcn_dx / meas_fcn_dx returns None in the reference too)");
        return SSMQ_E_UNSUPPORTED;
    }
    if (!user && f->n_idx == 0 && din != D && din != 1) {
        set_error("Taylor-GPQD: a Jacobian of 1 < din < D columns without a state index has no placement (numpy raises there)");
        return SSMQ_E_UNSUPPORTED;
    }
    TaylorGpqdArgs a;
    a.D = D; a.E = E; a.din = din; a.fid = f->id; a.time_stride = time_stride; a.bcast = (f->n_idx == 0 && din == 1 && D > 1) ? 1 : 0;
    a.mean = d_mean; a.cov = d_cov; a.time = d_time; a.cov_add = d_cov_add;
    a.mean_f = d_mean_f; a.cov_f = d_cov_f; a.cov_fx = d_cov_fx; a.model_var = h->d_tg_mvar; a.integ_var = h->d_tg_ivar;
    a.status = d_status; a.B = B; a.ld = ld;
    a.cov_scale = cov_scale; a.ccov_scale = ccov_scale; a.alpha = h->tg_alpha;
    for (int d = 0; d < SSMQ_MAX_DIM; ++d) a.ell[d] = d < D ? h->tg_ell[d] : 1.0;
    a.fp = fp;
    if (user) return rtc_launch_taylor_gpqd(f, a, s, name, dry_run);
    if (name) *name = "k_taylor_gpqd";
    if (dry_run) return SSMQ_OK;
    const dim3 grid((unsigned)((B + 255) / 256)), block(256);
    const bool generic = ssmq::sw("SSMQ_TAYLOR_GPQD_GENERIC") != nullptr;      // the run-time-size body for every shape (tests)
    if (generic) hipLaunchKernelGGL((k_taylor_gpqd<0, 0>), grid, block, 0, s, a);
    else if (D == 1 && E == 1) hipLaunchKernelGGL((k_taylor_gpqd<1, 1>), grid, block, 0, s, a);
    else if (D == 2 && E == 1) hipLaunchKernelGGL((k_taylor_gpqd<2, 1>), grid, block, 0, s, a);
    else if (D == 2 && E == 2) hipLaunchKernelGGL((k_taylor_gpqd<2, 2>), grid, block, 0, s, a);
    else if (D == 4 && E == 4) hipLaunchKernelGGL((k_taylor_gpqd<4, 4>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_taylor_gpqd<0, 0>), grid, block, 0, s, a);
    return hip_fail(hipGetLastError(), "k_taylor_gpqd");
}

}  // namespace ssmq
