// The linearisation transform's argument block (both routes) and its kernel for a user model (ssmq_rtc.hip instantiates it at run
// time).  The built-in models keep k_linearize<DT, ET> of ssmq_linear.hip, which reaches the model through the run-time switches
// eval_integrand / jac_integrand and has register-resident bodies for four (D, E) pairs only; a user model's shape is known when
// its kernel is compiled, so every shape of the run-time route gets a register-resident body.
#pragma once
#include "ssmq_device.h"

namespace ssmq {

struct LinArgs {
    int32_t D, E, din, fid, time_stride, bcast;      // bcast: no state index and din == 1 < D
    const double *mean, *cov, *time, *cov_add;       // planes [D][ld], [D*D][ld]; time [B] or [1]; cov_add [E*E] or null
    double *mean_f, *cov_f, *cov_fx;                 // planes [E][ld], [E*E][ld], [E*D][ld]
    int32_t *status;
    int64_t B, ld;
    double cov_scale, ccov_scale;
    FPar fp;
};

// mean_f = f(mean), cov_fx = J cov, cov_f = cov_fx J' for the user functor Fn<F> (HAS_JAC): one trajectory per lane, the planes,
// the time argument and the cov_add / cov_scale / ccov_scale hooks of k_linearize.  Every dimension is a template argument: all
// loops unroll, every array index is static, nothing is addressed through memory.  The model reads the DIN leading state entries
// and its dout x DIN Jacobian lands in the DIN leading columns of the E x D matrix (pitch D); the columns behind them stay zero
// and their terms are left out of both products - they would add 0 * cov.  Sums run in the order of k_linearize.
template <int F, int D, int E, int DIN>
__global__ __launch_bounds__(256) void k_linearize_fn(const LinArgs a) {
    static_assert(Fn<F>::HAS_JAC, "k_linearize_fn: the integrand has no Jacobian");
    static_assert(DIN >= 1 && DIN <= D, "k_linearize_fn: the integrand reads the leading DIN <= D state entries");
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    const int64_t ld = a.ld;
    double x[D], o[E], J[E * D], C[E * D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = a.mean[d * ld + b];
    const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
    Fn<F> fn;
    fn.init(t, a.fp);
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = 0.0;
    fn.template eval<E>(x, o);
#pragma unroll
    for (int i = 0; i < E * D; ++i) J[i] = 0.0;
    fn.jac(x, J, D);
    // cov_fx = J cov (E x D): rows k < DIN of cov, each read once
#pragma unroll
    for (int i = 0; i < E * D; ++i) C[i] = 0.0;
#pragma unroll
    for (int k = 0; k < DIN; ++k)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double c = a.cov[(int64_t)(k * D + d) * ld + b];
#pragma unroll
            for (int e = 0; e < E; ++e) C[e * D + d] += J[e * D + k] * c;
        }
#pragma unroll
    for (int e = 0; e < E; ++e) a.mean_f[e * ld + b] = o[e];
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            double s = 0.0;
#pragma unroll
            for (int d = 0; d < DIN; ++d) s += C[e * D + d] * J[e2 * D + d];
            s *= a.cov_scale;
            if (a.cov_add) s += a.cov_add[e * E + e2];
            a.cov_f[(int64_t)(e * E + e2) * ld + b] = s;
        }
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) a.cov_fx[(int64_t)(e * D + d) * ld + b] = C[e * D + d] * a.ccov_scale;
    a.status[b] = 0;
}

}  // namespace ssmq
