// Gaussian-process quadrature with derivative observations at the sigma points (GPQ+D, SSMQ_FORM_GPQD; the reference's
// research/gpqd/gpqd_base.py: GaussianProcessDerTransform): the GP is conditioned on the integrand's values at all N sigma points
// and on its Jacobians at those of them that `der_mask` names.  With L = chol(cov) (lower), x_n = mean + L xi_n:
//
//   obs[e] = [f_e(x_0) .. f_e(x_N-1) | (J(x_n) L)[e, :] for every n with a derivative]         (the GP lives in the unit coordinates)
//   mean_f = obs wm,  cov_f = obs Wc obs' - mean_f mean_f' + model_var I [+ cov_add],  cov_fx = (obs Wcc') L'        (E, D)
//
// - BQTransform.apply of bq/bqmtran.py on the (E, M) observation matrix.  The kernels work on the FULL layout of MX = NMAX (1 + D)
// slots, NMAX = 2 D + 1: value of point n in slot n, derivative k of point n in slot NMAX + n D + k.  The handle expands the
// weights into that layout (gpqd_layout; the slots of absent points and of points without a derivative carry zero weights) and the
// kernels write zeros there, so neither the point count nor the subset changes an index: every register index is static.
//
// k_apply_gpqd<F, D, E, DIN>     one item per lane, obs in registers (E MX doubles): the route for D <= 2.
// k_apply_gpqd_lds<F, D, E, DIN> obs in LDS, G = 64 / IPW lanes per item, IPW items per 64-thread workgroup (16, or 8 where 16 would
//                                need more than 64 KB): the lanes of an item share its points, then the rows of Wc; partial sums meet
//                                in a butterfly over the G lanes.  The route for D >= 3.
// F < 0: a built-in model, reached through the run-time switch of gpqd_eval_builtin / jac_integrand, Jacobian placed as
// jac_front_builtin places it (ssmq_jacobian_kernel.h); F >= 0: the user functor Fn<F> with HAS_JAC, compiled at run time
// (ssmq_rtc.hip), Jacobian in the DIN leading columns.  The constants are wave-uniform in k_apply_gpqd (constant address space:
// scalar loads); in the LDS kernel the lanes of an item read different rows of Wc, which stay in L2 (66 KB at most, one block for
// the whole batch).  An item's result depends on its own inputs alone: no sum crosses items, the split over the G lanes is fixed.
// A pivot that is not positive: status 1, NaN outputs.  This header is also compiled by hiprtc: no host code.
#pragma once
#include "ssmq_device.h"
#include "ssmq_jacobian_kernel.h"

namespace ssmq {

struct GpqdArgs : LinArgs {
    const double *consts;        // gpqd_layout block
    int32_t N;                   // points in use, 2 .. NMAX
    uint32_t der_mask;           // bit n: point n carries a derivative observation
};

// offsets (doubles) into the constant block: xi [NMAX][D] | wm [MX] | Wcc [D][MX] | Wc [MX][MX] | model_var
struct GpqdLayout {
    int nmax, mx, xi, wm, Wcc, Wc, emv, total;
};
__host__ __device__ constexpr inline GpqdLayout gpqd_layout(int D) {
    GpqdLayout c{};
    c.nmax = 2 * D + 1;
    c.mx = c.nmax * (1 + D);
    c.xi = 0;
    c.wm = c.nmax * D;
    c.Wcc = c.wm + c.mx;
    c.Wc = c.Wcc + D * c.mx;
    c.emv = c.Wc + c.mx * c.mx;
    c.total = c.emv + 1;
    return c;
}
constexpr int kGpqdRegMaxD = 2;      // D <= 2: k_apply_gpqd, beyond: k_apply_gpqd_lds
constexpr int kGpqdLdsBlock = 64;
__host__ __device__ constexpr inline int gpqd_lds_items(int D, int E) {
    return E * gpqd_layout(D).mx * 16 * 8 <= 65536 ? 16 : 8;
}

// the built-in models that have a Jacobian and additive noise (ssmq_device.h: jac_integrand); a tracking model's case is compiled
// wherever its Jacobian's is (jacobian_fits: the launcher refuses the other pairs), so no shape gets a Jacobian without values
template <int D, int E>
__device__ __forceinline__ void gpqd_eval_builtin(int id, const double *xs, double t, const FPar &fp, double *o) {
#define SSMQ_CASE_IF(F, COND)                       \
    case F:                                         \
        if constexpr (COND) {                       \
            Fn<F> fn;                               \
            fn.init(t, fp);                         \
            fn.template eval<SSMQ_MAX_FIDX>(xs, o); \
        }                                           \
        break;
#define SSMQ_CASE(F) SSMQ_CASE_IF(F, true)
    switch (id) {
        SSMQ_CASE(SSMQ_F_UNGM_DYN)
        SSMQ_CASE(SSMQ_F_UNGM_MEAS)
        SSMQ_CASE(SSMQ_F_PENDULUM_DYN)
        SSMQ_CASE(SSMQ_F_PENDULUM_MEAS)
        SSMQ_CASE(SSMQ_F_CV_DYN)
        SSMQ_CASE_IF(SSMQ_F_CT_DYN, D >= 5 && E >= 5)
        SSMQ_CASE_IF(SSMQ_F_RADAR2D_MEAS, D >= 2 && E >= 2)
        SSMQ_CASE_IF(SSMQ_F_BEARING_MEAS, D >= 2)
        default: break;
    }
#undef SSMQ_CASE
#undef SSMQ_CASE_IF
}

// f(x) in o[E] and, if der, J(x) L in JL[E * D] (else untouched) at the point x[D]; L packed lower
template <int F, int D, int E, int DIN>
__device__ __forceinline__ void gpqd_point(const GpqdArgs &a, const double *x, const double *L, const double t, const bool der,
                                           double *o, double *JL) {
    double J[E * D];
    if constexpr (F >= 0) {
        static_assert(DIN >= 1 && DIN <= D, "the integrand reads the leading DIN <= D state entries");
        Fn<F> fn;
        fn.init(t, a.fp);
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = 0.0;
        fn.template eval<E>(x, o);
        if (der) {
#pragma unroll
            for (int i = 0; i < E * D; ++i) J[i] = 0.0;
            fn.jac(x, J, D);
        }
    } else {
        double xs[kMaxIntegrandIn], oo[SSMQ_MAX_DIM], Js[E * D];
#pragma unroll
        for (int k = 0; k < kMaxIntegrandIn; ++k) {
            const int src = a.fp.n_idx > 0 ? (k < a.fp.n_idx ? a.fp.idx[k] : 0) : (k < D ? k : 0);
            double v = x[0];                        // static register indices: a select chain over the D candidates
#pragma unroll
            for (int q = 1; q < D; ++q) v = (src == q) ? x[q] : v;
            xs[k] = k < D ? v : 0.0;
        }
#pragma unroll
        for (int e = 0; e < SSMQ_MAX_DIM; ++e) oo[e] = 0.0;
        gpqd_eval_builtin<D, E>(a.fid, xs, t, a.fp, oo);
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = oo[e];
        if (der) {
#pragma unroll
            for (int i = 0; i < E * D; ++i) Js[i] = 0.0;
            jac_integrand<E, D, false>(a.fid, xs, t, a.fp, Js, D, E);
            // placement into the columns of the full state, as jac_front_builtin (state index, broadcast of a one-column Jacobian)
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    double v = 0.0;
                    if (a.fp.n_idx > 0) {
#pragma unroll
                        for (int k = 0; k < D; ++k) v = (k < a.din && a.fp.idx[k] == d) ? Js[e * D + k] : v;
                    } else if (a.bcast) {
                        v = Js[e * D];
                    } else {
                        v = d < a.din ? Js[e * D + d] : 0.0;
                    }
                    J[e * D + d] = v;
                }
        }
    }
    if (der) {
        constexpr int K = F >= 0 ? DIN : D;      // only the K leading columns of a user Jacobian can be non-zero
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double s = 0.0;
#pragma unroll
                for (int r = k; r < K; ++r) s += J[e * D + r] * L[SSMQ_PK(r, k)];
                JL[e * D + k] = s;
            }
    }
}

// the outputs of one item from its sums: mf = obs wm, qf = obs Wc obs' (E x E), c1 = obs Wcc' (E x D)
template <int D, int E>
__device__ __forceinline__ void gpqd_store(const GpqdArgs &a, const int64_t b, const bool ok, const double *L, const double *mf,
                                           const double *qf, const double *c1, const double emv) {
    const int64_t ld = a.ld;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int e = 0; e < E; ++e) a.mean_f[e * ld + b] = ok ? mf[e] : nan;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            double s = qf[e * E + e2] - mf[e] * mf[e2] + (e == e2 ? emv : 0.0);
            s *= a.cov_scale;
            if (a.cov_add) s += a.cov_add[e * E + e2];
            a.cov_f[(int64_t)(e * E + e2) * ld + b] = ok ? s : nan;
        }
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double s = 0.0;
#pragma unroll
            for (int d = 0; d <= k; ++d) s += c1[e * D + d] * L[SSMQ_PK(k, d)];
            a.cov_fx[(int64_t)(e * D + k) * ld + b] = ok ? s * a.ccov_scale : nan;
        }
    a.status[b] = ok ? 0 : 1;
}

template <int F, int D, int E, int DIN>
__global__ __launch_bounds__(256) void k_apply_gpqd(const GpqdArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    constexpr GpqdLayout cl = gpqd_layout(D);
    constexpr int NMAX = cl.nmax, MX = cl.mx;
    const int64_t ld = a.ld;
    const cdouble_p c = (cdouble_p)a.consts;
    double m[D], L[D * (D + 1) / 2], obs[E * MX];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = a.mean[d * ld + b];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[SSMQ_PK(i, j)] = a.cov[(int64_t)(i * D + j) * ld + b];
    const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
    const bool ok = chol_packed<D>(L);
#pragma unroll
    for (int i = 0; i < E * MX; ++i) obs[i] = 0.0;
#pragma unroll
    for (int n = 0; n < NMAX; ++n) {
        if (n < a.N) {                                   // (wave-uniform)
            const bool der = (a.der_mask >> n) & 1u;
            double x[D], o[E], JL[E * D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k <= d; ++k) s += L[SSMQ_PK(d, k)] * c[cl.xi + n * D + k];
                x[d] = m[d] + s;
            }
#pragma unroll
            for (int i = 0; i < E * D; ++i) JL[i] = 0.0;
            gpqd_point<F, D, E, DIN>(a, x, L, t, der, o, JL);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                obs[e * MX + n] = o[e];
#pragma unroll
                for (int k = 0; k < D; ++k) obs[e * MX + NMAX + n * D + k] = der ? JL[e * D + k] : 0.0;
            }
        }
    }
    double mf[E], qf[E * E], c1[E * D];
#pragma unroll
    for (int e = 0; e < E; ++e) mf[e] = 0.0;
#pragma unroll
    for (int i = 0; i < E * E; ++i) qf[i] = 0.0;
#pragma unroll
    for (int i = 0; i < E * D; ++i) c1[i] = 0.0;
#pragma unroll
    for (int i = 0; i < MX; ++i) {
        const double wmi = c[cl.wm + i];
        double tq[E];
#pragma unroll
        for (int e = 0; e < E; ++e) tq[e] = 0.0;
#pragma unroll
        for (int j = 0; j < MX; ++j) {
            const double w = c[cl.Wc + i * MX + j];
#pragma unroll
            for (int e = 0; e < E; ++e) tq[e] += w * obs[e * MX + j];
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            mf[e] += wmi * obs[e * MX + i];
#pragma unroll
            for (int e2 = 0; e2 < E; ++e2) qf[e * E + e2] += obs[e * MX + i] * tq[e2];
#pragma unroll
            for (int d = 0; d < D; ++d) c1[e * D + d] += c[cl.Wcc + d * MX + i] * obs[e * MX + i];
        }
    }
    gpqd_store<D, E>(a, b, ok, L, mf, qf, c1, c[cl.emv]);
}

template <int F, int D, int E, int DIN>
__global__ __launch_bounds__(kGpqdLdsBlock) void k_apply_gpqd_lds(const GpqdArgs a) {
    constexpr GpqdLayout cl = gpqd_layout(D);
    constexpr int NMAX = cl.nmax, MX = cl.mx, IPW = gpqd_lds_items(D, E), G = kGpqdLdsBlock / IPW;
    __shared__ double s_obs[E * MX * IPW];               // slot i of output e of item `it` at (e MX + i) IPW + it
    const int it = threadIdx.x / G, g = threadIdx.x % G;
    const int64_t b0 = (int64_t)blockIdx.x * IPW + it;
    const bool active = b0 < a.B;
    const int64_t b = active ? b0 : a.B - 1;             // (an idle item repeats the last one and stores nothing)
    const int64_t ld = a.ld;
    const double *c = a.consts;
    double m[D], L[D * (D + 1) / 2];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = a.mean[d * ld + b];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[SSMQ_PK(i, j)] = a.cov[(int64_t)(i * D + j) * ld + b];
    const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
    const bool ok = chol_packed<D>(L);
    // the points of this lane: n = g, g + G, ..; every slot of the full layout is written, zeros where there is no observation
#pragma unroll 1
    for (int n = g; n < NMAX; n += G) {
        const bool have = n < a.N, der = have && ((a.der_mask >> n) & 1u);
        double x[D], o[E], JL[E * D];
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = 0.0;
#pragma unroll
        for (int i = 0; i < E * D; ++i) JL[i] = 0.0;
        if (have) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k <= d; ++k) s += L[SSMQ_PK(d, k)] * c[cl.xi + n * D + k];
                x[d] = m[d] + s;
            }
            gpqd_point<F, D, E, DIN>(a, x, L, t, der, o, JL);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            s_obs[(e * MX + n) * IPW + it] = o[e];
#pragma unroll
            for (int k = 0; k < D; ++k) s_obs[(e * MX + NMAX + n * D + k) * IPW + it] = der ? JL[e * D + k] : 0.0;
        }
    }
    __syncthreads();
    double mf[E], qf[E * E], c1[E * D];
#pragma unroll
    for (int e = 0; e < E; ++e) mf[e] = 0.0;
#pragma unroll
    for (int i = 0; i < E * E; ++i) qf[i] = 0.0;
#pragma unroll
    for (int i = 0; i < E * D; ++i) c1[i] = 0.0;
    // the rows of this lane: i = g, g + G, ..; a row without an observation has zero weights and is left out
#pragma unroll 1
    for (int i = g; i < MX; i += G) {
        const int n = i < NMAX ? i : (i - NMAX) / D;
        if (n >= a.N || (i >= NMAX && !((a.der_mask >> n) & 1u))) continue;
        double oi[E], tq[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            oi[e] = s_obs[(e * MX + i) * IPW + it];
            tq[e] = 0.0;
        }
        const double *wrow = c + cl.Wc + i * MX;
#pragma unroll 1
        for (int j = 0; j < MX; ++j) {
            const double w = wrow[j];
#pragma unroll
            for (int e = 0; e < E; ++e) tq[e] += w * s_obs[(e * MX + j) * IPW + it];
        }
        const double wmi = c[cl.wm + i];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            mf[e] += wmi * oi[e];
#pragma unroll
            for (int e2 = 0; e2 < E; ++e2) qf[e * E + e2] += oi[e] * tq[e2];
#pragma unroll
            for (int d = 0; d < D; ++d) c1[e * D + d] += c[cl.Wcc + d * MX + i] * oi[e];
        }
    }
    // the G partial sums of an item sit in adjacent lanes: butterfly, every lane ends with the same bits
#pragma unroll
    for (int s = 1; s < G; s <<= 1) {
#pragma unroll
        for (int e = 0; e < E; ++e) mf[e] += __shfl_xor(mf[e], s, 64);
#pragma unroll
        for (int i = 0; i < E * E; ++i) qf[i] += __shfl_xor(qf[i], s, 64);
#pragma unroll
        for (int i = 0; i < E * D; ++i) c1[i] += __shfl_xor(c1[i], s, 64);
    }
    if (active && g == 0) gpqd_store<D, E>(a, b, ok, L, mf, qf, c1, c[cl.emv]);
}

}  // namespace ssmq
