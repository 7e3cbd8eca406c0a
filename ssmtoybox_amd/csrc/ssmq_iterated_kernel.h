// Iterated posterior linearisation update (IPLF; with the linearisation transform the iterated EKF): the measurement update of an
// additive-noise Gaussian filter repeated J times per step, each time with the measurement moments taken around the CURRENT
// posterior (m_i, P_i) instead of the prior (m-, P-):
//     y^, S_y, C = tf_obs(m_i, P_i)              A = C P_i^-1     b = y^ - A m_i     Omega = S_y - A P_i A'
//     S = A P- A' + Omega + R                    K = P- A' S^-1
//     m_{i+1} = m- + K (y - A m- - b)            P_{i+1} = P- - K S K'            (m_0, P_0) = (m-, P-)
// With L = chol(P_i) and V = C L^-T:  A = V L^-1 and A P_i A' = V V', so only P_i (by the transform itself) and S are factored,
// Omega never is.  One body (iplf_update<>) for the whole-pass kernel k_iplf_loop<> - one trajectory per lane, the time loop and
// the iteration loop in one launch, the transforms through moment_transform_core<> with the template arguments fused_pass<> uses -
// and for the per-item kernel k_iplf_update<> of the launch-loop route (ssmq_filter_iterated.hip), so both routes round alike up to
// the transforms.  Host-free: the run-time compiler instantiates k_iplf_loop<> for user models.
#pragma once
#include "ssmq_filter_fused_kernel.h"

namespace ssmq {

struct IplfArgs {
    const double *y;            // [T][Y][ld]
    const double *m0, *P0;      // [D][ld], [D*D][ld] (lower triangle read)
    double *fm, *fP;            // [T][D][ld], [T][D*D][ld]
    double *delta;              // [T][ld] or null: max_d |m_J - m_{J-1}| / sqrt(P_J[d][d]) of every step
    int32_t *status;            // [B]: 0 or 1 + first failing step
    const double *c_dyn, *c_obs, *gqg;
    const double *radd;         // [Y*Y]: what the measurement transform adds to its covariance (here R, at every iterate)
    int64_t B, ld;
    int32_t T, iters, emv_dyn, emv_obs;
    double nu_dyn, nu_obs;
    FPar fd, fo;
};

// One re-linearised update.  mp, Pp: the prior (Pp packed lower); mi, Li: the iterate, Li = chol(P_i) packed; yh, Sy, C: the
// measurement moments at the iterate, Sy = S_y + R packed lower, C [Y][D] row-major = cov(h, x); y: the measurement.  Out: mn, Pn
// (packed lower; may alias nothing above).  Returns false when S is not positive definite (the results are then garbage).
// DT, YT > 0: dimensions fixed at compile time, everything in registers; 0: d_rt, y_rt <= SSMQ_MAX_DIM at run time.
// The substitutions and the update are the sums of tri_solve_fwd / tri_solve_bwd / sandwich (ssmq_device.h) written out: as helper
// calls the D = 5, Y = 4 k_ipls_pass<> came out with other spills and a third slower.
template <int DT, int YT>
__device__ __forceinline__ bool iplf_update(int d_rt, int y_rt, const double *mp, const double *Pp, const double *mi, const double *Li,
                                            const double *yh, const double *Sy, const double *C, const double *y, double *mn,
                                            double *Pn) {
    const int D = DT ? DT : d_rt, Y = YT ? YT : y_rt;
    constexpr int DM = DT ? DT : SSMQ_MAX_DIM, YM = YT ? YT : SSMQ_MAX_DIM;
    constexpr int UD = DT ? DT : 1, UY = YT ? YT : 1;
    double V[YM * DM], A[YM * DM], Tm[DM * YM], K[DM * YM], S[YM * (YM + 1) / 2], S0[YM * (YM + 1) / 2], r[YM];
    // V = C L^-T (forward substitution per row), A = V L^-1 (backward substitution)
#pragma unroll UY
    for (int e = 0; e < Y; ++e) {
#pragma unroll UD
        for (int i = 0; i < D; ++i) {
            double s = C[e * D + i];
#pragma unroll UD
            for (int q = 0; q < i; ++q) s -= Li[SSMQ_PK(i, q)] * V[e * D + q];
            V[e * D + i] = div_nr(s, Li[SSMQ_PK(i, i)]);
        }
#pragma unroll UD
        for (int i = D - 1; i >= 0; --i) {
            double s = V[e * D + i];
#pragma unroll UD
            for (int q = i + 1; q < D; ++q) s -= Li[SSMQ_PK(q, i)] * A[e * D + q];
            A[e * D + i] = div_nr(s, Li[SSMQ_PK(i, i)]);
        }
    }
    // Tm = P- A'  (D x Y)
#pragma unroll UD
    for (int d = 0; d < D; ++d)
#pragma unroll UY
        for (int e = 0; e < Y; ++e) {
            double s = 0.0;
#pragma unroll UD
            for (int q = 0; q < D; ++q) s += Pp[d >= q ? SSMQ_PK(d, q) : SSMQ_PK(q, d)] * A[e * D + q];
            Tm[d * Y + e] = s;
        }
    // S = (S_y + R) + (A P- A' - V V'): the bracket is A (P- - P_i) A', zero up to rounding in the first iteration
#pragma unroll UY
    for (int e = 0; e < Y; ++e) {
#pragma unroll UY
        for (int e2 = 0; e2 <= e; ++e2) {
            double apa = 0.0, vv = 0.0;
#pragma unroll UD
            for (int d = 0; d < D; ++d) {
                apa += A[e * D + d] * Tm[d * Y + e2];
                vv += V[e * D + d] * V[e2 * D + d];
            }
            S0[SSMQ_PK(e, e2)] = S[SSMQ_PK(e, e2)] = Sy[SSMQ_PK(e, e2)] + (apa - vv);
        }
        // y - A m- - b = (y - y^) - A (m- - m_i)
        double s = y[e] - yh[e];
#pragma unroll UD
        for (int d = 0; d < D; ++d) s -= A[e * D + d] * (mp[d] - mi[d]);
        r[e] = s;
    }
    bool ok;
    if (YT == 1) {   // scalar measurement: one division, as the fused time loop
        ok = S[0] > 0.0;
#pragma unroll UD
        for (int d = 0; d < D; ++d) K[d] = div_nr(Tm[d], S[0]);
    } else {
        ok = chol_packed<YT>(Y, S);
#pragma unroll UD
        for (int d = 0; d < D; ++d) {
#pragma unroll UY
            for (int i = 0; i < Y; ++i) {
                double s = Tm[d * Y + i];
#pragma unroll UY
                for (int q = 0; q < i; ++q) s -= S[SSMQ_PK(i, q)] * K[d * Y + q];
                K[d * Y + i] = div_nr(s, S[SSMQ_PK(i, i)]);
            }
#pragma unroll UY
            for (int i = Y - 1; i >= 0; --i) {
                double s = K[d * Y + i];
#pragma unroll UY
                for (int q = i + 1; q < Y; ++q) s -= S[SSMQ_PK(q, i)] * K[d * Y + q];
                K[d * Y + i] = div_nr(s, S[SSMQ_PK(i, i)]);
            }
        }
    }
#pragma unroll UD
    for (int d = 0; d < D; ++d) {
        double s = 0.0;
#pragma unroll UY
        for (int i = 0; i < Y; ++i) s += K[d * Y + i] * r[i];
        mn[d] = mp[d] + s;
    }
    // P_{i+1} = P- - (K S) K', lower triangle
#pragma unroll UD
    for (int d = 0; d < D; ++d) {
        double w[YM];
#pragma unroll UY
        for (int j = 0; j < Y; ++j) {
            double s = 0.0;
#pragma unroll UY
            for (int i = 0; i < Y; ++i) s += K[d * Y + i] * S0[i >= j ? SSMQ_PK(i, j) : SSMQ_PK(j, i)];
            w[j] = s;
        }
#pragma unroll UD
        for (int d2 = 0; d2 <= d; ++d2) {
            double s = 0.0;
#pragma unroll UY
            for (int j = 0; j < Y; ++j) s += w[j] * K[d2 * Y + j];
            Pn[SSMQ_PK(d, d2)] = Pp[SSMQ_PK(d, d2)] - s;
        }
    }
    return ok;
}

// max_d |mn[d] - mo[d]| / sqrt(Pn[d][d]); NaN when an operand is (the maximum is taken by comparisons that a NaN poisons)
template <int DT>
__device__ __forceinline__ double iplf_delta(int d_rt, const double *mn, const double *mo, const double *Pn) {
    const int D = DT ? DT : d_rt;
    constexpr int UD = DT ? DT : 1;
    double worst = 0.0;
#pragma unroll UD
    for (int d = 0; d < D; ++d) {
        const double v = fabs(mn[d] - mo[d]) / sqrt(Pn[SSMQ_PK(d, d)]);
        worst = (v <= worst) ? worst : v;      // (a NaN v is taken, and then stays: NaN <= x is false)
    }
    return worst;
}

// The whole pass: one trajectory per lane, grid of ceil(B / 64) blocks.
template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT>
__global__ SSMQ_PASS_LAUNCH_BOUNDS(D, FORM) void k_iplf_loop(const IplfArgs a) {
    const uint32_t b = blockIdx.x * kSmallBlock + threadIdx.x;
    if ((int64_t)b >= a.B) return;
    const int64_t ld = a.ld;
    constexpr int DP = D * (D + 1) / 2;
    double m[D], Pl[DP];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = a.m0[d * ld + b];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Pl[SSMQ_PK(i, j)] = a.P0[(i * D + j) * ld + b];
    const CoreParams cpd{(cdouble_p)a.c_dyn, (cdouble_p)a.gqg, a.emv_dyn, a.nu_dyn, 1.0, 1.0};
    const CoreParams cpo{(cdouble_p)a.c_obs, (cdouble_p)a.radd, a.emv_obs, a.nu_obs, 1.0, 1.0};
    FPar fd = a.fd, fo = a.fo;
    const double nan = __builtin_nan("");
    int32_t agg = 0;       // 1 + first failing step
#pragma unroll 1
    for (int k = 0; k < a.T; ++k) {
        const double t = (double)k;   // both transforms of step k + 1 use time index k, at every iteration
        if constexpr (HasTimeTable<FD>::value) { fd.tval = ((cdouble_p)a.fd.ttab)[k]; fd.use_tval = 1; }   // host: non-null
        if constexpr (HasTimeTable<FO>::value) { fo.tval = ((cdouble_p)a.fo.ttab)[k]; fo.use_tval = 1; }
        double yk[Y];
#pragma unroll
        for (int i = 0; i < Y; ++i) yk[i] = a.y[((int64_t)k * Y + i) * ld + b];
        // ---- time update: predictive state moments, + G Q G' ---------------------------------------------------------------
        RegSinkNoCross<D, D> pr;
        bool ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, false, OPT, RegSinkNoCross<D, D>>(m, Pl, t, fd, cpd, pr);
        // ---- J measurement updates of the prior, each linearised around the iterate -----------------------------------------
        double mi[D], Li[DP], dlt = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) mi[d] = pr.mf[d];
#pragma unroll
        for (int i = 0; i < DP; ++i) Li[i] = pr.cv[i];
#pragma unroll 1
        for (int it = 0; it < a.iters; ++it) {
            RegSink<D, Y> ob;
            // (the core leaves chol(P_i) in Li: the factor A = C P_i^-1 needs)
            ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, OPT, RegSink<D, Y>>(mi, Li, t, fo, cpo, ob) && ok;
            double mn[D], Pn[DP];
            ok = iplf_update<D, Y>(D, Y, pr.mf, pr.cv, mi, Li, ob.mf, ob.cv, &ob.cx[0][0], yk, mn, Pn) && ok;
            dlt = iplf_delta<D>(D, mn, mi, Pn);
#pragma unroll
            for (int d = 0; d < D; ++d) mi[d] = mn[d];
#pragma unroll
            for (int i = 0; i < DP; ++i) Li[i] = Pn[i];
        }
        // from the first failing step on every output of the trajectory is NaN (the NaN state fails every later factorisation)
        if (agg == 0 && !ok) agg = k + 1;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            m[d] = (agg == 0) ? mi[d] : nan;
            SSMQ_STORE(a.fm[((int64_t)k * D + d) * ld + b], m[d]);
        }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const double p = (agg == 0) ? Li[SSMQ_PK(i, j)] : nan;   // both triangles from the one value
                Pl[SSMQ_PK(i, j)] = p;
                SSMQ_STORE(a.fP[((int64_t)k * D * D + i * D + j) * ld + b], p);
                if (j != i) SSMQ_STORE(a.fP[((int64_t)k * D * D + j * D + i) * ld + b], p);
            }
        if (a.delta) SSMQ_STORE(a.delta[(int64_t)k * ld + b], (agg == 0) ? dlt : nan);
    }
    a.status[b] = agg;
}

// ---- the launch-loop route: one update per launch, on the planes one application of the measurement transform left ----------
struct IplfUpdArgs {
    const double *m_pr, *P_pr;        // [D][ld], [D*D][ld]: the prior of the step (lower triangle read)
    const double *m_it, *P_it;        // the iterate the measurement transform was applied at (the prior in the first iteration)
    const double *y_mean, *P_y, *P_yx;   // [Y][ld], [Y*Y][ld] (S_y + R, lower triangle read), [Y*D][ld]
    const double *y;                  // [Y][ld]
    double *m_out, *P_out;            // [D][ld], [D*D][ld]: the next iterate (may be m_it / P_it: a lane reads before it writes)
    double *delta;                    // [ld] of this step, or null (the host passes it with the last iteration alone)
    int32_t *status;                  // [B] aggregated: 0, else 1 + first failing step
    const int32_t *st_dyn, *st_obs;   // [B]: nonzero = that transform's Cholesky failed in this step / iteration
    int64_t B, ld;
    int32_t step, D, Y;
};

constexpr int kIplfUpdBlock = 64;

// DT, YT > 0: registers; 0, 0: run-time shapes up to SSMQ_MAX_DIM, private arrays in scratch
template <int DT, int YT>
__global__ __launch_bounds__(kIplfUpdBlock) void k_iplf_update(const IplfUpdArgs a) {
    const uint32_t b = blockIdx.x * kIplfUpdBlock + threadIdx.x;
    if ((int64_t)b >= a.B) return;
    const int64_t ld = a.ld;
    const int D = DT ? DT : a.D, Y = YT ? YT : a.Y;
    constexpr int DM = DT ? DT : SSMQ_MAX_DIM, YM = YT ? YT : SSMQ_MAX_DIM;
    constexpr int UD = DT ? DT : 1, UY = YT ? YT : 1;
    double mp[DM], Pp[DM * (DM + 1) / 2], mi[DM], Li[DM * (DM + 1) / 2], yh[YM], Sy[YM * (YM + 1) / 2], C[YM * DM], yk[YM];
    double mn[DM], Pn[DM * (DM + 1) / 2];
#pragma unroll UD
    for (int d = 0; d < D; ++d) {
        mp[d] = a.m_pr[(int64_t)d * ld + b];
        mi[d] = a.m_it[(int64_t)d * ld + b];
#pragma unroll UD
        for (int j = 0; j <= d; ++j) {
            Pp[SSMQ_PK(d, j)] = a.P_pr[((int64_t)d * D + j) * ld + b];
            Li[SSMQ_PK(d, j)] = a.P_it[((int64_t)d * D + j) * ld + b];
        }
    }
#pragma unroll UY
    for (int i = 0; i < Y; ++i) {
        yh[i] = a.y_mean[(int64_t)i * ld + b];
        yk[i] = a.y[(int64_t)i * ld + b];
#pragma unroll UY
        for (int j = 0; j <= i; ++j) Sy[SSMQ_PK(i, j)] = a.P_y[((int64_t)i * Y + j) * ld + b];
#pragma unroll UD
        for (int d = 0; d < D; ++d) C[i * D + d] = a.P_yx[((int64_t)i * D + d) * ld + b];
    }
    bool ok = chol_packed<DT>(D, Li);
    ok = iplf_update<DT, YT>(D, Y, mp, Pp, mi, Li, yh, Sy, C, yk, mn, Pn) && ok;
    int32_t agg = a.status[b];
    int32_t bad = ok ? 0 : 1;
    if (a.st_dyn) bad |= a.st_dyn[b];
    if (a.st_obs) bad |= a.st_obs[b];
    if (agg == 0 && bad) agg = a.step + 1;
    a.status[b] = agg;
    const double nan = __builtin_nan("");
    const bool good = (agg == 0);
    const double dlt = iplf_delta<DT>(D, mn, mi, Pn);
#pragma unroll UD
    for (int d = 0; d < D; ++d) {
        a.m_out[(int64_t)d * ld + b] = good ? mn[d] : nan;
#pragma unroll UD
        for (int j = 0; j <= d; ++j) {
            const double p = good ? Pn[SSMQ_PK(d, j)] : nan;   // both triangles from the one value
            a.P_out[((int64_t)d * D + j) * ld + b] = p;
            if (j != d) a.P_out[((int64_t)j * D + d) * ld + b] = p;
        }
    }
    if (a.delta) a.delta[b] = good ? dlt : nan;
}

}  // namespace ssmq
