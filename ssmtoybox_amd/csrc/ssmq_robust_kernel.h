// Outlier-robust measurement update (Agamennoni et al. 2012; Piche, Sarkka, Hartikainen 2012): the measurement update of an
// additive-noise Gaussian filter under Student-t measurement noise, r | lambda ~ N(0, R / lambda), lambda ~ Gamma(dof / 2, dof / 2).
// ONE measurement transform per step, at the prior: y^, P_h (without noise), C = tf_obs(m-, P-), e = y - y^, lambda_0 = 1; then the
// variational fixed point in measurement space, i = 0 .. J-2:
//     S_i = P_h + R / lambda_i        r^ = (R / lambda_i) S_i^-1 e        Psi = r^ r^' + P_h - P_h S_i^-1 P_h
//     gamma = sum_ab iR[a][b] Psi[a][b]        lambda_{i+1} = (dof + Y) / (dof + gamma)
// and one state update with the last weight: S = P_h + R / lambda_{J-1}, K = C' S^-1, m = m- + K e, P = P- - K S K'.
// Only Y x Y matrices are factored; nothing is transformed again.  One body (robust_update<>) for the whole-pass kernel
// k_robust_loop<> - one trajectory per lane, the time loop and the fixed point in one launch, the transforms through
// moment_transform_core<> with the template arguments fused_pass<> uses - and for the per-item kernel k_robust_update<> of the
// launch-loop route (ssmq_filter_robust.hip), so both routes round alike up to the transforms.  Host-free: the run-time compiler
// instantiates k_robust_loop<> for user models.
#pragma once
#include "ssmq_filter_fused_kernel.h"

namespace ssmq {

struct RobustArgs {
    const double *y;            // [T][Y][ld]
    const double *m0, *P0;      // [D][ld], [D*D][ld] (lower triangle read)
    double *fm, *fP;            // [T][D][ld], [T][D*D][ld]
    double *lam, *delta;        // [T][ld] each: the weight the update used, |lambda_{J-1} - lambda_{J-2}| / lambda_{J-1}
    int32_t *status;            // [B]: 0 or 1 + first failing step
    const double *c_dyn, *c_obs, *gqg;
    const double *radd;         // [Y*Y]: what the measurement transform adds to its covariance (here zeros: P_h carries no noise)
    const double *rr, *ir;      // [Y*Y] each: the scale matrix R and its inverse (lower triangles read)
    int64_t B, ld;
    int32_t T, iters, emv_dyn, emv_obs;
    double nu_dyn, nu_obs, dof;
    FPar fd, fo;
};

// The fixed point and the state update of one step.  mp, Pp: the prior (Pp packed lower); e = y - y^; Ph: P_h packed lower; C [Y][D]
// row-major = cov(h, x); R, iR: row-major [Y][Y], lower triangles read (wave-uniform: scalar loads).  Out: mn, Pn (packed lower), lam
// = lambda_{J-1}, dlt = |lambda_{J-1} - lambda_{J-2}| / lambda_{J-1} (0 for J = 1).  Returns false when a factorisation fails, a
// weight is not a positive finite number or the updated mean is not finite (a NaN measurement; the results are then garbage).
// DT, YT > 0: dimensions fixed at compile time, everything in registers; 0: d_rt, y_rt <= SSMQ_MAX_DIM at run time.
// The state update is gain_from_cov<> and sandwich<> (ssmq_device.h), what kalman_update_item (ssmq_update.h) is made of, with
// P_h + R / lambda for P_y; those two take compile-time sizes, so the run-time shape has their sums on run-time loops.
template <int DT, int YT>
__device__ __forceinline__ bool robust_update(int d_rt, int y_rt, int iters, double dof, const double *mp, const double *Pp, const double *e,
                                              const double *Ph, const double *C, const cdouble_p R, const cdouble_p iR, double *mn,
                                              double *Pn, double &lam, double &dlt) {
    const int D = DT ? DT : d_rt, Y = YT ? YT : y_rt;
    constexpr int DM = DT ? DT : SSMQ_MAX_DIM, YM = YT ? YT : SSMQ_MAX_DIM;
    constexpr int UD = DT ? DT : 1, UY = YT ? YT : 1;
    constexpr int YP = YM * (YM + 1) / 2;
    double Rl[YP], S[YP];
    bool ok = true;
    lam = 1.0;
    dlt = 0.0;
#pragma unroll 1
    for (int it = 0; it + 1 < iters; ++it) {
        const double il = div_nr(1.0, lam);
#pragma unroll UY
        for (int a = 0; a < Y; ++a)
#pragma unroll UY
            for (int b = 0; b <= a; ++b) {
                Rl[SSMQ_PK(a, b)] = R[a * Y + b] * il;
                S[SSMQ_PK(a, b)] = Ph[SSMQ_PK(a, b)] + Rl[SSMQ_PK(a, b)];
            }
        double gamma = 0.0;
        if (YT == 1) {   // scalar measurement: one division, as the fused time loop
            ok = ok && (S[0] > 0.0);
            const double is = div_nr(1.0, S[0]);
            const double rh = Rl[0] * (is * e[0]);
            gamma = iR[0] * (rh * rh + (Ph[0] - Ph[0] * (is * Ph[0])));
        } else {
            ok = chol_packed<YT>(Y, S) && ok;
            // z = S^-1 e;  W = L^-1 P_h (column by column), P_h S^-1 P_h = W' W
            double z[YM], W[YM * YM], rh[YM];
#pragma unroll UY
            for (int i = 0; i < Y; ++i) {
                double s = e[i];
#pragma unroll UY
                for (int q = 0; q < i; ++q) s -= S[SSMQ_PK(i, q)] * z[q];
                z[i] = div_nr(s, S[SSMQ_PK(i, i)]);
            }
#pragma unroll UY
            for (int i = Y - 1; i >= 0; --i) {
                double s = z[i];
#pragma unroll UY
                for (int q = i + 1; q < Y; ++q) s -= S[SSMQ_PK(q, i)] * z[q];
                z[i] = div_nr(s, S[SSMQ_PK(i, i)]);
            }
#pragma unroll UY
            for (int c = 0; c < Y; ++c)
#pragma unroll UY
                for (int i = 0; i < Y; ++i) {
                    double s = Ph[i >= c ? SSMQ_PK(i, c) : SSMQ_PK(c, i)];
#pragma unroll UY
                    for (int q = 0; q < i; ++q) s -= S[SSMQ_PK(i, q)] * W[q * Y + c];
                    W[i * Y + c] = div_nr(s, S[SSMQ_PK(i, i)]);
                }
#pragma unroll UY
            for (int a = 0; a < Y; ++a) {
                double s = 0.0;
#pragma unroll UY
                for (int b = 0; b < Y; ++b) s += Rl[a >= b ? SSMQ_PK(a, b) : SSMQ_PK(b, a)] * z[b];
                rh[a] = s;
            }
            // gamma = sum_ab iR[a][b] Psi[a][b]: the diagonal once, the strict lower triangle twice (both are symmetric)
#pragma unroll UY
            for (int a = 0; a < Y; ++a)
#pragma unroll UY
                for (int b = 0; b <= a; ++b) {
                    double ww = 0.0;
#pragma unroll UY
                    for (int q = 0; q < Y; ++q) ww += W[q * Y + a] * W[q * Y + b];
                    const double psi = rh[a] * rh[b] + (Ph[SSMQ_PK(a, b)] - ww);
                    const double t = iR[a * Y + b] * psi;
                    gamma += (a == b) ? t : t + t;
                }
        }
        const double ln = (dof + (double)Y) / (dof + gamma);   // IEEE division: dof + Y == dof + gamma gives 1.0 exactly
        ok = ok && (ln > 0.0) && (ln < __builtin_inf());
        dlt = fabs(ln - lam) / ln;
        lam = ln;
    }
    // ---- the state update with the last weight ----------------------------------------------------------------------------------
    const double il = div_nr(1.0, lam);
    double S0[YP];
#pragma unroll UY
    for (int a = 0; a < Y; ++a)
#pragma unroll UY
        for (int b = 0; b <= a; ++b) S0[SSMQ_PK(a, b)] = S[SSMQ_PK(a, b)] = Ph[SSMQ_PK(a, b)] + R[a * Y + b] * il;
    if constexpr (DT > 0 && YT > 0) {
        double G[DT][YT];
        ok = gain_from_cov<DT, YT>(*(double (*)[YT * (YT + 1) / 2])S, [&](int i, int d) { return C[i * DT + d]; }, G) && ok;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < YT; ++i) s += G[d][i] * e[i];
            mn[d] = mp[d] + s;
        }
        sandwich<DT, YT>(G, [&](int i, int j) { return S0[i >= j ? SSMQ_PK(i, j) : SSMQ_PK(j, i)]; },
                         [&](int d, int d2, double s) { if (d2 <= d) Pn[SSMQ_PK(d, d2)] = Pp[SSMQ_PK(d, d2)] - s; });
    } else {
        double G[DM * YM], w[YM];
        ok = chol_packed<0>(Y, S) && ok;
        for (int d = 0; d < D; ++d) {
            for (int i = 0; i < Y; ++i) {
                double s = C[i * D + d];
                for (int q = 0; q < i; ++q) s -= S[SSMQ_PK(i, q)] * G[d * Y + q];
                G[d * Y + i] = div_nr(s, S[SSMQ_PK(i, i)]);
            }
            for (int i = Y - 1; i >= 0; --i) {
                double s = G[d * Y + i];
                for (int q = i + 1; q < Y; ++q) s -= S[SSMQ_PK(q, i)] * G[d * Y + q];
                G[d * Y + i] = div_nr(s, S[SSMQ_PK(i, i)]);
            }
        }
        for (int d = 0; d < D; ++d) {
            double s = 0.0;
            for (int i = 0; i < Y; ++i) s += G[d * Y + i] * e[i];
            mn[d] = mp[d] + s;
            for (int j = 0; j < Y; ++j) {
                double u = 0.0;
                for (int i = 0; i < Y; ++i) u += G[d * Y + i] * S0[i >= j ? SSMQ_PK(i, j) : SSMQ_PK(j, i)];
                w[j] = u;
            }
            for (int d2 = 0; d2 <= d; ++d2) {
                double u = 0.0;
                for (int j = 0; j < Y; ++j) u += w[j] * G[d2 * Y + j];
                Pn[SSMQ_PK(d, d2)] = Pp[SSMQ_PK(d, d2)] - u;
            }
        }
    }
    // a NaN measurement reaches the mean alone (the covariance and, for J = 1, the weight do not read it)
#pragma unroll UD
    for (int d = 0; d < D; ++d) ok = ok && (fabs(mn[d]) < __builtin_inf());
    return ok;
}

// The whole pass: one trajectory per lane, grid of ceil(B / 64) blocks.
template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT = 0>
__global__ SSMQ_PASS_LAUNCH_BOUNDS(D, FORM) void k_robust_loop(const RobustArgs a) {
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
        const double t = (double)k;   // both transforms of step k + 1 use time index k
        if constexpr (HasTimeTable<FD>::value) { fd.tval = ((cdouble_p)a.fd.ttab)[k]; fd.use_tval = 1; }   // host: non-null
        if constexpr (HasTimeTable<FO>::value) { fo.tval = ((cdouble_p)a.fo.ttab)[k]; fo.use_tval = 1; }
        double e[Y];
#pragma unroll
        for (int i = 0; i < Y; ++i) e[i] = a.y[((int64_t)k * Y + i) * ld + b];
        // ---- time update: predictive state moments, + G Q G' ---------------------------------------------------------------
        RegSinkNoCross<D, D> pr;
        bool ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, false, OPT, RegSinkNoCross<D, D>>(m, Pl, t, fd, cpd, pr);
        // ---- the one measurement transform of the step, at the prior, without noise ----------------------------------------
        double L2[DP];
#pragma unroll
        for (int i = 0; i < DP; ++i) L2[i] = pr.cv[i];
        RegSink<D, Y> ob;
        ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, OPT, RegSink<D, Y>>(pr.mf, L2, t, fo, cpo, ob) && ok;
#pragma unroll
        for (int i = 0; i < Y; ++i) e[i] -= ob.mf[i];
        // ---- fixed point in measurement space, state update ----------------------------------------------------------------
        double mn[D], Pn[DP], lam, dlt;
        ok = robust_update<D, Y>(D, Y, a.iters, a.dof, pr.mf, pr.cv, e, ob.cv, &ob.cx[0][0], (cdouble_p)a.rr, (cdouble_p)a.ir, mn, Pn, lam,
                                 dlt) && ok;
        // from the first failing step on every output of the trajectory is NaN (the NaN state fails every later factorisation)
        if (agg == 0 && !ok) agg = k + 1;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            m[d] = (agg == 0) ? mn[d] : nan;
            SSMQ_STORE(a.fm[((int64_t)k * D + d) * ld + b], m[d]);
        }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const double p = (agg == 0) ? Pn[SSMQ_PK(i, j)] : nan;   // both triangles from the one value
                Pl[SSMQ_PK(i, j)] = p;
                SSMQ_STORE(a.fP[((int64_t)k * D * D + i * D + j) * ld + b], p);
                if (j != i) SSMQ_STORE(a.fP[((int64_t)k * D * D + j * D + i) * ld + b], p);
            }
        SSMQ_STORE(a.lam[(int64_t)k * ld + b], (agg == 0) ? lam : nan);
        SSMQ_STORE(a.delta[(int64_t)k * ld + b], (agg == 0) ? dlt : nan);
    }
    a.status[b] = agg;
}

// ---- the launch-loop route: one update per launch, on the planes the two transforms of the step left ---------------------------
struct RobustUpdArgs {
    const double *m_pr, *P_pr;        // [D][ld], [D*D][ld]: the prior of the step (lower triangle read)
    const double *y_mean, *P_y, *P_yx;   // [Y][ld], [Y*Y][ld] (P_h: no noise added; lower triangle read), [Y*D][ld]
    const double *y;                  // [Y][ld]
    double *m_out, *P_out;            // [D][ld], [D*D][ld]
    double *lam, *delta;              // [ld] each, of this step
    int32_t *status;                  // [B] aggregated: 0, else 1 + first failing step
    const int32_t *st_dyn, *st_obs;   // [B]: nonzero = that transform's Cholesky failed in this step
    const double *rr, *ir;            // [Y*Y] each
    int64_t B, ld;
    int32_t step, D, Y, iters;
    double dof;
};

constexpr int kRobustUpdBlock = 64;

// DT, YT > 0: registers; 0, 0: run-time shapes up to SSMQ_MAX_DIM, private arrays in scratch
template <int DT, int YT>
__global__ __launch_bounds__(kRobustUpdBlock) void k_robust_update(const RobustUpdArgs a) {
    const uint32_t b = blockIdx.x * kRobustUpdBlock + threadIdx.x;
    if ((int64_t)b >= a.B) return;
    const int64_t ld = a.ld;
    const int D = DT ? DT : a.D, Y = YT ? YT : a.Y;
    constexpr int DM = DT ? DT : SSMQ_MAX_DIM, YM = YT ? YT : SSMQ_MAX_DIM;
    constexpr int UD = DT ? DT : 1, UY = YT ? YT : 1;
    double mp[DM], Pp[DM * (DM + 1) / 2], e[YM], Ph[YM * (YM + 1) / 2], C[YM * DM];
    double mn[DM], Pn[DM * (DM + 1) / 2];
#pragma unroll UD
    for (int d = 0; d < D; ++d) {
        mp[d] = a.m_pr[(int64_t)d * ld + b];
#pragma unroll UD
        for (int j = 0; j <= d; ++j) Pp[SSMQ_PK(d, j)] = a.P_pr[((int64_t)d * D + j) * ld + b];
    }
#pragma unroll UY
    for (int i = 0; i < Y; ++i) {
        e[i] = a.y[(int64_t)i * ld + b] - a.y_mean[(int64_t)i * ld + b];
#pragma unroll UY
        for (int j = 0; j <= i; ++j) Ph[SSMQ_PK(i, j)] = a.P_y[((int64_t)i * Y + j) * ld + b];
#pragma unroll UD
        for (int d = 0; d < D; ++d) C[i * D + d] = a.P_yx[((int64_t)i * D + d) * ld + b];
    }
    double lam, dlt;
    const bool ok = robust_update<DT, YT>(D, Y, a.iters, a.dof, mp, Pp, e, Ph, C, (cdouble_p)a.rr, (cdouble_p)a.ir, mn, Pn, lam, dlt);
    int32_t agg = a.status[b];
    int32_t bad = ok ? 0 : 1;
    if (a.st_dyn) bad |= a.st_dyn[b];
    if (a.st_obs) bad |= a.st_obs[b];
    if (agg == 0 && bad) agg = a.step + 1;
    a.status[b] = agg;
    const double nan = __builtin_nan("");
    const bool good = (agg == 0);
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
    a.lam[b] = good ? lam : nan;
    a.delta[b] = good ? dlt : nan;
}

}  // namespace ssmq
