// Missing and gated measurements: the measurement update of an additive-noise Gaussian filter when only some of the Y components of
// y_k arrived, and a chi-square gate in front of it.  Per step: ONE measurement transform at the prior (y^, P_h without noise,
// C = cov(h, x)), a bit mask w (bit i set: component i was observed), o = popcount(w), subscript o = the observed rows and columns:
//     S = P_h + R      e = y_k - y^      d2 = e_o' S_oo^-1 e_o      ll = -(o log 2 pi + log det S_oo + d2) / 2      (both 0 for o = 0)
//     take = (o > 0) and not (d2 > gate[o])
//     take:  K = C_o' S_oo^-1,  m = m- + K e_o,  P = P- - K S_oo K'          else:  m = m-,  P = P-  (bit for bit the prior)
// The observed rows are NOT compressed into a smaller system: an index that depends on the mask would send the private arrays to
// scratch, a branch on o would diverge within the wave.  The unobserved components are decoupled in place, by selects: for every
// unobserved i, e_i = 0, S_ii = 1, S_ij = S_ji = 0, C_i. = 0 - and then the static Y x Y code of the robust update runs
// (chol_packed<>, gain_from_cov<>, sandwich<>; Y = 1: one division).  Row i of the factor is then the unit vector, every term an
// unobserved row contributes to a sum is an exact zero and log 1 = 0, so the result is the subset update, rounded as a compressed
// factorisation in the same order would round it.  Selects, never a product with 0: the value of an unobserved y_i may be anything
// (NaN, Inf) and never reaches arithmetic - the select comes before the subtraction.  Gating is a select between the updated moments
// and the prior.  One body (masked_update<>) for the whole-pass kernel k_masked_loop<> - the structure and launch bounds of
// k_robust_loop<> - and for the per-item kernel k_masked_update<> of the launch-loop route (ssmq_filter_masked.hip).  Host-free: the
// run-time compiler instantiates k_masked_loop<> for user models.
#pragma once
#include "ssmq_filter_fused_kernel.h"

namespace ssmq {

struct MaskedArgs {
    const double *y;            // [T][Y][ld]
    const uint32_t *mask;       // [T][ld], bit i: component i observed; null: component i is observed iff y_i == y_i (NaN = missing)
    const double *m0, *P0;      // [D][ld], [D*D][ld] (lower triangle read)
    double *fm, *fP;            // [T][D][ld], [T][D*D][ld]
    uint32_t *used;             // [T][ld]: the mask the update applied (0: nothing offered, or the gate rejected)
    double *nis, *ll;           // [T][ld]: d2 and ll of the offered components
    int32_t *status;            // [B]: 0 or 1 + first failing step
    const double *c_dyn, *c_obs, *gqg;
    const double *radd;         // [Y*Y]: what the measurement transform adds to its covariance (here zeros: P_h carries no noise)
    const double *rr;           // [Y*Y]: R (lower triangle read)
    const double *gate;         // [Y+1]: entry o = threshold for o observed components (+inf: no gate), entry 0 not read
    int64_t B, ld;
    int32_t T, emv_dyn, emv_obs;
    double nu_dyn, nu_obs;
    FPar fd, fo;
};

// The mask of a step when no plane is given: bit i set iff y_i is not a NaN.
template <int YT>
__device__ __forceinline__ uint32_t mask_from_nan(int y_rt, const double *y) {
    const int Y = YT ? YT : y_rt;
    constexpr int UY = YT ? YT : 1;
    uint32_t w = 0;
#pragma unroll UY
    for (int i = 0; i < Y; ++i) w |= (y[i] == y[i]) ? (1u << i) : 0u;
    return w;
}

// The update of one step.  mp, Pp: the prior (Pp packed lower); y: the measurement; yh: y^; Ph: P_h packed lower; C [Y][D] row-major
// = cov(h, x); R: row-major [Y][Y], lower triangle read, gate [Y+1] (wave-uniform: scalar loads); w: the mask, bits at or above Y
// ignored.  Out: mn, Pn (packed lower), used (w when the update was applied, else 0), nis = d2, ll.  Returns false when the
// factorisation fails or a mean that goes out is not finite (an observed NaN component; a NaN d2 does not gate, so the update runs
// and fails here; the results are then garbage).  DT, YT > 0: dimensions fixed at compile time, everything in registers; 0: d_rt,
// y_rt <= SSMQ_MAX_DIM at run time.
template <int DT, int YT>
__device__ __forceinline__ bool masked_update(int d_rt, int y_rt, uint32_t w, const double *mp, const double *Pp, const double *y,
                                              const double *yh, const double *Ph, const double *C, const cdouble_p R, const cdouble_p gate,
                                              double *mn, double *Pn, uint32_t &used, double &nis, double &ll) {
    const int D = DT ? DT : d_rt, Y = YT ? YT : y_rt;
    constexpr int DM = DT ? DT : SSMQ_MAX_DIM, YM = YT ? YT : SSMQ_MAX_DIM;
    constexpr int UD = DT ? DT : 1, UY = YT ? YT : 1;
    constexpr int YP = YM * (YM + 1) / 2;
    w &= (1u << Y) - 1u;   // (Y <= SSMQ_MAX_DIM = 16)
    const int o = __builtin_popcount(w);
    double e[YM], S[YP], S0[YP];
    double thr = __builtin_inf();
    // ---- decouple the unobserved components: selects alone -------------------------------------------------------------------------
#pragma unroll UY
    for (int a = 0; a < Y; ++a) {
        const bool oa = (w >> a) & 1u;
        const double ya = oa ? y[a] : yh[a];   // (the select first: an unobserved y_a is not an operand of anything)
        e[a] = ya - yh[a];
        thr = (o == a + 1) ? gate[a + 1] : thr;
#pragma unroll UY
        for (int b = 0; b <= a; ++b) {
            const bool ob = (w >> b) & 1u;
            const double s = Ph[SSMQ_PK(a, b)] + R[a * Y + b];
            S0[SSMQ_PK(a, b)] = S[SSMQ_PK(a, b)] = (oa && ob) ? s : (a == b ? 1.0 : 0.0);
        }
    }
    bool ok = true;
    double d2 = 0.0, ldet = 0.0;
    double um[DM], uP[DM * (DM + 1) / 2];   // the updated moments
    if constexpr (DT > 0 && YT > 0) {
        double G[DT][YT];
        ok = gain_from_cov<DT, YT>(*(double (*)[YT * (YT + 1) / 2])S, [&](int i, int d) { return ((w >> i) & 1u) ? C[i * DT + d] : 0.0; }, G);
        if constexpr (YT == 1) {   // scalar measurement: S is not factored
            d2 = div_nr(e[0] * e[0], S[0]);
            ldet = log(S[0]);
        } else {
            double v[YT];
            tri_solve_fwd<YT>(S, [&](int i) { return e[i]; }, v);
            double lg = 0.0;
#pragma unroll
            for (int i = 0; i < YT; ++i) {
                d2 += v[i] * v[i];
                lg += log(S[SSMQ_PK(i, i)]);
            }
            ldet = lg + lg;
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < YT; ++i) s += G[d][i] * e[i];
            um[d] = mp[d] + s;
        }
        sandwich<DT, YT>(G, [&](int i, int j) { return S0[i >= j ? SSMQ_PK(i, j) : SSMQ_PK(j, i)]; },
                         [&](int d, int d2_, double s) { if (d2_ <= d) uP[SSMQ_PK(d, d2_)] = Pp[SSMQ_PK(d, d2_)] - s; });
    } else {
        double G[DM * YM], t[YM];
        ok = chol_packed<0>(Y, S);
        double lg = 0.0;
        for (int i = 0; i < Y; ++i) {
            double s = e[i];
            for (int q = 0; q < i; ++q) s -= S[SSMQ_PK(i, q)] * t[q];
            t[i] = div_nr(s, S[SSMQ_PK(i, i)]);
            d2 += t[i] * t[i];
            lg += log(S[SSMQ_PK(i, i)]);
        }
        ldet = lg + lg;
        for (int d = 0; d < D; ++d) {
            for (int i = 0; i < Y; ++i) {
                double s = ((w >> i) & 1u) ? C[i * D + d] : 0.0;
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
            um[d] = mp[d] + s;
            for (int j = 0; j < Y; ++j) {
                double u = 0.0;
                for (int i = 0; i < Y; ++i) u += G[d * Y + i] * S0[i >= j ? SSMQ_PK(i, j) : SSMQ_PK(j, i)];
                t[j] = u;
            }
            for (int d2_ = 0; d2_ <= d; ++d2_) {
                double u = 0.0;
                for (int j = 0; j < Y; ++j) u += t[j] * G[d2_ * Y + j];
                uP[SSMQ_PK(d, d2_)] = Pp[SSMQ_PK(d, d2_)] - u;
            }
        }
    }
    // ---- scores of what was offered; the gate: a select between the update and the prior ----------------------------------------------
    const bool take = (o > 0) && !(d2 > thr);
    nis = (o > 0) ? d2 : 0.0;
    ll = (o > 0) ? -0.5 * ((double)o * 1.8378770664093453 /* log(2 pi) */ + ldet + d2) : 0.0;
    used = take ? w : 0u;
#pragma unroll UD
    for (int d = 0; d < D; ++d) {
        mn[d] = take ? um[d] : mp[d];
        ok = ok && (fabs(mn[d]) < __builtin_inf());
#pragma unroll UD
        for (int j = 0; j <= d; ++j) Pn[SSMQ_PK(d, j)] = take ? uP[SSMQ_PK(d, j)] : Pp[SSMQ_PK(d, j)];
    }
    return ok;
}

// The whole pass: one trajectory per lane, grid of ceil(B / 64) blocks.
template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT = 0>
__global__ SSMQ_PASS_LAUNCH_BOUNDS(D, FORM) void k_masked_loop(const MaskedArgs a) {
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
        double yk[Y];
#pragma unroll
        for (int i = 0; i < Y; ++i) yk[i] = a.y[((int64_t)k * Y + i) * ld + b];
        const uint32_t w = a.mask ? a.mask[(int64_t)k * ld + b] : mask_from_nan<Y>(Y, yk);   // (wave-uniform choice)
        // ---- time update: predictive state moments, + G Q G' ---------------------------------------------------------------
        RegSinkNoCross<D, D> pr;
        bool ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, false, OPT, RegSinkNoCross<D, D>>(m, Pl, t, fd, cpd, pr);
        // ---- the measurement transform, at the prior, without noise: at every step, whatever the mask ------------------------
        double L2[DP];
#pragma unroll
        for (int i = 0; i < DP; ++i) L2[i] = pr.cv[i];
        RegSink<D, Y> ob;
        ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, OPT, RegSink<D, Y>>(pr.mf, L2, t, fo, cpo, ob) && ok;
        // ---- the update over the observed components, behind the gate ------------------------------------------------------
        double mn[D], Pn[DP], nis, ll;
        uint32_t used;
        ok = masked_update<D, Y>(D, Y, w, pr.mf, pr.cv, yk, ob.mf, ob.cv, &ob.cx[0][0], (cdouble_p)a.rr, (cdouble_p)a.gate, mn, Pn, used, nis,
                                 ll) && ok;
        // from the first failing step on every output of the trajectory is NaN (the NaN state fails every later step), used is 0
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
        SSMQ_STORE(a.used[(int64_t)k * ld + b], (agg == 0) ? used : 0u);
        SSMQ_STORE(a.nis[(int64_t)k * ld + b], (agg == 0) ? nis : nan);
        SSMQ_STORE(a.ll[(int64_t)k * ld + b], (agg == 0) ? ll : nan);
    }
    a.status[b] = agg;
}

// ---- the launch-loop route: one update per launch, on the planes the two transforms of the step left ---------------------------
struct MaskedUpdArgs {
    const double *m_pr, *P_pr;        // [D][ld], [D*D][ld]: the prior of the step (lower triangle read)
    const double *y_mean, *P_y, *P_yx;   // [Y][ld], [Y*Y][ld] (P_h: no noise added; lower triangle read), [Y*D][ld]
    const double *y;                  // [Y][ld]
    const uint32_t *mask;             // [ld] of this step, or null: NaN = missing
    double *m_out, *P_out;            // [D][ld], [D*D][ld]
    uint32_t *used;                   // [ld] of this step
    double *nis, *ll;                 // [ld] each, of this step
    int32_t *status;                  // [B] aggregated: 0, else 1 + first failing step
    const int32_t *st_dyn, *st_obs;   // [B]: nonzero = that transform's Cholesky failed in this step
    const double *rr, *gate;          // [Y*Y], [Y+1]
    int64_t B, ld;
    int32_t step, D, Y;
};

constexpr int kMaskedUpdBlock = 64;

// DT, YT > 0: registers; 0, 0: run-time shapes up to SSMQ_MAX_DIM, private arrays in scratch
template <int DT, int YT>
__global__ __launch_bounds__(kMaskedUpdBlock) void k_masked_update(const MaskedUpdArgs a) {
    const uint32_t b = blockIdx.x * kMaskedUpdBlock + threadIdx.x;
    if ((int64_t)b >= a.B) return;
    const int64_t ld = a.ld;
    const int D = DT ? DT : a.D, Y = YT ? YT : a.Y;
    constexpr int DM = DT ? DT : SSMQ_MAX_DIM, YM = YT ? YT : SSMQ_MAX_DIM;
    constexpr int UD = DT ? DT : 1, UY = YT ? YT : 1;
    double mp[DM], Pp[DM * (DM + 1) / 2], yk[YM], yh[YM], Ph[YM * (YM + 1) / 2], C[YM * DM];
    double mn[DM], Pn[DM * (DM + 1) / 2];
#pragma unroll UD
    for (int d = 0; d < D; ++d) {
        mp[d] = a.m_pr[(int64_t)d * ld + b];
#pragma unroll UD
        for (int j = 0; j <= d; ++j) Pp[SSMQ_PK(d, j)] = a.P_pr[((int64_t)d * D + j) * ld + b];
    }
#pragma unroll UY
    for (int i = 0; i < Y; ++i) {
        yk[i] = a.y[(int64_t)i * ld + b];
        yh[i] = a.y_mean[(int64_t)i * ld + b];
#pragma unroll UY
        for (int j = 0; j <= i; ++j) Ph[SSMQ_PK(i, j)] = a.P_y[((int64_t)i * Y + j) * ld + b];
#pragma unroll UD
        for (int d = 0; d < D; ++d) C[i * D + d] = a.P_yx[((int64_t)i * D + d) * ld + b];
    }
    const uint32_t w = a.mask ? a.mask[b] : mask_from_nan<YT>(Y, yk);
    double nis, ll;
    uint32_t used;
    const bool ok = masked_update<DT, YT>(D, Y, w, mp, Pp, yk, yh, Ph, C, (cdouble_p)a.rr, (cdouble_p)a.gate, mn, Pn, used, nis, ll);
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
    a.used[b] = good ? used : 0u;
    a.nis[b] = good ? nis : nan;
    a.ll[b] = good ? ll : nan;
}

}  // namespace ssmq
