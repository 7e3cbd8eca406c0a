// Innovation scores of a filter pass: normalised innovation squared (NIS) e' S^-1 e and the measurement log-likelihood
// log p(y_k | y_1..k-1) of every step of every trajectory, from the FILTERED moments the pass left in HBM.
//
// Step k's predictive measurement moments depend only on (fm[k-1], fP[k-1]) - on (m0, P0) for k = 0 - so the T B items are
// independent: k_innovation<> replays both transforms of the step with the code of the fused time loop (moment_transform_core<>,
// the template arguments fused_pass<> uses) and scores the innovation, one item per lane, no recursion.  The dispatch table, the
// scoring half on its own (k_innovation_score: the launch-loop route) and the per-trajectory totals: ssmq_innovation.hip.
#pragma once
#include "ssmq_filter_fused_kernel.h"

namespace ssmq {

struct InnovArgs {
    const double *y;            // [T][Y][ld]
    const double *m0, *P0;      // [D][ld], [D*D][ld]
    const double *fm, *fP;      // [T][D][ld], [T][D*D][ld]: the filtered moments (lower triangle of fP read)
    double *ymean, *S;          // [T][Y][ld], [T][Y*Y][ld], or null: not stored
    double *nis, *ll;           // [T][ld]
    const double *c_dyn, *c_obs, *gqg, *rr;
    int64_t B, ld;
    int32_t T, emv_dyn, emv_obs, nblk;   // nblk: blocks of 64 trajectories per step
    double nu_dyn, nu_obs;
    FPar fd, fo;
};

// e = y - y_mean; S: in = packed lower triangle of the innovation covariance, out = its Cholesky factor (the operation order of
// chol_packed<>).  nis = |L^-1 e|^2, ll = -(Y log 2 pi + log det S + nis) / 2.  Returns false at a non-positive (or NaN) pivot.
// YT > 0: Y fixed at compile time, everything in registers; YT = 0: Y = y_rt <= SSMQ_MAX_DIM at run time.
// The factor and the forward substitution are chol_packed<> and tri_solve_fwd<> (ssmq_device.h) written out, with log det and nis
// accumulated on the way: as helper calls the kernels came out with other register counts and the run-time-size one 5 % longer.
template <int YT>
__device__ __forceinline__ bool innovation_score(int y_rt, const double *e, double *S, double &nis, double &ll) {
    const int Y = YT ? YT : y_rt;
    constexpr int UN = YT ? YT : 1;   // fixed Y: unrolled in full; run-time Y: loops
    double v[YT ? YT : SSMQ_MAX_DIM];
    bool ok = true;
    double lg = 0.0, q = 0.0;
#pragma unroll UN
    for (int j = 0; j < Y; ++j) {
        double ajj = S[SSMQ_PK(j, j)];
#pragma unroll UN
        for (int k = 0; k < j; ++k) ajj -= S[SSMQ_PK(j, k)] * S[SSMQ_PK(j, k)];
        ok = ok && (ajj > 0.0);
        double r;
        sqrt_rsqrt(ajj, ajj, r);
        S[SSMQ_PK(j, j)] = ajj;
        lg += log(ajj);
#pragma unroll UN
        for (int i = j + 1; i < Y; ++i) {
            double s = S[SSMQ_PK(i, j)];
#pragma unroll UN
            for (int k = 0; k < j; ++k) s -= S[SSMQ_PK(i, k)] * S[SSMQ_PK(j, k)];
            S[SSMQ_PK(i, j)] = s * r;
        }
    }
#pragma unroll UN
    for (int i = 0; i < Y; ++i) {
        double s = e[i];
#pragma unroll UN
        for (int k = 0; k < i; ++k) s -= S[SSMQ_PK(i, k)] * v[k];
        v[i] = div_nr(s, S[SSMQ_PK(i, i)]);
        q += v[i] * v[i];
    }
    nis = q;
    ll = -0.5 * ((double)Y * 1.8378770664093453 /* log(2 pi) */ + 2.0 * lg + q);
    return ok;
}

// One item (step, trajectory) per lane.  1-D grid of T nblk blocks (T may exceed the 65 535 of grid.y): step = blockIdx.x / nblk.
// Launch bounds: those of k_filter_fused<> of the same shape.
template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT>
__global__ __launch_bounds__(kSmallBlock, (SSMQ_FUSED_FORCE_OCC ? SSMQ_FUSED_FORCE_OCC
                                           : (D >= 6 ? 1 : ((D >= 5 && FORM == SSMQ_FORM_SIGMA) ? SSMQ_FUSED_OCC_D5_SIGMA : 2)))) void k_innovation(const InnovArgs a) {
    const int k = (int)(blockIdx.x / (uint32_t)a.nblk);
    const uint32_t b = (blockIdx.x - (uint32_t)k * (uint32_t)a.nblk) * kSmallBlock + threadIdx.x;
    if (k >= a.T || (int64_t)b >= a.B) return;
    const int64_t ld = a.ld;
    // inputs of step k: the filtered moments of step k - 1, the initial moments for k = 0 (wave-uniform choice)
    const double *mi = k == 0 ? a.m0 : a.fm + (int64_t)(k - 1) * D * ld;
    const double *Pi = k == 0 ? a.P0 : a.fP + (int64_t)(k - 1) * D * D * ld;
    double m[D], Pl[D * (D + 1) / 2], yk[Y];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = mi[d * ld + b];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Pl[SSMQ_PK(i, j)] = Pi[(i * D + j) * ld + b];
#pragma unroll
    for (int i = 0; i < Y; ++i) yk[i] = a.y[((int64_t)k * Y + i) * ld + b];
    const double t = (double)k;   // both transforms of step k + 1 use time index k (ssinf.py:104, 276-288)
    FPar fd = a.fd, fo = a.fo;
    if constexpr (HasTimeTable<FD>::value) { fd.tval = ((cdouble_p)a.fd.ttab)[k]; fd.use_tval = 1; }   // host: non-null
    if constexpr (HasTimeTable<FO>::value) { fo.tval = ((cdouble_p)a.fo.ttab)[k]; fo.use_tval = 1; }
    const CoreParams cpd{(cdouble_p)a.c_dyn, (cdouble_p)a.gqg, a.emv_dyn, a.nu_dyn, 1.0, 1.0};
    const CoreParams cpo{(cdouble_p)a.c_obs, (cdouble_p)a.rr, a.emv_obs, a.nu_obs, 1.0, 1.0};
    bool ok = true;
#pragma unroll
    for (int d = 0; d < D; ++d) ok = ok && (m[d] == m[d]);   // a NaN mean: the filter failed earlier
    // ---- predictive state moments, + G Q G' (ssinf.py:276-279) ------------------------------------------------------------
    RegSinkNoCross<D, D> pr;
    ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, false, OPT, RegSinkNoCross<D, D>>(m, Pl, t, fd, cpd, pr) && ok;
    // ---- predictive measurement moments, + R (ssinf.py:287-291) -----------------------------------------------------------
    double L2[D * (D + 1) / 2];
#pragma unroll
    for (int i = 0; i < D * (D + 1) / 2; ++i) L2[i] = pr.cv[i];
    RegSink<D, Y> ob;
    ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, OPT, RegSink<D, Y>>(pr.mf, L2, t, fo, cpo, ob) && ok;
    // ---- the innovation and its scores -------------------------------------------------------------------------------------
    double e[Y], S[Y * (Y + 1) / 2], nis, ll;
#pragma unroll
    for (int i = 0; i < Y; ++i) e[i] = yk[i] - ob.mf[i];
#pragma unroll
    for (int i = 0; i < Y * (Y + 1) / 2; ++i) S[i] = ob.cv[i];
    ok = innovation_score<Y>(Y, e, S, nis, ll) && ok;
    const double nan = __builtin_nan("");
    SSMQ_STORE(a.nis[(int64_t)k * ld + b], ok ? nis : nan);
    SSMQ_STORE(a.ll[(int64_t)k * ld + b], ok ? ll : nan);
    if (a.ymean) {
#pragma unroll
        for (int i = 0; i < Y; ++i) SSMQ_STORE(a.ymean[((int64_t)k * Y + i) * ld + b], ok ? ob.mf[i] : nan);
    }
    if (a.S) {
#pragma unroll
        for (int i = 0; i < Y; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const double v = ok ? ob.cv[SSMQ_PK(i, j)] : nan;   // both triangles from the one value
                SSMQ_STORE(a.S[((int64_t)k * Y * Y + i * Y + j) * ld + b], v);
                if (j != i) SSMQ_STORE(a.S[((int64_t)k * Y * Y + j * Y + i) * ld + b], v);
            }
    }
}

}  // namespace ssmq
