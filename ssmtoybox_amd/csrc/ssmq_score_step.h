// The filter step of the likelihood-scoring kernels, once: one lane runs one additive-noise Gaussian (or Studentian) recursion and
// keeps scores, no filtered moment.  A step is
//     predict_and_score<>     the two moment_transform_core<> calls of fused_pass<> (ssmq_filter_fused_kernel.h) - predictive state
//                             moments + G Q G', predictive measurement moments at the prior + R - and innovation_score<>
//                             (ssmq_innovation_kernel.h) on e = y_k - y^_k, S_k -> nis_k, ll_k
//     kalman_update_lower<>   the measurement update as gain_from_cov<> and sandwich<> (ssmq_device.h) define it - the sums
//                             fused_pass<> writes out -, into the mean and the lower triangle the next step reads
// and what calls them:
//     k_innovation<>          predict_and_score<> on stored moments, one (step, trajectory) per lane (below)
//     k_imm_loop<>            both halves per mode, between its barriers (ssmq_imm_kernel.h)
//     score_rows_lane<>       the whole recursion of item (p, b) of the row kernels k_filter_sweep<> and k_filter_score<>, which
//                             differ in where a row's constants come from (ScoreRow); k_noise_sweep<> runs the same statements
//                             from a copy of its own (ssmq_noise_sweep_kernel.h says why): a change here is a change there
// predict_and_score<>, kalman_update_lower<>, step_inputs<> and load_x0<> hold no break, no return out of a loop and no barrier:
// k_imm_loop<> depends on it.
//
// Failures of a row item, per lane: the first step j whose scores are not finite numbers (a factorisation failed, an input is not
// finite) sets status = 1 + j, the lane leaves the loop and its totals (and the remaining steps) are NaN; a row whose weights failed
// (st0 = -1) gives status = -1 and NaN.  No LDS, no cross-lane operation: nothing an item does depends on the items around it.
#pragma once
#include "ssmq_innovation_kernel.h"

namespace ssmq {

// What the argument structs of the row kernels share: item (p, b) is measurement sequence b under row p, index p * ld + b.
struct ScoreOut {
    const double *y;                   // [T][Y][ld]
    double *ll_total, *nis_mean;       // [P][ld]
    double *ll_steps, *nis_steps;      // [P][T][ld] or null (nis_steps: k_filter_score<> only)
    int32_t *status;                   // [P][ld]
    int64_t B, ld;
    int32_t T;
    FPar fd, fo;                       // fd.ttab / fo.ttab: the time tables [T] of the integrands that have one
};

// What belongs to a row: wave-uniform, read by scalar loads through the constant address space.
struct ScoreRow {
    CoreParams cpd, cpo;               // constant block, noise term, emv mode and tp_nu of either transform; the scales 1.0
    cdouble_p x0;                      // m0 [D] | P0 [D*D] (lower triangle read)
    double dof, lnorm;                 // Studentian recursion: the filter's dof, the constant of the Student-t density
    cdouble_p ssc;                     // Studentian recursion: scale [T]
};

template <int D>
__device__ __forceinline__ void load_x0(cdouble_p x0, double (&m)[D], double (&Pl)[D * (D + 1) / 2]) {
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = x0[d];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Pl[SSMQ_PK(i, j)] = x0[D + i * D + j];
}

// The measurement of step k and, for the integrands that have a time table (host: non-null), its entry.
template <int Y, int FD, int FO>
__device__ __forceinline__ void step_inputs(const double *y, int k, int64_t ld, int64_t b, double (&yk)[Y], FPar &fd, FPar &fo) {
#pragma unroll
    for (int i = 0; i < Y; ++i) yk[i] = y[((int64_t)k * Y + i) * ld + b];
    if constexpr (HasTimeTable<FD>::value) { fd.tval = ((cdouble_p)fd.ttab)[k]; fd.use_tval = 1; }
    if constexpr (HasTimeTable<FO>::value) { fo.tval = ((cdouble_p)fo.ttab)[k]; fo.use_tval = 1; }
}

// m, Pl: in = the moments the step starts from, Pl out = its Cholesky factor.  pr / ob: the predictive state and measurement
// moments; S: out = the Cholesky factor of ob.cv (the Studentian score reads its pivots).  Returns whether both transforms and the
// factorisation of S succeeded; the caller ands its own "the step started from finite moments" to it.
template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT>
__device__ __forceinline__ bool predict_and_score(const double (&m)[D], double (&Pl)[D * (D + 1) / 2], double t, const FPar &fd, const FPar &fo,
                                                  const CoreParams &cpd, const CoreParams &cpo, const double (&yk)[Y], RegSinkNoCross<D, D> &pr,
                                                  RegSink<D, Y> &ob, double (&S)[Y * (Y + 1) / 2], double &nis, double &ll) {
    // ---- time update: predictive state moments, + G Q G' (ssinf.py:276-279) --------------------------------------------------
    bool ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, false, OPT, RegSinkNoCross<D, D>>(m, Pl, t, fd, cpd, pr);
    // ---- predictive measurement moments at the prior, + R (ssinf.py:287-291) -------------------------------------------------
    double L2[D * (D + 1) / 2];
#pragma unroll
    for (int i = 0; i < D * (D + 1) / 2; ++i) L2[i] = pr.cv[i];
    ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, OPT, RegSink<D, Y>>(pr.mf, L2, t, fo, cpo, ob) && ok;
    // ---- the innovation and its scores ---------------------------------------------------------------------------------------
    double e[Y];
#pragma unroll
    for (int i = 0; i < Y; ++i) e[i] = yk[i] - ob.mf[i];
#pragma unroll
    for (int i = 0; i < Y * (Y + 1) / 2; ++i) S[i] = ob.cv[i];
    return innovation_score<Y>(Y, e, S, nis, ll) && ok;
}

// k_innovation<>: predict_and_score<> on the filtered moments a pass left in HBM (InnovArgs, ssmq_innovation_kernel.h).
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
    RegSinkNoCross<D, D> pr;
    RegSink<D, Y> ob;
    double S[Y * (Y + 1) / 2], nis, ll;
    ok = predict_and_score<D, Y, ND, NO, FD, FO, FORM, TP, SELO, OPT>(m, Pl, t, fd, fo, cpd, cpo, yk, pr, ob, S, nis, ll) && ok;
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

// The measurement update from the moments predict_and_score<> left.  STU: the next scale matrix is sc2 = (dof + nis) / (dof + Y)
// times the Kalman-form one.
template <int D, int Y, int STU>
__device__ __forceinline__ void kalman_update_lower(const RegSinkNoCross<D, D> &pr, const RegSink<D, Y> &ob, const double (&yk)[Y], double sc2,
                                                    double (&m)[D], double (&Pl)[D * (D + 1) / 2]) {
    double S[Y * (Y + 1) / 2];
#pragma unroll
    for (int i = 0; i < Y * (Y + 1) / 2; ++i) S[i] = ob.cv[i];
    double G[D][Y];
    gain_from_cov<D, Y>(S, [&](int i, int d) { return ob.cx[i][d]; }, G);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < Y; ++i) s += G[d][i] * (yk[i] - ob.mf[i]);
        m[d] = pr.mf[d] + s;
    }
    sandwich<D, Y>(G, [&](int i, int j) { return ob.cv[i >= j ? SSMQ_PK(i, j) : SSMQ_PK(j, i)]; },
                   [&](int d, int d2, double s) {
                       if (d2 <= d) {   // the lower triangle: what the next step reads
                           const double q = pr.cv[SSMQ_PK(d, d2)] - s;
                           Pl[SSMQ_PK(d, d2)] = STU ? sc2 * q : q;
                       }
                   });
}

// The recursion of item (p, b) and its outputs.  st0: 0, or -1 for a row whose weights failed (no step runs).  STU: the Studentian
// recursion - the transformed covariances become scale matrices (cov_scale / ccov_scale from the row's scale table) before the noise
// term (ssinf.py:672-693), the score is the Student-t density
//     ll_k = lnorm - 1/2 log det S_y - (dof + Y) / 2 log1p(nis_k / dof),
// the log-determinant from the pivots in innovation_score<>'s order.  NISS: the kernel has per-step NIS planes (o.nis_steps or null).
template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int STU, bool NISS>
__device__ __forceinline__ void score_rows_lane(const ScoreRow &row, const ScoreOut &o, int p, uint32_t b, int32_t st0) {
    const int64_t ld = o.ld, T = o.T;
    const int64_t item = (int64_t)p * ld + b;
    const double nan = __builtin_nan("");
    int k = 0;
    int32_t st = st0;
    double sl = 0.0, sn = 0.0;
    if (st == 0) {
        CoreParams cpd = row.cpd, cpo = row.cpo;
        double m[D], Pl[D * (D + 1) / 2];
        load_x0<D>(row.x0, m, Pl);
        FPar fd = o.fd, fo = o.fo;
#pragma unroll 1
        for (; k < o.T; ++k) {
            double yk[Y];
            step_inputs<Y, FD, FO>(o.y, k, ld, b, yk, fd, fo);
            const double t = (double)k;   // both transforms of step k + 1 use time index k (ssinf.py:104, 276-288)
            if constexpr (STU) {
                const double sc = row.ssc[k];
                cpd.cov_scale = sc;
                cpo.cov_scale = sc;
                cpo.ccov_scale = sc;
            }
            bool ok = true;
#pragma unroll
            for (int d = 0; d < D; ++d) ok = ok && (m[d] == m[d]);
            RegSinkNoCross<D, D> pr;
            RegSink<D, Y> ob;
            double S[Y * (Y + 1) / 2], nis, ll;
            ok = predict_and_score<D, Y, ND, NO, FD, FO, FORM, TP, SELO, 0>(m, Pl, t, fd, fo, cpd, cpo, yk, pr, ob, S, nis, ll) && ok;
            if constexpr (STU) {
                double lg = 0.0;
#pragma unroll
                for (int j = 0; j < Y; ++j) lg += log(S[SSMQ_PK(j, j)]);
                ll = row.lnorm - lg - 0.5 * (row.dof + (double)Y) * log1p(nis / row.dof);
            }
            if (!(ok && nis == nis && ll == ll)) {   // what k_innovation_total's scan finds: the first step with NaN scores
                st = k + 1;
                break;
            }
            if (o.ll_steps) SSMQ_STORE(o.ll_steps[((int64_t)p * T + k) * ld + b], ll);
            if constexpr (NISS)
                if (o.nis_steps) SSMQ_STORE(o.nis_steps[((int64_t)p * T + k) * ld + b], nis);
            sl += ll;
            sn += nis;
            double sc2 = 1.0;
            if constexpr (STU) sc2 = (row.dof + nis) / (row.dof + (double)Y);
            kalman_update_lower<D, Y, STU>(pr, ob, yk, sc2, m, Pl);
        }
    }
    if (st != 0) {
        sl = sn = nan;
        for (; k < o.T; ++k) {
            if (o.ll_steps) SSMQ_STORE(o.ll_steps[((int64_t)p * T + k) * ld + b], nan);
            if constexpr (NISS)
                if (o.nis_steps) SSMQ_STORE(o.nis_steps[((int64_t)p * T + k) * ld + b], nan);
        }
    }
    o.ll_total[item] = sl;
    o.nis_mean[item] = st != 0 ? nan : sn / (double)o.T;
    o.status[item] = st;
}

}  // namespace ssmq
