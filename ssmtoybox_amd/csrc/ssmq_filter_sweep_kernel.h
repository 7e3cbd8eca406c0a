// Kernel-parameter sweep of a BQ filter by measurement likelihood: k_filter_sweep<> runs the additive-noise Gaussian recursion of
// P parameter rows ("theta") on B measurement sequences in ONE launch and keeps of every item (p, b) only
//     loglik_total = sum_k log N(y_k; y^_k, S_k),   nis_mean = sum_k e_k' S_k^-1 e_k / T,   status
// (and, on request, the per-step log-likelihoods).  No filtered moment is stored.
//
// Mapping: one lane per item, item index p * ld + b with ld a multiple of 64 - every wave belongs to ONE theta, so the base of
// that theta's constant block (const_layout, the dense part: xi, wm, Wc', Wcc, emv, zero) is wave-uniform and the weights are
// read as the fused time loop reads them: scalar loads through the constant address space, served by the scalar cache.  The
// blocks sit side by side in HBM, [P][const_layout(..).total] per transform (ssmq_api_sweep.hip builds them from one
// theta-batched weights call per transform).
//
// Arithmetic: a step is the two moment_transform_core<> calls of fused_pass<> / k_innovation<> with the dense BQ template
// arguments (FORM = SSMQ_FORM_BQ, TP = 0, OPT = 0), innovation_score<> (ssmq_innovation_kernel.h) on the predictive measurement
// moments, then the measurement update as gain_from_cov<> and sandwich<> (ssmq_device.h) define it - the sums fused_pass<> writes
// out.  Nothing of it is restated here.
//
// Failures: per lane.  The first step j whose scores are not finite numbers (a factorisation failed, an input is not finite)
// sets status = 1 + j, the lane leaves the loop and its totals (and the remaining steps) are NaN; a theta whose weights failed
// (theta_status[p] != 0) gives status = -1 and NaN.  No barrier, no LDS, no cross-lane operation: nothing an item does depends
// on the items around it.
#pragma once
#include "ssmq_innovation_kernel.h"

namespace ssmq {

struct SweepArgs {
    const double *y;                   // [T][Y][ld]
    const double *c_dyn, *c_obs;       // [P][const_layout(D, D, ND, BQ).total], [P][const_layout(D, Y, NO, BQ).total]
    const double *gqg, *rr;            // [D*D], [Y*Y]
    const double *x0;                  // m0 [D] | P0 [D*D] (lower triangle read): the same for every item
    const int32_t *theta_status;       // [P]: nonzero = that row's weights failed
    double *ll_total, *nis_mean;       // [P][ld]
    double *ll_steps;                  // [P][T][ld] or null
    int32_t *status;                   // [P][ld]
    int64_t B, ld;
    int32_t T, P, nblk;                // nblk = ld / 64: blocks per theta
    int32_t emv_dyn, emv_obs;
    FPar fd, fo;                       // fd.ttab / fo.ttab: the time tables [T] of the integrands that have one
};

// Launch bounds: those of k_filter_fused<> for the BQ form of the same shape.
template <int D, int Y, int ND, int NO, int FD, int FO, int SELO>
__global__ __launch_bounds__(kSmallBlock, (D >= 6 ? 1 : 2)) void k_filter_sweep(const SweepArgs a) {
    const int p = (int)(blockIdx.x / (uint32_t)a.nblk);                  // wave-uniform: the block's theta
    const uint32_t b = (blockIdx.x - (uint32_t)p * (uint32_t)a.nblk) * kSmallBlock + threadIdx.x;
    if (p >= a.P || (int64_t)b >= a.B) return;
    const int64_t ld = a.ld, T = a.T;
    const int64_t item = (int64_t)p * ld + b;
    const double nan = __builtin_nan("");
    int k = 0;
    int32_t st = 0;
    double sl = 0.0, sn = 0.0;
    if (a.theta_status[p] != 0) {
        st = -1;
    } else {
        constexpr ConstLayout cld = const_layout(D, D, ND, SSMQ_FORM_BQ), clo = const_layout(D, Y, NO, SSMQ_FORM_BQ);
        const CoreParams cpd{(cdouble_p)(a.c_dyn + (size_t)p * cld.total), (cdouble_p)a.gqg, a.emv_dyn, 0.0, 1.0, 1.0};
        const CoreParams cpo{(cdouble_p)(a.c_obs + (size_t)p * clo.total), (cdouble_p)a.rr, a.emv_obs, 0.0, 1.0, 1.0};
        const cdouble_p x0 = (cdouble_p)a.x0;
        double m[D], Pl[D * (D + 1) / 2];
#pragma unroll
        for (int d = 0; d < D; ++d) m[d] = x0[d];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) Pl[SSMQ_PK(i, j)] = x0[D + i * D + j];
        FPar fd = a.fd, fo = a.fo;
#pragma unroll 1
        for (; k < a.T; ++k) {
            double yk[Y];
#pragma unroll
            for (int i = 0; i < Y; ++i) yk[i] = a.y[((int64_t)k * Y + i) * ld + b];
            const double t = (double)k;   // both transforms of step k + 1 use time index k (ssinf.py:104, 276-288)
            if constexpr (HasTimeTable<FD>::value) { fd.tval = ((cdouble_p)a.fd.ttab)[k]; fd.use_tval = 1; }   // host: non-null
            if constexpr (HasTimeTable<FO>::value) { fo.tval = ((cdouble_p)a.fo.ttab)[k]; fo.use_tval = 1; }
            bool ok = true;
#pragma unroll
            for (int d = 0; d < D; ++d) ok = ok && (m[d] == m[d]);
            // ---- time update: predictive state moments, + G Q G' ------------------------------------------------------------
            RegSinkNoCross<D, D> pr;
            ok = moment_transform_core<D, D, ND, FD, SSMQ_FORM_BQ, 0, 0, false, 0, RegSinkNoCross<D, D>>(m, Pl, t, fd, cpd, pr) && ok;
            // ---- predictive measurement moments at the prior, + R ----------------------------------------------------------
            double L2[D * (D + 1) / 2];
#pragma unroll
            for (int i = 0; i < D * (D + 1) / 2; ++i) L2[i] = pr.cv[i];
            RegSink<D, Y> ob;
            ok = moment_transform_core<D, Y, NO, FO, SSMQ_FORM_BQ, 0, SELO, true, 0, RegSink<D, Y>>(pr.mf, L2, t, fo, cpo, ob) && ok;
            // ---- the innovation and its scores, as k_innovation<> ------------------------------------------------------------
            double e[Y], S[Y * (Y + 1) / 2], nis, ll;
#pragma unroll
            for (int i = 0; i < Y; ++i) e[i] = yk[i] - ob.mf[i];
#pragma unroll
            for (int i = 0; i < Y * (Y + 1) / 2; ++i) S[i] = ob.cv[i];
            ok = innovation_score<Y>(Y, e, S, nis, ll) && ok;
            if (!(ok && nis == nis && ll == ll)) {   // what k_innovation_total's scan finds: the first step with NaN scores
                st = k + 1;
                break;
            }
            if (a.ll_steps) SSMQ_STORE(a.ll_steps[((int64_t)p * T + k) * ld + b], ll);
            sl += ll;
            sn += nis;
            // ---- measurement update: the sums of fused_pass<> ---------------------------------------------------------------
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
                               if (d2 <= d) Pl[SSMQ_PK(d, d2)] = pr.cv[SSMQ_PK(d, d2)] - s;   // the lower triangle: what the next step reads
                           });
        }
    }
    if (st != 0) {
        sl = sn = nan;
        if (a.ll_steps)
            for (; k < a.T; ++k) SSMQ_STORE(a.ll_steps[((int64_t)p * T + k) * ld + b], nan);
    }
    a.ll_total[item] = sl;
    a.nis_mean[item] = st != 0 ? nan : sn / (double)a.T;
    a.status[item] = st;
}

}  // namespace ssmq
