// Noise sweep of a Gaussian filter by measurement likelihood: k_noise_sweep<> keeps the WEIGHTS shared and varies what every filter
// has - the process-noise term G Q G', the measurement-noise covariance R and the initial moments - per row.  It runs the
// additive-noise Gaussian recursion of P rows on B measurement sequences in ONE launch and keeps of every item (p, b) only
//     loglik_total = sum_k log N(y_k; y^_k, S_k),   nis_mean = sum_k e_k' S_k^-1 e_k / T,   status
// (and, on request, the per-step log-likelihoods).  No filtered moment is stored.
//
// Mapping: that of k_filter_sweep<> - one lane per item, item index p * ld + b with ld a multiple of 64, so every wave belongs to
// ONE row.  What belongs to the row is wave-uniform and read by scalar loads through the constant address space:
//     gqg + p * gqg_stride [D*D],   rr + p * rr_stride [Y*Y],   x0 + p * x0_stride: m0 [D] | P0 [D*D] (lower triangle read).
// A stride of 0 is an array shared by all rows; the kernel does not branch on it.  The two constant blocks (const_layout(D, ., N,
// FORM): the blocks of two transform handles) are shared by all rows.  No LDS, no barrier, no cross-lane operation: nothing an item
// does depends on the items around it.
//
// Arithmetic: a step is what k_filter_sweep<> does, for every form of the fused time loop (FORM / TP: sigma-point, BQ, t-process BQ;
// tp_nu reaches CoreParams as fused_args() / fused_pass<> pass it) - the two moment_transform_core<> calls with the template
// arguments of the dense kernel of the form (OPT = 0), innovation_score<> (ssmq_innovation_kernel.h) on the predictive measurement
// moments, then the measurement update as gain_from_cov<> and sandwich<> (ssmq_device.h) define it.
//
// Failures: per lane, the rule of k_filter_sweep<>.  The first step j whose scores are not finite numbers (a factorisation failed -
// an indefinite Q, R or P0 row shows up here -, an input is not finite) sets status = 1 + j, the lane leaves the loop and its
// totals (and the remaining steps) are NaN.
//
// OWN COPY OF THE STEP, on purpose: this kernel does what score_rows_lane<> (ssmq_score_step.h) does for k_filter_sweep<> and
// k_filter_score<>, statement for statement, but keeps the statements here.  Routed through the shared function the outputs were
// bit-identical, yet six five-state instantiations gained 24 .. 48 bytes of scratch and three of them measured slower than before
// (reentry t-process N = 10: 0.191 / 0.194 ms against 0.181 / 0.182; coordinated turn GP N = 10 and 11: 1 %; profiles/README.md,
// r20).  A change to the step in ssmq_score_step.h has to be made here as well; tests/test_noise_sweep_gpu.py and
// tests/test_imm_gpu.py tie the two bit for bit (row = two-call path, IMM with one mode = row).
#pragma once
#include "ssmq_innovation_kernel.h"

namespace ssmq {

struct NoiseSweepArgs {
    const double *y;                   // [T][Y][ld]
    const double *c_dyn, *c_obs;       // const_layout(D, D, ND, FORM), const_layout(D, Y, NO, FORM): one block each, shared by all rows
    const double *gqg, *rr, *x0;       // row p at + p * stride: [D*D], [Y*Y], m0 [D] | P0 [D*D]
    int64_t gqg_stride, rr_stride, x0_stride;   // in doubles; 0: shared by all rows
    double *ll_total, *nis_mean;       // [P][ld]
    double *ll_steps;                  // [P][T][ld] or null
    int32_t *status;                   // [P][ld]
    int64_t B, ld;
    int32_t T, P, nblk;                // nblk = ld / 64: blocks per row
    int32_t emv_dyn, emv_obs;
    double nu_dyn, nu_obs;             // t-process form: the handles' tp_nu
    FPar fd, fo;                       // fd.ttab / fo.ttab: the time tables [T] of the integrands that have one
};

// Launch bounds: those of k_filter_fused<> for the same form and shape.
template <int D, int Y, int ND, int NO, int FD, int FO, int SELO, int FORM, int TP>
__global__ __launch_bounds__(kSmallBlock, (SSMQ_FUSED_FORCE_OCC ? SSMQ_FUSED_FORCE_OCC
                                           : (D >= 6 ? 1 : ((D >= 5 && FORM == SSMQ_FORM_SIGMA) ? SSMQ_FUSED_OCC_D5_SIGMA : 2)))) void k_noise_sweep(const NoiseSweepArgs a) {
    static_assert(FORM == SSMQ_FORM_BQ || (FORM == SSMQ_FORM_SIGMA && !TP), "k_noise_sweep: BQ form, or the sigma-point form without t-process");
    const int p = (int)(blockIdx.x / (uint32_t)a.nblk);                  // wave-uniform: the block's row
    const uint32_t b = (blockIdx.x - (uint32_t)p * (uint32_t)a.nblk) * kSmallBlock + threadIdx.x;
    if (p >= a.P || (int64_t)b >= a.B) return;
    const int64_t ld = a.ld, T = a.T;
    const int64_t item = (int64_t)p * ld + b;
    const double nan = __builtin_nan("");
    const CoreParams cpd{(cdouble_p)a.c_dyn, (cdouble_p)(a.gqg + (int64_t)p * a.gqg_stride), a.emv_dyn, a.nu_dyn, 1.0, 1.0};
    const CoreParams cpo{(cdouble_p)a.c_obs, (cdouble_p)(a.rr + (int64_t)p * a.rr_stride), a.emv_obs, a.nu_obs, 1.0, 1.0};
    const cdouble_p x0 = (cdouble_p)(a.x0 + (int64_t)p * a.x0_stride);
    double m[D], Pl[D * (D + 1) / 2];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = x0[d];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Pl[SSMQ_PK(i, j)] = x0[D + i * D + j];
    FPar fd = a.fd, fo = a.fo;
    int k = 0;
    int32_t st = 0;
    double sl = 0.0, sn = 0.0;
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
        // ---- time update: predictive state moments, + G Q_p G' ----------------------------------------------------------
        RegSinkNoCross<D, D> pr;
        ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, false, 0, RegSinkNoCross<D, D>>(m, Pl, t, fd, cpd, pr) && ok;
        // ---- predictive measurement moments at the prior, + R_p --------------------------------------------------------
        double L2[D * (D + 1) / 2];
#pragma unroll
        for (int i = 0; i < D * (D + 1) / 2; ++i) L2[i] = pr.cv[i];
        RegSink<D, Y> ob;
        ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, 0, RegSink<D, Y>>(pr.mf, L2, t, fo, cpo, ob) && ok;
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
