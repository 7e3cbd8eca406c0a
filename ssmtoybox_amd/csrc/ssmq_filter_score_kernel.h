// Scoring recursion of the t-process and Studentian filters: k_filter_score<> is k_filter_sweep<> (ssmq_filter_sweep_kernel.h) with the
// three things that kernel fixes made template arguments -
//   FORM   SSMQ_FORM_BQ (the t-process transforms) or SSMQ_FORM_SIGMA (the fully-symmetric rule of FullySymmetricStudent; one row),
//   TP     the t-process model variance (tp_nu and the iK block of const_layout), as moment_transform_core<.., TP = 1, ..> has it,
//   STU    the Studentian recursion: the transformed covariances become scale matrices (cov_scale / ccov_scale from the row's scale
//          table), the update factor sc2 = (dof + nis) / (dof + Y) carries the scale to the next step's Cholesky - what fused_pass<>
//          (ssmq_filter_fused_kernel.h) does with a.sscale / a.student_dof - and the score is the Student-t density below.
// It runs the recursion of P parameter rows on B measurement sequences in ONE launch and keeps of every item (p, b) only
//     loglik_total = sum_k ll_k,   nis_mean = sum_k nis_k / T,   status
// (and, on request, the per-step ll_k and nis_k).  No filtered moment is stored.
//
// The score of step k.  The Studentian update with the factor (dof + Delta^2) / (dof + Y) is the conditional of a joint Student t with
// `dof` degrees of freedom and the scale blocks S_x, S_yx, S_y = sc_k P_y + r_smat; the marginal of y_k under the same joint is
// t_dof(y_mean, S_y), so with e = y_k - y_mean and Delta^2 = e' S_y^-1 e
//     nis_k = Delta^2                                                          (expected value: Y dof / (dof - 2))
//     ll_k  = lgamma((dof + Y) / 2) - lgamma(dof / 2) - Y / 2 log(dof pi)  -  1/2 log det S_y  -  (dof + Y) / 2 log1p(Delta^2 / dof).
// dof is the FILTER's dof - the one in the update factor -, not dof_pr of the scale sequence.  The three constant terms are one number
// per (dof, Y) from the host (lnorm); the log-determinant comes from the Cholesky pivots innovation_score<> leaves in S.
// STU = 0: innovation_score<>'s Gaussian, as k_filter_sweep<>.
//
// Mapping: one lane per item, item index p * ld + b with ld a multiple of 64 - every wave belongs to ONE row.  What belongs to the row
// is wave-uniform and read by scalar loads through the constant address space: its two constant blocks ([P][const_layout(..).total]
// per transform; P = 1: the blocks of two transform handles) and its row block
//     nu_dyn | nu_obs | dof | lnorm | G q G' [D*D] | r [Y*Y] | m0 [D] | S0 [D*D] (lower triangle read) | scale [T]
// (score_row_doubles(); the three matrices scale with (dof - 2) / dof in the Studentian recursion, so they are the row's).
// No LDS, no barrier, no cross-lane operation: nothing an item does depends on the items around it.
//
// Arithmetic: a step is the two moment_transform_core<> calls of fused_pass<> (OPT = 0), innovation_score<> (ssmq_innovation_kernel.h)
// on the predictive measurement moments, then the update as gain_from_cov<> and sandwich<> (ssmq_device.h) define it.  Nothing of it
// is restated here.  Failures: as k_filter_sweep<> - the first step j whose scores are not finite numbers sets status = 1 + j, the
// lane leaves the loop and its totals (and the remaining steps) are NaN; a row whose weights failed gives status = -1 and NaN.
#pragma once
#include "ssmq_innovation_kernel.h"

namespace ssmq {

constexpr int kScoreRowHead = 4;   // nu_dyn | nu_obs | dof | lnorm
__host__ __device__ constexpr inline size_t score_row_doubles(int D, int Y, int T) {
    return ((size_t)kScoreRowHead + 2 * (size_t)D * D + (size_t)Y * Y + (size_t)D + (size_t)T + 1) / 2 * 2;
}

struct ScoreArgs {
    const double *y;                   // [T][Y][ld]
    const double *c_dyn, *c_obs;       // [P][const_layout(D, D, ND, FORM).total], [P][const_layout(D, Y, NO, FORM).total]
    const double *rows;                // [P][row_stride]: the row blocks
    const int32_t *theta_status;       // [P]: nonzero = that row's weights failed; null: no row has failed
    double *ll_total, *nis_mean;       // [P][ld]
    double *ll_steps, *nis_steps;      // [P][T][ld] or null
    int32_t *status;                   // [P][ld]
    int64_t B, ld, row_stride;
    int32_t T, P;                      // grid: (ld / 64 blocks per row, P rows), P <= 65 535
    int32_t emv_dyn, emv_obs;
    FPar fd, fo;                       // fd.ttab / fo.ttab: the time tables [T] of the integrands that have one
};

template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int STU>
__global__ __launch_bounds__(kSmallBlock, 2) void k_filter_score(const ScoreArgs a) {
    static_assert(FORM == SSMQ_FORM_BQ || (FORM == SSMQ_FORM_SIGMA && !TP), "k_filter_score: BQ form, or the sigma-point form without t-process");
    const int p = (int)blockIdx.y;                                       // the block's row: a scalar register, no division
    const uint32_t b = blockIdx.x * kSmallBlock + threadIdx.x;
    if (p >= a.P || (int64_t)b >= a.B) return;
    const int64_t ld = a.ld, T = a.T;
    const int64_t item = (int64_t)p * ld + b;
    const double nan = __builtin_nan("");
    int k = 0;
    int32_t st = 0;
    double sl = 0.0, sn = 0.0;
    if (a.theta_status && a.theta_status[p] != 0) {
        st = -1;
    } else {
        constexpr ConstLayout cld = const_layout(D, D, ND, FORM), clo = const_layout(D, Y, NO, FORM);
        const cdouble_p row = (cdouble_p)(a.rows + (size_t)p * a.row_stride);
        const cdouble_p gqg = row + kScoreRowHead, rr = gqg + D * D, x0 = rr + Y * Y, ssc = x0 + D + D * D;
        CoreParams cpd{(cdouble_p)(a.c_dyn + (size_t)p * cld.total), gqg, a.emv_dyn, TP ? row[0] : 0.0, 1.0, 1.0};
        CoreParams cpo{(cdouble_p)(a.c_obs + (size_t)p * clo.total), rr, a.emv_obs, TP ? row[1] : 0.0, 1.0, 1.0};
        const double dof = row[2], lnorm = row[3];
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
            if constexpr (STU) {   // transformed covariances become scale matrices before the noise term (ssinf.py:672-693)
                const double sc = ssc[k];
                cpd.cov_scale = sc;
                cpo.cov_scale = sc;
                cpo.ccov_scale = sc;
            }
            bool ok = true;
#pragma unroll
            for (int d = 0; d < D; ++d) ok = ok && (m[d] == m[d]);
            // ---- time update: predictive state moments, + G Q G' ------------------------------------------------------------
            RegSinkNoCross<D, D> pr;
            ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, false, 0, RegSinkNoCross<D, D>>(m, Pl, t, fd, cpd, pr) && ok;
            // ---- predictive measurement moments at the prior, + R ----------------------------------------------------------
            double L2[D * (D + 1) / 2];
#pragma unroll
            for (int i = 0; i < D * (D + 1) / 2; ++i) L2[i] = pr.cv[i];
            RegSink<D, Y> ob;
            ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, 0, RegSink<D, Y>>(pr.mf, L2, t, fo, cpo, ob) && ok;
            // ---- the innovation and its scores ------------------------------------------------------------------------------
            double e[Y], S[Y * (Y + 1) / 2], nis, ll;
#pragma unroll
            for (int i = 0; i < Y; ++i) e[i] = yk[i] - ob.mf[i];
#pragma unroll
            for (int i = 0; i < Y * (Y + 1) / 2; ++i) S[i] = ob.cv[i];
            ok = innovation_score<Y>(Y, e, S, nis, ll) && ok;   // S: now the Cholesky factor of S_y
            if constexpr (STU) {
                double lg = 0.0;                                // log det S_y / 2 from the pivots, in innovation_score<>'s order
#pragma unroll
                for (int j = 0; j < Y; ++j) lg += log(S[SSMQ_PK(j, j)]);
                ll = lnorm - lg - 0.5 * (dof + (double)Y) * log1p(nis / dof);
            }
            if (!(ok && nis == nis && ll == ll)) {   // the first step with NaN scores
                st = k + 1;
                break;
            }
            if (a.ll_steps) SSMQ_STORE(a.ll_steps[((int64_t)p * T + k) * ld + b], ll);
            if (a.nis_steps) SSMQ_STORE(a.nis_steps[((int64_t)p * T + k) * ld + b], nis);
            sl += ll;
            sn += nis;
            // ---- measurement update; Studentian: the next scale matrix is (dof + nis) / (dof + Y) times the Kalman-form one ----
            double sc2 = 1.0;
            if constexpr (STU) sc2 = (dof + nis) / (dof + (double)Y);
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
    }
    if (st != 0) {
        sl = sn = nan;
        for (; k < a.T; ++k) {
            if (a.ll_steps) SSMQ_STORE(a.ll_steps[((int64_t)p * T + k) * ld + b], nan);
            if (a.nis_steps) SSMQ_STORE(a.nis_steps[((int64_t)p * T + k) * ld + b], nan);
        }
    }
    a.ll_total[item] = sl;
    a.nis_mean[item] = st != 0 ? nan : sn / (double)a.T;
    a.status[item] = st;
}

}  // namespace ssmq
