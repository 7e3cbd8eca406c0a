// Scoring recursion of the t-process and Studentian filters: k_filter_score<> runs score_rows_lane<> (ssmq_score_step.h) with
//   FORM   SSMQ_FORM_BQ (the t-process transforms) or SSMQ_FORM_SIGMA (the fully-symmetric rule of FullySymmetricStudent; one row),
//   TP     the t-process model variance (tp_nu and the iK block of const_layout), as the transform core has it for TP = 1,
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
// STU = 0: innovation_score<>'s Gaussian.
//
// Mapping: one lane per item, item index p * ld + b with ld a multiple of 64 - every wave belongs to ONE row.  What belongs to the row
// is wave-uniform and read by scalar loads through the constant address space: its two constant blocks ([P][const_layout(..).total]
// per transform; P = 1: the blocks of two transform handles) and its row block
//     nu_dyn | nu_obs | dof | lnorm | G q G' [D*D] | r [Y*Y] | m0 [D] | S0 [D*D] (lower triangle read) | scale [T]
// (score_row_doubles(); the three matrices scale with (dof - 2) / dof in the Studentian recursion, so they are the row's).
// A row whose weights failed (theta_status[p] != 0) gives status = -1 and NaN.
#pragma once
#include "ssmq_score_step.h"

namespace ssmq {

constexpr int kScoreRowHead = 4;   // nu_dyn | nu_obs | dof | lnorm
__host__ __device__ constexpr inline size_t score_row_doubles(int D, int Y, int T) {
    return ((size_t)kScoreRowHead + 2 * (size_t)D * D + (size_t)Y * Y + (size_t)D + (size_t)T + 1) / 2 * 2;
}

struct ScoreArgs : ScoreOut {
    const double *c_dyn, *c_obs;       // [P][const_layout(D, D, ND, FORM).total], [P][const_layout(D, Y, NO, FORM).total]
    const double *rows;                // [P][row_stride]: the row blocks
    const int32_t *theta_status;       // [P]: nonzero = that row's weights failed; null: no row has failed
    int64_t row_stride;
    int32_t P;                         // grid: (ld / 64 blocks per row, P rows), P <= 65 535
    int32_t emv_dyn, emv_obs;
};

template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int STU>
__global__ __launch_bounds__(kSmallBlock, 2) void k_filter_score(const ScoreArgs a) {
    static_assert(FORM == SSMQ_FORM_BQ || (FORM == SSMQ_FORM_SIGMA && !TP), "k_filter_score: BQ form, or the sigma-point form without t-process");
    const int p = (int)blockIdx.y;                                       // the block's row: a scalar register, no division
    const uint32_t b = blockIdx.x * kSmallBlock + threadIdx.x;
    if (p >= a.P || (int64_t)b >= a.B) return;
    constexpr ConstLayout cld = const_layout(D, D, ND, FORM), clo = const_layout(D, Y, NO, FORM);
    const cdouble_p r = (cdouble_p)(a.rows + (size_t)p * a.row_stride);
    const cdouble_p gqg = r + kScoreRowHead, rr = gqg + D * D, x0 = rr + Y * Y, ssc = x0 + D + D * D;
    const ScoreRow row{{(cdouble_p)(a.c_dyn + (size_t)p * cld.total), gqg, a.emv_dyn, TP ? r[0] : 0.0, 1.0, 1.0},
                       {(cdouble_p)(a.c_obs + (size_t)p * clo.total), rr, a.emv_obs, TP ? r[1] : 0.0, 1.0, 1.0},
                       x0, r[2], r[3], ssc};
    score_rows_lane<D, Y, ND, NO, FD, FO, FORM, TP, SELO, STU, true>(row, a, p, b, a.theta_status && a.theta_status[p] != 0 ? -1 : 0);
}

}  // namespace ssmq
