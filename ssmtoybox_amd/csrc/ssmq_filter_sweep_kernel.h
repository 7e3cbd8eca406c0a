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
// The recursion, its outputs and the failure rule are score_rows_lane<> (ssmq_score_step.h) with the dense BQ template arguments
// (FORM = SSMQ_FORM_BQ, TP = 0), the Gaussian score and no per-step NIS; this kernel says where row p's constants are.  A theta
// whose weights failed (theta_status[p] != 0) gives status = -1 and NaN.
#pragma once
#include "ssmq_score_step.h"

namespace ssmq {

struct SweepArgs : ScoreOut {
    const double *c_dyn, *c_obs;       // [P][const_layout(D, D, ND, BQ).total], [P][const_layout(D, Y, NO, BQ).total]
    const double *gqg, *rr;            // [D*D], [Y*Y]
    const double *x0;                  // m0 [D] | P0 [D*D] (lower triangle read): the same for every item
    const int32_t *theta_status;       // [P]: nonzero = that row's weights failed
    int32_t P, nblk;                   // nblk = ld / 64: blocks per theta
    int32_t emv_dyn, emv_obs;
};

// Launch bounds: those of k_filter_fused<> for the BQ form of the same shape.
template <int D, int Y, int ND, int NO, int FD, int FO, int SELO>
__global__ __launch_bounds__(kSmallBlock, (D >= 6 ? 1 : 2)) void k_filter_sweep(const SweepArgs a) {
    const int p = (int)(blockIdx.x / (uint32_t)a.nblk);                  // wave-uniform: the block's theta
    const uint32_t b = (blockIdx.x - (uint32_t)p * (uint32_t)a.nblk) * kSmallBlock + threadIdx.x;
    if (p >= a.P || (int64_t)b >= a.B) return;
    constexpr ConstLayout cld = const_layout(D, D, ND, SSMQ_FORM_BQ), clo = const_layout(D, Y, NO, SSMQ_FORM_BQ);
    const ScoreRow row{{(cdouble_p)(a.c_dyn + (size_t)p * cld.total), (cdouble_p)a.gqg, a.emv_dyn, 0.0, 1.0, 1.0},
                       {(cdouble_p)(a.c_obs + (size_t)p * clo.total), (cdouble_p)a.rr, a.emv_obs, 0.0, 1.0, 1.0},
                       (cdouble_p)a.x0, 0.0, 0.0, nullptr};
    score_rows_lane<D, Y, ND, NO, FD, FO, SSMQ_FORM_BQ, 0, SELO, 0, false>(row, a, p, b, a.theta_status[p] != 0 ? -1 : 0);
}

}  // namespace ssmq
