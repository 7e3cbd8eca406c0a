// The fused filter time loop by TIME BLOCKS, for the host-array entry point (round 6; ssmq_filter_forward_piped in ssmq_api_study.hip).
//
// forward_pass takes the measurements as a host array and returns host arrays (ssinf.py:66-118).  At BASELINE configs[1] that is
// 8 MB up and 16 MB down around a 34 us kernel: 1.15 ms per call when upload, pass and downloads run back to back.  Here the pass is
// cut into K time blocks; k_filter_range runs the steps [kb, ke) of EVERY trajectory from the state the previous block's launch left
// in the hand-over buffer (the mechanism of the strip schedule, ssmq_filter_chunked.hip: mean, covariance triangle and status word
// as the registers held them, so the filtered moments are the whole-pass kernel's BITS), which lets the host feed block k + 1 and
// drain block k - 1 over PCIe while block k runs.  Launch boundaries order the hand-over; no flags, no spinning.
#include <cstring>
#include "ssmq_filter_fused_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {
namespace {

template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT, int STU>
__global__ __launch_bounds__(kSmallBlock, (D >= 6 ? 1 : ((D >= 5 && FORM == SSMQ_FORM_SIGMA) ? SSMQ_FUSED_OCC_D5_SIGMA : 2))) void k_filter_range(
    const FusedArgs a, int kb, int ke) {
    if ((int)threadIdx.x >= a.lpw) return;
    fused_pass<D, Y, ND, NO, FD, FO, FORM, TP, SELO, OPT, STU, true>(a, blockIdx.x, kb, ke, kb == 0, ke == a.T);
}

typedef void (*range_kernel)(const FusedArgs, int, int);
struct RangeEntry {
    FilterShape shape;
    range_kernel k;
    const char *name;
};
// STU as the whole-pass kernel of the shape has it for the Gaussian recursion (0 for the scalar models, -1 decided at run time for
// the others): another value contracts other products into multiply-adds and the last bits differ.
#define SSMQ_RG_ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                                                  \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT}, &k_filter_range<D, Y, N, N, FD, FO, FORM, TP, SELO, OPT, (D == 1 ? 0 : -1)>, \
     "k_filter_range<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO "," #FORM ",TP=" #TP ",SELO=" #SELO ",OPT=" #OPT ">"}
// the scalar UNGM filters and the reentry / coordinated-turn shapes of configs[2] and configs[3] with unscented points
const RangeEntry kRange[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, SSMQ_RG_ONE),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE_FAST, SSMQ_RG_ONE),
};

}  // namespace

// Doubles of hand-over state per block of 64 trajectories (FusedArgs::hand).
size_t range_hand_doubles(int D) { return ((size_t)D + (size_t)D * (D + 1) / 2 + 1) * 64; }

// 1: the steps [kb, ke) were queued on p.s (dry_run: a kernel exists); 0: no range kernel for this combination; < 0: error.
// The selection rule of try_launch_fused (opt_preference), Gaussian recursion only.
// `hand`: range_hand_doubles(D) doubles per block of 64 trajectories.
int try_launch_range(const FilterPass &p, int kb, int ke, double *hand) {
    if (!same_family(p)) return 0;
    for (const int opt : opt_preference(p.hd, p.ho))
        for (const RangeEntry &e : kRange) {
            if (opt < 0) break;
            if (!(e.shape == shape_of(p, opt))) continue;
            if (has_time_table(p.fd->id) && !p.ttab_dyn && !p.dry_run) return 0;      // the kernels read the table
            if (p.name) *p.name = e.name;
            if (p.dry_run) return 1;
            if (kb < 0 || ke > p.T || kb >= ke) return SSMQ_E_ARG;
            FusedArgs a = fused_args(p);
            a.sscale = nullptr; a.student_dof = 0.0;      // Gaussian recursion only (the larger shapes decide it at run time)
            a.hand = hand;                                // the state a block of steps leaves for the next launch
            hipLaunchKernelGGL(e.k, dim3((unsigned)((p.B + 63) / 64)), dim3(kSmallBlock), 0, p.s, a, kb, ke);
            const int rc = hip_fail(hipGetLastError(), e.name);
            return rc ? rc : 1;
        }
    return 0;
}

}  // namespace ssmq
