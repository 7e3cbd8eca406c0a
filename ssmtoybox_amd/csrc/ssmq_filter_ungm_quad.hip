// The scalar UNGM filter pass (BQ form, Gaussian recursion: GPQ-Kalman and the other BQ filters of SSMQ_SHAPES_UNGM; the headline,
// BASELINE configs[1]) with ONE TRAJECTORY ON THE FOUR LANES OF A QUAD, for batches whose waves each sit alone on a SIMD.  Such a
// wave is bound by the instructions it issues per step, and the one piece of a step that does the same work once per sigma point
// is the dynamics integrand x / 2 + 25 x / (1 + x^2) + 8 cos(1.2 k): ten instructions and a reciprocal per point.  Here lane q of a
// quad evaluates it at point q alone and the N values are broadcast to the quad (`v_mov_b32_dpp quad_perm:[n,n,n,n]`, two per
// double); from there every lane runs the sums, the measurement transform and the update of the one-lane kernel on a replicated
// state - fused_pass<..., QUAD = true> (ssmq_filter_fused_kernel.h), QuadScalarPoints (ssmq_quad.h).  No partial sums, no
// all-reduce: every value comes from the same operations in the same order as in k_filter_fused<1, 1, N, N, ..., OPT = 0, STU = 0>,
// so the results are the same bits (tests/test_ungm_quad_gpu.py).  All four lanes issue the step's two stores - same address, same
// bits: a store block predicated on the lane would end each step in a branch.  16 trajectories per wave: four times the waves of
// the one-lane kernel, taken while they still have a SIMD each (try_launch_quad).
#include "ssmq_filter_fused_kernel.h"

namespace ssmq {
namespace {

template <int N>
__global__ __launch_bounds__(kSmallBlock, 2) void k_filter_ungm_quad(const FusedArgs a) {
    fused_pass<1, 1, N, N, SSMQ_F_UNGM_DYN, SSMQ_F_UNGM_MEAS, SSMQ_FORM_BQ, 0, 0, 0, 0, false, true>(a, blockIdx.x, 0, a.T, true, true);
}

typedef void (*ungm_quad_kernel)(const FusedArgs);
struct UngmQuadEntry {
    int N;
    ungm_quad_kernel k;
    const char *name;
};
#define SSMQ_UQ(N) {N, &k_filter_ungm_quad<N>, "k_filter_ungm_quad<N=" #N ",SSMQ_FORM_BQ,TP=0>"}
const UngmQuadEntry kUngmQuad[] = {SSMQ_UQ(2), SSMQ_UQ(3), SSMQ_UQ(5)};

}  // namespace

// try_launch_quad's entry for the scalar UNGM shapes (its switches and its bound on the batch have been applied; the pass is
// Gaussian and same_family): 1 launched on `waves` blocks (dry_run: would be), 0 not this shape family, < 0 error.
int try_launch_ungm_quad(const FilterPass &p, int64_t waves) {
    const ssmq_transform *hd = p.hd, *ho = p.ho;
    if (p.fd->id != SSMQ_F_UNGM_DYN || p.fo->id != SSMQ_F_UNGM_MEAS || hd->D != 1 || hd->E != 1 || ho->D != 1 || ho->E != 1) return 0;
    if (hd->form != SSMQ_FORM_BQ || hd->tp_nu > 0.0 || ho->N != hd->N || p.sel_obs != 0) return 0;
    if (!p.ttab_dyn && !p.dry_run) return 0;          // the kernels read the time table
    for (const UngmQuadEntry &e : kUngmQuad) {
        if (e.N != hd->N) continue;
        if (p.name) *p.name = e.name;
        if (p.dry_run) return 1;
        FusedArgs a = fused_args(p);
        a.lpw = kQuadTraj;
        hipLaunchKernelGGL(e.k, dim3((unsigned)waves), dim3(kSmallBlock), 0, p.s, a);
        const int rc = hip_fail(hipGetLastError(), e.name);
        return rc ? rc : 1;
    }
    return 0;
}

}  // namespace ssmq
