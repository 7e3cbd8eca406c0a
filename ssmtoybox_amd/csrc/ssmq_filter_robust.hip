// Outlier-robust pass (ssmq_filter_robust_dev): the dispatch table of k_robust_loop<> (ssmq_robust_kernel.h) - every shape the fused
// time loop is instantiated for, the dense kernels (OPT 0), the whole pass in one launch - and the launch-loop route of every other
// pair: per step apply dyn | apply obs (no noise added) | k_robust_update<D, Y>.
#include "ssmq_robust_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

#define SSMQ_ROBUST_ONE(...) SSMQ_PASS_ENTRY(RobustArgs, k_robust_loop, __VA_ARGS__)
static const PassEntry<RobustArgs> kRobust[] = {SSMQ_PASS_TABLE(SSMQ_ROBUST_ONE)};

int try_launch_robust(const FilterPass &p, const RobustPass &r) {
    return try_launch_pass(p, kRobust, SSMQ_RTC_ROBUST, [&](RobustArgs &a) {
        a.lam = r.lam; a.delta = r.delta; a.rr = r.rr; a.ir = r.ir; a.dof = r.dof; a.iters = r.iterations;
    });
}

int robust_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, const RobustPass &r, const double *tvec, void *ws) {
    return update_launch_loop(h_dyn, h_obs, p, 1, tvec, ws, [&](const ItemPlanes &c, bool) {
        RobustUpdArgs a;
        memset(&a, 0, sizeof(a));
        a.lam = r.lam + (int64_t)c.step * c.ld; a.delta = r.delta + (int64_t)c.step * c.ld;
        a.rr = r.rr; a.ir = r.ir; a.dof = r.dof; a.iters = r.iterations;
        return launch_item_update(a, c, "robust", kRobustUpdBlock, [&](auto d, auto y, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((k_robust_update<decltype(d)::value, decltype(y)::value>), grid, block, 0, p.s, a);
        });
    });
}

}  // namespace ssmq
