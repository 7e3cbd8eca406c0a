// Iterated posterior linearisation pass (ssmq_filter_iterated_dev): the dispatch table of k_iplf_loop<> (ssmq_iterated_kernel.h) -
// every shape the fused time loop is instantiated for, the dense kernels (OPT 0), the whole pass in one launch - and the launch-loop
// route of every other pair: per step apply dyn, then J x (apply obs at the iterate planes | k_iplf_update<D, Y>).
#include "ssmq_iterated_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

#define SSMQ_IPLF_ONE(...) SSMQ_PASS_ENTRY(IplfArgs, k_iplf_loop, __VA_ARGS__)
static const PassEntry<IplfArgs> kIplf[] = {SSMQ_PASS_TABLE(SSMQ_IPLF_ONE)};

int try_launch_iterated(const FilterPass &p, const IplfPass &r) {
    return try_launch_pass(p, kIplf, SSMQ_RTC_ITERATED, [&](IplfArgs &a) { a.delta = r.delta; a.iters = r.iterations; });
}

int iterated_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, const IplfPass &r, const double *tvec, void *ws) {
    return update_launch_loop(h_dyn, h_obs, p, r.iterations, tvec, ws, [&](const ItemPlanes &c, bool last) {
        IplfUpdArgs a;
        memset(&a, 0, sizeof(a));
        a.m_it = c.m_at; a.P_it = c.P_at;
        a.delta = (last && r.delta) ? r.delta + (int64_t)c.step * c.ld : nullptr;
        return launch_item_update(a, c, "iplf", kIplfUpdBlock, [&](auto d, auto y, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((k_iplf_update<decltype(d)::value, decltype(y)::value>), grid, block, 0, p.s, a);
        });
    });
}

}  // namespace ssmq
