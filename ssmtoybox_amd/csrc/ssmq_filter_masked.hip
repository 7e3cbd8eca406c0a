// Masked pass (ssmq_filter_masked_dev): the dispatch table of k_masked_loop<> (ssmq_masked_kernel.h) - every shape the fused time loop
// is instantiated for, the dense kernels (OPT 0), the whole pass in one launch - and the launch-loop route of every other pair: per
// step apply dyn | apply obs (no noise added) | k_masked_update<D, Y>.  And the detection-mask generator (ssmq_detection_mask_dev).
#include <cstring>
#include "ssmq_masked_kernel.h"
#include "ssmq_filter_shapes.h"
#include "ssmq_rng.h"

namespace ssmq {

#define SSMQ_MASKED_ONE(...) SSMQ_PASS_ENTRY(MaskedArgs, k_masked_loop, __VA_ARGS__)
static const PassEntry<MaskedArgs> kMasked[] = {SSMQ_PASS_TABLE(SSMQ_MASKED_ONE)};

int try_launch_masked(const FilterPass &p, const MaskedPass &r) {
    return try_launch_pass(p, kMasked, SSMQ_RTC_MASKED, [&](MaskedArgs &a) {
        a.mask = r.mask; a.used = r.used; a.nis = r.nis; a.ll = r.ll; a.rr = r.rr; a.gate = r.gate;
    });
}

int masked_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, const MaskedPass &r, const double *tvec, void *ws) {
    return update_launch_loop(h_dyn, h_obs, p, 1, tvec, ws, [&](const ItemPlanes &c, bool) {
        MaskedUpdArgs a;
        memset(&a, 0, sizeof(a));
        const int64_t at = (int64_t)c.step * c.ld;
        a.mask = r.mask ? r.mask + at : nullptr;
        a.used = r.used + at; a.nis = r.nis + at; a.ll = r.ll + at; a.rr = r.rr; a.gate = r.gate;
        return launch_item_update(a, c, "masked", kMaskedUpdBlock, [&](auto d, auto y, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((k_masked_update<decltype(d)::value, decltype(y)::value>), grid, block, 0, p.s, a);
        });
    });
}

// ---- detection masks drawn on the device ----------------------------------------------------------------------------------------
// Bit i of mask[k][b] is set iff u < p[i], u one 53-bit uniform in (0, 1) of ssmq_rng.h (uniform_one): Philox4x32-10 keyed by
// (seed lo, seed hi), counter = (traj lo, traj hi, k, kDetectTag | i) with traj = traj_offset + b,
//     u = (((o0 >> 5) << 26 | o1 >> 6) + 0.5) 2^-53     from the first two output words.
// The simulator's tags are below 1 << 18 and the particle kernels' purposes are 8 .. 14 << 28: nibble 15 is this generator's alone.
// per_component = 0: one draw per (k, b), counter word 3 = kDetectTag, against p[0]; all Y bits go together.  The bits depend on
// (seed, traj, k, i) alone, not on B, ld or the launch geometry.
namespace {
constexpr uint32_t kDetectTag = 15u << 28;
constexpr int kDetectBlock = 256;
struct DetectArgs {
    uint32_t *mask;   // [T][ld]
    int64_t B, ld;
    int32_t T, Y, per_component, k0;   // k0: the step of blockIdx.y = 0
    uint64_t seed, traj_offset;
    double p[SSMQ_MAX_DIM];
};

__global__ __launch_bounds__(kDetectBlock) void k_detection_mask(const DetectArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kDetectBlock + threadIdx.x;
    const int k = a.k0 + (int)blockIdx.y;
    if (b >= a.B) return;
    const uint64_t traj = a.traj_offset + (uint64_t)b;
    uint32_t w = 0;
    if (a.per_component) {
        for (int i = 0; i < a.Y; ++i) w |= (uniform_one(a.seed, traj, (uint32_t)k, kDetectTag | (uint32_t)i) < a.p[i]) ? (1u << i) : 0u;
    } else {
        w = (uniform_one(a.seed, traj, (uint32_t)k, kDetectTag) < a.p[0]) ? ((1u << a.Y) - 1u) : 0u;
    }
    a.mask[(int64_t)k * a.ld + b] = w;
}
}  // namespace

int launch_detection_mask(int64_t B, int64_t ld, int T, int Y, const double *p_detect, uint64_t seed, uint64_t traj_offset, int per_component,
                          uint32_t *d_mask, hipStream_t s) {
    DetectArgs a;
    memset(&a, 0, sizeof(a));
    a.mask = d_mask; a.B = B; a.ld = ld; a.T = T; a.Y = Y; a.per_component = per_component; a.seed = seed; a.traj_offset = traj_offset;
    for (int i = 0; i < Y; ++i) a.p[i] = p_detect[i];
    for (int k0 = 0; k0 < T; k0 += 65535) {   // (the grid's second dimension holds 65535 steps)
        DetectArgs c = a;
        c.k0 = k0;
        const int n = T - k0 < 65535 ? T - k0 : 65535;
        hipLaunchKernelGGL(k_detection_mask, dim3((unsigned)((B + kDetectBlock - 1) / kDetectBlock), (unsigned)n), dim3(kDetectBlock), 0, s, c);
        const int rc = hip_fail(hipGetLastError(), "k_detection_mask");
        if (rc) return rc;
    }
    return SSMQ_OK;
}

}  // namespace ssmq
