// Masked pass (ssmq_filter_masked_dev): the dispatch table of k_masked_loop<> (ssmq_masked_kernel.h) - every shape the fused time loop
// is instantiated for, the dense kernels (OPT 0), the whole pass in one launch - and the launch-loop route of every other pair: per
// step apply dyn | apply obs (no noise added) | k_masked_update<D, Y>.  And the detection-mask generator (ssmq_detection_mask_dev).
#include <cstring>
#include "ssmq_masked_kernel.h"
#include "ssmq_filter_shapes.h"
#include "ssmq_rng.h"

namespace ssmq {

template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT>
static hipError_t launch_masked(const MaskedArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_masked_loop<D, Y, ND, NO, FD, FO, FORM, TP, SELO, OPT>), dim3((unsigned)((a.B + kSmallBlock - 1) / kSmallBlock)),
                       dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*masked_fn)(const MaskedArgs &, hipStream_t);
struct MaskedEntry {
    FilterShape shape;
    masked_fn fn;
    const char *name;
};
#define SSMQ_MASKED_ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                                      \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT},                                                                    \
     &launch_masked<D, Y, N, N, FD, FO, FORM, TP, SELO, OPT>,                                                      \
     "k_masked_loop<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO "," #FORM ",TP=" #TP ",SELO=" #SELO ",OPT=" #OPT ">"}

// every shape of ssmq_filter_shapes.h, dense (the LDL' and reflection fast paths are not instantiated for this kernel)
static const MaskedEntry kMasked[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, SSMQ_MASKED_ONE),
    SSMQ_SHAPES_MID(SSMQ_SHAPE, SSMQ_MASKED_ONE),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE, SSMQ_MASKED_ONE),
    SSMQ_SHAPES_HEAVY_SR(SSMQ_SHAPE, SSMQ_MASKED_ONE),
};

// (p.rr is the block of zeros the measurement transform adds: the caller builds the pass's constants without R)
MaskedArgs masked_args(const FilterPass &p, const MaskedPass &r) {
    MaskedArgs a;
    memset(&a, 0, sizeof(a));
    a.y = p.y; a.mask = r.mask; a.m0 = p.m0; a.P0 = p.P0; a.fm = p.fm; a.fP = p.fP; a.used = r.used; a.nis = r.nis; a.ll = r.ll;
    a.status = p.status;
    a.c_dyn = p.hd->d_small; a.c_obs = p.ho->d_small; a.gqg = p.gqg; a.zero = p.rr; a.rr = r.rr; a.gate = r.gate;
    a.B = p.B; a.ld = p.ld; a.T = p.T;
    a.emv_dyn = p.hd->emv_mode; a.emv_obs = p.ho->emv_mode; a.nu_dyn = p.hd->tp_nu; a.nu_obs = p.ho->tp_nu;
    fill_fpar(p.fd, &a.fd);
    fill_fpar(p.fo, &a.fo);
    a.fd.ttab = p.ttab_dyn;
    a.fo.ttab = p.ttab_obs;
    return a;
}

// 1: launched (dry run: a kernel exists, its name set), 0: no one-launch kernel for this pair, < 0: error
int try_launch_masked(const FilterPass &p, const MaskedPass &r) {
    if (is_user_integrand(p.fd) || is_user_integrand(p.fo)) return rtc_launch_masked(p, r);
    if (!same_family(p)) return 0;
    for (const MaskedEntry &e : kMasked) {
        if (!(e.shape == shape_of(p, 0))) continue;
        if (has_time_table(p.fd->id) && !p.ttab_dyn && !p.dry_run) return 0;   // the kernels read the table
        if (p.name) *p.name = e.name;
        if (p.dry_run) return 1;
        const int rc = hip_fail(e.fn(masked_args(p, r), p.s), e.name);
        return rc ? rc : 1;
    }
    return 0;
}

// ---- the launch loop -----------------------------------------------------------------------------------------------------------
template <int D, int Y>
static void launch_masked_upd(const MaskedUpdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_masked_update<D, Y>), dim3((unsigned)((a.B + kMaskedUpdBlock - 1) / kMaskedUpdBlock)), dim3(kMaskedUpdBlock), 0, s,
                       a);
}

// the (D, Y) pairs k_robust_update is instantiated for run in registers, every other pair up to SSMQ_MAX_DIM on run-time loops
static int launch_masked_update(const MaskedUpdArgs &a, hipStream_t s) {
    const int D = a.D, Y = a.Y;
    if (D < 1 || Y < 1 || D > SSMQ_MAX_DIM || Y > SSMQ_MAX_DIM) {
        set_error("masked update: D or Y above SSMQ_MAX_DIM");
        return SSMQ_E_UNSUPPORTED;
    }
#define SSMQ_MASKED_UPD(d, y_)                               \
    if (D == d && Y == y_) {                                 \
        launch_masked_upd<d, y_>(a, s);                      \
        return hip_fail(hipGetLastError(), "k_masked_update"); \
    }
    SSMQ_MASKED_UPD(1, 1)
    SSMQ_MASKED_UPD(2, 1)
    SSMQ_MASKED_UPD(2, 2)
    SSMQ_MASKED_UPD(3, 1)
    SSMQ_MASKED_UPD(4, 2)
    SSMQ_MASKED_UPD(5, 2)
    SSMQ_MASKED_UPD(5, 4)
    SSMQ_MASKED_UPD(6, 2)
#undef SSMQ_MASKED_UPD
    launch_masked_upd<0, 0>(a, s);
    return hip_fail(hipGetLastError(), "k_masked_update (run-time shape)");
}

// ws: robust_ws_bytes() - the planes of the filter's launch loop (m_pr | P_pr | C_xx | y_mean | P_y | P_yx | one unused D x D | two
// status planes); tvec: device [T] = 0 .. T-1 (the pass's constants).  Plain launches on p.s, no graph.
int masked_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, const MaskedPass &r, const double *tvec, void *ws) {
    const int D = h_dyn->D, Y = h_obs->E;
    const int64_t B = p.B, ld = p.ld;
    double *w = (double *)ws;
    double *m_pr = w; w += (size_t)ld * D;
    double *P_pr = w; w += (size_t)ld * D * D;
    double *C_xx = w; w += (size_t)ld * D * D;
    double *y_mean = w; w += (size_t)ld * Y;
    double *P_y = w; w += (size_t)ld * Y * Y;
    double *P_yx = w; w += (size_t)ld * Y * D;
    w += (size_t)ld * D * D;
    int32_t *st_a = (int32_t *)w, *st_b = st_a + ld;
    int rc = hip_fail(hipMemsetAsync(p.status, 0, sizeof(int32_t) * ld, p.s), "hipMemsetAsync");
    for (int k = 0; k < p.T && !rc; ++k) {
        const double *m_in = k == 0 ? p.m0 : p.fm + (int64_t)(k - 1) * D * ld;
        const double *P_in = k == 0 ? p.P0 : p.fP + (int64_t)(k - 1) * D * D * ld;
        rc = apply_dev_impl(h_dyn, p.fd, B, ld, m_in, P_in, tvec + k, 0, m_pr, P_pr, C_xx, st_a, p.gqg, nullptr, false, 1.0, 1.0,
                            p.ttab_dyn, false);
        if (!rc)   // (p.rr: zeros - P_y is P_h)
            rc = apply_dev_impl(h_obs, p.fo, B, ld, m_pr, P_pr, tvec + k, 0, y_mean, P_y, P_yx, st_b, p.rr, nullptr, false, 1.0, 1.0,
                                p.ttab_obs, false);
        if (rc) break;
        MaskedUpdArgs a;
        memset(&a, 0, sizeof(a));
        a.m_pr = m_pr; a.P_pr = P_pr; a.y_mean = y_mean; a.P_y = P_y; a.P_yx = P_yx;
        a.y = p.y + (int64_t)k * Y * ld;
        a.mask = r.mask ? r.mask + (int64_t)k * ld : nullptr;
        a.m_out = p.fm + (int64_t)k * D * ld;
        a.P_out = p.fP + (int64_t)k * D * D * ld;
        a.used = r.used + (int64_t)k * ld;
        a.nis = r.nis + (int64_t)k * ld;
        a.ll = r.ll + (int64_t)k * ld;
        a.status = p.status; a.st_dyn = st_a; a.st_obs = st_b; a.rr = r.rr; a.gate = r.gate; a.B = B; a.ld = ld; a.step = k; a.D = D; a.Y = Y;
        rc = launch_masked_update(a, p.s);
    }
    return rc;
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
