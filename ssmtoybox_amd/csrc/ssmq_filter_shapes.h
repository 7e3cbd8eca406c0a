// The model shapes the time-loop kernels are instantiated for, once, and the rules by which a pass picks among the instantiations
// of a shape.  Host only: included by the table files (ssmq_filter_fused.hip, ssmq_filter_chunked.hip, ssmq_filter_piped.hip, those of
// the scoring kernels, ...) and by the run-time compiler's host code, never embedded in the text it compiles.
#pragma once
#include <array>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include "ssmq_fused.h"
#include "ssmq_host.h"

// One instantiation is ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT) - the table file's own entry macro.  A shape expands to its BQ,
// t-process BQ and sigma-point kernels ...
#define SSMQ_SHAPE(ONE, FD, FO, D, Y, N, SELO)        \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 0, SELO, 0),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 1, SELO, 0),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_SIGMA, 0, SELO, 0)
// ... and a "fast" shape also to the LDL' / unscented-point / reflection-symmetry fast paths of ssmq_apply_small.h (OPT: SSMQ_OPT_*)
#define SSMQ_SHAPE_FAST(ONE, FD, FO, D, Y, N, SELO)   \
    SSMQ_SHAPE(ONE, FD, FO, D, Y, N, SELO),           \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 0, SELO, 7),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 0, SELO, 3),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 1, SELO, 2),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_SIGMA, 0, SELO, 2)

// The groups; X is SSMQ_SHAPE or SSMQ_SHAPE_FAST.  A new model family is one line in one of them.
// scalar UNGM (BASELINE configs[1] and the six filters of the reference's UNGM studies): 2, 3 and 5 points
#define SSMQ_SHAPES_UNGM(X, ONE)                           \
    X(ONE, SSMQ_F_UNGM_DYN, SSMQ_F_UNGM_MEAS, 1, 1, 2, 0), \
    X(ONE, SSMQ_F_UNGM_DYN, SSMQ_F_UNGM_MEAS, 1, 1, 3, 0), \
    X(ONE, SSMQ_F_UNGM_DYN, SSMQ_F_UNGM_MEAS, 1, 1, 5, 0)
// two to four states: unscented (2 D + 1) and spherical-radial (2 D) point sets
#define SSMQ_SHAPES_MID(X, ONE)                                                                                   \
    X(ONE, SSMQ_F_PENDULUM_DYN, SSMQ_F_PENDULUM_MEAS, 2, 1, 5, 0),                                                  \
    X(ONE, SSMQ_F_REENTRY1D_DYN, SSMQ_F_RANGE_MEAS, 3, 1, 7, 0),   /* tests/test_ssinf.py:40-50 of the reference */ \
    X(ONE, SSMQ_F_CV_DYN, SSMQ_F_RADAR2D_MEAS, 4, 2, 9, 0),        /* constant velocity + radar (Student filters) */ \
    X(ONE, SSMQ_F_PENDULUM_DYN, SSMQ_F_PENDULUM_MEAS, 2, 1, 4, 0),                                                  \
    X(ONE, SSMQ_F_REENTRY1D_DYN, SSMQ_F_RANGE_MEAS, 3, 1, 6, 0),                                                    \
    X(ONE, SSMQ_F_CV_DYN, SSMQ_F_RADAR2D_MEAS, 4, 2, 8, 0)
// five or six states (BASELINE configs[2] and configs[3]: 2 000+ vector instructions per step) with unscented points ...
#define SSMQ_SHAPES_HEAVY_UT(X, ONE)                                    \
    X(ONE, SSMQ_F_REENTRY2D_DYN, SSMQ_F_RADAR2D_MEAS, 5, 2, 11, 0),      \
    X(ONE, SSMQ_F_REENTRY2D_BIAS_DYN, SSMQ_F_RADAR2D_MEAS, 6, 2, 13, 0), \
    X(ONE, SSMQ_F_CT_DYN, SSMQ_F_BEARING_MEAS, 5, 4, 11, 1)
// ... and with spherical-radial points (the cubature Kalman filter and every BQ transform built with 'sr')
#define SSMQ_SHAPES_HEAVY_SR(X, ONE)                                    \
    X(ONE, SSMQ_F_REENTRY2D_DYN, SSMQ_F_RADAR2D_MEAS, 5, 2, 10, 0),      \
    X(ONE, SSMQ_F_REENTRY2D_BIAS_DYN, SSMQ_F_RADAR2D_MEAS, 6, 2, 12, 0), \
    X(ONE, SSMQ_F_CT_DYN, SSMQ_F_BEARING_MEAS, 5, 4, 10, 1)

// The (D, Y) pairs the per-item update kernels of the launch loops (k_kalman_update and those of the update variants) are instantiated
// for, in registers; every other pair up to SSMQ_MAX_DIM runs on run-time loops.  X(D, Y), no separator.
#define SSMQ_UPDATE_PAIRS(X) X(1, 1) X(2, 1) X(2, 2) X(3, 1) X(4, 2) X(5, 2) X(5, 4) X(6, 2)

namespace ssmq {

// The OPT values a pass asks its table for, best first, -1 = no such variant for these handles: the fast path BOTH handles qualify
// for - reflection-symmetric weights on top of LDL' and unscented points (7, plain BQ only), LDL' and / or unscented points - and
// the dense kernel.
inline std::array<int, 3> opt_preference(const ssmq_transform *hd, const ssmq_transform *ho) {
    const int both = hd->opt_mask & ho->opt_mask;
    const bool plain = !(hd->tp_nu > 0.0 || hd->form == SSMQ_FORM_SIGMA);
    return {(plain && (both & 7) == 7) ? 7 : -1, both & (plain ? 3 : SSMQ_OPT_UT), 0};
}

// The entry of a dispatch table for a key: entries carry the key as `shape` (a FilterShape, or a type that extends it), null = no
// instantiation.
template <class Entry, size_t N, class Key>
const Entry *find_entry(const Entry (&table)[N], const Key &shape) {
    for (const Entry &e : table)
        if (e.shape == shape) return &e;
    return nullptr;
}

// ---- the whole-pass kernels of the measurement-update variants: Args has the members filled below, by these names -----------------
template <class Args>
struct PassEntry {
    FilterShape shape;
    hipError_t (*fn)(const Args &, hipStream_t);
    const char *name;
};
template <class Args, void (*Kernel)(const Args)>
hipError_t launch_pass_kernel(const Args &a, hipStream_t s) {
    hipLaunchKernelGGL(Kernel, dim3((unsigned)((a.B + kSmallBlock - 1) / kSmallBlock)), dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}
// One entry of a table file: ONE(...) of the groups above is SSMQ_PASS_ENTRY(Args, kernel, ...)
#define SSMQ_PASS_ENTRY(ARGS, KERNEL, FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                        \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT},                                                                    \
     &launch_pass_kernel<ARGS, &KERNEL<D, Y, N, N, FD, FO, FORM, TP, SELO, OPT>>,                                  \
     #KERNEL "<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO "," #FORM ",TP=" #TP ",SELO=" #SELO ",OPT=" #OPT ">"}
// every shape of the groups above, dense (the LDL' and reflection fast paths are not instantiated for these kernels)
#define SSMQ_PASS_TABLE(ONE) \
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, ONE), SSMQ_SHAPES_MID(SSMQ_SHAPE, ONE), SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE, ONE), SSMQ_SHAPES_HEAVY_SR(SSMQ_SHAPE, ONE)

// The common members of the arguments from the pass, the variant's own by fill(a); then the table, or for a pair with a user member the
// run-time compiler (rtc_kind: SSMQ_RTC_*).  1: launched (dry run: a kernel exists, its name set), 0: no one-launch kernel for this
// pair, < 0: error
template <class Args, size_t N, class Fill>
int try_launch_pass(const FilterPass &p, const PassEntry<Args> (&table)[N], int rtc_kind, Fill fill) {
    const bool user = is_user_integrand(p.fd) || is_user_integrand(p.fo);
    const PassEntry<Args> *e = nullptr;
    if (!user) {
        if (!same_family(p) || !(e = find_entry(table, shape_of(p, 0)))) return 0;
        if (has_time_table(p.fd->id) && !p.ttab_dyn && !p.dry_run) return 0;   // the kernels read the table
        if (p.name) *p.name = e->name;
        if (p.dry_run) return 1;
    } else if (p.dry_run) {
        return rtc_launch_pass(p, rtc_kind, nullptr, nullptr, nullptr, 0);
    }
    Args a;
    memset(&a, 0, sizeof(a));
    a.y = p.y; a.m0 = p.m0; a.P0 = p.P0; a.fm = p.fm; a.fP = p.fP; a.status = p.status;
    a.c_dyn = p.hd->d_small; a.c_obs = p.ho->d_small; a.gqg = p.gqg; a.radd = p.rr; a.B = p.B; a.ld = p.ld; a.T = p.T;
    a.emv_dyn = p.hd->emv_mode; a.emv_obs = p.ho->emv_mode; a.nu_dyn = p.hd->tp_nu; a.nu_obs = p.ho->tp_nu;
    fill_fpar(p.fd, &a.fd);
    fill_fpar(p.fo, &a.fo);
    a.fd.ttab = p.ttab_dyn;
    a.fo.ttab = p.ttab_obs;
    fill(a);
    if (user) return rtc_launch_pass(p, rtc_kind, &a, &a.fd, &a.fo, a.B);
    const int rc = hip_fail(e->fn(a, p.s), e->name);
    return rc ? rc : 1;
}

// f(integral_constant D, integral_constant Y) for the instantiation of a pair of SSMQ_UPDATE_PAIRS; false: not one of them
template <class F>
bool for_update_pair(int D, int Y, F f) {
#define SSMQ_UPDATE_PAIR_(d, y_)                                                \
    if (D == d && Y == y_) {                                                    \
        f(std::integral_constant<int, d>{}, std::integral_constant<int, y_>{}); \
        return true;                                                            \
    }
    SSMQ_UPDATE_PAIRS(SSMQ_UPDATE_PAIR_)
#undef SSMQ_UPDATE_PAIR_
    return false;
}

// The per-item kernel k_<variant>_update<D, Y> of a launch loop for run-time D, Y: the common members of its arguments from the
// planes of the step (update_launch_loop), the variant's own filled by the caller; block_size: the kernel's; launch(d, y, grid,
// block) launches the instantiation <d, y>, <0, 0> = run-time shapes.  The names of an error are put together only when there is one.
template <class Args, class Launch>
int launch_item_update(Args &a, const ItemPlanes &c, const char *variant, int block_size, Launch launch) {
    a.m_pr = c.m_pr; a.P_pr = c.P_pr; a.y_mean = c.y_mean; a.P_y = c.P_y; a.P_yx = c.P_yx; a.y = c.y; a.m_out = c.m_out; a.P_out = c.P_out;
    a.status = c.status; a.st_dyn = c.st_dyn; a.st_obs = c.st_obs; a.B = c.B; a.ld = c.ld; a.step = c.step; a.D = c.D; a.Y = c.Y;
    const int D = a.D, Y = a.Y;
    if (D < 1 || Y < 1 || D > SSMQ_MAX_DIM || Y > SSMQ_MAX_DIM) {
        set_error(std::string(variant) + " update: D or Y above SSMQ_MAX_DIM");
        return SSMQ_E_UNSUPPORTED;
    }
    const dim3 grid((unsigned)((a.B + block_size - 1) / block_size)), block(block_size);
    const bool in_registers = for_update_pair(D, Y, [&](auto d, auto y) { launch(d, y, grid, block); });
    if (!in_registers) launch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, grid, block);
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return SSMQ_OK;
    return hip_fail(err, ("k_" + std::string(variant) + (in_registers ? "_update" : "_update (run-time shape)")).c_str());
}

// has_time_table() is what the host goes by, HasTimeTable<> what the kernels are compiled with: the same set of integrands
template <int... F>
constexpr bool time_table_ids_agree(std::integer_sequence<int, F...>) {
    return ((HasTimeTable<F>::value == has_time_table(F)) && ...);
}
static_assert(time_table_ids_agree(std::make_integer_sequence<int, SSMQ_F_USER_FIRST + SSMQ_F_USER_SLOTS>{}),
              "has_time_table() and HasTimeTable<> disagree");

}  // namespace ssmq
