// Outlier-robust pass (ssmq_filter_robust_dev): the dispatch table of k_robust_loop<> (ssmq_robust_kernel.h) - every shape the fused
// time loop is instantiated for, the dense kernels (OPT 0), the whole pass in one launch - and the launch-loop route of every other
// pair: per step apply dyn | apply obs (no noise added) | k_robust_update<D, Y>.
#include <cstring>
#include "ssmq_robust_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT>
static hipError_t launch_robust(const RobustArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_robust_loop<D, Y, ND, NO, FD, FO, FORM, TP, SELO, OPT>), dim3((unsigned)((a.B + kSmallBlock - 1) / kSmallBlock)),
                       dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*robust_fn)(const RobustArgs &, hipStream_t);
struct RobustEntry {
    FilterShape shape;
    robust_fn fn;
    const char *name;
};
#define SSMQ_ROBUST_ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                                      \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT},                                                                    \
     &launch_robust<D, Y, N, N, FD, FO, FORM, TP, SELO, OPT>,                                                      \
     "k_robust_loop<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO "," #FORM ",TP=" #TP ",SELO=" #SELO ",OPT=" #OPT ">"}

// every shape of ssmq_filter_shapes.h, dense (the LDL' and reflection fast paths are not instantiated for this kernel)
static const RobustEntry kRobust[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, SSMQ_ROBUST_ONE),
    SSMQ_SHAPES_MID(SSMQ_SHAPE, SSMQ_ROBUST_ONE),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE, SSMQ_ROBUST_ONE),
    SSMQ_SHAPES_HEAVY_SR(SSMQ_SHAPE, SSMQ_ROBUST_ONE),
};

// (p.rr is the block of zeros the measurement transform adds: the caller builds the pass's constants without R)
RobustArgs robust_args(const FilterPass &p, const RobustPass &r) {
    RobustArgs a;
    memset(&a, 0, sizeof(a));
    a.y = p.y; a.m0 = p.m0; a.P0 = p.P0; a.fm = p.fm; a.fP = p.fP; a.lam = r.lam; a.delta = r.delta; a.status = p.status;
    a.c_dyn = p.hd->d_small; a.c_obs = p.ho->d_small; a.gqg = p.gqg; a.zero = p.rr; a.rr = r.rr; a.ir = r.ir;
    a.B = p.B; a.ld = p.ld; a.T = p.T; a.iters = r.iterations; a.dof = r.dof;
    a.emv_dyn = p.hd->emv_mode; a.emv_obs = p.ho->emv_mode; a.nu_dyn = p.hd->tp_nu; a.nu_obs = p.ho->tp_nu;
    fill_fpar(p.fd, &a.fd);
    fill_fpar(p.fo, &a.fo);
    a.fd.ttab = p.ttab_dyn;
    a.fo.ttab = p.ttab_obs;
    return a;
}

// 1: launched (dry run: a kernel exists, its name set), 0: no one-launch kernel for this pair, < 0: error
int try_launch_robust(const FilterPass &p, const RobustPass &r) {
    if (is_user_integrand(p.fd) || is_user_integrand(p.fo)) return rtc_launch_robust(p, r);
    if (!same_family(p)) return 0;
    for (const RobustEntry &e : kRobust) {
        if (!(e.shape == shape_of(p, 0))) continue;
        if (has_time_table(p.fd->id) && !p.ttab_dyn && !p.dry_run) return 0;   // the kernels read the table
        if (p.name) *p.name = e.name;
        if (p.dry_run) return 1;
        const int rc = hip_fail(e.fn(robust_args(p, r), p.s), e.name);
        return rc ? rc : 1;
    }
    return 0;
}

// ---- the launch loop -----------------------------------------------------------------------------------------------------------
template <int D, int Y>
static void launch_robust_upd(const RobustUpdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_robust_update<D, Y>), dim3((unsigned)((a.B + kRobustUpdBlock - 1) / kRobustUpdBlock)), dim3(kRobustUpdBlock), 0, s,
                       a);
}

// the (D, Y) pairs k_kalman_update is instantiated for run in registers, every other pair up to SSMQ_MAX_DIM on run-time loops
static int launch_robust_update(const RobustUpdArgs &a, hipStream_t s) {
    const int D = a.D, Y = a.Y;
    if (D < 1 || Y < 1 || D > SSMQ_MAX_DIM || Y > SSMQ_MAX_DIM) {
        set_error("robust update: D or Y above SSMQ_MAX_DIM");
        return SSMQ_E_UNSUPPORTED;
    }
#define SSMQ_ROBUST_UPD(d, y_)                               \
    if (D == d && Y == y_) {                                 \
        launch_robust_upd<d, y_>(a, s);                      \
        return hip_fail(hipGetLastError(), "k_robust_update"); \
    }
    SSMQ_ROBUST_UPD(1, 1)
    SSMQ_ROBUST_UPD(2, 1)
    SSMQ_ROBUST_UPD(2, 2)
    SSMQ_ROBUST_UPD(3, 1)
    SSMQ_ROBUST_UPD(4, 2)
    SSMQ_ROBUST_UPD(5, 2)
    SSMQ_ROBUST_UPD(5, 4)
    SSMQ_ROBUST_UPD(6, 2)
#undef SSMQ_ROBUST_UPD
    launch_robust_upd<0, 0>(a, s);
    return hip_fail(hipGetLastError(), "k_robust_update (run-time shape)");
}

// the planes of the filter's launch loop (m_pr | P_pr | C_xx | y_mean | P_y | P_yx | one unused D x D | two status planes)
size_t robust_ws_bytes(int D, int Y, int64_t ld) {
    return sizeof(double) * (size_t)ld * (D + 3 * D * D + Y + Y * Y + Y * D) + 2 * sizeof(int32_t) * (size_t)ld;
}

// ws: robust_ws_bytes(); tvec: device [T] = 0 .. T-1 (the pass's constants).  Plain launches on p.s, no graph.
int robust_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, const RobustPass &r, const double *tvec, void *ws) {
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
        RobustUpdArgs a;
        memset(&a, 0, sizeof(a));
        a.m_pr = m_pr; a.P_pr = P_pr; a.y_mean = y_mean; a.P_y = P_y; a.P_yx = P_yx;
        a.y = p.y + (int64_t)k * Y * ld;
        a.m_out = p.fm + (int64_t)k * D * ld;
        a.P_out = p.fP + (int64_t)k * D * D * ld;
        a.lam = r.lam + (int64_t)k * ld;
        a.delta = r.delta + (int64_t)k * ld;
        a.status = p.status; a.st_dyn = st_a; a.st_obs = st_b; a.rr = r.rr; a.ir = r.ir; a.B = B; a.ld = ld; a.step = k; a.D = D; a.Y = Y;
        a.iters = r.iterations; a.dof = r.dof;
        rc = launch_robust_update(a, p.s);
    }
    return rc;
}

}  // namespace ssmq
