// Iterated posterior linearisation pass (ssmq_filter_iterated_dev): the dispatch table of k_iplf_loop<> (ssmq_iterated_kernel.h) -
// every shape the fused time loop is instantiated for, the dense kernels (OPT 0), the whole pass in one launch - and the launch-loop
// route of every other pair: per step apply dyn, then J x (apply obs at the iterate planes | k_iplf_update<D, Y>).
#include <cstring>
#include "ssmq_iterated_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT>
static hipError_t launch_iplf(const IplfArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_iplf_loop<D, Y, ND, NO, FD, FO, FORM, TP, SELO, OPT>), dim3((unsigned)((a.B + kSmallBlock - 1) / kSmallBlock)),
                       dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*iplf_fn)(const IplfArgs &, hipStream_t);
struct IplfEntry {
    FilterShape shape;
    iplf_fn fn;
    const char *name;
};
#define SSMQ_IPLF_ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                                        \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT},                                                                    \
     &launch_iplf<D, Y, N, N, FD, FO, FORM, TP, SELO, OPT>,                                                        \
     "k_iplf_loop<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO "," #FORM ",TP=" #TP ",SELO=" #SELO ",OPT=" #OPT ">"}

// every shape of ssmq_filter_shapes.h, dense (the LDL' and reflection fast paths are not instantiated for this kernel)
static const IplfEntry kIplf[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, SSMQ_IPLF_ONE),
    SSMQ_SHAPES_MID(SSMQ_SHAPE, SSMQ_IPLF_ONE),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE, SSMQ_IPLF_ONE),
    SSMQ_SHAPES_HEAVY_SR(SSMQ_SHAPE, SSMQ_IPLF_ONE),
};

IplfArgs iplf_args(const FilterPass &p, int iterations, double *delta) {
    IplfArgs a;
    memset(&a, 0, sizeof(a));
    a.y = p.y; a.m0 = p.m0; a.P0 = p.P0; a.fm = p.fm; a.fP = p.fP; a.delta = delta; a.status = p.status;
    a.c_dyn = p.hd->d_small; a.c_obs = p.ho->d_small; a.gqg = p.gqg; a.rr = p.rr; a.B = p.B; a.ld = p.ld; a.T = p.T; a.iters = iterations;
    a.emv_dyn = p.hd->emv_mode; a.emv_obs = p.ho->emv_mode; a.nu_dyn = p.hd->tp_nu; a.nu_obs = p.ho->tp_nu;
    fill_fpar(p.fd, &a.fd);
    fill_fpar(p.fo, &a.fo);
    a.fd.ttab = p.ttab_dyn;
    a.fo.ttab = p.ttab_obs;
    return a;
}

// 1: launched (dry run: a kernel exists, its name set), 0: no one-launch kernel for this pair, < 0: error
int try_launch_iterated(const FilterPass &p, int iterations, double *delta) {
    if (is_user_integrand(p.fd) || is_user_integrand(p.fo)) return rtc_launch_iterated(p, iterations, delta);
    if (!same_family(p)) return 0;
    for (const IplfEntry &e : kIplf) {
        if (!(e.shape == shape_of(p, 0))) continue;
        if (has_time_table(p.fd->id) && !p.ttab_dyn && !p.dry_run) return 0;   // the kernels read the table
        if (p.name) *p.name = e.name;
        if (p.dry_run) return 1;
        const int rc = hip_fail(e.fn(iplf_args(p, iterations, delta), p.s), e.name);
        return rc ? rc : 1;
    }
    return 0;
}

// ---- the launch loop -----------------------------------------------------------------------------------------------------------
template <int D, int Y>
static void launch_iplf_upd(const IplfUpdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_iplf_update<D, Y>), dim3((unsigned)((a.B + kIplfUpdBlock - 1) / kIplfUpdBlock)), dim3(kIplfUpdBlock), 0, s, a);
}

// the (D, Y) pairs k_kalman_update is instantiated for run in registers, every other pair up to SSMQ_MAX_DIM on run-time loops
static int launch_iplf_update(const IplfUpdArgs &a, hipStream_t s) {
    const int D = a.D, Y = a.Y;
    if (D < 1 || Y < 1 || D > SSMQ_MAX_DIM || Y > SSMQ_MAX_DIM) {
        set_error("iplf update: D or Y above SSMQ_MAX_DIM");
        return SSMQ_E_UNSUPPORTED;
    }
#define SSMQ_IPLF_UPD(d, y_)                               \
    if (D == d && Y == y_) {                               \
        launch_iplf_upd<d, y_>(a, s);                      \
        return hip_fail(hipGetLastError(), "k_iplf_update"); \
    }
    SSMQ_IPLF_UPD(1, 1)
    SSMQ_IPLF_UPD(2, 1)
    SSMQ_IPLF_UPD(2, 2)
    SSMQ_IPLF_UPD(3, 1)
    SSMQ_IPLF_UPD(4, 2)
    SSMQ_IPLF_UPD(5, 2)
    SSMQ_IPLF_UPD(5, 4)
    SSMQ_IPLF_UPD(6, 2)
#undef SSMQ_IPLF_UPD
    launch_iplf_upd<0, 0>(a, s);
    return hip_fail(hipGetLastError(), "k_iplf_update (run-time shape)");
}

size_t iterated_ws_bytes(int D, int Y, int64_t ld) {
    return sizeof(double) * (size_t)ld * (2 * D + 3 * D * D + Y + Y * Y + Y * D) + 2 * sizeof(int32_t) * (size_t)ld;
}

// ws: iterated_ws_bytes(); tvec: device [T] = 0 .. T-1 (the pass's constants).  Plain launches on p.s, no graph.
int iterated_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, int iterations, double *delta,
                         const double *tvec, void *ws) {
    const int D = h_dyn->D, Y = h_obs->E;
    const int64_t B = p.B, ld = p.ld;
    double *w = (double *)ws;
    double *m_pr = w; w += (size_t)ld * D;
    double *P_pr = w; w += (size_t)ld * D * D;
    double *C_xx = w; w += (size_t)ld * D * D;
    double *y_mean = w; w += (size_t)ld * Y;
    double *P_y = w; w += (size_t)ld * Y * Y;
    double *P_yx = w; w += (size_t)ld * Y * D;
    double *m_it = w; w += (size_t)ld * D;
    double *P_it = w; w += (size_t)ld * D * D;
    int32_t *st_a = (int32_t *)w, *st_b = st_a + ld;
    int rc = hip_fail(hipMemsetAsync(p.status, 0, sizeof(int32_t) * ld, p.s), "hipMemsetAsync");
    for (int k = 0; k < p.T && !rc; ++k) {
        const double *m_in = k == 0 ? p.m0 : p.fm + (int64_t)(k - 1) * D * ld;
        const double *P_in = k == 0 ? p.P0 : p.fP + (int64_t)(k - 1) * D * D * ld;
        rc = apply_dev_impl(h_dyn, p.fd, B, ld, m_in, P_in, tvec + k, 0, m_pr, P_pr, C_xx, st_a, p.gqg, nullptr, false, 1.0, 1.0,
                            p.ttab_dyn, false);
        for (int i = 0; i < iterations && !rc; ++i) {
            const bool last = i == iterations - 1;
            const double *mi = i == 0 ? m_pr : m_it, *Pi = i == 0 ? P_pr : P_it;
            rc = apply_dev_impl(h_obs, p.fo, B, ld, mi, Pi, tvec + k, 0, y_mean, P_y, P_yx, st_b, p.rr, nullptr, false, 1.0, 1.0,
                                p.ttab_obs, false);
            if (rc) break;
            IplfUpdArgs a;
            memset(&a, 0, sizeof(a));
            a.m_pr = m_pr; a.P_pr = P_pr; a.m_it = mi; a.P_it = Pi; a.y_mean = y_mean; a.P_y = P_y; a.P_yx = P_yx;
            a.y = p.y + (int64_t)k * Y * ld;
            a.m_out = last ? p.fm + (int64_t)k * D * ld : m_it;
            a.P_out = last ? p.fP + (int64_t)k * D * D * ld : P_it;
            a.delta = (last && delta) ? delta + (int64_t)k * ld : nullptr;
            a.status = p.status; a.st_dyn = st_a; a.st_obs = st_b; a.B = B; a.ld = ld; a.step = k; a.D = D; a.Y = Y;
            rc = launch_iplf_update(a, p.s);
        }
    }
    return rc;
}

}  // namespace ssmq
