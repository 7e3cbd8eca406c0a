// Iterated posterior linearisation smoother (ssmq_smoother_iterated_dev): the dispatch table of k_ipls_pass<> (ssmq_ipls_kernel.h) -
// every shape the fused time loop is instantiated for, the dense transforms, one launch per iteration.  A pair with a user integrand
// goes to the run-time compiler (ssmq_rtc.hip); every other pair has no kernel (the entry point refuses it).
#include <cstring>
#include "ssmq_ipls_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO>
static hipError_t launch_ipls(const IplsArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_ipls_pass<D, Y, ND, NO, FD, FO, FORM, TP, SELO>), dim3((unsigned)((a.B + kSmallBlock - 1) / kSmallBlock)),
                       dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*ipls_fn)(const IplsArgs &, hipStream_t);
struct IplsEntry {
    FilterShape shape;
    ipls_fn fn;
    const char *name;
};
#define SSMQ_IPLS_ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                                        \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT},                                                                    \
     &launch_ipls<D, Y, N, N, FD, FO, FORM, TP, SELO>,                                                             \
     "k_ipls_pass<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO "," #FORM ",TP=" #TP ",SELO=" #SELO ">"}

// every shape of ssmq_filter_shapes.h, dense
static const IplsEntry kIpls[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, SSMQ_IPLS_ONE),
    SSMQ_SHAPES_MID(SSMQ_SHAPE, SSMQ_IPLS_ONE),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE, SSMQ_IPLS_ONE),
    SSMQ_SHAPES_HEAVY_SR(SSMQ_SHAPE, SSMQ_IPLS_ONE),
};

IplsArgs ipls_args(const FilterPass &p, const IplsPlanes &q) {
    IplsArgs a;
    memset(&a, 0, sizeof(a));
    a.y = p.y; a.m0 = p.m0; a.P0 = p.P0; a.fm = p.fm; a.fP = p.fP; a.status = p.status;
    a.lin_m = q.lin_m; a.lin_P = q.lin_P; a.pm = q.pm; a.pP = q.pP; a.pC = q.pC;
    a.sm0 = q.sm0; a.sP0 = q.sP0; a.sm = q.sm; a.sP = q.sP; a.delta = q.delta;
    a.c_dyn = p.hd->d_small; a.c_obs = p.ho->d_small; a.gqg = p.gqg; a.rr = p.rr; a.B = p.B; a.ld = p.ld; a.T = p.T;
    a.emv_dyn = p.hd->emv_mode; a.emv_obs = p.ho->emv_mode; a.nu_dyn = p.hd->tp_nu; a.nu_obs = p.ho->tp_nu;
    fill_fpar(p.fd, &a.fd);
    fill_fpar(p.fo, &a.fo);
    a.fd.ttab = p.ttab_dyn;
    a.fo.ttab = p.ttab_obs;
    return a;
}

// One iteration.  1: launched (dry run: a kernel exists, its name set), 0: no kernel for this pair, < 0: error
int try_launch_ipls(const FilterPass &p, const IplsPlanes &q) {
    if (is_user_integrand(p.fd) || is_user_integrand(p.fo)) {
        IplsArgs a = ipls_args(p, q);
        return rtc_launch_pass(p, SSMQ_RTC_SMOOTHER_ITERATED, &a, &a.fd, &a.fo, a.B);
    }
    if (!same_family(p)) return 0;
    for (const IplsEntry &e : kIpls) {
        if (!(e.shape == shape_of(p, 0))) continue;
        if (has_time_table(p.fd->id) && !p.ttab_dyn && !p.dry_run) return 0;   // the kernels read the table
        if (p.name) *p.name = e.name;
        if (p.dry_run) return 1;
        const int rc = hip_fail(e.fn(ipls_args(p, q), p.s), e.name);
        return rc ? rc : 1;
    }
    return 0;
}

}  // namespace ssmq
