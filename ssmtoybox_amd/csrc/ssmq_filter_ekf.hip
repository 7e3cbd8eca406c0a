// The extended Kalman filter's time loop in one kernel for the built-in models: the instantiations of k_ekf_loop<D, Y, KEEP>
// (ssmq_ekf_loop_kernel.h, where the kernel is described) and its launcher.  Taken by ExtendedKalman - both handles a
// linearisation - on additive-noise pairs of built-in models that have a Jacobian, at the (D, Y) pairs those models can form;
// everything else (Taylor-GPQD, user models, other shapes, a transition with a state index) keeps the launch loop of
// filter_forward_impl.  SSMQ_NO_EKF_LOOP=1 switches this kernel off alone, SSMQ_NO_FUSED=1 with every other time-loop kernel.
#include "ssmq_device.h"
#include "ssmq_host.h"
#include "ssmq_math.h"
#include "ssmq_ekf_loop_kernel.h"

namespace ssmq {

template <int D, int Y, bool KEEP>
static hipError_t launch_ekf(const EkfLoopArgs &a, hipStream_t s) {
    const unsigned grid = (unsigned)((a.B + kEkfBlock - 1) / kEkfBlock);
    hipLaunchKernelGGL((k_ekf_loop<D, Y, KEEP>), dim3(grid), dim3(kEkfBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*ekf_fn)(const EkfLoopArgs &, hipStream_t);
struct EkfEntry {
    int D, Y;
    ekf_fn fn[2];            // [KEEP]
    const char *name[2];
};
#define SSMQ_EKF(D, Y) \
    {D, Y, {&launch_ekf<D, Y, false>, &launch_ekf<D, Y, true>}, {"k_ekf_loop<D=" #D ",Y=" #Y ">", "k_ekf_loop_keep<D=" #D ",Y=" #Y ">"}}
static const EkfEntry kEkf[] = {SSMQ_EKF(1, 1), SSMQ_EKF(2, 1), SSMQ_EKF(2, 2), SSMQ_EKF(4, 1), SSMQ_EKF(4, 2), SSMQ_EKF(4, 4),
                                 SSMQ_EKF(5, 2), SSMQ_EKF(5, 4)};

// 1 launched (dry_run: a kernel exists, its name set), 0 this pass keeps the launch loop, < 0 error
int try_launch_ekf_loop(const FilterPass &p, double *pm, double *pP, double *pC) {
    if (p.hd->form != SSMQ_FORM_TAYLOR1 || p.ho->form != SSMQ_FORM_TAYLOR1 || ssmq::sw("SSMQ_NO_EKF_LOOP")) return 0;
    if (is_user_integrand(p.fd) || is_user_integrand(p.fo) || p.sscale || p.student_dof != 0.0) return 0;
    if (!integrand_has_jacobian(p.fd->id) || !integrand_has_jacobian(p.fo->id) || p.fd->n_idx != 0) return 0;
    const int D = p.hd->D, Y = p.ho->E;
    if (p.hd->E != D || p.ho->D != D) return 0;
    // what the launch loop's transforms would refuse stays theirs to refuse (check_integrand, launch_jacobian)
    FInfo fi[2];
    const ssmq_transform *hs[2] = {p.hd, p.ho};
    const ssmq_integrand *fs[2] = {p.fd, p.fo};
    for (int i = 0; i < 2; ++i) {
        if (!integrand_info(fs[i]->id, &fi[i])) return 0;
        if (fs[i]->id == SSMQ_F_BEARING_MEAS) fi[i].dout = fs[i]->n_par / 2;      // (one output per sensor: check_integrand)
        if (fi[i].dout != hs[i]->E || fs[i]->n_idx < 0 || fs[i]->n_idx > SSMQ_MAX_FIDX) return 0;
        if (fs[i]->n_idx > 0) {
            if (fs[i]->n_idx < fi[i].din) return 0;
            for (int k = 0; k < fs[i]->n_idx; ++k)
                if (fs[i]->idx[k] < 0 || fs[i]->idx[k] >= D) return 0;
        } else if (fi[i].din > D) {
            return 0;
        }
    }
    const int keep = (pm && pP && pC) ? 1 : 0;
    for (const EkfEntry &e : kEkf) {
        if (e.D != D || e.Y != Y) continue;
        if (!p.dry_run && ((has_time_table(p.fd->id) && !p.ttab_dyn) || (has_time_table(p.fo->id) && !p.ttab_obs))) return 0;
        if (p.name) *p.name = e.name[keep];
        if (p.dry_run) return 1;
        EkfLoopArgs a;
        memset(&a, 0, sizeof(a));
        LinArgs *ls[2] = {&a.dyn, &a.obs};
        for (int i = 0; i < 2; ++i) {
            LinArgs &l = *ls[i];
            l.D = D; l.E = hs[i]->E; l.din = fi[i].din; l.fid = fs[i]->id;
            l.bcast = (fs[i]->n_idx == 0 && fi[i].din == 1 && D > 1) ? 1 : 0;       // (as launch_jacobian)
            l.cov_scale = l.ccov_scale = 1.0;
            fill_fpar(fs[i], &l.fp);
        }
        a.dyn.fp.ttab = p.ttab_dyn; a.obs.fp.ttab = p.ttab_obs;
        a.y = p.y; a.m0 = p.m0; a.P0 = p.P0; a.fm = p.fm; a.fP = p.fP; a.status = p.status;
        a.pm = pm; a.pP = pP; a.pC = pC;
        a.gqg = p.gqg; a.rr = p.rr; a.B = p.B; a.ld = p.ld; a.T = p.T;
        const int rc = hip_fail(e.fn[keep](a, p.s), e.name[keep]);
        return rc ? rc : 1;
    }
    return 0;
}

}  // namespace ssmq
