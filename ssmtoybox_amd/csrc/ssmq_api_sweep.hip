// C ABI of libssmq (include/ssmq.h), the kernel-parameter sweep of a BQ filter by measurement likelihood: the refusals, one
// theta-batched weights call per transform, the per-theta constant blocks and the one launch of k_filter_sweep<>
// (ssmq_filter_sweep.hip).
#include <string>
#include <vector>
#include "ssmq_filter_sweep_kernel.h"
#include "ssmq_host.h"

namespace ssmq {

const char *find_sweep_kernel(const FilterShape &shape);
int launch_sweep(const FilterShape &shape, const SweepArgs &a, hipStream_t s);

static const char kSweepRange[] =
    "filter_sweep: GP (kind 0) and Bayes-Sard (kind 1) transforms with the 'rbf' kernel on the built-in additive-noise model pairs of "
    "the fused time loop, D <= 6, Y <= 4, 2 <= N <= 2 D + 1 points (the same count for both transforms), Gaussian recursion";

static int sweep_refuse(int code, const std::string &why) {
    set_error(why + " - " + kSweepRange);
    return code;
}

// What both entry points check, in this order, before anything else happens; *shape: the key of the kernel's table.
static int sweep_route(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int kind_dyn, int kind_obs, int N_dyn, int N_obs, int D, int Y,
                       FilterShape *shape, const char **name) {
    if (!f_dyn || !f_obs || D < 1 || Y < 1 || N_dyn < 1 || N_obs < 1) return sweep_refuse(SSMQ_E_ARG, "filter_sweep: bad argument");
    auto kinds = [&]() {
        for (int kind : {kind_dyn, kind_obs})
            if (kind != SSMQ_SWEEP_GP && kind != SSMQ_SWEEP_BS)
                return sweep_refuse(SSMQ_E_UNSUPPORTED, "filter_sweep: the t-process and multi-output models are not implemented");
        return (int)SSMQ_OK;
    };
    int selo = 0;
    if (int rc = additive_pair_route(sweep_refuse, "filter_sweep", f_dyn, f_obs, D, kinds, &selo)) return rc;
    if (D > 6 || Y > 4) return sweep_refuse(SSMQ_E_UNSUPPORTED, "filter_sweep: dimension out of range");
    if (N_dyn > 2 * D + 1 || N_obs > 2 * D + 1 || N_dyn < 2 || N_obs < 2)
        return sweep_refuse(SSMQ_E_UNSUPPORTED, "filter_sweep: point count out of range");
    *shape = {f_dyn->id, f_obs->id, D, Y, N_dyn, N_obs, SSMQ_FORM_BQ, 0, selo, 0};
    const char *kn = selo < 0 ? nullptr : find_sweep_kernel(*shape);
    if (!kn) return sweep_refuse(SSMQ_E_UNSUPPORTED, "filter_sweep: no kernel for this pair of models and point sets");
    if (name) *name = kn;
    return SSMQ_OK;
}

// The weights of P parameter rows of one transform (host arrays, the layouts of ssmq_weights_gp): status [P]; < 0: error
static int sweep_weights(int kind, int D, int N, const double *xi, const double *par, int P, double jitter, const int32_t *mulind, int NB,
                         std::vector<double> &wm, std::vector<double> &Wc, std::vector<double> &Wcc, std::vector<double> &mv,
                         std::vector<int32_t> &st) {
    wm.assign((size_t)P * N, 0.0); Wc.assign((size_t)P * N * N, 0.0); Wcc.assign((size_t)P * D * N, 0.0); mv.assign(P, 0.0); st.assign(P, 0);
    const int rc = kind == SSMQ_SWEEP_GP
                       ? ssmq_weights_gp(D, N, xi, par, P, jitter, wm.data(), Wc.data(), Wcc.data(), nullptr, nullptr, nullptr, nullptr, mv.data(),
                                         nullptr, st.data())
                       : ssmq_weights_bs(D, N, xi, par, P, jitter, mulind, NB, wm.data(), Wc.data(), Wcc.data(), nullptr, nullptr, nullptr, nullptr,
                                         mv.data(), nullptr, st.data());
    return rc < 0 ? rc : SSMQ_OK;
}

// Row p's constant block as upload_consts (ssmq_api_transform.hip) lays out the dense part of a BQ handle's: points and Wc
// transposed, emv = model_var on every entry (the kernels read the diagonal: SSMQ_EMV_DIAG), the rest - t-process inverse, fast-path
// data, point records: nothing the dense kernels read - zero.  (Also the dense part of the t-process blocks: ssmq_api_score.hip.)
void sweep_block(int D, int E, int N, const double *xi, const double *wm, const double *Wc, const double *Wcc, double model_var, double *s) {
    const ConstLayout cs = const_layout(D, E, N, SSMQ_FORM_BQ);
    std::fill(s, s + cs.total, 0.0);
    for (int d = 0; d < D; ++d)
        for (int n = 0; n < N; ++n) {
            s[cs.xi + n * D + d] = xi[d * N + n];
            s[cs.Wcc + d * N + n] = Wcc[d * N + n];
        }
    for (int n = 0; n < N; ++n) s[cs.wm + n] = wm[n];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) s[cs.Wc + j * N + i] = Wc[i * N + j];
    for (int i = 0; i < E * E; ++i) s[cs.emv + i] = model_var;
}

}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_filter_sweep_kernel_name(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int kind_dyn, int kind_obs, int N_dyn,
                                             int N_obs, int D, int Y, char *buf, int len) {
    if (!buf || len <= 0) return sweep_refuse(SSMQ_E_ARG, "filter_sweep: bad argument");
    FilterShape shape;
    const char *name = nullptr;
    if (int rc = sweep_route(f_dyn, f_obs, kind_dyn, kind_obs, N_dyn, N_obs, D, Y, &shape, &name)) return rc;
    snprintf(buf, len, "%s", name);
    return SSMQ_OK;
}

extern "C" int ssmq_filter_sweep_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int kind_dyn, int kind_obs, const double *xi_dyn,
                                     int N_dyn, const double *xi_obs, int N_obs, const int32_t *mulind_dyn, int NB_dyn, const int32_t *mulind_obs,
                                     int NB_obs, const double *par_dyn, const double *par_obs, int P, double jitter_dyn, double jitter_obs, int D,
                                     int Y, int64_t B, int64_t ld, int T, const double *d_y, const double *x0_mean, const double *x0_cov,
                                     const double *GQG, const double *R, double *d_loglik_total, double *d_nis_mean, double *d_loglik_steps,
                                     int32_t *d_status, int32_t *theta_status) {
    FilterShape shape;
    if (int rc = sweep_route(f_dyn, f_obs, kind_dyn, kind_obs, N_dyn, N_obs, D, Y, &shape, nullptr)) return rc;
    if (!xi_dyn || !xi_obs || !par_dyn || !par_obs || P < 1 || B < 0 || ld < B || ld % kSmallBlock != 0 || T < 0 || !d_y || !x0_mean || !x0_cov ||
        !d_loglik_total || !d_nis_mean || !d_status || !theta_status || (kind_dyn == SSMQ_SWEEP_BS && (!mulind_dyn || NB_dyn < 1 || NB_dyn > N_dyn)) ||
        (kind_obs == SSMQ_SWEEP_BS && (!mulind_obs || NB_obs < 1 || NB_obs > N_obs)))
        return sweep_refuse(SSMQ_E_ARG, "filter_sweep: bad argument (P >= 1, ld a multiple of 64 and >= B, at most N basis functions)");
    if ((int64_t)P * (ld / kSmallBlock) >= (int64_t)1 << 31) return sweep_refuse(SSMQ_E_ARG, "filter_sweep: P * ld / 64 must stay below 2^31");
    if (int rc = ensure_device()) return rc;
    // ---- the weights of every row, one theta-batched call per transform ------------------------------------------------------
    std::vector<double> wm[2], Wc[2], Wcc[2], mv[2];
    std::vector<int32_t> st[2];
    int rc;
    if ((rc = sweep_weights(kind_dyn, D, N_dyn, xi_dyn, par_dyn, P, jitter_dyn, mulind_dyn, NB_dyn, wm[0], Wc[0], Wcc[0], mv[0], st[0])) ||
        (rc = sweep_weights(kind_obs, D, N_obs, xi_obs, par_obs, P, jitter_obs, mulind_obs, NB_obs, wm[1], Wc[1], Wcc[1], mv[1], st[1])))
        return rc;
    for (int p = 0; p < P; ++p) theta_status[p] = st[0][p] + 4 * st[1][p];
    if (B == 0) return SSMQ_OK;
    if (T == 0) return score_empty("filter_sweep", P, ld, theta_status, d_loglik_total, d_nis_mean, d_status);
    // ---- one host image: c_dyn [P][block] | c_obs [P][block] | pass constants | m0 | P0 | theta_status ----------------------
    const size_t nd = const_layout(D, D, N_dyn, SSMQ_FORM_BQ).total, no = const_layout(D, Y, N_obs, SSMQ_FORM_BQ).total;
    const size_t npc = pass_consts_doubles(D, Y, T), nx0 = ((size_t)D + (size_t)D * D + 7) / 8 * 8;
    const size_t n_dbl = P * nd + P * no + npc + nx0;
    std::vector<double> host(n_dbl + ((size_t)P + 1) / 2, 0.0);
    for (int p = 0; p < P; ++p) {
        sweep_block(D, D, N_dyn, xi_dyn, wm[0].data() + (size_t)p * N_dyn, Wc[0].data() + (size_t)p * N_dyn * N_dyn,
                    Wcc[0].data() + (size_t)p * D * N_dyn, mv[0][p], host.data() + p * nd);
        sweep_block(D, Y, N_obs, xi_obs, wm[1].data() + (size_t)p * N_obs, Wc[1].data() + (size_t)p * N_obs * N_obs,
                    Wcc[1].data() + (size_t)p * D * N_obs, mv[1][p], host.data() + P * nd + p * no);
    }
    double *hpc = host.data() + P * nd + P * no, *hx0 = hpc + npc;
    const PassConsts pc = fill_pass_consts(hpc, f_dyn, f_obs, D, Y, T, GQG, R, nullptr);
    std::copy(x0_mean, x0_mean + D, hx0);
    std::copy(x0_cov, x0_cov + (size_t)D * D, hx0 + D);
    memcpy(host.data() + n_dbl, theta_status, sizeof(int32_t) * P);
    DeviceImage img;
    if ((rc = img.alloc(host.size()))) return rc;
    double *const dev = img.dev;
    hipStream_t s = stream();
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    a.y = d_y; a.c_dyn = dev; a.c_obs = dev + P * nd; a.gqg = dev + P * nd + P * no; a.rr = a.gqg + pc.rr; a.x0 = a.gqg + npc;
    a.theta_status = (const int32_t *)(dev + n_dbl);
    a.ll_total = d_loglik_total; a.nis_mean = d_nis_mean; a.ll_steps = d_loglik_steps; a.status = d_status;
    a.B = B; a.ld = ld; a.T = T; a.P = P; a.nblk = (int32_t)(ld / kSmallBlock);
    a.emv_dyn = a.emv_obs = SSMQ_EMV_DIAG;
    fill_fpar(f_dyn, &a.fd);
    fill_fpar(f_obs, &a.fo);
    a.fd.ttab = pc.has_ttab_dyn ? a.gqg + pc.ttab_dyn : nullptr;
    a.fo.ttab = pc.has_ttab_obs ? a.gqg + pc.ttab_obs : nullptr;
    rc = img.upload(host, "filter_sweep: upload");
    if (!rc) rc = launch_sweep(shape, a, s);
    const int rs = hip_fail(hipStreamSynchronize(s), "filter_sweep");
    return rc ? rc : rs;
}
