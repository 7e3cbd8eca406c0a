// C ABI of libssmq (include/ssmq.h), the filters: the time loop with its per-context workspace and captured launch graph
// (FilterCache), the filter for models that take their noise as an argument, both smoothers, the Student filter, the error sums
// over filtered trajectories and the simulator.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "ssmq_host.h"
#include "ssmq_fused.h"

using namespace ssmq;

namespace {
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return hip_fail(hipMalloc(&p, bytes ? bytes : 8), "hipMalloc"); }
    double *d() { return (double *)p; }
};
}  // namespace

// ---- filter recursion around the path ---------------------------------------------------------------------------------
extern "C" {
int ssmq_kalman_update_dev(int D, int Y, int64_t B, int64_t ld, const double *d_m_pr, const double *d_P_pr,
                           const double *d_y_mean, const double *d_P_y, const double *d_P_yx, const double *d_y,
                           double *d_m_fi, double *d_P_fi, int32_t *d_status) {
    if (D < 1 || Y < 1 || B < 0 || ld < B || !d_m_pr || !d_P_pr || !d_y_mean || !d_P_y || !d_P_yx || !d_y || !d_m_fi ||
        !d_P_fi || !d_status)
        return SSMQ_E_ARG;
    if (D > SSMQ_MAX_DIM || Y > SSMQ_MAX_DIM) {   // refused before the status words are cleared: a refused call writes nothing
        set_error("kalman update: D or Y above SSMQ_MAX_DIM");
        return SSMQ_E_UNSUPPORTED;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * B, stream()));
    return launch_kalman_update(D, Y, B, ld, d_m_pr, d_P_pr, d_y_mean, d_P_y, d_P_yx, d_y, d_m_fi, d_P_fi, d_status,
                                stream());
}
}  // extern "C"

namespace {
// Grow-only device workspace + captured launch sequence of the filter loop, kept between calls so that a repeated
// forward pass (Monte-Carlo studies, bench.py) neither allocates nor pays 3 T kernel-launch latencies: the whole time
// loop is replayed as one hipGraph while the argument set is unchanged.
struct FilterCache {
    void *ws = nullptr;               // planes of the launch loop and its two status planes
    size_t ws_bytes = 0;
    void *consts = nullptr;           // the pass's constants (PassConsts layout, ssmq_host.h) of every single-filter route, grow-only ...
    size_t consts_bytes = 0;
    std::vector<double> consts_host;  // ... and what the block holds
    void *robust = nullptr;           // R | R^-1 of the outlier-robust pass, [Y*Y] each, grow-only ...
    size_t robust_bytes = 0;
    std::vector<double> robust_host;  // ... and what the block holds
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<uint64_t> key;
    void drop_graph() {
        if (exec) hipGraphExecDestroy(exec);
        if (graph) hipGraphDestroy(graph);
        exec = nullptr;
        graph = nullptr;
        key.clear();
    }
};
FilterCache &fc_of_ctx() {
    Ctx &c = ssmq::ctx();
    if (!c.fc) c.fc = new FilterCache;
    return *(FilterCache *)c.fc;
}
#define g_fc (fc_of_ctx())
// drops the captured loop on every exit of a scope whose temporaries the graph points into
struct GraphDropGuard {
    ~GraphDropGuard() { g_fc.drop_graph(); }
};

// The constants of one pass in the context's block: filled on the host, uploaded when they differ from what the block holds.
// The captured launch loop reads the block and has the scale baked into its kernel arguments by value, so any change drops it.
int cached_pass_consts(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int T, const double *GQG, const double *R,
                       const double *sscale, hipStream_t s, PassConsts *pc) {
    FilterCache &c = g_fc;
    std::vector<double> h(pass_consts_doubles(D, Y, T));
    *pc = fill_pass_consts(h.data(), f_dyn, f_obs, D, Y, T, GQG, R, sscale);
    const size_t need = sizeof(double) * h.size();
    if (h == c.consts_host) return SSMQ_OK;
    c.drop_graph();
    c.consts_host.clear();
    if (c.consts_bytes < need) {
        if (c.consts) {
            SSMQ_HIP(hipStreamSynchronize(s));
            hipFree(c.consts);
        }
        c.consts = nullptr;
        c.consts_bytes = 0;
        SSMQ_HIP(hipMalloc(&c.consts, need));
        c.consts_bytes = need;
    }
    // (stream order: earlier passes that read the block are done before the copy lands)
    SSMQ_HIP(hipMemcpyAsync(c.consts, h.data(), need, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    c.consts_host.swap(h);
    return SSMQ_OK;
}
}  // namespace

namespace ssmq {
void drop_filter_cache() {
    g_fc.drop_graph();
    if (g_fc.ws) hipFree(g_fc.ws);
    if (g_fc.consts) hipFree(g_fc.consts);
    if (g_fc.robust) hipFree(g_fc.robust);
    g_fc.ws = g_fc.consts = g_fc.robust = nullptr;
    g_fc.ws_bytes = g_fc.consts_bytes = g_fc.robust_bytes = 0;
    g_fc.consts_host.clear();
    g_fc.robust_host.clear();
}

// Which of the launch loop's special forms a pair of an additive-noise Gaussian filter has, after the refusals every entry point
// of the time loop makes for them (keep: the predictive moments are kept for a smoother; student: Studentian recursion)
struct PairForms {
    bool user, mo, trunc, gq;
};
static int pair_forms(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                      bool keep, bool student, PairForms *out) {
    const bool user = is_user_integrand(f_dyn) || is_user_integrand(f_obs);
    if (user && keep) return refuse_user_integrand("smoother (predictive moments kept)");
    // a multi-output transform: the Gaussian forward pass through the launch loop, nothing else
    const bool mo = is_mo(h_dyn) || is_mo(h_obs);
    if (mo && user) return refuse_user_integrand("multi-output transform (k_apply_mo)");
    if (mo && keep) return refuse_mo("smoother (predictive moments kept)");
    if (mo && student) return refuse_mo("Studentian filter");
    // a truncated sigma-point transform: the measurement transform of the Gaussian launch loop (forward pass and smoother) next to
    // a sigma-point dynamics transform, nothing else
    const bool trunc = is_trunc(h_obs);
    if (trunc && h_dyn->form != SSMQ_FORM_SIGMA) return refuse_trunc("filter whose dynamics transform is not a sigma-point rule");
    if (trunc && user) return refuse_user_integrand("truncated sigma-point transform (k_apply_trunc)");
    if (trunc && student) return refuse_trunc("Studentian filter");
    // GPQ with derivative observations: both transforms of this form, the Gaussian launch loop (forward pass and smoother)
    const bool gq = is_gpqd(h_dyn) || is_gpqd(h_obs);
    if (gq && !(is_gpqd(h_dyn) && is_gpqd(h_obs))) return refuse_gpqd("filter with only one GPQ+D transform");
    if (gq && student) return refuse_gpqd("Studentian filter");
    *out = {user, mo, trunc, gq};
    return SSMQ_OK;
}

// A pair with a user member whose both transforms read a Jacobian (linearisation, Taylor-GPQD, GPQ+D) runs the launch loop, each
// transform of a user member a launch of the kernel compiled for it at run time: compiled and loaded here - a stream that is being
// captured must not meet a compile - and a member without a Jacobian is refused here.
static int prepare_user_ekf(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                            bool gq) {
    const ssmq_transform *hs2[2] = {h_dyn, h_obs};
    const ssmq_integrand *fs2[2] = {f_dyn, f_obs};
    for (int i = 0; i < 2; ++i) {
        FInfo fi;
        int rc = check_integrand(hs2[i], fs2[i], &fi);
        if (rc) return rc;
        if (is_user_integrand(fs2[i])) {
            if ((rc = gq ? rtc_prepare_gpqd(hs2[i], fs2[i]) : rtc_prepare_jacobian(hs2[i], fs2[i]))) return rc;
        } else if (!integrand_has_jacobian(fs2[i]->id)) {
            set_error("filter_forward: built-in integrand " + std::to_string(fs2[i]->id) + " has no Jacobian (its dyn_fcn_dx / meas_fcn_dx "
                      "returns None in the reference too)");
            return SSMQ_E_UNSUPPORTED;
        }
    }
    return SSMQ_OK;
}
static bool jac_form(const ssmq_transform *h) { return h->form == SSMQ_FORM_TAYLOR1 || is_taylor_gpqd(h); }

// the plane workspace of the launch loops, grow-only (a captured loop points into it: growing drops the graph)
static int ensure_ws(size_t need) {
    if (g_fc.ws_bytes >= need) return SSMQ_OK;
    g_fc.drop_graph();
    if (g_fc.ws) hipFree(g_fc.ws);
    g_fc.ws = nullptr;
    g_fc.ws_bytes = 0;
    SSMQ_HIP(hipMalloc(&g_fc.ws, need));
    g_fc.ws_bytes = need;
    return SSMQ_OK;
}

int make_filter_pass(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                     int64_t B, int64_t ld, int T, const double *y, const double *m0, const double *P0, double *fm, double *fP,
                     int32_t *status, hipStream_t stream, FilterPass *out) {
    FInfo fio;
    if (!integrand_info(f_obs->id, &fio)) {
        set_error("unknown integrand id");
        return SSMQ_E_ARG;
    }
    FilterPass p;
    p.hd = h_dyn; p.fd = f_dyn; p.ho = h_obs; p.fo = f_obs; p.sel_obs = sel_pattern(f_obs, fio.din);
    p.B = B; p.ld = ld; p.T = T; p.y = y; p.m0 = m0; p.P0 = P0; p.fm = fm; p.fP = fP; p.status = status; p.s = stream;
    *out = p;
    return SSMQ_OK;
}

// sscale (host, [T]) / student_dof: Studentian recursion (ssinf.py:634-736); null / 0 for the Gaussian filters.
int filter_forward_impl(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                               const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y,
                               const double *d_m0, const double *d_P0, const double *GQG, const double *R,
                               double *d_fm, double *d_fP, int32_t *d_status, const double *sscale,
                               double student_dof, double *d_pm, double *d_pP, double *d_pC) {
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || B < 0 || ld < B || T < 0 || !d_y || !d_m0 || !d_P0 || !d_fm || !d_fP ||
        !d_status) {
        set_error("filter_forward: bad argument");
        return SSMQ_E_ARG;
    }
    if (is_trunc(h_dyn)) return refuse_trunc("filter with a truncated DYNAMICS transform");
    const int D = h_dyn->D, Y = h_obs->E;
    if (h_dyn->E != D || h_obs->D != D) {
        set_error("filter_forward: additive-noise filter needs dyn (D -> D) and obs (D -> Y) transforms");
        return SSMQ_E_ARG;
    }
    PairForms pf;
    if (int rf = pair_forms(h_dyn, f_dyn, h_obs, f_obs, d_pm || d_pP || d_pC, sscale || student_dof != 0.0, &pf)) return rf;
    const bool user = pf.user, mo = pf.mo, trunc = pf.trunc, gq = pf.gq;
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    if (T == 0) {   // nothing to filter: every trajectory is trivially fine
        SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * ld, stream()));
        return SSMQ_OK;
    }
    hipStream_t s = stream();
    FilterPass pass;
    PassConsts pc;
    if ((rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_status, s, &pass)) ||
        (rc = cached_pass_consts(f_dyn, f_obs, D, Y, T, GQG, R, sscale, s, &pc)))
        return rc;
    const double *cs = (const double *)g_fc.consts, *gqg = cs, *rr = cs + pc.rr, *tvec = cs + pc.steps;
    const double *hs = g_fc.consts_host.data() + pc.scale;      // the scale on the host: ones for a Gaussian filter
    wire_pass_consts(pass, cs, pc);
    pass.student_dof = student_dof;
    // A pair of models of which one or both are user-defined integrands: the whole-pass kernel compiled for them at run time
    // (ssmq_rtc.hip), or an error - and the launch loop for the extended Kalman filters alone (both transforms a linearisation or
    // Taylor-GPQD: no time-loop kernel reads a Jacobian), each transform of a user member a launch of the kernel compiled for it.
    // Those kernels are compiled and loaded here, before the loop is captured, and a member without a Jacobian is refused here.
    const bool user_ekf = user && ((jac_form(h_dyn) && jac_form(h_obs)) || gq);
    if (user && !user_ekf) return (rc = rtc_launch_fused(pass)) < 0 ? rc : SSMQ_OK;
    if (user_ekf && (rc = prepare_user_ekf(h_dyn, f_dyn, h_obs, f_obs, gq))) return rc;
    // workspace carve-up (doubles first, then the two int32 status planes)
    const size_t n_dbl = (size_t)ld * (D + 3 * D * D + Y + Y * Y + Y * D);
    const size_t need = sizeof(double) * n_dbl + 2 * sizeof(int32_t) * (size_t)ld;
    if ((rc = ensure_ws(need))) return rc;
    double *w = (double *)g_fc.ws;
    double *m_pr = w; w += (size_t)ld * D;
    double *P_pr = w; w += (size_t)ld * D * D;
    double *C_xx = w; w += (size_t)ld * D * D;
    double *y_mean = w; w += (size_t)ld * Y;
    double *P_y = w; w += (size_t)ld * Y * Y;
    double *P_yx = w; w += (size_t)ld * Y * D;
    double *smat = w; w += (size_t)ld * D * D;   // Studentian: rescaled scale matrix fed to the next time update
    int32_t *st_a = (int32_t *)w, *st_b = st_a + ld;
    // one fused kernel for the whole time loop when this (models, shapes, form) combination has one (it does not keep
    // the predictive moments, so a pass that has to store them for the smoother takes the launch loop)
    const bool keep_pred = d_pm && d_pP && d_pC;
    if (!ssmq::sw("SSMQ_NO_FUSED") && !keep_pred && !mo && !user_ekf && !trunc && !gq) {
        rc = try_launch_fused(pass);
        if (rc < 0) return rc;
        if (rc == 1) return SSMQ_OK;
    }
    if (!ssmq::sw("SSMQ_NO_FUSED") && keep_pred && !sscale && student_dof == 0.0 && !trunc && !gq) {
        // smoother: the time loop in one kernel that also leaves the predictive moments of every step in HBM (the extended Kalman
        // filter's k_ekf_loop, or the sigma-point / BQ kernel)
        if (!mo && !user_ekf) {
            rc = try_launch_ekf_loop(pass, d_pm, d_pP, d_pC);
            if (rc < 0) return rc;
            if (rc == 1) return SSMQ_OK;
        }
        rc = try_launch_fused_aug(pass, AugExtras{D, 0, 0, gqg, rr, gqg, d_pm, d_pP, d_pC});    // (no noise inputs: the block is not read)
        if (rc < 0) return rc;
        if (rc == 1) return SSMQ_OK;
    }
    // which kernel variant apply_dev_impl picks depends on the handles' current constants: key_of_pair carries them
    std::vector<uint64_t> key;
    key_of_pair(key, h_dyn, f_dyn, h_obs, f_obs);
    for (const void *p : {(const void *)d_y, (const void *)d_m0, (const void *)d_P0, (const void *)d_fm, (const void *)d_fP,
                          (const void *)d_status, (const void *)g_fc.ws, (const void *)cs, (const void *)d_pm, (const void *)d_pP,
                          (const void *)d_pC})
        key.push_back((uint64_t)(uintptr_t)p);
    for (uint64_t v : {(uint64_t)B, (uint64_t)ld, (uint64_t)T, (uint64_t)(sscale ? 1 : 0)}) key.push_back(v);
    key_bytes(key, &student_dof, 8);
    if (!(g_fc.exec && g_fc.key == key)) {
        g_fc.drop_graph();
        SSMQ_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        rc = hip_fail(hipMemsetAsync(d_status, 0, sizeof(int32_t) * ld, s), "hipMemsetAsync");
        for (int k = 0; k < T && !rc; ++k) {
            const double *m_in = k == 0 ? d_m0 : d_fm + (int64_t)(k - 1) * D * ld;
            const double *P_in = k == 0 ? d_P0 : (student_dof > 0.0 ? smat : d_fP + (int64_t)(k - 1) * D * D * ld);
            if (keep_pred) {   // predictive moments of every step stay in HBM for the backward pass (ssinf.py:105-107)
                m_pr = d_pm + (int64_t)k * D * ld;
                P_pr = d_pP + (int64_t)k * D * D * ld;
                C_xx = d_pC + (int64_t)k * D * D * ld;
            }
            rc = apply_dev_impl(h_dyn, f_dyn, B, ld, m_in, P_in, tvec + k, 0, m_pr, P_pr, C_xx, st_a, gqg, nullptr, false,
                                hs[k], 1.0, pass.ttab_dyn, false);
            if (!rc)
                rc = apply_dev_impl(h_obs, f_obs, B, ld, m_pr, P_pr, tvec + k, 0, y_mean, P_y, P_yx, st_b, rr, nullptr,
                                    false, hs[k], hs[k], pass.ttab_obs, false);
            if (!rc)
                rc = launch_kalman_update_ex(D, Y, B, ld, m_pr, P_pr, y_mean, P_y, P_yx, d_y + (int64_t)k * Y * ld,
                                             d_fm + (int64_t)k * D * ld, d_fP + (int64_t)k * D * D * ld, d_status,
                                             st_a, st_b, k, s, student_dof, smat, 0);
        }
        hipGraph_t g = nullptr;
        hipError_t ce = hipStreamEndCapture(s, &g);
        if (rc) {
            if (g) hipGraphDestroy(g);
            return rc;
        }
        SSMQ_HIP(ce);
        g_fc.graph = g;
        SSMQ_HIP(hipGraphInstantiate(&g_fc.exec, g_fc.graph, nullptr, nullptr, 0));
        g_fc.key = key;
    }
    SSMQ_HIP(hipGraphLaunch(g_fc.exec, s));
    return SSMQ_OK;
}
}  // namespace ssmq

extern "C" int ssmq_filter_forward_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                       const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y,
                                       const double *d_m0, const double *d_P0, const double *GQG, const double *R,
                                       double *d_fm, double *d_fP, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    return filter_forward_impl(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, d_y, d_m0, d_P0, GQG, R, d_fm, d_fP, d_status,
                               nullptr, 0.0);
}

// Filters whose models take the noise as an argument (ssinf.py:271-272, 282-283, 294-295): the moments are augmented with
// the noise statistics before each transform and the cross-covariance is cut back to the state columns. Plain launch
// loop (augment | apply | augment | apply | update per step); no fused kernel and no graph cache for this path yet.
// d_pm / d_pP / d_pC (all or none): predictive mean [T][D][ld], covariance [T][D*D][ld] and dynamics cross-covariance of
// every step for the RTS pass; *c_cols returns the number of columns stored per row of d_pC (D from the fused kernel,
// D + dq from the launch loop, whose transform writes the full E x (D + dq) block: d_pC must hold T * D * (D + dq) planes).
static int filter_forward_aug_impl(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                   const ssmq_integrand *f_obs, int dim_state, int64_t B, int64_t ld, int T,
                                   const double *d_y, const double *d_m0, const double *d_P0, const double *q_mean,
                                   const double *q_cov, int dq, const double *r_mean, const double *r_cov, int dr,
                                   double *d_fm, double *d_fP, int32_t *d_status, double *d_pm, double *d_pP,
                                   double *d_pC, int *c_cols) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("filter with non-additive noise (augmented moments)");
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo("filter with non-additive noise (augmented moments)");
    if (is_trunc(h_dyn) || is_trunc(h_obs)) return refuse_trunc("filter with non-additive noise (augmented moments)");
    if (is_gpqd(h_dyn) || is_gpqd(h_obs)) return refuse_gpqd("filter with non-additive noise (augmented moments)");
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || dim_state <= 0 || dq < 0 || dr < 0 || B < 0 || ld < B || T < 0 || !d_y ||
        !d_m0 || !d_P0 || !d_fm || !d_fP || !d_status || (dq > 0 && (!q_mean || !q_cov)) ||
        (dr > 0 && (!r_mean || !r_cov))) {
        set_error("filter_forward_aug: bad argument");
        return SSMQ_E_ARG;
    }
    const int D = dim_state, Da = D + dq, Do = D + dr, Y = h_obs->E;
    if (h_dyn->D != Da || h_dyn->E != D || h_obs->D != Do) {
        set_error("filter_forward_aug: transforms must be (dim_state + dq -> dim_state) and (dim_state + dr -> dim_y)");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    if (T == 0) {
        SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * ld, s));
        SSMQ_HIP(hipStreamSynchronize(s));
        return SSMQ_OK;
    }
    // small constants first (the time tables and steps in the context's block, the noise statistics in a block of this call);
    // the plane workspace only if the launch loop is needed
    FilterPass pass;
    PassConsts pc;
    if ((rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_status, s, &pass)) ||
        (rc = cached_pass_consts(f_dyn, f_obs, D, Y, T, nullptr, nullptr, nullptr, s, &pc)))
        return rc;
    wire_pass_consts(pass, (const double *)g_fc.consts, pc);
    const double *tvec = pass.gqg + pc.steps, *ttab_d = pass.ttab_dyn, *ttab_o = pass.ttab_obs;
    DevBuf cs;
    if ((rc = cs.alloc(sizeof(double) * ((size_t)dq + (dq ? (size_t)dq * dq : (size_t)D * D) + dr + (dr ? (size_t)dr * dr : (size_t)Y * Y))))) return rc;
    double *w = cs.d();
    double *d_qm = w; w += dq;
    double *d_qc = w; w += dq ? (size_t)dq * dq : (size_t)D * D;
    double *d_rm = w; w += dr;
    double *d_rc = w; w += dr ? (size_t)dr * dr : (size_t)Y * Y;

    std::vector<double> zq((size_t)D * D, 0.0), zr((size_t)Y * Y, 0.0);
    if (dq) SSMQ_HIP(hipMemcpyAsync(d_qm, q_mean, sizeof(double) * dq, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(d_qc, q_cov ? q_cov : zq.data(), sizeof(double) * (dq ? (size_t)dq * dq : (size_t)D * D),
                            hipMemcpyHostToDevice, s));
    if (dr) SSMQ_HIP(hipMemcpyAsync(d_rm, r_mean, sizeof(double) * dr, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(d_rc, r_cov ? r_cov : zr.data(), sizeof(double) * (dr ? (size_t)dr * dr : (size_t)Y * Y),
                            hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * ld, s));
    SSMQ_HIP(hipStreamSynchronize(s));   // the host staging vectors above go out of scope with this call

    // one kernel for the whole time loop when this combination has an instantiation (ssmq_filter_fused.hip)
    if (!ssmq::sw("SSMQ_NO_FUSED")) {
        // noise block q_mean | q_cov | r_mean | r_cov and the additive terms (zeros for a non-additive model)
        std::vector<double> hn, ha((size_t)D * D + (size_t)Y * Y, 0.0);
        for (int i = 0; i < dq; ++i) hn.push_back(q_mean[i]);
        for (int i = 0; i < dq * dq; ++i) hn.push_back(q_cov[i]);
        for (int i = 0; i < dr; ++i) hn.push_back(r_mean[i]);
        for (int i = 0; i < dr * dr; ++i) hn.push_back(r_cov[i]);
        hn.push_back(0.0);
        if (!dq && q_cov) for (int i = 0; i < D * D; ++i) ha[i] = q_cov[i];
        if (!dr && r_cov) for (int i = 0; i < Y * Y; ++i) ha[(size_t)D * D + i] = r_cov[i];
        DevBuf dn, da;
        if ((rc = dn.alloc(sizeof(double) * hn.size())) || (rc = da.alloc(sizeof(double) * ha.size()))) return rc;
        SSMQ_HIP(hipMemcpyAsync(dn.p, hn.data(), sizeof(double) * hn.size(), hipMemcpyHostToDevice, s));
        SSMQ_HIP(hipMemcpyAsync(da.p, ha.data(), sizeof(double) * ha.size(), hipMemcpyHostToDevice, s));
        rc = try_launch_fused_aug(pass, AugExtras{D, dq, dr, da.d(), da.d() + (size_t)D * D, dn.d(), d_pm, d_pP, d_pC});
        hipError_t e = hipStreamSynchronize(s);
        if (rc < 0) return rc;
        SSMQ_HIP(e);
        if (rc == 1) {
            if (c_cols) *c_cols = D;
            return SSMQ_OK;
        }
        rc = 0;
    }

    DevBuf ws, st;
    const size_t n_dbl = (size_t)ld * (Da + Da * Da + D + D * D + D * Da + Do + Do * Do + Y + Y * Y + Y * Do);
    if ((rc = ws.alloc(sizeof(double) * n_dbl)) || (rc = st.alloc(2 * sizeof(int32_t) * (size_t)ld))) return rc;
    w = ws.d();
    double *ma = w; w += (size_t)ld * Da;
    double *Pa = w; w += (size_t)ld * Da * Da;
    double *m_pr = w; w += (size_t)ld * D;
    double *P_pr = w; w += (size_t)ld * D * D;
    double *C_xx = w; w += (size_t)ld * D * Da;
    double *mo = w; w += (size_t)ld * Do;
    double *Po = w; w += (size_t)ld * Do * Do;
    double *y_mean = w; w += (size_t)ld * Y;
    double *P_y = w; w += (size_t)ld * Y * Y;
    double *P_yx = w; w += (size_t)ld * Y * Do;
    int32_t *st_a = (int32_t *)st.p, *st_b = st_a + ld;

    if (c_cols) *c_cols = Da;
    for (int k = 0; k < T && !rc; ++k) {
        const double *m_in = k == 0 ? d_m0 : d_fm + (int64_t)(k - 1) * D * ld;
        const double *P_in = k == 0 ? d_P0 : d_fP + (int64_t)(k - 1) * D * D * ld;
        if (d_pm) {      // predictive moments of every step stay in HBM for the backward pass (ssinf.py:105-107)
            m_pr = d_pm + (int64_t)k * D * ld;
            P_pr = d_pP + (int64_t)k * D * D * ld;
            C_xx = d_pC + (int64_t)k * D * Da * ld;
        }
        if (dq) {
            rc = launch_augment(m_in, P_in, d_qm, d_qc, ma, Pa, D, dq, B, ld, s);
            if (!rc)
                rc = apply_dev_impl(h_dyn, f_dyn, B, ld, ma, Pa, tvec + k, 0, m_pr, P_pr, C_xx, st_a, nullptr, nullptr, false,
                                    1.0, 1.0, ttab_d, false);
        } else {
            rc = apply_dev_impl(h_dyn, f_dyn, B, ld, m_in, P_in, tvec + k, 0, m_pr, P_pr, C_xx, st_a, d_qc, nullptr, false,
                                1.0, 1.0, ttab_d, false);
        }
        if (rc) break;
        if (dr) {
            rc = launch_augment(m_pr, P_pr, d_rm, d_rc, mo, Po, D, dr, B, ld, s);
            if (!rc)
                rc = apply_dev_impl(h_obs, f_obs, B, ld, mo, Po, tvec + k, 0, y_mean, P_y, P_yx, st_b, nullptr, nullptr, false,
                                    1.0, 1.0, ttab_o, false);
        } else {
            rc = apply_dev_impl(h_obs, f_obs, B, ld, m_pr, P_pr, tvec + k, 0, y_mean, P_y, P_yx, st_b, d_rc, nullptr, false,
                                1.0, 1.0, ttab_o, false);
        }
        if (!rc)
            rc = launch_kalman_update_ex(D, Y, B, ld, m_pr, P_pr, y_mean, P_y, P_yx, d_y + (int64_t)k * Y * ld,
                                         d_fm + (int64_t)k * D * ld, d_fP + (int64_t)k * D * D * ld, d_status, st_a, st_b,
                                         k, s, 0.0, nullptr, Do);
    }
    hipError_t se = hipStreamSynchronize(s);   // workspace is released on return
    if (rc) return rc;
    SSMQ_HIP(se);
    return SSMQ_OK;
}

extern "C" int ssmq_filter_forward_aug_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                           const ssmq_integrand *f_obs, int dim_state, int64_t B, int64_t ld, int T,
                                           const double *d_y, const double *d_m0, const double *d_P0,
                                           const double *q_mean, const double *q_cov, int dq, const double *r_mean,
                                           const double *r_cov, int dr, double *d_fm, double *d_fP,
                                           int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    return filter_forward_aug_impl(h_dyn, f_dyn, h_obs, f_obs, dim_state, B, ld, T, d_y, d_m0, d_P0, q_mean, q_cov, dq,
                                   r_mean, r_cov, dr, d_fm, d_fP, d_status, nullptr, nullptr, nullptr, nullptr);
}

// Forward pass + RTS smoother for models that take their noise as an argument: backward_pass of the reference is model-
// agnostic (ssinf.py:120-147, 325-344); the cross-covariance it needs is the one _time_update cut back to the state
// columns (:294-295).  Arguments as ssmq_filter_forward_aug_dev, outputs as ssmq_filter_smooth_dev.  Synchronous.
extern "C" int ssmq_filter_smooth_aug_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                          const ssmq_integrand *f_obs, int dim_state, int64_t B, int64_t ld, int T,
                                          const double *d_y, const double *d_m0, const double *d_P0,
                                          const double *q_mean, const double *q_cov, int dq, const double *r_mean,
                                          const double *r_cov, int dr, double *d_fm, double *d_fP, double *d_sm,
                                          double *d_sP, int32_t *d_status) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("ssmq_filter_smooth_aug_dev");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo("ssmq_filter_smooth_aug_dev");
    if (is_trunc(h_dyn) || is_trunc(h_obs)) return refuse_trunc("ssmq_filter_smooth_aug_dev");
    if (is_gpqd(h_dyn) || is_gpqd(h_obs)) return refuse_gpqd("ssmq_filter_smooth_aug_dev");
    if (!h_dyn || !d_sm || !d_sP || dim_state <= 0 || dq < 0 || B < 0 || T < 0 || ld < B) {
        set_error("filter_smooth_aug: bad argument");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    const int D = dim_state;
    if (T == 0)
        return filter_forward_aug_impl(h_dyn, f_dyn, h_obs, f_obs, D, B, ld, T, d_y, d_m0, d_P0, q_mean, q_cov, dq, r_mean,
                                       r_cov, dr, d_fm, d_fP, d_status, nullptr, nullptr, nullptr, nullptr);
    DevBuf pm, pP, pC;
    if ((rc = pm.alloc(sizeof(double) * (size_t)T * D * ld)) || (rc = pP.alloc(sizeof(double) * (size_t)T * D * D * ld)) ||
        (rc = pC.alloc(sizeof(double) * (size_t)T * D * (D + dq) * ld)))
        return rc;
    int c_cols = D;
    rc = filter_forward_aug_impl(h_dyn, f_dyn, h_obs, f_obs, D, B, ld, T, d_y, d_m0, d_P0, q_mean, q_cov, dq, r_mean, r_cov,
                                 dr, d_fm, d_fP, d_status, pm.d(), pP.d(), pC.d(), &c_cols);
    if (rc) return rc;
    rc = launch_rts_backward(D, B, ld, T, d_fm, d_fP, pm.d(), pP.d(), pC.d(), d_sm, d_sP, d_status, stream(), c_cols);
    hipError_t e = hipStreamSynchronize(stream());
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

// backward_pass alone (ssinf.py:120-147, 325-344) over moments a caller kept from its own forward pass - the marginalised
// filter, whose forward pass is driven from the host (BFGS per step)
extern "C" int ssmq_rts_backward_dev(int D, int64_t B, int64_t ld, int T, const double *d_fm, const double *d_fP,
                                     const double *d_pm, const double *d_pP, const double *d_pC, double *d_sm, double *d_sP,
                                     int32_t *d_status) {
    if (D < 1 || B < 0 || T < 0 || ld < B || !d_fm || !d_fP || !d_pm || !d_pP || !d_pC || !d_sm || !d_sP || !d_status) {
        set_error("rts_backward: bad argument");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0 || T == 0) return SSMQ_OK;
    rc = launch_rts_backward(D, B, ld, T, d_fm, d_fP, d_pm, d_pP, d_pC, d_sm, d_sP, d_status, stream(), D);
    hipError_t e = hipStreamSynchronize(stream());
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

extern "C" int ssmq_filter_smooth_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                      const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y,
                                      const double *d_m0, const double *d_P0, const double *GQG, const double *R,
                                      double *d_fm, double *d_fP, double *d_sm, double *d_sP, int32_t *d_status) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("ssmq_filter_smooth_dev");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo("ssmq_filter_smooth_dev");
    if (is_trunc(h_dyn)) return refuse_trunc("ssmq_filter_smooth_dev with a truncated DYNAMICS transform");
    if (!h_dyn || !d_sm || !d_sP || B < 0 || T < 0 || ld < B) {
        set_error("filter_smooth: bad argument");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    if (T == 0) {
        if (d_status) SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * ld, stream()));
        SSMQ_HIP(hipStreamSynchronize(stream()));
        return SSMQ_OK;
    }
    const int D = h_dyn->D;
    DevBuf pm, pP, pC;
    if ((rc = pm.alloc(sizeof(double) * (size_t)T * D * ld)) || (rc = pP.alloc(sizeof(double) * (size_t)T * D * D * ld)) ||
        (rc = pC.alloc(sizeof(double) * (size_t)T * D * D * ld)))
        return rc;
    // a captured launch loop points into pm / pP / pC, which are released when this call returns - on every path
    GraphDropGuard drop_on_exit;
    rc = filter_forward_impl(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, d_y, d_m0, d_P0, GQG, R, d_fm, d_fP, d_status,
                             nullptr, 0.0, pm.d(), pP.d(), pC.d());
    if (rc) return rc;
    rc = launch_rts_backward(D, B, ld, T, d_fm, d_fP, pm.d(), pP.d(), pC.d(), d_sm, d_sP, d_status, stream(), D);
    if (rc) {
        hipStreamSynchronize(stream());
        return rc;
    }
    SSMQ_HIP(hipStreamSynchronize(stream()));
    return SSMQ_OK;
}

extern "C" int ssmq_student_filter_forward_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn,
                                               ssmq_transform *h_obs, const ssmq_integrand *f_obs, int64_t B,
                                               int64_t ld, int T, const double *d_y, const double *d_m0,
                                               const double *d_S0, const double *GqG, const double *r_smat,
                                               const double *scale, double dof, double *d_fm, double *d_fP,
                                               int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo("ssmq_student_filter_forward_dev");
    if (is_trunc(h_dyn) || is_trunc(h_obs)) return refuse_trunc("ssmq_student_filter_forward_dev");
    if (is_gpqd(h_dyn) || is_gpqd(h_obs)) return refuse_gpqd("ssmq_student_filter_forward_dev");
    if (!scale || !(dof > 0.0)) {
        set_error("student_filter_forward: scale[T] and dof > 0 are required");
        return SSMQ_E_ARG;
    }
    return filter_forward_impl(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, d_y, d_m0, d_S0, GqG, r_smat, d_fm, d_fP, d_status,
                               scale, dof);
}

extern "C" int ssmq_filter_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn,
                                       const ssmq_transform *h_obs, const ssmq_integrand *f_obs, char *buf, int len) {
    return ssmq_filter_kernel_name_batch(h_dyn, f_dyn, h_obs, f_obs, 0, buf, len);
}

extern "C" int ssmq_filter_kernel_name_batch(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                             const ssmq_integrand *f_obs, int64_t B, char *buf, int len) {
    return ssmq_filter_kernel_name_shape(h_dyn, f_dyn, h_obs, f_obs, B, 0, 0, buf, len);
}

extern "C" int ssmq_filter_kernel_name_shape(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                             const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, char *buf, int len) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || !buf || len <= 0 || B < 0 || ld < 0 || T < 0 || (ld > 0 && ld < B)) return SSMQ_E_ARG;
    const char *name = nullptr;
    FilterPass query;
    int rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &query);
    if (rc) return rc;
    query.name = &name; query.dry_run = true;
    const bool mo = is_mo(h_dyn) || is_mo(h_obs);       // no fused time loop takes the multi-output form
    if (mo && (is_user_integrand(f_dyn) || is_user_integrand(f_obs))) return refuse_user_integrand("multi-output transform (k_apply_mo)");
    // (the extended Kalman filters of a user model run the launch loop: filter_forward_impl)
    const bool ekf = (h_dyn->form == SSMQ_FORM_TAYLOR1 || is_taylor_gpqd(h_dyn)) && (h_obs->form == SSMQ_FORM_TAYLOR1 || is_taylor_gpqd(h_obs));
    const bool user = is_user_integrand(f_dyn) || is_user_integrand(f_obs);
    // (a truncated measurement transform runs the launch loop: filter_forward_impl, which also makes the refusals)
    if (is_trunc(h_dyn)) return refuse_trunc("filter with a truncated DYNAMICS transform");
    if (is_trunc(h_obs) && h_dyn->form != SSMQ_FORM_SIGMA) return refuse_trunc("filter whose dynamics transform is not a sigma-point rule");
    if (is_trunc(h_obs) && user) return refuse_user_integrand("truncated sigma-point transform (k_apply_trunc)");
    const bool gq = is_gpqd(h_dyn) || is_gpqd(h_obs);      // (both, or filter_forward_impl refuses: the launch loop)
    if (gq && !(is_gpqd(h_dyn) && is_gpqd(h_obs))) return refuse_gpqd("filter with only one GPQ+D transform");
    rc = mo || gq || is_trunc(h_obs) || (user && ekf) || (ssmq::sw("SSMQ_NO_FUSED") && !user) ? 0 : try_launch_fused(query);
    if (rc < 0) return rc;
    snprintf(buf, len, "%s", rc == 1 ? name : "hipGraph of 3 T launches (apply dyn | apply obs | k_kalman_update)");
    return SSMQ_OK;
}

// ---- innovation scores of a pass (include/ssmq.h: ssmq_filter_innovations_dev) --------------------------------------------------
// The checks both entry points share, in the order of filter_forward_impl; the one-launch route is asked for where that function
// asks for the fused time loop (SSMQ_NO_FUSED switches it off for the table shapes, as there).
static const char kInnovLoopName[] = "launch loop of 3 T launches (apply dyn | apply obs | k_innovation_score)";
static int innovations_route(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                             const ssmq_integrand *f_obs, PairForms *pf, bool *user_ekf, bool *one_launch) {
    if (is_trunc(h_dyn)) return refuse_trunc("innovation scores with a truncated DYNAMICS transform");
    if (h_dyn->E != h_dyn->D || h_obs->D != h_dyn->D) {
        set_error("filter_innovations: additive-noise Gaussian recursion only (dyn D -> D, obs D -> Y): models that take their noise as an "
                  "argument are not implemented");
        return SSMQ_E_UNSUPPORTED;
    }
    if (int rc = pair_forms(h_dyn, f_dyn, h_obs, f_obs, false, false, pf)) return rc;
    *user_ekf = pf->user && ((jac_form(h_dyn) && jac_form(h_obs)) || pf->gq);
    *one_launch = (pf->user && !*user_ekf) || (!ssmq::sw("SSMQ_NO_FUSED") && !pf->user && !pf->mo && !pf->trunc && !pf->gq);
    return SSMQ_OK;
}

extern "C" int ssmq_filter_innovations_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                           const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y,
                                           const double *d_m0, const double *d_P0, const double *d_fm, const double *d_fP,
                                           const double *GQG, const double *R, double *d_ymean, double *d_S, double *d_nis,
                                           double *d_ll, double *d_total, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || B < 0 || ld < B || T < 0 || !d_y || !d_m0 || !d_P0 || !d_fm || !d_fP || !d_nis ||
        !d_ll || !d_total || !d_status) {
        set_error("filter_innovations: bad argument");
        return SSMQ_E_ARG;
    }
    PairForms pf;
    bool user_ekf = false, one_launch = false;
    int rc = innovations_route(h_dyn, f_dyn, h_obs, f_obs, &pf, &user_ekf, &one_launch);
    if (rc) return rc;
    const int D = h_dyn->D, Y = h_obs->E;
    if ((rc = ensure_device())) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    if (T == 0) {   // nothing to score: every trajectory is trivially fine, its totals are empty sums
        SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * ld, s));
        SSMQ_HIP(hipMemsetAsync(d_total, 0, sizeof(double) * 2 * ld, s));
        return SSMQ_OK;
    }
    FilterPass pass;
    PassConsts pc;
    // (the pass's fm / fP are the filtered moments here: read, never written)
    if ((rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, d_y, d_m0, d_P0, const_cast<double *>(d_fm),
                               const_cast<double *>(d_fP), d_status, s, &pass)) ||
        (rc = cached_pass_consts(f_dyn, f_obs, D, Y, T, GQG, R, nullptr, s, &pc)))
        return rc;
    const double *cs = (const double *)g_fc.consts, *gqg = cs, *rr = cs + pc.rr, *tvec = cs + pc.steps;
    wire_pass_consts(pass, cs, pc);
    const InnovOut out{d_ymean, d_S, d_nis, d_ll};
    rc = one_launch ? try_launch_innovation(pass, out) : 0;
    if (rc < 0) return rc;
    if (rc == 0) {
        if (pf.user && !user_ekf) {
            set_error("filter_innovations: no run-time kernel for this pair of user integrands");
            return SSMQ_E_UNSUPPORTED;
        }
        if (user_ekf && (rc = prepare_user_ekf(h_dyn, f_dyn, h_obs, f_obs, pf.gq))) return rc;
        // the launch loop: per step apply dyn on plane k - 1 | apply obs | k_innovation_score, on the filter's workspace
        const size_t n_dbl = (size_t)ld * (D + 3 * D * D + Y + Y * Y + Y * D);
        if ((rc = ensure_ws(sizeof(double) * n_dbl + 2 * sizeof(int32_t) * (size_t)ld))) return rc;
        double *w = (double *)g_fc.ws;
        double *m_pr = w; w += (size_t)ld * D;
        double *P_pr = w; w += (size_t)ld * D * D;
        double *C_xx = w; w += (size_t)ld * D * D;
        double *y_mean = w; w += (size_t)ld * Y;
        double *P_y = w; w += (size_t)ld * Y * Y;
        double *P_yx = w; w += (size_t)ld * Y * D;
        w += (size_t)ld * D * D;
        int32_t *st_a = (int32_t *)w, *st_b = st_a + ld;
        for (int k = 0; k < T && !rc; ++k) {
            const double *m_in = k == 0 ? d_m0 : d_fm + (int64_t)(k - 1) * D * ld;
            const double *P_in = k == 0 ? d_P0 : d_fP + (int64_t)(k - 1) * D * D * ld;
            rc = apply_dev_impl(h_dyn, f_dyn, B, ld, m_in, P_in, tvec + k, 0, m_pr, P_pr, C_xx, st_a, gqg, nullptr, false, 1.0, 1.0,
                                pass.ttab_dyn, false);
            if (!rc)
                rc = apply_dev_impl(h_obs, f_obs, B, ld, m_pr, P_pr, tvec + k, 0, y_mean, P_y, P_yx, st_b, rr, nullptr, false, 1.0, 1.0,
                                    pass.ttab_obs, false);
            if (!rc)
                rc = launch_innovation_score(D, Y, B, ld, d_y + (int64_t)k * Y * ld, y_mean, P_y, m_in, st_a, st_b,
                                             d_ymean ? d_ymean + (int64_t)k * Y * ld : nullptr,
                                             d_S ? d_S + (int64_t)k * Y * Y * ld : nullptr, d_nis + (int64_t)k * ld,
                                             d_ll + (int64_t)k * ld, s);
        }
        if (rc) return rc;
    }
    return launch_innovation_total(B, ld, T, d_nis, d_ll, d_total, d_status, s);
}

extern "C" int ssmq_innovations_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                            const ssmq_integrand *f_obs, int64_t B, char *buf, int len) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || !buf || len <= 0 || B < 0) return SSMQ_E_ARG;
    PairForms pf;
    bool user_ekf = false, one_launch = false;
    int rc = innovations_route(h_dyn, f_dyn, h_obs, f_obs, &pf, &user_ekf, &one_launch);
    if (rc) return rc;
    const char *name = nullptr;
    FilterPass query;
    if ((rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, B, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &query))) return rc;
    query.name = &name; query.dry_run = true;
    rc = one_launch ? try_launch_innovation(query, InnovOut{nullptr, nullptr, nullptr, nullptr}) : 0;
    if (rc < 0) return rc;
    snprintf(buf, len, "%s", rc == 1 ? name : kInnovLoopName);
    return SSMQ_OK;
}

// ---- the measurement-update variants: iterated posterior linearisation, outlier-robust, masked (include/ssmq.h) ------------------------
// The refusals and the route choice are those of the innovation scores (innovations_route); flag bit 0 forces the launch loop.  Each
// entry point keeps its null checks, its argument checks and its constants; what follows them is update_pass_dev / update_kernel_name.
static const char kIplfLoopName[] = "launch loop of (1 + 2 J) T launches (apply dyn | J x (apply obs | k_iplf_update))";
static const char kRobustLoopName[] = "launch loop of 3 T launches (apply dyn | apply obs | k_robust_update)";
static const char kMaskedLoopName[] = "launch loop of 3 T launches (apply dyn | apply obs | k_masked_update)";

// R | R^-1 as the host image of the variants' block of the context: false when R is not finite, not symmetric or not positive definite.  The
// inverse by Cholesky, R = L L': column j of R^-1 from L z = e_j, L' x = z; symmetrised by its lower triangle (the kernels read that).
static bool robust_consts(int Y, const double *R, std::vector<double> *out) {
    std::vector<double> L((size_t)Y * Y, 0.0), h(2 * (size_t)Y * Y, 0.0), v(Y);
    for (int i = 0; i < Y; ++i)
        for (int j = 0; j < Y; ++j)
            if (!std::isfinite(R[i * Y + j]) || R[i * Y + j] != R[j * Y + i]) return false;
    for (int j = 0; j < Y; ++j) {
        double ajj = R[j * Y + j];
        for (int k = 0; k < j; ++k) ajj -= L[j * Y + k] * L[j * Y + k];
        if (!(ajj > 0.0)) return false;
        L[j * Y + j] = std::sqrt(ajj);
        for (int i = j + 1; i < Y; ++i) {
            double s = R[i * Y + j];
            for (int k = 0; k < j; ++k) s -= L[i * Y + k] * L[j * Y + k];
            L[i * Y + j] = s / L[j * Y + j];
        }
    }
    for (int j = 0; j < Y; ++j) {
        for (int i = 0; i < Y; ++i) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= L[i * Y + k] * v[k];
            v[i] = s / L[i * Y + i];
        }
        for (int i = Y - 1; i >= 0; --i) {
            double s = v[i];
            for (int k = i + 1; k < Y; ++k) s -= L[k * Y + i] * v[k];
            v[i] = s / L[i * Y + i];
        }
        for (int i = j; i < Y; ++i) h[(size_t)Y * Y + i * Y + j] = h[(size_t)Y * Y + j * Y + i] = v[i];
    }
    std::copy(R, R + (size_t)Y * Y, h.begin());
    for (double x : h)
        if (!std::isfinite(x)) return false;
    out->swap(h);
    return true;
}

// ... uploaded when it differs from what the block holds (as cached_pass_consts)
static int cached_robust_consts(std::vector<double> &h, hipStream_t s) {
    FilterCache &c = g_fc;
    if (h == c.robust_host) return SSMQ_OK;
    const size_t need = sizeof(double) * h.size();
    c.robust_host.clear();
    if (c.robust_bytes < need) {
        if (c.robust) {
            SSMQ_HIP(hipStreamSynchronize(s));
            hipFree(c.robust);
        }
        c.robust = nullptr;
        c.robust_bytes = 0;
        SSMQ_HIP(hipMalloc(&c.robust, need));
        c.robust_bytes = need;
    }
    SSMQ_HIP(hipMemcpyAsync(c.robust, h.data(), need, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    c.robust_host.swap(h);
    return SSMQ_OK;
}

// The pass after the entry point's own checks.  PassIO: the planes and sizes every entry point takes.  UpdateVariant: what differs -
// who: the prefix of its errors; R_pass: what the measurement transform adds (R, or null: zeros); consts(Y, &host): the variant's own
// device block (R | R^-1, R | gate; left empty: none) or an error, checked where the entry points always checked it - after the
// route, before the device; try_launch(pass, block), loop(pass, block, tvec, ws): the variant's two routes, block = that block on
// the device (the iterated pass has none and ignores it).
struct PassIO {
    int64_t B, ld;
    int T;
    const double *d_y, *d_m0, *d_P0, *GQG;
    double *d_fm, *d_fP;
    int32_t *d_status;
};
template <class Consts, class Try, class Loop>
struct UpdateVariant {
    const char *who;
    const double *R_pass;
    Consts consts;       // int(int Y, std::vector<double> *host)
    Try try_launch;      // int(const FilterPass &pass, const double *block)
    Loop loop;           // int(const FilterPass &pass, const double *block, const double *tvec, void *ws)
};
template <class Consts, class Try, class Loop>
static UpdateVariant<Consts, Try, Loop> update_variant(const char *who, const double *R_pass, Consts consts, Try try_launch, Loop loop) {
    return {who, R_pass, consts, try_launch, loop};
}
template <class Variant>
static int update_pass_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                           const PassIO &io, bool force_loop, const Variant &v) {
    const int64_t B = io.B, ld = io.ld;
    const int T = io.T;
    PairForms pf;
    bool user_ekf = false, one_launch = false;
    int rc = innovations_route(h_dyn, f_dyn, h_obs, f_obs, &pf, &user_ekf, &one_launch);
    if (rc) return rc;
    if (force_loop && !pf.user) one_launch = false;      // (a user pair without Jacobians has no launch loop)
    const int D = h_dyn->D, Y = h_obs->E;
    std::vector<double> host;
    if ((rc = v.consts(Y, &host))) return rc;
    if ((rc = ensure_device())) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    if (T == 0) {   // nothing to filter: every trajectory is trivially fine
        SSMQ_HIP(hipMemsetAsync(io.d_status, 0, sizeof(int32_t) * ld, s));
        return SSMQ_OK;
    }
    FilterPass pass;
    PassConsts pc;
    // (one image of the variants' block at a time, uploaded when it differs from what the block holds)
    if ((rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, io.d_y, io.d_m0, io.d_P0, io.d_fm, io.d_fP, io.d_status, s, &pass)) ||
        (rc = cached_pass_consts(f_dyn, f_obs, D, Y, T, io.GQG, v.R_pass, nullptr, s, &pc)) || (!host.empty() && (rc = cached_robust_consts(host, s))))
        return rc;
    const double *cs = (const double *)g_fc.consts, *block = (const double *)g_fc.robust;
    wire_pass_consts(pass, cs, pc);
    rc = one_launch ? v.try_launch(pass, block) : 0;
    if (rc < 0) return rc;
    if (rc == 1) return SSMQ_OK;
    if (pf.user && !user_ekf) {
        set_error(std::string(v.who) + ": no run-time kernel for this pair of user integrands");
        return SSMQ_E_UNSUPPORTED;
    }
    if (user_ekf && (rc = prepare_user_ekf(h_dyn, f_dyn, h_obs, f_obs, pf.gq))) return rc;
    if ((rc = ensure_ws(update_ws_bytes(D, Y, ld)))) return rc;
    return v.loop(pass, block, cs + pc.steps, g_fc.ws);
}

// The name of what update_pass_dev would run: try_launch(query) on a dry-run pass, else the launch loop's
template <class Try>
static int update_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                              int64_t B, bool force_loop, const char *loop_name, char *buf, int len, Try try_launch) {
    PairForms pf;
    bool user_ekf = false, one_launch = false;
    int rc = innovations_route(h_dyn, f_dyn, h_obs, f_obs, &pf, &user_ekf, &one_launch);
    if (rc) return rc;
    if (force_loop && !pf.user) one_launch = false;
    const char *name = nullptr;
    FilterPass query;
    if ((rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, B, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &query))) return rc;
    query.name = &name; query.dry_run = true;
    rc = one_launch ? try_launch(query) : 0;
    if (rc < 0) return rc;
    snprintf(buf, len, "%s", rc == 1 ? name : loop_name);
    return SSMQ_OK;
}

static bool iterations_ok(int iterations) {
    if (iterations >= 1 && iterations <= SSMQ_ITERATED_MAX) return true;
    set_error("filter_iterated: 1 <= iterations <= " + std::to_string(SSMQ_ITERATED_MAX));
    return false;
}

extern "C" int ssmq_filter_iterated_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                        const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, int iterations, int flags,
                                        const double *d_y, const double *d_m0, const double *d_P0, const double *GQG, const double *R,
                                        double *d_fm, double *d_fP, double *d_delta, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || B < 0 || ld < B || T < 0 || !d_y || !d_m0 || !d_P0 || !d_fm || !d_fP || !d_status ||
        (flags & ~1)) {
        set_error("filter_iterated: bad argument");
        return SSMQ_E_ARG;
    }
    if (!iterations_ok(iterations)) return SSMQ_E_ARG;
    const IplfPass ip{iterations, d_delta};
    auto consts = [](int, std::vector<double> *) { return SSMQ_OK; };
    auto try_launch = [&](const FilterPass &pass, const double *) { return try_launch_iterated(pass, ip); };
    auto loop = [&](const FilterPass &pass, const double *, const double *tvec, void *ws) { return iterated_launch_loop(h_dyn, h_obs, pass, ip, tvec, ws); };
    return update_pass_dev(h_dyn, f_dyn, h_obs, f_obs, PassIO{B, ld, T, d_y, d_m0, d_P0, GQG, d_fm, d_fP, d_status}, flags & 1,
                           update_variant("filter_iterated", R, consts, try_launch, loop));
}

extern "C" int ssmq_iterated_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                         const ssmq_integrand *f_obs, int64_t B, int iterations, int flags, char *buf, int len) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || !buf || len <= 0 || B < 0 || (flags & ~1)) return SSMQ_E_ARG;
    if (!iterations_ok(iterations)) return SSMQ_E_ARG;
    return update_kernel_name(h_dyn, f_dyn, h_obs, f_obs, B, flags & 1, kIplfLoopName, buf, len,
                              [&](const FilterPass &q) { return try_launch_iterated(q, IplfPass{iterations, nullptr}); });
}

// the argument checks both entry points share, after the null checks; R may be null for the name query
static int robust_arg_checks(int iterations, int flags, double dof) {
    if (flags & ~SSMQ_ROBUST_LAUNCH_LOOP) {
        set_error("filter_robust: flags: bit 0 alone");
        return SSMQ_E_ARG;
    }
    if (iterations < 1 || iterations > SSMQ_ITERATED_MAX) {
        set_error("filter_robust: 1 <= iterations <= " + std::to_string(SSMQ_ITERATED_MAX));
        return SSMQ_E_ARG;
    }
    if (!(dof > 0.0) || !std::isfinite(dof)) {
        set_error("filter_robust: dof must be a positive finite number");
        return SSMQ_E_ARG;
    }
    return SSMQ_OK;
}

extern "C" int ssmq_filter_robust_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                                      int64_t B, int64_t ld, int T, int iterations, int flags, const double *d_y, const double *d_m0,
                                      const double *d_P0, const double *GQG, const double *R, double dof, double *d_fm, double *d_fP,
                                      double *d_lam, double *d_delta, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || B < 0 || ld < B || T < 0 || !d_y || !d_m0 || !d_P0 || !R || !d_fm || !d_fP || !d_lam ||
        !d_delta || !d_status) {
        set_error("filter_robust: bad argument");
        return SSMQ_E_ARG;
    }
    int rc = robust_arg_checks(iterations, flags, dof);
    if (rc) return rc;
    const size_t YY = (size_t)h_obs->E * h_obs->E;
    // (the pass's constants without R: its rr block is the zeros the measurement transform adds)
    auto rp = [&](const double *rb) { return RobustPass{iterations, dof, rb, rb + YY, d_lam, d_delta}; };
    auto consts = [&](int Y, std::vector<double> *h) {
        if (robust_consts(Y, R, h)) return SSMQ_OK;
        set_error("filter_robust: R must be a finite symmetric positive definite matrix");
        return SSMQ_E_ARG;
    };
    auto try_launch = [&](const FilterPass &pass, const double *rb) { return try_launch_robust(pass, rp(rb)); };
    auto loop = [&](const FilterPass &pass, const double *rb, const double *tvec, void *ws) { return robust_launch_loop(h_dyn, h_obs, pass, rp(rb), tvec, ws); };
    return update_pass_dev(h_dyn, f_dyn, h_obs, f_obs, PassIO{B, ld, T, d_y, d_m0, d_P0, GQG, d_fm, d_fP, d_status}, flags & SSMQ_ROBUST_LAUNCH_LOOP,
                           update_variant("filter_robust", nullptr, consts, try_launch, loop));
}

extern "C" int ssmq_robust_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                       const ssmq_integrand *f_obs, int64_t B, int iterations, int flags, char *buf, int len) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || !buf || len <= 0 || B < 0) return SSMQ_E_ARG;
    int rc = robust_arg_checks(iterations, flags, 1.0);
    if (rc) return rc;
    return update_kernel_name(h_dyn, f_dyn, h_obs, f_obs, B, flags & SSMQ_ROBUST_LAUNCH_LOOP, kRobustLoopName, buf, len, [&](const FilterPass &q) {
        return try_launch_robust(q, RobustPass{iterations, 1.0, nullptr, nullptr, nullptr, nullptr});
    });
}

// R | gate as the host image of a device block ([Y*Y] | [Y+1]; gate null: +inf everywhere): false, with the error set, when R is
// not finite or not symmetric or a gate entry 1 .. Y is not a positive number or +inf
static bool masked_consts(int Y, const double *R, const double *gate, std::vector<double> *out) {
    std::vector<double> h((size_t)Y * Y + Y + 1, HUGE_VAL);
    for (int i = 0; i < Y; ++i)
        for (int j = 0; j < Y; ++j) {
            if (!std::isfinite(R[i * Y + j]) || R[i * Y + j] != R[j * Y + i]) {
                set_error("filter_masked: R must be a finite symmetric matrix");
                return false;
            }
            h[(size_t)i * Y + j] = R[i * Y + j];
        }
    for (int o = 1; gate && o <= Y; ++o) {
        if (!(gate[o] > 0.0)) {   // (NaN included)
            set_error("filter_masked: gate entries 1 .. Y must be positive numbers or +inf");
            return false;
        }
        h[(size_t)Y * Y + o] = gate[o];
    }
    out->swap(h);
    return true;
}

static int masked_flag_check(int flags) {
    if (flags & ~SSMQ_MASKED_LAUNCH_LOOP) {
        set_error("filter_masked: flags: bit 0 alone");
        return SSMQ_E_ARG;
    }
    return SSMQ_OK;
}

extern "C" int ssmq_filter_masked_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                                      int64_t B, int64_t ld, int T, int flags, const double *d_y, const uint32_t *d_mask, const double *d_m0,
                                      const double *d_P0, const double *GQG, const double *R, const double *gate, double *d_fm, double *d_fP,
                                      uint32_t *d_used, double *d_nis, double *d_loglik, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || B < 0 || ld < B || T < 0 || !d_y || !d_m0 || !d_P0 || !R || !d_fm || !d_fP || !d_used ||
        !d_nis || !d_loglik || !d_status) {
        set_error("filter_masked: bad argument");
        return SSMQ_E_ARG;
    }
    int rc = masked_flag_check(flags);
    if (rc) return rc;
    const size_t YY = (size_t)h_obs->E * h_obs->E;
    // (the pass's constants without R, as the robust pass; R | gate in the variants' block)
    auto mp = [&](const double *rb) { return MaskedPass{d_mask, rb, rb + YY, d_used, d_nis, d_loglik}; };
    auto consts = [&](int Y, std::vector<double> *h) { return masked_consts(Y, R, gate, h) ? SSMQ_OK : SSMQ_E_ARG; };
    auto try_launch = [&](const FilterPass &pass, const double *rb) { return try_launch_masked(pass, mp(rb)); };
    auto loop = [&](const FilterPass &pass, const double *rb, const double *tvec, void *ws) { return masked_launch_loop(h_dyn, h_obs, pass, mp(rb), tvec, ws); };
    return update_pass_dev(h_dyn, f_dyn, h_obs, f_obs, PassIO{B, ld, T, d_y, d_m0, d_P0, GQG, d_fm, d_fP, d_status}, flags & SSMQ_MASKED_LAUNCH_LOOP,
                           update_variant("filter_masked", nullptr, consts, try_launch, loop));
}

extern "C" int ssmq_masked_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                       const ssmq_integrand *f_obs, int64_t B, int flags, char *buf, int len) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || !buf || len <= 0 || B < 0) return SSMQ_E_ARG;
    int rc = masked_flag_check(flags);
    if (rc) return rc;
    return update_kernel_name(h_dyn, f_dyn, h_obs, f_obs, B, flags & SSMQ_MASKED_LAUNCH_LOOP, kMaskedLoopName, buf, len, [&](const FilterPass &q) {
        return try_launch_masked(q, MaskedPass{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
    });
}

extern "C" int ssmq_detection_mask_dev(int64_t B, int64_t ld, int T, int Y, const double *p_detect, uint64_t seed, uint64_t traj_offset,
                                       int per_component, uint32_t *d_mask) {
    if (B < 0 || ld < B || T < 0 || Y < 1 || Y > SSMQ_MAX_DIM || !p_detect || !d_mask) {
        set_error("detection_mask: bad argument (1 <= Y <= " + std::to_string(SSMQ_MAX_DIM) + ")");
        return SSMQ_E_ARG;
    }
    for (int i = 0; i < (per_component ? Y : 1); ++i)
        if (!(p_detect[i] >= 0.0 && p_detect[i] <= 1.0)) {
            set_error("detection_mask: p_detect must lie in [0, 1]");
            return SSMQ_E_ARG;
        }
    if (int rc = ensure_device()) return rc;
    if (B == 0 || T == 0) return SSMQ_OK;
    return launch_detection_mask(B, ld, T, Y, p_detect, seed, traj_offset, per_component ? 1 : 0, d_mask, stream());
}

// ---- iterated posterior linearisation smoother (include/ssmq.h: ssmq_smoother_iterated_dev) ------------------------------------------
// The refusals of the innovation scores, then: a pair runs k_ipls_pass<> (a table shape, or a user pair compiled at run time) or is
// refused - there is no launch-loop route.  Both entry points ask the table by a dry run, before anything is written.
static int ipls_route(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                      int iterations, const char **name) {
    if (iterations < 1 || iterations > SSMQ_ITERATED_MAX) {
        set_error("smoother_iterated: 1 <= iterations <= " + std::to_string(SSMQ_ITERATED_MAX));
        return SSMQ_E_ARG;
    }
    PairForms pf;
    bool user_ekf = false, one_launch = false;
    int rc = innovations_route(h_dyn, f_dyn, h_obs, f_obs, &pf, &user_ekf, &one_launch);
    if (rc) return rc;
    FilterPass query;
    if ((rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &query))) return rc;
    query.name = name; query.dry_run = true;
    const bool covered = !user_ekf && !pf.mo && !pf.trunc && !pf.gq && !jac_form(h_dyn) && !jac_form(h_obs);
    rc = covered ? try_launch_ipls(query, IplsPlanes{}) : 0;
    if (rc < 0) return rc;
    if (rc == 1) return SSMQ_OK;
    set_error("smoother_iterated: covers the sigma-point and BQ pairs the fused time loop is instantiated for (unscented and "
              "spherical-radial point sets of the built-in model pairs) and user models through the run-time compiler; not other point "
              "counts (Gauss-Hermite), linearisation, Taylor-GPQD, GPQ+D, truncated or multi-output transforms");
    return SSMQ_E_UNSUPPORTED;
}

extern "C" int ssmq_smoother_iterated_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                          const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y, const double *d_m0,
                                          const double *d_P0, const double *GQG, const double *R, int iterations, int flags,
                                          const double *d_lin_m, const double *d_lin_P, double *d_fm, double *d_fP, double *d_sm,
                                          double *d_sP, double *d_sm0, double *d_sP0, double *d_delta, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || B < 0 || ld < B || T < 0 || !d_y || !d_m0 || !d_P0 || !d_fm || !d_fP || !d_sm || !d_sP ||
        !d_sm0 || !d_sP0 || !d_status || flags != 0 || (d_lin_m == nullptr) != (d_lin_P == nullptr)) {
        set_error("smoother_iterated: bad argument (flags is reserved: 0; lin_m and lin_P come together)");
        return SSMQ_E_ARG;
    }
    const char *name = nullptr;
    int rc = ipls_route(h_dyn, f_dyn, h_obs, f_obs, iterations, &name);
    if (rc) return rc;
    const int D = h_dyn->D, Y = h_obs->E;
    if ((rc = ensure_device())) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * ld, s));
    if (T == 0) {   // nothing to smooth: the initial state is its own smoothed state
        SSMQ_HIP(hipMemcpyAsync(d_sm0, d_m0, sizeof(double) * D * ld, hipMemcpyDeviceToDevice, s));
        SSMQ_HIP(hipMemcpyAsync(d_sP0, d_P0, sizeof(double) * D * D * ld, hipMemcpyDeviceToDevice, s));
        if (d_delta) SSMQ_HIP(hipMemsetAsync(d_delta, 0, sizeof(double) * ld, s));
        SSMQ_HIP(hipStreamSynchronize(s));
        return SSMQ_OK;
    }
    // the planes the two sweeps share and, for more than one iteration, one or two sets of smoothed moments [T+1][D + D*D][ld]
    const size_t DP = (size_t)D * (D + 1) / 2, set = (size_t)(T + 1) * (D + D * D) * ld;
    const int n_sets = iterations == 1 ? 0 : (iterations == 2 ? 1 : 2);
    DevBuf ws, sets;
    if ((rc = ws.alloc(sizeof(double) * (size_t)T * (D + DP + (size_t)D * D) * ld)) || (rc = sets.alloc(sizeof(double) * set * n_sets))) return rc;
    FilterPass pass;
    PassConsts pc;
    if ((rc = make_filter_pass(h_dyn, f_dyn, h_obs, f_obs, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_status, s, &pass)) ||
        (rc = cached_pass_consts(f_dyn, f_obs, D, Y, T, GQG, R, nullptr, s, &pc)))
        return rc;
    wire_pass_consts(pass, (const double *)g_fc.consts, pc);
    IplsPlanes q;
    q.pm = ws.d(); q.pP = q.pm + (size_t)T * D * ld; q.pC = q.pP + (size_t)T * DP * ld;
    q.lin_m = d_lin_m; q.lin_P = d_lin_P;
    for (int i = 0; i < iterations && !rc; ++i) {
        const bool last = i == iterations - 1;
        double *om = last ? nullptr : sets.d() + (size_t)(i & 1) * set, *oP = last ? nullptr : om + (size_t)(T + 1) * D * ld;
        q.sm0 = last ? d_sm0 : om;  q.sm = last ? d_sm : om + (size_t)D * ld;
        q.sP0 = last ? d_sP0 : oP;  q.sP = last ? d_sP : oP + (size_t)D * D * ld;
        q.delta = last ? d_delta : nullptr;
        rc = try_launch_ipls(pass, q);
        rc = rc == 1 ? 0 : (rc == 0 ? SSMQ_E_UNSUPPORTED : rc);
        q.lin_m = om; q.lin_P = oP;
    }
    hipError_t e = hipStreamSynchronize(s);      // (the workspace is released when this call returns)
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

extern "C" int ssmq_smoother_iterated_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                                  const ssmq_integrand *f_obs, int iterations, char *buf, int len) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || !buf || len <= 0) return SSMQ_E_ARG;
    const char *name = nullptr;
    int rc = ipls_route(h_dyn, f_dyn, h_obs, f_obs, iterations, &name);
    if (rc) return rc;
    snprintf(buf, len, "%s", name ? name : "k_ipls_pass");
    return SSMQ_OK;
}

static int metrics_impl(int phase, int D, int64_t B, int64_t ld, int T, const double *d_x, const double *d_fm,
                        const double *d_fP, const int32_t *d_status, const double *mse, double *sums) {
    if (D < 1 || D > SSMQ_MAX_DIM || B < 0 || ld < B || T < 0 || !d_x || !d_fm || !d_fP || !sums || (phase == 2 && !mse)) {
        set_error("error_sums: bad argument");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    const int NV = phase == 1 ? metrics_values_per_step(D) : 2;     // values per step handed back
    const int NI = phase == 1 ? NV : 3;                             // ... and reduced on the device
    if (T == 0) return SSMQ_OK;
    if (B == 0) {
        memset(sums, 0, sizeof(double) * (size_t)T * NV);
        return SSMQ_OK;
    }
    hipStream_t s = stream();
    DevBuf partial, out, dm, left;
    if ((rc = partial.alloc(sizeof(double) * (size_t)T * metrics_chunks(B) * NI)) ||
        (rc = out.alloc(sizeof(double) * (size_t)T * NI)) || (rc = dm.alloc(sizeof(double) * (size_t)T * D * D)) ||
        (rc = left.alloc((size_t)T * metrics_chunks(B) * metrics_left_bytes())))
        return rc;
    if (phase == 2) SSMQ_HIP(hipMemcpyAsync(dm.p, mse, sizeof(double) * (size_t)T * D * D, hipMemcpyHostToDevice, s));
    rc = launch_metrics(phase, D, B, ld, T, d_x, d_fm, d_fP, d_status, dm.d(), partial.d(), (uint8_t *)left.p, out.d(), s);
    if (rc) {
        hipStreamSynchronize(s);
        return rc;
    }
    std::vector<double> h((size_t)T * NI);
    SSMQ_HIP(hipMemcpyAsync(h.data(), out.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    // entries whose covariance is not positive definite were left out by the streaming kernels (they factor P): the
    // reference's formulas do not need a positive-definite P (utils.py:143-148, 426-432) - a second pass adds them
    const int i_ok = D + 2 + D * D, i_cnt = phase == 1 ? i_ok + 1 : 1, i_sum = phase == 1 ? D + 1 : 0;
    bool left_out = false;
    for (int t = 0; t < T && !left_out; ++t)
        left_out = phase == 1 ? h[(size_t)t * NI + i_ok] > h[(size_t)t * NI + i_cnt] : h[(size_t)t * NI + 2] > 0.0;
    if (left_out) {
        rc = launch_metrics_indef(phase, D, B, ld, T, d_x, d_fm, d_fP, d_status, dm.d(), partial.d(), (uint8_t *)left.p, out.d(), s);
        std::vector<double> extra((size_t)T * 2);
        if (!rc) rc = hip_fail(hipMemcpyAsync(extra.data(), out.p, sizeof(double) * extra.size(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
        hipError_t e = hipStreamSynchronize(s);
        if (rc) return rc;
        SSMQ_HIP(e);
        for (int t = 0; t < T; ++t) {
            h[(size_t)t * NI + i_sum] += extra[(size_t)t * 2];
            h[(size_t)t * NI + i_cnt] += extra[(size_t)t * 2 + 1];
        }
    }
    for (int t = 0; t < T; ++t)
        for (int v = 0; v < NV; ++v) sums[(size_t)t * NV + v] = h[(size_t)t * NI + v];
    return SSMQ_OK;
}

extern "C" int ssmq_error_sums_width(int D) { return D >= 1 && D <= SSMQ_MAX_DIM ? metrics_values_per_step(D) : SSMQ_E_ARG; }

extern "C" int ssmq_error_sums_dev(int D, int64_t B, int64_t ld, int T, const double *d_x, const double *d_fm,
                                   const double *d_fP, const int32_t *d_status, double *sums) {
    return metrics_impl(1, D, B, ld, T, d_x, d_fm, d_fP, d_status, nullptr, sums);
}

extern "C" int ssmq_lcr_sums_dev(int D, int64_t B, int64_t ld, int T, const double *d_x, const double *d_fm,
                                 const double *d_fP, const int32_t *d_status, const double *mse, double *sums) {
    return metrics_impl(2, D, B, ld, T, d_x, d_fm, d_fP, d_status, mse, sums);
}

extern "C" int ssmq_traj_scores_rows(int D) { return D >= 1 && D <= SSMQ_MAX_DIM ? D + 3 : SSMQ_E_ARG; }

extern "C" int ssmq_traj_scores_dev(int D, int64_t B, int64_t ld, int T, int k0, const double *d_x, const double *d_fm,
                                    const double *d_fP, const int32_t *d_status, const double *mse, double *d_scores) {
    if (D < 1 || D > SSMQ_MAX_DIM || B < 0 || ld < B || ld < 1 || T < 1 || k0 < 0 || k0 >= T || !d_x || !d_fm || !d_fP || !d_scores) {
        set_error("traj_scores: bad argument (1 <= D <= 16, 0 <= B <= ld, 0 <= k0 < T)");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t s = stream();
    DevBuf dm;
    if (mse) {
        if ((rc = dm.alloc(sizeof(double) * (size_t)T * D * D))) return rc;
        SSMQ_HIP(hipMemcpyAsync(dm.p, mse, sizeof(double) * (size_t)T * D * D, hipMemcpyHostToDevice, s));
    }
    rc = launch_traj_scores(D, B, ld, T, k0, d_x, d_fm, d_fP, d_status, mse ? dm.d() : nullptr, d_scores, s);
    hipError_t e = hipStreamSynchronize(s);
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

extern "C" int ssmq_simulate_rv_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, const ssmq_rv *x0,
                                    const ssmq_rv *q, const ssmq_rv *r, const double *G, int dyn_additive, int obs_additive,
                                    int64_t B, int64_t ld, int T, int continuous, double dt, uint64_t seed,
                                    uint64_t traj_offset, double *d_x, double *d_y) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("ssmq_simulate_rv_dev");
    const int mode = (f_dyn ? 1 : 0) | (f_obs ? 2 : 0);
    auto rv_ok = [](const ssmq_rv *v, int dim) {
        return v && v->dim == dim && v->chol && v->kind >= SSMQ_RV_GAUSS && v->kind <= SSMQ_RV_MIXTURE &&
               (v->kind != SSMQ_RV_STUDENT || v->dof > 2.0) &&
               (v->kind == SSMQ_RV_MIXTURE ? (v->n_comp >= 1 && v->n_comp <= 8 && v->alpha) : v->n_comp <= 1);
    };
    int dq = (f_dyn && q) ? q->dim : 0, dr = (f_obs && r) ? r->dim : 0;
    if (!mode || D < 1 || D > SSMQ_MAX_DIM || B < 0 || ld < B || T < 0 || !d_x ||
        (f_dyn && (!rv_ok(x0, D) || dq < 1 || dq > SSMQ_MAX_DIM || !rv_ok(q, dq))) ||
        (f_obs && (!d_y || Y < 1 || Y > SSMQ_MAX_DIM || dr < 1 || dr > SSMQ_MAX_DIM || !rv_ok(r, dr))) ||
        (continuous && (!f_dyn || !(dt > 0.0)))) {
        set_error("simulate: bad argument");
        return SSMQ_E_ARG;
    }
    if (!f_obs) Y = 0;
    FInfo fid, fio;
    if (f_dyn) {
        const int in_dyn = D + (dyn_additive ? 0 : dq);
        if (!integrand_info(f_dyn->id, &fid) || fid.dout != D || f_dyn->n_idx != 0 ||
            (!continuous && (fid.din > in_dyn || in_dyn > kMaxIntegrandIn))) {
            set_error("simulate: transition integrand / dimension mismatch (state + noise inputs: at most 16)");
            return SSMQ_E_ARG;
        }
        if (continuous && !has_continuous_dynamics(f_dyn->id)) {
            set_error("simulate: this model has no continuous-time dynamics (dyn_fcn_cont is defined for the reentry-1D, "
                      "reentry-2D and constant-turn-rate-and-speed models only, ssmod.py:429-432, 569-585, 779-780)");
            return SSMQ_E_UNSUPPORTED;
        }
        if (continuous && dq < (f_dyn->id == SSMQ_F_CTRS_DYN ? 1 : 3)) {
            set_error("simulate: the continuous-time dynamics read three noise components");
            return SSMQ_E_ARG;
        }
    }
    if (f_obs) {
        const int in_obs = D + (obs_additive ? 0 : dr);
        if (!integrand_info(f_obs->id, &fio) || (fio.dout ? fio.dout : Y) != Y || (obs_additive && dr != Y) ||
            f_obs->n_idx > SSMQ_MAX_FIDX || f_obs->n_idx < 0 || (f_obs->n_idx == 0 && (fio.din > in_obs || in_obs > kMaxIntegrandIn))) {
            set_error("simulate: measurement integrand / dimension mismatch");
            return SSMQ_E_ARG;
        }
        for (int k = 0; k < f_obs->n_idx; ++k)
            if (f_obs->idx[k] < 0 || f_obs->idx[k] >= in_obs) {
                set_error("simulate: measurement state index out of range");
                return SSMQ_E_ARG;
            }
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0 || T == 0) return SSMQ_OK;
    SimLaunch h;
    memset(&h, 0, sizeof(h));
    std::vector<double> hc;
    auto put_rv = [&](const ssmq_rv *v, SimRv *out) {
        out->off = (int)hc.size();
        if (!v) {
            out->kind = SSMQ_RV_GAUSS; out->dim = 0; out->ncomp = 1; out->dof = 0.0;
            hc.push_back(1.0);
            return;
        }
        const int nc = v->kind == SSMQ_RV_MIXTURE ? v->n_comp : 1, n = v->dim;
        out->kind = v->kind; out->dim = n; out->ncomp = nc; out->dof = v->dof;
        for (int k = 0; k < nc; ++k) hc.push_back(v->kind == SSMQ_RV_MIXTURE ? v->alpha[k] : 1.0);
        for (int i = 0; i < nc * n; ++i) hc.push_back(v->mean ? v->mean[i] : 0.0);
        for (int i = 0; i < nc * n * n; ++i) hc.push_back(v->chol[i]);
    };
    put_rv(f_dyn ? x0 : nullptr, &h.rv[0]);
    put_rv(f_dyn ? q : nullptr, &h.rv[1]);
    put_rv(f_obs ? r : nullptr, &h.rv[2]);
    h.g_off = (int)hc.size();
    for (int i = 0; i < D * dq; ++i)        // default noise gain eye(D, dq)  (ssmod.py:52)
        hc.push_back(G ? G[i] : ((i / dq) == (i % dq) ? 1.0 : 0.0));
    DevBuf dc;
    if ((rc = dc.alloc(sizeof(double) * std::max<size_t>(hc.size(), 1)))) return rc;
    hipStream_t s = stream();
    SSMQ_HIP(hipMemcpyAsync(dc.p, hc.data(), sizeof(double) * hc.size(), hipMemcpyHostToDevice, s));
    h.mode = mode; h.D = D; h.Y = Y; h.dq = dq; h.dr = dr; h.dyn_additive = dyn_additive; h.obs_additive = obs_additive; h.T = T;
    h.continuous = continuous ? 1 : 0; h.dt = dt; h.B = B; h.ld = ld; h.seed = seed; h.traj_offset = traj_offset;
    h.f_dyn = f_dyn; h.f_obs = f_obs; h.d_consts = dc.d(); h.d_x = d_x; h.d_y = d_y;
    rc = launch_simulate(h, s);
    hipError_t e = hipStreamSynchronize(s);
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

// the Gaussian case with plain arrays (the round-1 entry point)
extern "C" int ssmq_simulate_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int dr,
                                 int dyn_additive, int obs_additive, int64_t B, int64_t ld, int T,
                                 const double *x0_mean, const double *x0_chol, const double *q_mean,
                                 const double *q_chol, const double *G, const double *r_mean, const double *r_chol,
                                 uint64_t seed, uint64_t traj_offset, double *d_x, double *d_y) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("ssmq_simulate_dev");
    ssmq_rv x0{SSMQ_RV_GAUSS, D, 1, 0, 0.0, x0_mean, x0_chol, nullptr};
    ssmq_rv q{SSMQ_RV_GAUSS, dq, 1, 0, 0.0, q_mean, q_chol, nullptr};
    ssmq_rv r{SSMQ_RV_GAUSS, dr, 1, 0, 0.0, r_mean, r_chol, nullptr};
    if (f_dyn && (!x0_mean || !x0_chol || !q_chol)) {
        set_error("simulate: bad argument");
        return SSMQ_E_ARG;
    }
    return ssmq_simulate_rv_dev(f_dyn, f_obs, D, Y, &x0, &q, &r, G, dyn_additive, obs_additive, B, ld, T, 0, 0.0, seed,
                                traj_offset, d_x, d_y);
}
