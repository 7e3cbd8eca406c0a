// C ABI of libssmq (include/ssmq.h), the theta-batched filter step: one step per kernel-parameter item, from host arrays
// (ssmq_gp_theta_step, with its captured graphs) or on items that are already on the device (theta_dev_*, for ssmq_marginal_device.hip).
#include <algorithm>
#include <cstring>
#include <vector>
#include "ssmq_host.h"
#include "ssmq_update.h"

using namespace ssmq;

#define g_stage (ssmq::stage_of_ctx())

namespace {
struct ThetaGraph {
    std::vector<uint64_t> key;
    hipGraph_t graph;
    hipGraphExec_t exec;
};
std::vector<ThetaGraph> &theta_graphs_of_ctx() {
    Ctx &c = ssmq::ctx();
    if (!c.theta_graphs) c.theta_graphs = new std::vector<ThetaGraph>;
    return *(std::vector<ThetaGraph> *)c.theta_graphs;
}
#define g_theta_graphs (theta_graphs_of_ctx())
void drop_theta_graphs() {
    for (auto &g : g_theta_graphs) {
        if (g.exec) hipGraphExecDestroy(g.exec);
        if (g.graph) hipGraphDestroy(g.graph);
    }
    g_theta_graphs.clear();
}
}  // namespace
namespace ssmq {
void drop_theta_step_graphs() { drop_theta_graphs(); }
}

// One filter step per parameter item: weights(theta_dyn) -> dyn transform -> + GQG -> weights(theta_obs) -> obs transform
// -> + R -> measurement update and log N(y | y_mean, P_y).  Everything between the host arrays stays on the device.
static int gp_theta_step_impl(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                              const ssmq_integrand *f_obs, int64_t P, const double *par_dyn, const double *par_obs,
                              double jitter, const double *mean, const double *cov, int shared_state,
                              const double *y, int shared_y, double time, const double *times, const double *GQG, const double *R,
                              double *post_mean, double *post_cov, double *loglik, int32_t *status);

extern "C" int ssmq_gp_theta_step(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                  const ssmq_integrand *f_obs, int64_t P, const double *par_dyn, const double *par_obs,
                                  double jitter, const double *mean, const double *cov, int shared_state,
                                  const double *y, int shared_y, double time, const double *GQG, const double *R,
                                  double *post_mean, double *post_cov, double *loglik, int32_t *status) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("ssmq_gp_theta_step");
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo("ssmq_gp_theta_step");
    if (is_trunc(h_dyn) || is_trunc(h_obs)) return refuse_trunc("ssmq_gp_theta_step");
    if (is_gpqd(h_dyn) || is_gpqd(h_obs)) return refuse_gpqd("ssmq_gp_theta_step");
    if (is_taylor_gpqd(h_dyn) || is_taylor_gpqd(h_obs)) return refuse_taylor_gpqd("ssmq_gp_theta_step");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    return gp_theta_step_impl(h_dyn, f_dyn, h_obs, f_obs, P, par_dyn, par_obs, jitter, mean, cov, shared_state, y, shared_y, time,
                              nullptr, GQG, R, post_mean, post_cov, loglik, status);
}

// the same with a time of its own per item (times [P]): items of different time steps in one call - the batched marginalised
// filter lets every trajectory run ahead at its own pace (csrc/ssmq_marginal.hip)
extern "C" int ssmq_gp_theta_step_times(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                        const ssmq_integrand *f_obs, int64_t P, const double *par_dyn, const double *par_obs,
                                        double jitter, const double *mean, const double *cov, int shared_state,
                                        const double *y, int shared_y, const double *times, const double *GQG, const double *R,
                                        double *post_mean, double *post_cov, double *loglik, int32_t *status) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("ssmq_gp_theta_step_times");
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo("ssmq_gp_theta_step_times");
    if (is_trunc(h_dyn) || is_trunc(h_obs)) return refuse_trunc("ssmq_gp_theta_step_times");
    if (is_gpqd(h_dyn) || is_gpqd(h_obs)) return refuse_gpqd("ssmq_gp_theta_step_times");
    if (is_taylor_gpqd(h_dyn) || is_taylor_gpqd(h_obs)) return refuse_taylor_gpqd("ssmq_gp_theta_step_times");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!times) {
        set_error("gp_theta_step_times: times is NULL");
        return SSMQ_E_ARG;
    }
    return gp_theta_step_impl(h_dyn, f_dyn, h_obs, f_obs, P, par_dyn, par_obs, jitter, mean, cov, shared_state, y, shared_y, 0.0,
                              times, GQG, R, post_mean, post_cov, loglik, status);
}

static int gp_theta_step_impl(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                              const ssmq_integrand *f_obs, int64_t P, const double *par_dyn, const double *par_obs,
                              double jitter, const double *mean, const double *cov, int shared_state,
                              const double *y, int shared_y, double time, const double *times, const double *GQG, const double *R,
                              double *post_mean, double *post_cov, double *loglik, int32_t *status) {
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || P < 0 || P > 0x7fffffff || !par_dyn || !par_obs || !mean || !cov || !y ||
        !post_mean || !post_cov || !loglik) {
        set_error("gp_theta_step: bad argument");
        return SSMQ_E_ARG;
    }
    // Din > D: dynamics that take their noise as an argument - the caller passes the AUGMENTED moments [m; q_mean],
    // blockdiag(P, Q) (ssinf.py:1174-1176) and GQG = NULL; the measurement model is additive (the reference builds its
    // measurement transform on dim_state inputs, ssinf.py:1288, so it cannot run a non-additive one either)
    const int Din = h_dyn->D, D = h_dyn->E, Y = h_obs->E, Nd = h_dyn->N, No = h_obs->N;
    if (Din < D || h_obs->D != D || h_dyn->form != SSMQ_FORM_BQ || h_obs->form != SSMQ_FORM_BQ ||
        h_dyn->tp_nu > 0.0 || h_obs->tp_nu > 0.0) {
        set_error("gp_theta_step: needs GP-quadrature transforms (D + dq) -> D and D -> Y");
        return SSMQ_E_ARG;
    }
    FInfo fid, fio;
    int rc = check_integrand(h_dyn, f_dyn, &fid);
    if (rc || (rc = check_integrand(h_obs, f_obs, &fio))) return rc;
    if (wide_lds_bytes(Din, D, Nd) > 160 * 1024 - 64 || wide_lds_bytes(D, Y, No) > 160 * 1024 - 64) {
        set_error("gp_theta_step: shape too large for the LDS-resident generic kernel");
        return SSMQ_E_UNSUPPORTED;
    }
    if ((rc = ensure_device())) return rc;
    if (P == 0) return SSMQ_OK;
    hipStream_t s = stream();
    const int64_t ld = (P + 63) / 64 * 64;
    const WideLayout cld = wide_layout(Din, D, Nd, SSMQ_FORM_BQ), clo = wide_layout(D, Y, No, SSMQ_FORM_BQ);
    const int64_t ns = shared_state ? 1 : P;
    // ---- one device arena and two pinned host blocks, kept between calls (the marginalised filter calls this once per
    // BFGS iteration with a handful of items: forty allocations and three synchronisations per call were 310 us) -----------
    // input block, same layout on host and device:  xi_dyn | xi_obs | par_dyn | par_obs | mean | cov | y (planes) | GQG | R | t
    const size_t n_in = (size_t)Din * Nd + (size_t)D * No + (size_t)P * (1 + Din) + (size_t)P * (1 + D) +
                        (size_t)ns * (Din + Din * Din) + (size_t)ld * Y + (size_t)D * D + (size_t)Y * Y + (times ? (size_t)ld : 1);
    // work planes: m_pr D | P_pr D*D | C_xx D*D | y_mean Y | P_y Y*Y | P_yx Y*D, then the output block m_fi D | P_fi D*D |
    // loglik 1 | merged status (int32), then the five partial status vectors
    const size_t n_mid = (size_t)D + (size_t)D * D + (size_t)D * Din + Y + (size_t)Y * Y + (size_t)Y * D;
    const size_t n_out = (size_t)D + (size_t)D * D + 1;
    const size_t out_bytes = sizeof(double) * n_out * ld + sizeof(int32_t) * ld;
    const size_t ws_d = gp_weights_wide_ws_bytes(Din, Nd, P), ws_o = gp_weights_wide_ws_bytes(D, No, P);
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t off_in = 0, off_cd = al(sizeof(double) * n_in), off_co = off_cd + al(sizeof(double) * P * cld.total),
                 off_mid = off_co + al(sizeof(double) * P * clo.total), off_out = off_mid + al(sizeof(double) * n_mid * ld),
                 off_st = off_out + al(out_bytes), off_ws = off_st + al(sizeof(int32_t) * 5 * ld),
                 total = off_ws + std::max(ws_d, ws_o);
    if ((rc = g_stage.reserve(total, sizeof(double) * n_in, out_bytes))) return rc;
    char *dev = (char *)g_stage.dev;
    double *hin = (double *)g_stage.hin;
    {
        double *h = hin;
        auto put = [&](const double *src, size_t n) {
            memcpy(h, src, sizeof(double) * n);
            h += n;
        };
        put(h_dyn->xi.data(), (size_t)Din * Nd);
        put(h_obs->xi.data(), (size_t)D * No);
        put(par_dyn, (size_t)P * (1 + Din));
        put(par_obs, (size_t)P * (1 + D));
        put(mean, (size_t)ns * Din);
        put(cov, (size_t)ns * Din * Din);
        for (int k = 0; k < Y; ++k) {                      // measurements straight into the plane layout
            for (int64_t i = 0; i < P; ++i) h[(size_t)k * ld + i] = y[(shared_y ? 0 : (size_t)i * Y) + k];
            for (int64_t i = P; i < ld; ++i) h[(size_t)k * ld + i] = 0.0;
        }
        h += (size_t)ld * Y;
        if (GQG) put(GQG, (size_t)D * D); else { memset(h, 0, sizeof(double) * D * D); h += (size_t)D * D; }
        if (R) put(R, (size_t)Y * Y); else { memset(h, 0, sizeof(double) * Y * Y); h += (size_t)Y * Y; }
        if (times) {
            for (int64_t i = 0; i < ld; ++i) *h++ = i < P ? times[i] : 0.0;
        } else {
            *h++ = time;
        }
    }
    double *in = (double *)(dev + off_in);
    double *xid = in; in += (size_t)Din * Nd;
    double *xio = in; in += (size_t)D * No;
    double *pard = in; in += (size_t)P * (1 + Din);
    double *paro = in; in += (size_t)P * (1 + D);
    double *min_ = in; in += (size_t)ns * Din;
    double *cin = in; in += (size_t)ns * Din * Din;
    double *ysoa = in; in += (size_t)ld * Y;
    double *gq = in; in += (size_t)D * D;
    double *rr = in; in += (size_t)Y * Y;
    double *tt = in;
    double *cd = (double *)(dev + off_cd), *co = (double *)(dev + off_co);
    int32_t *st_wd = (int32_t *)(dev + off_st), *st_wo = st_wd + ld, *st_td = st_wo + ld, *st_to = st_td + ld, *st_up = st_to + ld;
    // everything between the two pinned blocks as ONE unit.  The launch-per-stage route (ten launches + two copies) runs
    // eagerly the first time a (shape, item count) is seen, is captured into a hipGraph the second time and replayed from
    // then on: the marginalised filter calls this hundreds of times with two item counts (gradient: param_dim + 1,
    // marginalisation: 2 param_dim); 89 -> 76 us per call at P = 7
    // two launches - k_theta_weights (both transforms' weights, LDS-resident) and k_theta_chain (transform -> transform ->
    // update -> log-likelihood by the wave that owns the item) - where the point sets fit; else the launch per stage
    // ... or ONE launch with a lane per item for the small systems (k_theta_item, round 5)
    const bool item_route = theta_item_supported(Din, D, Y, Nd, No);
    const bool two_launch = item_route || (theta_chain_supported(Din, D, Y, Nd, No) && gp_theta_weights_fits(Din, Nd, D, No));
    auto enqueue = [&]() -> int {
    int rc;
    SSMQ_HIP(hipMemcpyAsync(dev + off_in, hin, sizeof(double) * n_in, hipMemcpyHostToDevice, s));
    if (item_route) {
        double *wo_ = (double *)(dev + off_out);
        double *m_fi = wo_, *P_fi = wo_ + ld * D, *ll = P_fi + ld * D * D;
        if ((rc = launch_theta_item(Din, D, Y, Nd, No, f_dyn, f_obs, h_dyn->emv_mode, h_obs->emv_mode, xid, xio, pard, paro, min_, cin,
                                    shared_state ? 0 : Din, shared_state ? 0 : (int64_t)Din * Din, ysoa, tt, times ? 1 : 0, gq, rr, jitter,
                                    m_fi, P_fi, ll, (int32_t *)(ll + ld), ld, P, nullptr, s)))
            return rc;
        SSMQ_HIP(hipMemcpyAsync(g_stage.hout, dev + off_out, out_bytes, hipMemcpyDeviceToHost, s));
        return SSMQ_OK;
    }
    if (!two_launch) {
        SSMQ_HIP(hipMemsetAsync(st_wd, 0, sizeof(int32_t) * 5 * ld, s));
        if ((rc = gp_weights_wide_consts(Din, D, Nd, xid, pard, (int)P, jitter, cd, st_wd, dev + off_ws, ws_d))) return rc;
        if ((rc = gp_weights_wide_consts(D, Y, No, xio, paro, (int)P, jitter, co, st_wo, dev + off_ws, ws_o))) return rc;
    } else {
        // every flag vector is written by the two kernels themselves (padding items beyond P are never read back)
        const int dd[2] = {Din, D}, ee[2] = {D, Y}, nn[2] = {Nd, No};
        const double *const xx[2] = {xid, xio}, *const pp[2] = {pard, paro};
        double *const cc[2] = {cd, co};
        int32_t *const ss[2] = {st_wd, st_wo};
        if ((rc = gp_theta_weights_pair(dd, ee, nn, xx, pp, (int)P, jitter, cc, ss))) return rc;
    }
    double *w = (double *)(dev + off_mid);
    double *m_pr = w; w += ld * D;
    double *P_pr = w; w += ld * D * D;
    double *C_xx = w; w += ld * D * Din;
    double *y_mean = w; w += ld * Y;
    double *P_y = w; w += ld * Y * Y;
    double *P_yx = w;
    w = (double *)(dev + off_out);
    double *m_fi = w; w += ld * D;
    double *P_fi = w; w += ld * D * D;
    double *ll = w; w += ld;
    int32_t *st_all = (int32_t *)w;
    WideArgs a;
    memset(&a, 0, sizeof(a));
    a.D = Din; a.E = D; a.N = Nd; a.form = SSMQ_FORM_BQ; a.mode = SSMQ_WIDE_FULL; a.fid = f_dyn->id; a.time_stride = times ? 1 : 0;
    a.emv_mode = h_dyn->emv_mode; a.tp_nu = 0.0; a.cov_scale = a.ccov_scale = 1.0;
    a.consts = cd; a.consts_stride = cld.total; a.cov_add = gq;
    a.mean = min_; a.cov = cin; a.time = tt; a.es_in = 1; a.bs_mean = shared_state ? 0 : Din;
    a.bs_cov = shared_state ? 0 : (int64_t)Din * Din;
    a.mean_f = m_pr; a.cov_f = P_pr; a.cov_fx = C_xx; a.es_out = ld; a.bs_mf = a.bs_cf = a.bs_cfx = 1; a.status = st_td;
    fill_fpar(f_dyn, &a.fp);
    const WideArgs a_dyn = a;
    if (!two_launch && (rc = hip_fail(launch_apply_wide(a, P, s), "k_apply_wide(theta, dyn)"))) return rc;
    a.D = D; a.E = Y; a.N = No; a.fid = f_obs->id; a.emv_mode = h_obs->emv_mode; a.consts = co; a.consts_stride = clo.total;
    a.cov_add = rr; a.mean = m_pr; a.cov = P_pr; a.es_in = ld; a.bs_mean = a.bs_cov = 1;
    a.mean_f = y_mean; a.cov_f = P_y; a.cov_fx = P_yx; a.status = st_to;
    fill_fpar(f_obs, &a.fp);
    if (two_launch) {
        const UpdArgs u{m_pr, P_pr, y_mean, P_y, P_yx, ysoa, m_fi, P_fi, st_up, nullptr, nullptr, P, ld, 0, D, Y, 0.0, nullptr, D};
        if ((rc = hip_fail(launch_theta_chain(a_dyn, a, u, ysoa, ll, st_wd, st_all, P, s), "k_theta_chain"))) return rc;
    } else {
    if ((rc = hip_fail(launch_apply_wide(a, P, s), "k_apply_wide(theta, obs)"))) return rc;
    if ((rc = launch_kalman_update(D, Y, P, ld, m_pr, P_pr, y_mean, P_y, P_yx, ysoa, m_fi, P_fi, st_up, s))) return rc;
    // log-likelihood and the merged status flags in one launch (the five partial vectors are contiguous, pitch ld)
    if ((rc = launch_gauss_logpdf(Y, P, ld, ysoa, y_mean, P_y, ll, s, st_wd, st_all))) return rc;
    }
    SSMQ_HIP(hipMemcpyAsync(g_stage.hout, dev + off_out, out_bytes, hipMemcpyDeviceToHost, s));
    return SSMQ_OK;
    };
    {
        std::vector<uint64_t> key = {(uint64_t)(uintptr_t)dev, (uint64_t)(uintptr_t)hin, (uint64_t)(uintptr_t)g_stage.hout, (uint64_t)P,
                                     (uint64_t)Din, (uint64_t)D, (uint64_t)Y, (uint64_t)Nd, (uint64_t)No, (uint64_t)shared_state,
                                     (uint64_t)h_dyn->emv_mode, (uint64_t)h_obs->emv_mode, (uint64_t)total, (uint64_t)two_launch, (uint64_t)(times ? 1 : 0)};
        uint64_t jb;
        memcpy(&jb, &jitter, sizeof(jb));
        key.push_back(jb);
        for (const ssmq_integrand *f : {f_dyn, f_obs}) {
            // what the kernels read of the descriptor: id, counts and the USED parameter / index slots (not the padding or the
            // unused tail, which a caller may leave uninitialised: every call would then look like a new graph)
            uint64_t hsh = 1469598103934665603ull;
            auto mix = [&](const void *p, size_t n) {
                const unsigned char *pb = (const unsigned char *)p;
                for (size_t i = 0; i < n; ++i) hsh = (hsh ^ pb[i]) * 1099511628211ull;
            };
            const int np_ = f->n_par < 0 ? 0 : (f->n_par > SSMQ_MAX_FPAR ? SSMQ_MAX_FPAR : f->n_par);
            const int ni_ = f->n_idx < 0 ? 0 : (f->n_idx > SSMQ_MAX_FIDX ? SSMQ_MAX_FIDX : f->n_idx);
            mix(&f->id, sizeof(f->id)); mix(&f->n_par, sizeof(f->n_par)); mix(&f->n_idx, sizeof(f->n_idx));
            mix(f->par, sizeof(f->par[0]) * np_); mix(f->idx, sizeof(f->idx[0]) * ni_);
            key.push_back(hsh);
        }
        ThetaGraph *tg = nullptr;
        for (auto &g : g_theta_graphs)
            if (g.key == key) tg = &g;
        // two launches + two copies: replay measured no faster (52 us either way).  Per-item times = the batched marginalised
        // filter, whose item count changes from round to round: every new count would be captured, instantiated and evict an
        // older entry of the six-slot cache without ever being replayed.
        if (two_launch || times || ssmq::sw("SSMQ_NO_THETA_GRAPH")) {
            if ((rc = enqueue())) return rc;
        } else if (!tg) {
            if (g_theta_graphs.size() >= 6) {       // the oldest entry goes, not all of them (a filter alternates between two item counts)
                if (g_theta_graphs.front().exec) hipGraphExecDestroy(g_theta_graphs.front().exec);
                if (g_theta_graphs.front().graph) hipGraphDestroy(g_theta_graphs.front().graph);
                g_theta_graphs.erase(g_theta_graphs.begin());
            }
            g_theta_graphs.push_back(ThetaGraph{key, nullptr, nullptr});
            if ((rc = enqueue())) return rc;
        } else {
            if (!tg->exec) {
                SSMQ_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
                rc = enqueue();
                hipGraph_t g = nullptr;
                hipError_t ce = hipStreamEndCapture(s, &g);
                if (rc || ce != hipSuccess) {
                    if (g) hipGraphDestroy(g);
                    return rc ? rc : hip_fail(ce, "hipStreamEndCapture(theta step)");
                }
                const hipError_t ie = hipGraphInstantiate(&tg->exec, g, nullptr, nullptr, 0);
                if (ie != hipSuccess) {
                    hipGraphDestroy(g);
                    tg->exec = nullptr;
                    return hip_fail(ie, "hipGraphInstantiate(theta step)");
                }
                tg->graph = g;
            }
            SSMQ_HIP(hipGraphLaunch(tg->exec, s));
        }
    }
    SSMQ_HIP(hipStreamSynchronize(s));
    // planes -> the caller's item-major arrays
    const double *ho = (const double *)g_stage.hout;
    const int32_t *hst = (const int32_t *)(ho + n_out * ld);
    for (int e = 0; e < D; ++e)
        for (int64_t i = 0; i < P; ++i) post_mean[(size_t)i * D + e] = ho[(size_t)e * ld + i];
    const double *hp = ho + (size_t)D * ld;
    for (int e = 0; e < D * D; ++e)
        for (int64_t i = 0; i < P; ++i) post_cov[(size_t)i * D * D + e] = hp[(size_t)e * ld + i];
    memcpy(loglik, hp + (size_t)D * D * ld, sizeof(double) * P);
    int first = 0;
    for (int64_t i = 0; i < P; ++i) {
        if (status) status[i] = hst[i];
        if (hst[i] && !first) first = (int)std::min<int64_t>(i + 1, 0x7fffffff);
    }
    return first;
}

// ---- the theta-batched step with its items ALREADY on the device and their number in device memory --------------------------
// (the device-resident rounds of the batched marginalised filter, ssmq_marginal_device.hip: no host copy and no synchronisation per
// round; the kernels are the two of gp_theta_step_impl's two-launch route, launched on an upper bound of the item count.)
namespace ssmq {
bool theta_dev_supported(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs) {
    if (!h_dyn || !h_obs || !f_dyn || !f_obs) return false;
    const int Din = h_dyn->D, D = h_dyn->E, Y = h_obs->E, Nd = h_dyn->N, No = h_obs->N;
    if (Din < D || h_obs->D != D || h_dyn->form != SSMQ_FORM_BQ || h_obs->form != SSMQ_FORM_BQ || h_dyn->tp_nu > 0.0 || h_obs->tp_nu > 0.0)
        return false;
    FInfo fi;
    if (check_integrand(h_dyn, f_dyn, &fi) || check_integrand(h_obs, f_obs, &fi))
        return false;
    return theta_item_supported(Din, D, Y, Nd, No) || (theta_chain_supported(Din, D, Y, Nd, No) && gp_theta_weights_fits(Din, Nd, D, No));
}

size_t theta_dev_bytes(const ssmq_transform *h_dyn, const ssmq_transform *h_obs, int64_t cap) {
    ThetaDev t;
    return theta_dev_carve(t, h_dyn, h_obs, cap, nullptr);
}

// lays the arena out (base may be null: size only); returns its size in bytes
size_t theta_dev_carve(ThetaDev &t, const ssmq_transform *h_dyn, const ssmq_transform *h_obs, int64_t cap, void *base) {
    const int Din = h_dyn->D, D = h_dyn->E, Y = h_obs->E, Nd = h_dyn->N, No = h_obs->N;
    const int64_t ld = (cap + 63) / 64 * 64;
    const WideLayout cld = wide_layout(Din, D, Nd, SSMQ_FORM_BQ), clo = wide_layout(D, Y, No, SSMQ_FORM_BQ);
    t.Din = Din; t.D = D; t.Y = Y; t.Nd = Nd; t.No = No; t.cap = cap; t.ld = ld;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? (char *)base + off : nullptr;
        off += (bytes + 255) / 256 * 256;
        return p;
    };
    t.xid = (double *)take(sizeof(double) * Din * Nd);
    t.xio = (double *)take(sizeof(double) * D * No);
    t.gq = (double *)take(sizeof(double) * D * D);
    t.rr = (double *)take(sizeof(double) * Y * Y);
    t.pard = (double *)take(sizeof(double) * cap * (1 + Din));
    t.paro = (double *)take(sizeof(double) * cap * (1 + D));
    t.mean = (double *)take(sizeof(double) * cap * Din);
    t.cov = (double *)take(sizeof(double) * cap * Din * Din);
    t.ysoa = (double *)take(sizeof(double) * ld * Y);
    t.tt = (double *)take(sizeof(double) * ld);
    t.cd = (double *)take(sizeof(double) * cap * cld.total);
    t.co = (double *)take(sizeof(double) * cap * clo.total);
    t.mid = (double *)take(sizeof(double) * ld * ((size_t)D + (size_t)D * D + (size_t)D * Din + Y + (size_t)Y * Y + (size_t)Y * D));
    t.m_fi = (double *)take(sizeof(double) * ld * D);
    t.P_fi = (double *)take(sizeof(double) * ld * D * D);
    t.ll = (double *)take(sizeof(double) * ld);
    t.st_all = (int32_t *)take(sizeof(int32_t) * ld);
    t.st5 = (int32_t *)take(sizeof(int32_t) * 5 * ld);
    return off;
}

// uploads what does not change between rounds: the unit points of both transforms, G Q G' (zeros for dynamics that take their
// noise as an argument) and R
int theta_dev_upload_static(const ThetaDev &t, const ssmq_transform *h_dyn, const ssmq_transform *h_obs, const double *GQG, const double *R,
                            hipStream_t s) {
    SSMQ_HIP(hipMemcpyAsync(t.xid, h_dyn->xi.data(), sizeof(double) * t.Din * t.Nd, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(t.xio, h_obs->xi.data(), sizeof(double) * t.D * t.No, hipMemcpyHostToDevice, s));
    if (GQG) SSMQ_HIP(hipMemcpyAsync(t.gq, GQG, sizeof(double) * t.D * t.D, hipMemcpyHostToDevice, s));
    else SSMQ_HIP(hipMemsetAsync(t.gq, 0, sizeof(double) * t.D * t.D, s));
    if (R) SSMQ_HIP(hipMemcpyAsync(t.rr, R, sizeof(double) * t.Y * t.Y, hipMemcpyHostToDevice, s));
    else SSMQ_HIP(hipMemsetAsync(t.rr, 0, sizeof(double) * t.Y * t.Y, s));
    SSMQ_HIP(hipStreamSynchronize(s));        // (the host vectors may go away)
    return SSMQ_OK;
}

// weights of both transforms, then transform -> transform -> update -> log-likelihood per item: two launches covering
// `bound` items (>= the count the kernels read from *d_count; 0 < bound <= t.cap)
int theta_dev_enqueue(const ThetaDev &t, const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                      const ssmq_integrand *f_obs, double jitter, int64_t bound, const int32_t *d_count, hipStream_t s) {
    if (bound < 1 || bound > t.cap) {
        set_error("theta_dev_enqueue: bad bound");
        return SSMQ_E_ARG;
    }
    const int Din = t.Din, D = t.D, Y = t.Y, Nd = t.Nd, No = t.No;
    const int64_t ld = t.ld;
    if (theta_item_supported(Din, D, Y, Nd, No))
        return launch_theta_item(Din, D, Y, Nd, No, f_dyn, f_obs, h_dyn->emv_mode, h_obs->emv_mode, t.xid, t.xio, t.pard, t.paro, t.mean, t.cov,
                                 Din, (int64_t)Din * Din, t.ysoa, t.tt, 1, t.gq, t.rr, jitter, t.m_fi, t.P_fi, t.ll, t.st_all, ld, bound,
                                 d_count, s);
    const WideLayout cld = wide_layout(Din, D, Nd, SSMQ_FORM_BQ), clo = wide_layout(D, Y, No, SSMQ_FORM_BQ);
    int32_t *st_wd = t.st5, *st_wo = st_wd + ld, *st_td = st_wo + ld, *st_to = st_td + ld, *st_up = st_to + ld;
    int rc;
    {
        const int dd[2] = {Din, D}, ee[2] = {D, Y}, nn[2] = {Nd, No};
        const double *const xx[2] = {t.xid, t.xio}, *const pp[2] = {t.pard, t.paro};
        double *const cc[2] = {t.cd, t.co};
        int32_t *const ss[2] = {st_wd, st_wo};
        if ((rc = gp_theta_weights_pair(dd, ee, nn, xx, pp, (int)bound, jitter, cc, ss, d_count))) return rc;
    }
    double *w = t.mid;
    double *m_pr = w; w += ld * D;
    double *P_pr = w; w += ld * D * D;
    double *C_xx = w; w += ld * D * Din;
    double *y_mean = w; w += ld * Y;
    double *P_y = w; w += ld * Y * Y;
    double *P_yx = w;
    WideArgs a;
    memset(&a, 0, sizeof(a));
    a.D = Din; a.E = D; a.N = Nd; a.form = SSMQ_FORM_BQ; a.mode = SSMQ_WIDE_FULL; a.fid = f_dyn->id; a.time_stride = 1;
    a.emv_mode = h_dyn->emv_mode; a.tp_nu = 0.0; a.cov_scale = a.ccov_scale = 1.0;
    a.consts = t.cd; a.consts_stride = cld.total; a.cov_add = t.gq;
    a.mean = t.mean; a.cov = t.cov; a.time = t.tt; a.es_in = 1; a.bs_mean = Din; a.bs_cov = (int64_t)Din * Din;
    a.mean_f = m_pr; a.cov_f = P_pr; a.cov_fx = C_xx; a.es_out = ld; a.bs_mf = a.bs_cf = a.bs_cfx = 1; a.status = st_td;
    fill_fpar(f_dyn, &a.fp);
    const WideArgs a_dyn = a;
    a.D = D; a.E = Y; a.N = No; a.fid = f_obs->id; a.emv_mode = h_obs->emv_mode; a.consts = t.co; a.consts_stride = clo.total;
    a.cov_add = t.rr; a.mean = m_pr; a.cov = P_pr; a.es_in = ld; a.bs_mean = a.bs_cov = 1;
    a.mean_f = y_mean; a.cov_f = P_y; a.cov_fx = P_yx; a.status = st_to;
    fill_fpar(f_obs, &a.fp);
    const UpdArgs u{m_pr, P_pr, y_mean, P_y, P_yx, t.ysoa, t.m_fi, t.P_fi, st_up, nullptr, nullptr, bound, ld, 0, D, Y, 0.0, nullptr, D};
    return hip_fail(launch_theta_chain(a_dyn, a, u, t.ysoa, t.ll, st_wd, t.st_all, bound, s, d_count), "k_theta_chain(device rounds)");
}
}  // namespace ssmq
