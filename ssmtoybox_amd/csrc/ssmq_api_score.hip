// C ABI of libssmq (include/ssmq.h), the scoring recursion of the t-process and Studentian filters: ssmq_student_scores_dev (one
// Studentian pass from two transform handles) and ssmq_filter_sweep_t_dev (P rows of (par_dyn, par_obs, nu, dof) of a t-process
// filter, Gaussian or Studentian recursion) - the refusals, the row blocks and the one launch of k_filter_score<>
// (ssmq_filter_score.hip).
#include <cmath>
#include <string>
#include <vector>
#include "ssmq_filter_score_kernel.h"
#include "ssmq_host.h"

namespace ssmq {

const char *find_score_kernel(const ScoreShape &shape);
int launch_score(const ScoreShape &shape, const ScoreArgs &a, hipStream_t s);
// row p's dense constant block (ssmq_api_sweep.hip)
void sweep_block(int D, int E, int N, const double *xi, const double *wm, const double *Wc, const double *Wcc, double model_var, double *s);

static const char kScoreRange[] =
    "student_scores / filter_sweep_t: t-process transforms (weights of the 'rbf' kernel) with the Gaussian or the Studentian recursion, "
    "fully-symmetric (sigma-point) transforms with the Studentian recursion, on the built-in additive-noise model pairs of the fused "
    "time loop with D <= 4, Y <= 2, 2 <= N <= 2 D + 1 points (the same count for both transforms); P <= 65535 rows";

static int score_refuse(int code, const std::string &why) {
    set_error(why + " - " + kScoreRange);
    return code;
}

// What every entry point checks first, in this order; *shape: the key of the kernel's table.
static int score_route(const char *who, const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int N_dyn, int N_obs, int D, int Y, int form,
                       int tp, int stu, ScoreShape *shape, const char **name) {
    const std::string w(who);
    if (!f_dyn || !f_obs || D < 1 || Y < 1 || N_dyn < 1 || N_obs < 1) return score_refuse(SSMQ_E_ARG, w + ": bad argument");
    int selo = 0;
    if (int rc = additive_pair_route(score_refuse, w, f_dyn, f_obs, D, [] { return (int)SSMQ_OK; }, &selo)) return rc;
    if (D > 4 || Y > 2) return score_refuse(SSMQ_E_UNSUPPORTED, w + ": dimension out of range");
    if (N_dyn > 2 * D + 1 || N_obs > 2 * D + 1 || N_dyn < 2 || N_obs < 2) return score_refuse(SSMQ_E_UNSUPPORTED, w + ": point count out of range");
    *shape = {{f_dyn->id, f_obs->id, D, Y, N_dyn, N_obs, form, tp, selo, 0}, stu};
    const char *kn = selo < 0 ? nullptr : find_score_kernel(*shape);
    if (!kn) return score_refuse(SSMQ_E_UNSUPPORTED, w + ": no kernel for this pair of models, point sets, form and recursion");
    if (name) *name = kn;
    return SSMQ_OK;
}

// The handles of ssmq_student_scores_*: both t-process BQ, or both sigma-point; *form / *tp receive the kernel's arguments.
static int score_handles(const char *who, const ssmq_transform *h_dyn, const ssmq_transform *h_obs, int *form, int *tp) {
    const std::string w(who);
    if (!h_dyn || !h_obs) return score_refuse(SSMQ_E_ARG, w + ": bad argument");
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo(who);
    if (is_trunc(h_dyn) || is_trunc(h_obs)) return refuse_trunc(who);
    if (is_gpqd(h_dyn) || is_gpqd(h_obs)) return refuse_gpqd(who);
    if (is_taylor_gpqd(h_dyn) || is_taylor_gpqd(h_obs)) return refuse_taylor_gpqd(who);
    const bool tpd = h_dyn->tp_nu > 0.0, tpo = h_obs->tp_nu > 0.0;
    if (h_dyn->form != h_obs->form || tpd != tpo || h_obs->D != h_dyn->D || h_dyn->E != h_dyn->D ||
        !((h_dyn->form == SSMQ_FORM_BQ && tpd) || (h_dyn->form == SSMQ_FORM_SIGMA && !tpd)) || !h_dyn->d_small || !h_obs->d_small)
        return score_refuse(SSMQ_E_UNSUPPORTED, w + ": both transforms t-process BQ, or both sigma-point rules, of one state dimension");
    *form = h_dyn->form;
    *tp = tpd ? 1 : 0;
    return SSMQ_OK;
}

// lgamma((dof + Y) / 2) - lgamma(dof / 2) - Y / 2 log(dof pi): the constant of the Student-t density
static double student_lnorm(double dof, int Y) { return std::lgamma(0.5 * (dof + Y)) - std::lgamma(0.5 * dof) - 0.5 * Y * std::log(dof * M_PI); }

// One row block (ssmq_filter_score_kernel.h); null gqg / rr = zeros, null scale = ones, dof <= 0: Gaussian recursion (dof, lnorm unused)
static void score_row(double *r, int D, int Y, int T, double nu_dyn, double nu_obs, double dof, const double *gqg, const double *rr,
                      const double *m0, const double *S0, const double *scale) {
    std::fill(r, r + score_row_doubles(D, Y, T), 0.0);
    r[0] = nu_dyn; r[1] = nu_obs; r[2] = dof > 0.0 ? dof : 1.0; r[3] = dof > 0.0 ? student_lnorm(dof, Y) : 0.0;
    double *q = r + kScoreRowHead;
    if (gqg) std::copy(gqg, gqg + D * D, q);
    q += D * D;
    if (rr) std::copy(rr, rr + Y * Y, q);
    q += Y * Y;
    std::copy(m0, m0 + D, q);
    q += D;
    std::copy(S0, S0 + D * D, q);
    q += D * D;
    for (int k = 0; k < T; ++k) q[k] = scale ? scale[k] : 1.0;
}

// T == 0 (ssmq_host.h): also the empty pass of ssmq_filter_sweep_dev and ssmq_filter_noise_sweep_dev
int score_empty(const char *who, int P, int64_t ld, const int32_t *theta_status, double *d_ll_total, double *d_nis_mean, int32_t *d_status) {
    hipStream_t s = stream();
    const size_t items = (size_t)P * ld;
    SSMQ_HIP(hipMemsetAsync(d_ll_total, 0, sizeof(double) * items, s));
    SSMQ_HIP(hipMemsetAsync(d_nis_mean, 0, sizeof(double) * items, s));
    SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * items, s));
    for (int p = 0; theta_status && p < P; ++p)
        if (theta_status[p]) {
            SSMQ_HIP(hipMemsetAsync(d_ll_total + (size_t)p * ld, 0xff, sizeof(double) * ld, s));    // (all bits set: a NaN; -1)
            SSMQ_HIP(hipMemsetAsync(d_nis_mean + (size_t)p * ld, 0xff, sizeof(double) * ld, s));
            SSMQ_HIP(hipMemsetAsync(d_status + (size_t)p * ld, 0xff, sizeof(int32_t) * ld, s));
        }
    return hip_fail(hipStreamSynchronize(s), who);
}

// The launch both entry points end in.  consts: host image c_dyn [P][nd] | c_obs [P][no], or empty with d_c_dyn / d_c_obs the blocks
// of two handles (P = 1); rows: host [P][score_row_doubles]; theta_status: host [P] or null.  One upload, one launch, synchronous.
struct ScoreCall {
    const char *who;
    const ssmq_integrand *fd, *fo;
    ScoreShape shape;
    int emv_dyn, emv_obs, P, T;
    int64_t B, ld;
    const double *d_y, *d_c_dyn, *d_c_obs;
    const int32_t *theta_status;
    double *ll_total, *nis_mean, *ll_steps, *nis_steps;
    int32_t *status;
};
static int score_launch(const ScoreCall &c, const std::vector<double> &consts, const std::vector<double> &rows) {
    const int D = c.shape.D, Y = c.shape.Y, T = c.T, P = c.P;
    const size_t nd = const_layout(D, D, c.shape.ND, c.shape.form).total, no = const_layout(D, Y, c.shape.NO, c.shape.form).total;
    const size_t rs = score_row_doubles(D, Y, T), ntt = ((size_t)2 * T + 7) / 8 * 8;
    const size_t o_rows = consts.size(), o_tt = o_rows + rows.size(), n_dbl = o_tt + ntt;
    std::vector<double> host(n_dbl + ((size_t)P + 1) / 2, 0.0);
    std::copy(consts.begin(), consts.end(), host.begin());
    std::copy(rows.begin(), rows.end(), host.begin() + o_rows);
    const bool ttd = time_table(c.fd->id, T, host.data() + o_tt), tto = time_table(c.fo->id, T, host.data() + o_tt + T);
    if (c.theta_status) memcpy(host.data() + n_dbl, c.theta_status, sizeof(int32_t) * P);
    hipStream_t s = stream();
    DeviceImage img;
    if (int rc = img.alloc(host.size())) return rc;
    double *const dev = img.dev;
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.y = c.d_y;
    a.c_dyn = consts.empty() ? c.d_c_dyn : dev;
    a.c_obs = consts.empty() ? c.d_c_obs : dev + (size_t)P * nd;
    a.rows = dev + o_rows; a.row_stride = (int64_t)rs;
    a.theta_status = c.theta_status ? (const int32_t *)(dev + n_dbl) : nullptr;
    a.ll_total = c.ll_total; a.nis_mean = c.nis_mean; a.ll_steps = c.ll_steps; a.nis_steps = c.nis_steps; a.status = c.status;
    a.B = c.B; a.ld = c.ld; a.T = T; a.P = P;
    a.emv_dyn = c.emv_dyn; a.emv_obs = c.emv_obs;
    fill_fpar(c.fd, &a.fd);
    fill_fpar(c.fo, &a.fo);
    a.fd.ttab = ttd ? dev + o_tt : nullptr;
    a.fo.ttab = tto ? dev + o_tt + T : nullptr;
    int rc = img.upload(host, c.who);
    if (!rc) rc = launch_score(c.shape, a, s);
    const int rs2 = hip_fail(hipStreamSynchronize(s), c.who);
    return rc ? rc : rs2;
}

}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_student_scores_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                               const ssmq_integrand *f_obs, char *buf, int len) {
    if (!buf || len <= 0) return score_refuse(SSMQ_E_ARG, "student_scores: bad argument");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    int form = 0, tp = 0;
    ScoreShape shape;
    const char *name = nullptr;
    if (int rc = score_handles("student_scores", h_dyn, h_obs, &form, &tp)) return rc;
    if (int rc = score_route("student_scores", f_dyn, f_obs, h_dyn->N, h_obs->N, h_dyn->D, h_obs->E, form, tp, 1, &shape, &name)) return rc;
    snprintf(buf, len, "%s", name);
    return SSMQ_OK;
}

extern "C" int ssmq_student_scores_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                                       int64_t B, int64_t ld, int T, const double *d_y, const double *x0_mean, const double *x0_smat,
                                       const double *GqG, const double *r_smat, const double *scale, double dof, double *d_nis,
                                       double *d_loglik, double *d_loglik_total, double *d_nis_mean, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    int form = 0, tp = 0;
    ScoreShape shape;
    if (int rc = score_handles("student_scores", h_dyn, h_obs, &form, &tp)) return rc;
    const int D = h_dyn->D, Y = h_obs->E;
    if (int rc = score_route("student_scores", f_dyn, f_obs, h_dyn->N, h_obs->N, D, Y, form, tp, 1, &shape, nullptr)) return rc;
    if (B < 0 || ld < B || ld % kSmallBlock != 0 || T < 0 || !d_y || !x0_mean || !x0_smat || (T > 0 && !scale) || !(dof > 2.0) || !std::isfinite(dof) ||
        !d_loglik_total || !d_nis_mean || !d_status)
        return score_refuse(SSMQ_E_ARG, "student_scores: bad argument (ld a multiple of 64 and >= B, scale [T], dof > 2)");
    if (int rc = ensure_device()) return rc;
    if (B == 0) return SSMQ_OK;
    if (T == 0) return score_empty("student_scores", 1, ld, nullptr, d_loglik_total, d_nis_mean, d_status);
    std::vector<double> rows(score_row_doubles(D, Y, T));
    score_row(rows.data(), D, Y, T, h_dyn->tp_nu, h_obs->tp_nu, dof, GqG, r_smat, x0_mean, x0_smat, scale);
    ScoreCall c{"student_scores", f_dyn, f_obs, shape, h_dyn->emv_mode, h_obs->emv_mode, 1, T, B, ld, d_y,
                h_dyn->d_small, h_obs->d_small, nullptr, d_loglik_total, d_nis_mean, d_loglik, d_nis, d_status};
    return score_launch(c, std::vector<double>(), rows);
}

extern "C" int ssmq_filter_sweep_t_kernel_name(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int recursion, int N_dyn, int N_obs,
                                               int D, int Y, char *buf, int len) {
    if (!buf || len <= 0 || (recursion != SSMQ_RECURSION_GAUSS && recursion != SSMQ_RECURSION_STUDENT))
        return score_refuse(SSMQ_E_ARG, "filter_sweep_t: bad argument");
    ScoreShape shape;
    const char *name = nullptr;
    if (int rc = score_route("filter_sweep_t", f_dyn, f_obs, N_dyn, N_obs, D, Y, SSMQ_FORM_BQ, 1, recursion, &shape, &name)) return rc;
    snprintf(buf, len, "%s", name);
    return SSMQ_OK;
}

extern "C" int ssmq_filter_sweep_t_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int recursion, const double *xi_dyn, int N_dyn,
                                       const double *xi_obs, int N_obs, const double *par_dyn, const double *par_obs, const double *nu_dyn,
                                       const double *nu_obs, const double *dof, int P, double jitter_dyn, double jitter_obs, int D, int Y,
                                       int64_t B, int64_t ld, int T, const double *d_y, const double *x0_mean, const double *x0_mat,
                                       const double *GQG, const double *R, const double *scale, double *d_loglik_total, double *d_nis_mean,
                                       double *d_loglik_steps, int32_t *d_status, int32_t *theta_status) {
    if (recursion != SSMQ_RECURSION_GAUSS && recursion != SSMQ_RECURSION_STUDENT) return score_refuse(SSMQ_E_ARG, "filter_sweep_t: bad recursion");
    const bool stu = recursion == SSMQ_RECURSION_STUDENT;
    ScoreShape shape;
    if (int rc = score_route("filter_sweep_t", f_dyn, f_obs, N_dyn, N_obs, D, Y, SSMQ_FORM_BQ, 1, recursion, &shape, nullptr)) return rc;
    if (!xi_dyn || !xi_obs || !par_dyn || !par_obs || !nu_dyn || !nu_obs || P < 1 || B < 0 || ld < B || ld % kSmallBlock != 0 || T < 0 || !d_y ||
        !x0_mean || !x0_mat || !d_loglik_total || !d_nis_mean || !d_status || !theta_status || (stu && (!dof || (T > 0 && !scale))))
        return score_refuse(SSMQ_E_ARG, "filter_sweep_t: bad argument (P >= 1, ld a multiple of 64 and >= B; Studentian recursion: dof [P], scale [P][T])");
    if (P > 65535) return score_refuse(SSMQ_E_UNSUPPORTED, "filter_sweep_t: too many rows");
    for (int p = 0; p < P; ++p) {
        if (!(nu_dyn[p] > 0.0) || !(nu_obs[p] > 0.0) || !std::isfinite(nu_dyn[p]) || !std::isfinite(nu_obs[p]))
            return score_refuse(SSMQ_E_ARG, "filter_sweep_t: nu of row " + std::to_string(p) + " is not a positive number");
        if (stu && (!(dof[p] > 2.0) || !std::isfinite(dof[p])))
            return score_refuse(SSMQ_E_ARG, "filter_sweep_t: dof of row " + std::to_string(p) + " is not above 2");
    }
    if (int rc = ensure_device()) return rc;
    // ---- the weights of every row, one theta-batched call per transform (with the inverse kernel matrix of the t-process) ------
    const int N[2] = {N_dyn, N_obs}, E[2] = {D, Y};
    const double *xi[2] = {xi_dyn, xi_obs}, *par[2] = {par_dyn, par_obs}, jit[2] = {jitter_dyn, jitter_obs};
    std::vector<double> wm[2], Wc[2], Wcc[2], iK[2], mv[2];
    std::vector<int32_t> st[2];
    for (int q = 0; q < 2; ++q) {
        wm[q].assign((size_t)P * N[q], 0.0); Wc[q].assign((size_t)P * N[q] * N[q], 0.0); Wcc[q].assign((size_t)P * D * N[q], 0.0);
        iK[q].assign((size_t)P * N[q] * N[q], 0.0); mv[q].assign(P, 0.0); st[q].assign(P, 0);
        const int rc = ssmq_weights_gp(D, N[q], xi[q], par[q], P, jit[q], wm[q].data(), Wc[q].data(), Wcc[q].data(), iK[q].data(), nullptr, nullptr,
                                       nullptr, mv[q].data(), nullptr, st[q].data());
        if (rc < 0) return rc;
    }
    for (int p = 0; p < P; ++p) theta_status[p] = st[0][p] + 4 * st[1][p];
    if (B == 0) return SSMQ_OK;
    if (T == 0) return score_empty("filter_sweep_t", P, ld, theta_status, d_loglik_total, d_nis_mean, d_status);
    // ---- the constant blocks (the dense part as ssmq_filter_sweep_dev lays it out, + iK transposed) and the row blocks ---------
    const ConstLayout cl[2] = {const_layout(D, D, N_dyn, SSMQ_FORM_BQ), const_layout(D, Y, N_obs, SSMQ_FORM_BQ)};
    std::vector<double> consts((size_t)P * (cl[0].total + cl[1].total), 0.0);
    const size_t rs = score_row_doubles(D, Y, T);
    std::vector<double> rows((size_t)P * rs);
    for (int p = 0; p < P; ++p) {
        for (int q = 0; q < 2; ++q) {
            double *blk = consts.data() + (q ? (size_t)P * cl[0].total : 0) + (size_t)p * cl[q].total;
            sweep_block(D, E[q], N[q], xi[q], wm[q].data() + (size_t)p * N[q], Wc[q].data() + (size_t)p * N[q] * N[q],
                        Wcc[q].data() + (size_t)p * D * N[q], mv[q][p], blk);
            const double *ik = iK[q].data() + (size_t)p * N[q] * N[q];
            for (int i = 0; i < N[q]; ++i)
                for (int j = 0; j < N[q]; ++j) blk[cl[q].iK + j * N[q] + i] = ik[i * N[q] + j];
        }
        score_row(rows.data() + (size_t)p * rs, D, Y, T, nu_dyn[p], nu_obs[p], stu ? dof[p] : 0.0, GQG ? GQG + (size_t)p * D * D : nullptr,
                  R ? R + (size_t)p * Y * Y : nullptr, x0_mean, x0_mat + (size_t)p * D * D, stu ? scale + (size_t)p * T : nullptr);
    }
    // the model variance of a t-process transform built with one output (the t-process filters of ssinf.py): the whole matrix for E > 1
    ScoreCall c{"filter_sweep_t", f_dyn, f_obs, shape, D == 1 ? SSMQ_EMV_DIAG : SSMQ_EMV_BROADCAST,
                Y == 1 ? SSMQ_EMV_DIAG : SSMQ_EMV_BROADCAST, P, T, B, ld, d_y, nullptr, nullptr, theta_status, d_loglik_total, d_nis_mean,
                d_loglik_steps, nullptr, d_status};
    return score_launch(c, consts, rows);
}
