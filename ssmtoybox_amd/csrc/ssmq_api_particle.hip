// C entry points of the bootstrap particle filter (include/ssmq.h: ssmq_particle_filter_dev, ssmq_particle_kernel_name): the range
// check, the host-side constants (noise factors padded to the kernel's strides, the measurement density's log-normaliser) and the
// launch of k_particle_filter<D> (ssmq_particle.hip).  And of the particle smoothers over its cloud (ssmq_particle_smoother_dev,
// ssmq_particle_smoother_kernel_name): the range check, the whitening data of the marginal smoother (the inverse factor of G Q G',
// refused where the transition has no density) and the launch of k_particle_smooth<D> / k_particle_lineage<D>
// (ssmq_particle_smooth.hip).  The *_rv entry points describe the initial state and the process noise by ssmq_rv (Gaussian or
// Student-t) and share everything else with the four above: all-Gaussian descriptors run the same kernels on the same arguments.
#include <cmath>
#include <cstdio>
#include "ssmq_particle.h"

namespace ssmq {
namespace {

// models that take their noise as an argument: no likelihood in closed form
bool pf_noise_is_argument(int fid) { return fid == SSMQ_F_UNGMNA_DYN || fid == SSMQ_F_UNGMNA_MEAS || fid == SSMQ_F_CTRS_DYN; }

// everything about a call that can be decided without a device: SSMQ_OK, SSMQ_E_ARG or SSMQ_E_UNSUPPORTED (error text set)
int pf_check(const char *what, const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N, const ssmq_rv *r) {
    char msg[512];
    if (!f_dyn || !f_obs || !r) {
        snprintf(msg, sizeof(msg), "%s: null model or noise pointer", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand(what);
    if (N < kPfMinN || N % 64 != 0) {
        snprintf(msg, sizeof(msg), "%s: N = %d particles - a multiple of 64, at least 64, is needed", what, N);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (D < 1 || Y < 1 || dq < 1) {
        snprintf(msg, sizeof(msg), "%s: D, Y and dq must be at least 1", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    const char *range = "built-in additive-noise models, 1 <= D <= 6, 1 <= Y <= 4, 1 <= dq <= 6, N a multiple of 64 in 64 .. 4096 with "
                        "(2 D + 1) N <= 13312 (the cloud lives in LDS), Gaussian or Student-t measurement noise";
    if (pf_noise_is_argument(f_dyn->id) || pf_noise_is_argument(f_obs->id)) {
        snprintf(msg, sizeof(msg), "%s: not implemented for models that take their noise as an argument (non-additive noise); range: %s",
                 what, range);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if (r->kind == SSMQ_RV_MIXTURE) {
        snprintf(msg, sizeof(msg), "%s: not implemented for Gaussian-mixture measurement noise; range: %s", what, range);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if (!pf_shape_ok(D, Y, dq, N)) {
        snprintf(msg, sizeof(msg), "%s: D = %d, Y = %d, dq = %d, N = %d is outside the range: %s", what, D, Y, dq, N, range);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if ((r->kind != SSMQ_RV_GAUSS && r->kind != SSMQ_RV_STUDENT) || r->dim != Y || r->n_comp > 1 || !r->chol ||
        (r->kind == SSMQ_RV_STUDENT && !(r->dof > 0.0))) {
        snprintf(msg, sizeof(msg), "%s: measurement noise must be SSMQ_RV_GAUSS or SSMQ_RV_STUDENT (dof > 0) of dimension Y with a factor", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    for (int e = 0; e < Y; ++e)
        if (!(r->chol[e * Y + e] > 0.0)) {
            snprintf(msg, sizeof(msg), "%s: the factor of R needs a positive diagonal", what);
            set_error(msg);
            return SSMQ_E_ARG;
        }
    FInfo fid, fio;
    if (!integrand_info(f_dyn->id, &fid) || fid.dout != D || fid.din != D || f_dyn->n_idx != 0) {
        snprintf(msg, sizeof(msg), "%s: transition integrand / dimension mismatch (D -> D, no state index)", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (!integrand_info(f_obs->id, &fio) || (fio.dout ? fio.dout : Y) != Y || f_obs->n_idx < 0 || f_obs->n_idx > SSMQ_MAX_FIDX ||
        (f_obs->n_idx == 0 && fio.din > D) || (f_obs->n_idx != 0 && f_obs->n_idx < fio.din)) {
        snprintf(msg, sizeof(msg), "%s: measurement integrand / dimension mismatch (a state index must name every input the integrand reads)", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    for (int k = 0; k < f_obs->n_idx; ++k)
        if (f_obs->idx[k] < 0 || f_obs->idx[k] >= D) {
            snprintf(msg, sizeof(msg), "%s: measurement state index out of range", what);
            set_error(msg);
            return SSMQ_E_ARG;
        }
    return SSMQ_OK;
}

// One side (the initial state or the process noise) of the *_rv entry points: kind and dof, and with dim >= 0 also the dimension, the
// component count and the factor.  *nu: 0 for Gaussian, the degrees of freedom for Student-t.
int pf_rv_side(const char *what, const char *side, const ssmq_rv *v, int dim, double *nu) {
    char msg[512];
    const char *range = "SSMQ_RV_GAUSS or SSMQ_RV_STUDENT with one component and dof >= 2 (the Gamma sampler of the Student-t draws, "
                        "Marsaglia-Tsang, needs the shape dof / 2 >= 1) for the initial state and the process noise";
    if (!v) {
        snprintf(msg, sizeof(msg), "%s: null descriptor of %s", what, side);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (v->kind == SSMQ_RV_MIXTURE) {
        snprintf(msg, sizeof(msg), "%s: not implemented for a Gaussian mixture as %s; range: %s", what, side, range);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if ((v->kind != SSMQ_RV_GAUSS && v->kind != SSMQ_RV_STUDENT) || (dim >= 0 && (v->dim != dim || v->n_comp > 1 || !v->chol)) ||
        (v->kind == SSMQ_RV_STUDENT && !(v->dof > 0.0 && std::isfinite(v->dof)))) {
        snprintf(msg, sizeof(msg), "%s: %s must be SSMQ_RV_GAUSS or SSMQ_RV_STUDENT (finite dof > 0)%s", what, side,
                 dim >= 0 ? " of dimension dq with one component and a factor" : "");
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (v->kind == SSMQ_RV_STUDENT && v->dof < 2.0) {
        snprintf(msg, sizeof(msg), "%s: dof = %g of %s is below 2; range: %s", what, v->dof, side, range);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    *nu = v->kind == SSMQ_RV_STUDENT ? v->dof : 0.0;
    return SSMQ_OK;
}

const char *pf_kernel_text(int qk) { return qk ? "k_particle_filter<D=%d, QK=1> (N = %d, %zu B of LDS per trajectory)"
                                                 : "k_particle_filter<D=%d> (N = %d, %zu B of LDS per trajectory)"; }

}  // namespace

// Largest and smallest eigenvalue of the symmetric n x n matrix A (row-major, n <= kPfMaxD) by cyclic Jacobi rotations.  Also the
// condition number ssmq_api_pcrlb.hip refuses by (declared in ssmq_pcrlb.h).
void ps_eig_range(const double *A, int n, double *lo, double *hi) {
    double M[kPfMaxD * kPfMaxD];
    for (int i = 0; i < n * n; ++i) M[i] = A[i];
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) (r == c ? diag : off) += M[r * n + c] * M[r * n + c];
        if (off <= 1e-60 * diag || off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                if (M[p * n + q] == 0.0) continue;
                const double theta = (M[q * n + q] - M[p * n + p]) / (2.0 * M[p * n + q]);
                const double tn = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
                for (int k = 0; k < n; ++k) {          // columns p, q
                    const double kp = M[k * n + p], kq = M[k * n + q];
                    M[k * n + p] = cs * kp - sn * kq;
                    M[k * n + q] = sn * kp + cs * kq;
                }
                for (int k = 0; k < n; ++k) {          // rows p, q
                    const double pk = M[p * n + k], qk = M[q * n + k];
                    M[p * n + k] = cs * pk - sn * qk;
                    M[q * n + k] = sn * pk + cs * qk;
                }
            }
    }
    *lo = *hi = M[0];
    for (int i = 1; i < n; ++i) {
        *lo = std::min(*lo, M[i * n + i]);
        *hi = std::max(*hi, M[i * n + i]);
    }
}

namespace {

// everything about a smoother call that can be decided without a device; fills the whitening data of the marginal method
int ps_check(const char *what, const ssmq_integrand *f_dyn, int D, int dq, int N, const double *q_mean, const double *q_chol,
             const double *G, int method, PsLaunch *h) {
    char msg[640];
    if (!f_dyn) {
        snprintf(msg, sizeof(msg), "%s: null model pointer", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (is_user_integrand(f_dyn)) return refuse_user_integrand(what);
    if (method != SSMQ_PS_MARGINAL && method != SSMQ_PS_GENEALOGY) {
        snprintf(msg, sizeof(msg), "%s: unknown method %d (SSMQ_PS_MARGINAL = 0, SSMQ_PS_GENEALOGY = 1)", what, method);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (N < kPfMinN || N % 64 != 0) {
        snprintf(msg, sizeof(msg), "%s: N = %d particles - a multiple of 64, at least 64, is needed", what, N);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (D < 1 || dq < 1) {
        snprintf(msg, sizeof(msg), "%s: D and dq must be at least 1", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    const char *range = "the cloud of ssmq_particle_filter_dev: built-in additive-noise models, 1 <= D <= 6, 1 <= dq <= 6, N a multiple of 64 "
                        "in 64 .. 4096 with (2 D + 1) N <= 13312";
    if (pf_noise_is_argument(f_dyn->id)) {
        snprintf(msg, sizeof(msg), "%s: not implemented for models that take their noise as an argument (non-additive noise); range: %s",
                 what, range);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if (!pf_shape_ok(D, 1, dq, N)) {
        snprintf(msg, sizeof(msg), "%s: D = %d, dq = %d, N = %d is outside the range: %s", what, D, dq, N, range);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    FInfo fid;
    if (!integrand_info(f_dyn->id, &fid) || fid.dout != D || fid.din != D || f_dyn->n_idx != 0) {
        snprintf(msg, sizeof(msg), "%s: transition integrand / dimension mismatch (D -> D, no state index)", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    h->f_dyn = f_dyn; h->D = D; h->N = N; h->method = method;
    if (method == SSMQ_PS_GENEALOGY) return SSMQ_OK;
    if (!q_chol) {
        snprintf(msg, sizeof(msg), "%s: the marginal method needs q_chol", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    const char *hint = "the transition has no density on the state space and the marginal smoother (FFBSm) does not exist; "
                       "use the genealogy method (method='genealogy')";
    if (dq != D) {
        snprintf(msg, sizeof(msg), "%s: dq = %d != D = %d, the process noise G Q G' is singular: %s", what, dq, D, hint);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    // Sigma = (G Lq)(G Lq)', its Cholesky factor Ls and condition number
    double GL[kPfMaxD * kPfMaxD], Sg[kPfMaxD * kPfMaxD], Ls[kPfMaxD * kPfMaxD];
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            double s = 0.0;
            for (int k = c; k < D; ++k) s += (G ? G[r * D + k] : (r == k ? 1.0 : 0.0)) * q_chol[k * D + c];
            GL[r * D + c] = s;
        }
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            double s = 0.0;
            for (int k = 0; k < D; ++k) s += GL[r * D + k] * GL[c * D + k];
            Sg[r * D + c] = s;
        }
    bool pd = true;
    for (int c = 0; c < D && pd; ++c)
        for (int r = c; r < D; ++r) {
            double s = Sg[r * D + c];
            for (int k = 0; k < c; ++k) s -= Ls[r * D + k] * Ls[c * D + k];
            if (r == c) {
                if (!(s > 0.0) || !std::isfinite(s)) { pd = false; break; }
                Ls[c * D + c] = sqrt(s);
            } else {
                Ls[r * D + c] = s / Ls[c * D + c];
            }
        }
    double lo = 0.0, hi = 0.0;
    if (pd) ps_eig_range(Sg, D, &lo, &hi);
    if (!pd || !(lo > 0.0)) {
        snprintf(msg, sizeof(msg), "%s: the process noise G Q G' is not positive definite: %s", what, hint);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if (!(hi / lo <= 1e12)) {
        snprintf(msg, sizeof(msg), "%s: the condition number of G Q G' is %.3g, above 1e12: the whitened distances of the marginal smoother "
                 "would carry no digits (method='genealogy' does not need them)", what, hi / lo);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    // Li = Ls^-1 by forward substitution, column by column
    memset(h->Li, 0, sizeof(h->Li));
    for (int c = 0; c < D; ++c)
        for (int r = c; r < D; ++r) {
            double s = r == c ? 1.0 : 0.0;
            for (int k = c; k < r; ++k) s -= Ls[r * D + k] * h->Li[k * kPfMaxD + c];
            h->Li[r * kPfMaxD + c] = s / Ls[r * D + r];
        }
    for (int r = 0; r < D; ++r) {
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += (G ? G[r * D + k] : (r == k ? 1.0 : 0.0)) * (q_mean ? q_mean[k] : 0.0);
        h->gq[r] = s;
    }
    return SSMQ_OK;
}

}  // namespace
}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_particle_kernel_name(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N,
                                         const ssmq_rv *r, char *buf, int len) {
    if (!buf || len < 1) {
        set_error("ssmq_particle_kernel_name: null buffer");
        return SSMQ_E_ARG;
    }
    int rc = pf_check("ssmq_particle_kernel_name", f_dyn, f_obs, D, Y, dq, N, r);
    if (rc) return rc;
    snprintf(buf, (size_t)len, pf_kernel_text(0), D, N, pf_lds_bytes(D, N));
    return SSMQ_OK;
}

// the pass of both filter entry points after their range checks (nu0, nuq: 0 = Gaussian)
static int pf_run(const char *what, const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N, int64_t B,
                  int64_t ld, int T, const double *d_y, const double *d_m0, const double *d_P0, const double *q_mean, const double *q_chol,
                  double nu0, double nuq, const double *G, const ssmq_rv *r, double ess_threshold, uint64_t seed, uint64_t traj_offset,
                  double *d_fm, double *d_fP, double *d_loglik, double *d_ess, int32_t *d_status, double *d_part, double *d_logw,
                  int32_t *d_anc) {
    int rc;
    if (T < 1 || B < 0 || ld < B || B > 0x7fffffff || !d_y || !d_m0 || !d_P0 || !q_chol || !d_fm || !d_fP || !d_loglik || !d_ess || !d_status ||
        ess_threshold != ess_threshold) {
        set_error(std::string(what) + ": bad argument (T >= 1, 0 <= B <= ld, non-null buffers and q_chol, ess_threshold not NaN)");
        return SSMQ_E_ARG;
    }
    PfLaunch h;
    memset(&h, 0, sizeof(h));
    h.nu0 = nu0; h.nuq = nuq;
    h.f_dyn = f_dyn; h.f_obs = f_obs; h.D = D; h.Y = Y; h.dq = dq; h.N = N; h.T = T; h.B = B; h.ld = ld; h.seed = seed;
    h.traj_offset = traj_offset; h.ess_threshold = ess_threshold;
    for (int i = 0; i < dq; ++i) {
        h.qm[i] = q_mean ? q_mean[i] : 0.0;
        for (int k = 0; k <= i; ++k) h.Lq[i * kPfMaxQ + k] = q_chol[i * dq + k];
    }
    for (int d = 0; d < D; ++d)        // default noise gain eye(D, dq)  (ssmod.py:52)
        for (int k = 0; k < dq; ++k) h.G[d * kPfMaxQ + k] = G ? G[d * dq + k] : (d == k ? 1.0 : 0.0);
    double logdet = 0.0;
    for (int e = 0; e < kPfMaxY; ++e) {
        h.Lr[e * kPfMaxY + e] = 1.0;
        if (e >= Y) continue;
        h.rm[e] = r->mean ? r->mean[e] : 0.0;
        for (int k = 0; k <= e; ++k) h.Lr[e * kPfMaxY + k] = r->chol[e * Y + k];
        logdet += log(r->chol[e * Y + e]);
    }
    h.student = r->kind == SSMQ_RV_STUDENT ? 1 : 0;
    h.dof = h.student ? r->dof : 0.0;
    // log-normaliser: Gaussian -Y/2 log(2 pi) - log det L; Student-t lgamma((dof + Y)/2) - lgamma(dof/2) - Y/2 log(dof pi) - log det L
    h.lognorm = h.student ? lgamma(0.5 * (h.dof + Y)) - lgamma(0.5 * h.dof) - 0.5 * Y * log(h.dof * M_PI) - logdet
                          : -0.5 * Y * log(2.0 * M_PI) - logdet;
    h.y = d_y; h.m0 = d_m0; h.P0 = d_P0; h.fm = d_fm; h.fP = d_fP; h.ll = d_loglik; h.ess = d_ess; h.status = d_status;
    h.part = d_part; h.logw = d_logw; h.anc = d_anc;
    rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    rc = launch_particle_filter(h, s);
    hipError_t e = hipStreamSynchronize(s);
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

extern "C" int ssmq_particle_filter_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N, int64_t B,
                                        int64_t ld, int T, const double *d_y, const double *d_m0, const double *d_P0,
                                        const double *q_mean, const double *q_chol, const double *G, const ssmq_rv *r,
                                        double ess_threshold, uint64_t seed, uint64_t traj_offset, double *d_fm, double *d_fP,
                                        double *d_loglik, double *d_ess, int32_t *d_status, double *d_part, double *d_logw,
                                        int32_t *d_anc) {
    int rc = pf_check("ssmq_particle_filter_dev", f_dyn, f_obs, D, Y, dq, N, r);
    if (rc) return rc;
    return pf_run("ssmq_particle_filter_dev", f_dyn, f_obs, D, Y, dq, N, B, ld, T, d_y, d_m0, d_P0, q_mean, q_chol, 0.0, 0.0, G, r,
                  ess_threshold, seed, traj_offset, d_fm, d_fP, d_loglik, d_ess, d_status, d_part, d_logw, d_anc);
}

extern "C" int ssmq_particle_kernel_name_rv(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N,
                                            const ssmq_rv *x0, const ssmq_rv *q, const ssmq_rv *r, char *buf, int len) {
    if (!buf || len < 1) {
        set_error("ssmq_particle_kernel_name_rv: null buffer");
        return SSMQ_E_ARG;
    }
    double nu0 = 0.0, nuq = 0.0;
    int rc = pf_check("ssmq_particle_kernel_name_rv", f_dyn, f_obs, D, Y, dq, N, r);
    if (!rc) rc = pf_rv_side("ssmq_particle_kernel_name_rv", "the initial state", x0, -1, &nu0);
    if (!rc) rc = pf_rv_side("ssmq_particle_kernel_name_rv", "the process noise", q, dq, &nuq);
    if (rc) return rc;
    snprintf(buf, (size_t)len, pf_kernel_text(pf_noise_kind(nu0, nuq)), D, N, pf_lds_bytes(D, N));
    return SSMQ_OK;
}

extern "C" int ssmq_particle_filter_rv_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N, int64_t B,
                                           int64_t ld, int T, const double *d_y, const double *d_m0, const double *d_P0,
                                           const ssmq_rv *x0, const ssmq_rv *q, const double *G, const ssmq_rv *r, double ess_threshold,
                                           uint64_t seed, uint64_t traj_offset, double *d_fm, double *d_fP, double *d_loglik,
                                           double *d_ess, int32_t *d_status, double *d_part, double *d_logw, int32_t *d_anc) {
    double nu0 = 0.0, nuq = 0.0;
    int rc = pf_check("ssmq_particle_filter_rv_dev", f_dyn, f_obs, D, Y, dq, N, r);
    if (!rc) rc = pf_rv_side("ssmq_particle_filter_rv_dev", "the initial state", x0, -1, &nu0);
    if (!rc) rc = pf_rv_side("ssmq_particle_filter_rv_dev", "the process noise", q, dq, &nuq);
    if (rc) return rc;
    return pf_run("ssmq_particle_filter_rv_dev", f_dyn, f_obs, D, Y, dq, N, B, ld, T, d_y, d_m0, d_P0, q->mean, q->chol, nu0, nuq, G, r,
                  ess_threshold, seed, traj_offset, d_fm, d_fP, d_loglik, d_ess, d_status, d_part, d_logw, d_anc);
}

extern "C" int ssmq_particle_smoother_kernel_name(const ssmq_integrand *f_dyn, int D, int dq, int N, const double *q_mean,
                                                  const double *q_chol, const double *G, int method, char *buf, int len) {
    if (!buf || len < 1) {
        set_error("ssmq_particle_smoother_kernel_name: null buffer");
        return SSMQ_E_ARG;
    }
    PsLaunch h;
    memset(&h, 0, sizeof(h));
    int rc = ps_check("ssmq_particle_smoother_kernel_name", f_dyn, D, dq, N, q_mean, q_chol, G, method, &h);
    if (rc) return rc;
    snprintf(buf, (size_t)len, "%s<D=%d> (N = %d, %zu B of LDS per trajectory)",
             method == SSMQ_PS_MARGINAL ? "k_particle_smooth" : "k_particle_lineage", D, N, ps_lds_bytes(method, D, N));
    return SSMQ_OK;
}

// the pass of both smoother entry points after their range checks (h: what ps_check filled, and nuq)
static int ps_run(const char *what, PsLaunch &h, int method, int64_t B, int64_t ld, int T, const double *d_part, const double *d_logw,
                  const int32_t *d_anc, const double *d_fm, const double *d_fP, const double *d_ess, const int32_t *d_status, double *d_sm,
                  double *d_sP, double *d_ess_s, double *d_logw_s, int32_t *d_lineage, int32_t *d_unique) {
    int rc;
    if (T < 1 || B < 0 || ld < B || B > 0x7fffffff || !d_part || !d_logw || !d_fm || !d_fP || !d_ess || !d_status || !d_sm || !d_sP ||
        !d_ess_s || (method == SSMQ_PS_GENEALOGY && !d_anc)) {
        set_error(std::string(what) + ": bad argument (T >= 1, 0 <= B <= ld, non-null buffers; d_anc for SSMQ_PS_GENEALOGY)");
        return SSMQ_E_ARG;
    }
    h.T = T; h.B = B; h.ld = ld;
    h.part = d_part; h.logw = d_logw; h.anc = d_anc; h.fm = d_fm; h.fP = d_fP; h.ess = d_ess; h.status = d_status;
    h.sm = d_sm; h.sP = d_sP; h.ess_s = d_ess_s; h.logw_s = d_logw_s;
    h.lineage = method == SSMQ_PS_GENEALOGY ? d_lineage : nullptr;
    h.unique = method == SSMQ_PS_GENEALOGY ? d_unique : nullptr;
    rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    rc = launch_particle_smoother(h, s);
    hipError_t e = hipStreamSynchronize(s);
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

extern "C" int ssmq_particle_smoother_dev(const ssmq_integrand *f_dyn, int D, int dq, int N, int64_t B, int64_t ld, int T,
                                          const double *q_mean, const double *q_chol, const double *G, int method, const double *d_part,
                                          const double *d_logw, const int32_t *d_anc, const double *d_fm, const double *d_fP,
                                          const double *d_ess, const int32_t *d_status, double *d_sm, double *d_sP, double *d_ess_s,
                                          double *d_logw_s, int32_t *d_lineage, int32_t *d_unique) {
    PsLaunch h;
    memset(&h, 0, sizeof(h));
    int rc = ps_check("ssmq_particle_smoother_dev", f_dyn, D, dq, N, q_mean, q_chol, G, method, &h);
    if (rc) return rc;
    return ps_run("ssmq_particle_smoother_dev", h, method, B, ld, T, d_part, d_logw, d_anc, d_fm, d_fP, d_ess, d_status, d_sm, d_sP, d_ess_s,
                  d_logw_s, d_lineage, d_unique);
}

// the range check of both *_rv smoother entry points: ps_check on the descriptor's mean and factor, and its degrees of freedom
static int ps_check_rv(const char *what, const ssmq_integrand *f_dyn, int D, int dq, int N, const ssmq_rv *q, const double *G, int method,
                       PsLaunch *h) {
    double nuq = 0.0;
    int rc = pf_rv_side(what, "the process noise", q, dq >= 1 ? dq : -1, &nuq);
    if (!rc) rc = ps_check(what, f_dyn, D, dq, N, q->mean, q->chol, G, method, h);
    if (rc) return rc;
    h->nuq = method == SSMQ_PS_MARGINAL ? nuq : 0.0;
    return SSMQ_OK;
}

extern "C" int ssmq_particle_smoother_kernel_name_rv(const ssmq_integrand *f_dyn, int D, int dq, int N, const ssmq_rv *q, const double *G,
                                                     int method, char *buf, int len) {
    if (!buf || len < 1) {
        set_error("ssmq_particle_smoother_kernel_name_rv: null buffer");
        return SSMQ_E_ARG;
    }
    PsLaunch h;
    memset(&h, 0, sizeof(h));
    int rc = ps_check_rv("ssmq_particle_smoother_kernel_name_rv", f_dyn, D, dq, N, q, G, method, &h);
    if (rc) return rc;
    snprintf(buf, (size_t)len, "%s<D=%d%s> (N = %d, %zu B of LDS per trajectory)",
             method == SSMQ_PS_MARGINAL ? "k_particle_smooth" : "k_particle_lineage", D, h.nuq > 0.0 ? ", QK=1" : "", N,
             ps_lds_bytes(method, D, N));
    return SSMQ_OK;
}

extern "C" int ssmq_particle_smoother_rv_dev(const ssmq_integrand *f_dyn, int D, int dq, int N, int64_t B, int64_t ld, int T,
                                             const ssmq_rv *q, const double *G, int method, const double *d_part, const double *d_logw,
                                             const int32_t *d_anc, const double *d_fm, const double *d_fP, const double *d_ess,
                                             const int32_t *d_status, double *d_sm, double *d_sP, double *d_ess_s, double *d_logw_s,
                                             int32_t *d_lineage, int32_t *d_unique) {
    PsLaunch h;
    memset(&h, 0, sizeof(h));
    int rc = ps_check_rv("ssmq_particle_smoother_rv_dev", f_dyn, D, dq, N, q, G, method, &h);
    if (rc) return rc;
    return ps_run("ssmq_particle_smoother_rv_dev", h, method, B, ld, T, d_part, d_logw, d_anc, d_fm, d_fP, d_ess, d_status, d_sm, d_sP,
                  d_ess_s, d_logw_s, d_lineage, d_unique);
}
