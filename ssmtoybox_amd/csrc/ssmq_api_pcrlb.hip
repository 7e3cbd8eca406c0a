// C entry points of the posterior Cramer-Rao bound (include/ssmq.h: ssmq_pcrlb_sums_dev, ssmq_pcrlb_sums_width,
// ssmq_pcrlb_kernel_name, ssmq_pcrlb_finalize): the range check, the host-side constants (Qi = (G Q G')^-1 and Ri = R^-1 by Cholesky),
// the workspace and the launch of the kernels of ssmq_pcrlb_kernel.h, and the recursion itself - host code in double, no device.
#include <cmath>
#include <cstdio>
#include "ssmq_pcrlb.h"

namespace ssmq {
namespace {

constexpr int kMaxN = kPcrlbHostMaxD;

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return hip_fail(hipMalloc(&p, bytes ? bytes : 8), "hipMalloc"); }
    double *d() { return (double *)p; }
};

// models that take their noise as an argument: no additive-noise information matrix
bool noise_is_argument(int fid) { return fid == SSMQ_F_UNGMNA_DYN || fid == SSMQ_F_UNGMNA_MEAS || fid == SSMQ_F_CTRS_DYN; }

// lower Cholesky factor of the symmetric n x n matrix A (row-major, lower triangle read): false at a pivot that is not positive and finite
bool chol_host(const double *A, int n, double *L) {
    for (int i = 0; i < n * n; ++i) L[i] = 0.0;
    for (int c = 0; c < n; ++c)
        for (int r = c; r < n; ++r) {
            double s = A[r * n + c];
            for (int k = 0; k < c; ++k) s -= L[r * n + k] * L[c * n + k];
            if (r == c) {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                L[c * n + c] = sqrt(s);
            } else {
                L[r * n + c] = s / L[c * n + c];
            }
        }
    return true;
}
// Inv = (L L')^-1 = Li' Li with Li = L^-1 by forward substitution; symmetric, both triangles from one value
void inv_from_chol(const double *L, int n, double *Inv) {
    double Li[kMaxN * kMaxN] = {};
    for (int c = 0; c < n; ++c)
        for (int r = c; r < n; ++r) {
            double s = r == c ? 1.0 : 0.0;
            for (int k = c; k < r; ++k) s -= L[r * n + k] * Li[k * n + c];
            Li[r * n + c] = s / L[r * n + r];
        }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k <= i; ++k) {
            double s = 0.0;
            for (int m = i; m < n; ++m) s += Li[m * n + i] * Li[m * n + k];
            Inv[i * n + k] = Inv[k * n + i] = s;
        }
}

const char *kRange = "additive Gaussian noise; models with a Jacobian on the device (built-in: UNGM, pendulum, constant velocity; user models "
                     "registered with one), 1 <= D <= 6, 1 <= Y <= 4, dq == D with G Q G' positive definite";

// The process noise of a call: SSMQ_OK with Qi = (G Q G')^-1 [D][D], or the refusal (error text set)
int noise_check(const char *what, int D, int dq, const ssmq_rv *q, const double *G, double *Qi) {
    char msg[640];
    if (q->kind == SSMQ_RV_STUDENT || q->kind == SSMQ_RV_MIXTURE) {
        snprintf(msg, sizeof(msg), "%s: not implemented for %s process noise; range: %s", what,
                 q->kind == SSMQ_RV_STUDENT ? "Student-t" : "Gaussian-mixture", kRange);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if (q->kind != SSMQ_RV_GAUSS || q->dim != dq || q->n_comp > 1 || !q->chol) {
        snprintf(msg, sizeof(msg), "%s: the process noise must be SSMQ_RV_GAUSS of dimension dq with a factor", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    const char *hint = "the transition has no density on the state space and the recursion of Tichavsky et al. does not apply as stated";
    if (dq != D) {
        snprintf(msg, sizeof(msg), "%s: dq = %d != D = %d, the process noise G Q G' is singular: %s; range: %s", what, dq, D, hint, kRange);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    double GL[kMaxN * kMaxN], Sg[kMaxN * kMaxN], Ls[kMaxN * kMaxN];
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            double s = 0.0;
            for (int k = c; k < D; ++k) s += (G ? G[r * D + k] : (r == k ? 1.0 : 0.0)) * q->chol[k * D + c];
            GL[r * D + c] = s;
        }
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            double s = 0.0;
            for (int k = 0; k < D; ++k) s += GL[r * D + k] * GL[c * D + k];
            Sg[r * D + c] = s;
        }
    const bool pd = chol_host(Sg, D, Ls);
    double lo = 0.0, hi = 0.0;
    if (pd) ps_eig_range(Sg, D, &lo, &hi);
    if (!pd || !(lo > 0.0)) {
        snprintf(msg, sizeof(msg), "%s: the process noise G Q G' is not positive definite: %s; range: %s", what, hint, kRange);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if (!(hi / lo <= 1e12)) {
        snprintf(msg, sizeof(msg), "%s: the condition number of G Q G' is %.3g, above 1e12: its inverse would carry no digits", what, hi / lo);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    inv_from_chol(Ls, D, Qi);
    return SSMQ_OK;
}

// everything about a call that can be decided without a device; fills the models, shapes and Qi / Ri of the launch
int pcrlb_check(const char *what, const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, const ssmq_rv *q,
                const double *G, const ssmq_rv *r, PcrlbLaunch *h) {
    char msg[640];
    if (!f_dyn || !f_obs || !q || !r) {
        snprintf(msg, sizeof(msg), "%s: null model or noise pointer", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    FInfo fid, fio;
    if (!integrand_info(f_dyn->id, &fid) || !integrand_info(f_obs->id, &fio)) {
        snprintf(msg, sizeof(msg), "%s: unknown integrand id", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (noise_is_argument(f_dyn->id) || noise_is_argument(f_obs->id)) {
        snprintf(msg, sizeof(msg), "%s: not implemented for models that take their noise as an argument (non-additive noise); range: %s", what,
                 kRange);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    for (const ssmq_integrand *f : {f_dyn, f_obs})
        if (is_user_integrand(f) ? !user_integrand_has_jacobian(f->id) : !integrand_has_jacobian(f->id)) {
            snprintf(msg, sizeof(msg), "%s: the %s model has no Jacobian on the device (a user model gets one through ssmq_integrand_define_dx); "
                     "range: %s", what, f == f_dyn ? "transition" : "measurement", kRange);
            set_error(msg);
            return SSMQ_E_UNSUPPORTED;
        }
    if (r->kind == SSMQ_RV_STUDENT || r->kind == SSMQ_RV_MIXTURE) {
        snprintf(msg, sizeof(msg), "%s: not implemented for %s measurement noise; range: %s", what,
                 r->kind == SSMQ_RV_STUDENT ? "Student-t" : "Gaussian-mixture", kRange);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    if (q->kind == SSMQ_RV_STUDENT || q->kind == SSMQ_RV_MIXTURE) return noise_check(what, D, dq, q, G, h->Qi);
    if (D < 1 || Y < 1 || dq < 1) {
        snprintf(msg, sizeof(msg), "%s: D, Y and dq must be at least 1", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if (D > kPcrlbHostMaxD || Y > kPcrlbHostMaxY) {
        snprintf(msg, sizeof(msg), "%s: D = %d, Y = %d is outside the range: %s", what, D, Y, kRange);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    for (const ssmq_integrand *f : {f_dyn, f_obs})
        if (is_user_integrand(f) && f->n_idx != 0) {
            snprintf(msg, sizeof(msg), "%s: user integrands take the leading state entries: no state index; range: %s", what, kRange);
            set_error(msg);
            return SSMQ_E_UNSUPPORTED;
        }
    if (fid.dout != D || f_dyn->n_idx != 0 || (is_user_integrand(f_dyn) ? fid.din > D : fid.din != D)) {
        snprintf(msg, sizeof(msg), "%s: transition integrand / dimension mismatch (D -> D, no state index)", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    if ((fio.dout ? fio.dout : Y) != Y || f_obs->n_idx < 0 || f_obs->n_idx > SSMQ_MAX_FIDX || (f_obs->n_idx == 0 && fio.din > D) ||
        (f_obs->n_idx != 0 && f_obs->n_idx < fio.din)) {
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
    // (a built-in Jacobian of 1 < din < D columns without a state index lands in the leading din columns: jac_front_builtin)
    if ((!is_user_integrand(f_dyn) && !pcrlb_builtin_dyn_shape(D)) || (!is_user_integrand(f_obs) && !pcrlb_builtin_obs_shape(D, Y))) {
        snprintf(msg, sizeof(msg), "%s: no kernel for this built-in shape (D = %d, Y = %d); range: %s", what, D, Y, kRange);
        set_error(msg);
        return SSMQ_E_UNSUPPORTED;
    }
    int rc = noise_check(what, D, dq, q, G, h->Qi);
    if (rc) return rc;
    if (r->kind != SSMQ_RV_GAUSS || r->dim != Y || r->n_comp > 1 || !r->chol) {
        snprintf(msg, sizeof(msg), "%s: the measurement noise must be SSMQ_RV_GAUSS of dimension Y with a factor", what);
        set_error(msg);
        return SSMQ_E_ARG;
    }
    double Lr[kMaxN * kMaxN] = {};
    for (int e = 0; e < Y; ++e) {
        if (!(r->chol[e * Y + e] > 0.0) || !std::isfinite(r->chol[e * Y + e])) {
            snprintf(msg, sizeof(msg), "%s: the factor of R needs a positive diagonal", what);
            set_error(msg);
            return SSMQ_E_ARG;
        }
        for (int k = 0; k <= e; ++k) Lr[e * Y + k] = r->chol[e * Y + k];
    }
    double Ri[kMaxN * kMaxN];
    inv_from_chol(Lr, Y, Ri);
    for (int i = 0; i < Y * Y; ++i) h->Ri[i] = Ri[i];
    h->f_dyn = f_dyn; h->f_obs = f_obs; h->D = D; h->Y = Y; h->din_dyn = fid.din; h->din_obs = fio.din;
    return SSMQ_OK;
}

}  // namespace
}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_pcrlb_sums_width(int D) { return D >= 1 && D <= kPcrlbHostMaxD ? pcrlb_sums_width(D) : SSMQ_E_ARG; }

extern "C" int ssmq_pcrlb_kernel_name(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, const ssmq_rv *q,
                                      const double *G, const ssmq_rv *r, char *buf, int len) {
    if (!buf || len < 1) {
        set_error("ssmq_pcrlb_kernel_name: null buffer");
        return SSMQ_E_ARG;
    }
    PcrlbLaunch h;
    memset(&h, 0, sizeof(h));
    int rc = pcrlb_check("ssmq_pcrlb_kernel_name", f_dyn, f_obs, D, Y, dq, q, G, r, &h);
    if (rc) return rc;
    h.B = 1; h.ld = 1; h.T = 1;
    const char *nd = nullptr, *no = nullptr;
    if ((rc = launch_pcrlb(h, nullptr, &nd, &no, true))) return rc;
    const std::string sd = is_user_integrand(f_dyn) ? std::string(nd) : std::string(nd) + "<" + std::to_string(D) + ", " + std::to_string(D) + ">";
    const std::string so = is_user_integrand(f_obs) ? std::string(no) : std::string(no) + "<" + std::to_string(D) + ", " + std::to_string(Y) + ">";
    snprintf(buf, (size_t)len, "%s | %s | k_pcrlb_rows", sd.c_str(), so.c_str());
    return SSMQ_OK;
}

extern "C" int ssmq_pcrlb_sums_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int64_t B, int64_t ld,
                                   int T, const double *d_x, const ssmq_rv *q, const double *G, const ssmq_rv *r, double *sums) {
    PcrlbLaunch h;
    memset(&h, 0, sizeof(h));
    int rc = pcrlb_check("ssmq_pcrlb_sums_dev", f_dyn, f_obs, D, Y, dq, q, G, r, &h);
    if (rc) return rc;
    if (T < 1 || B < 0 || ld < B || B > 0x7fffffff || !d_x || !sums) {
        set_error("ssmq_pcrlb_sums_dev: bad argument (T >= 1, 0 <= B <= ld, non-null d_x and sums)");
        return SSMQ_E_ARG;
    }
    const int S = pcrlb_sums_width(D);
    if ((int64_t)T * pcrlb_groups(B) > 0x7fffffff) {
        set_error("ssmq_pcrlb_sums_dev: T ceil(B / 256) workgroups exceed 2^31 - 1; split the steps over several calls");
        return SSMQ_E_ARG;
    }
    rc = ensure_device();
    if (rc) return rc;
    if (B == 0) {
        memset(sums, 0, sizeof(double) * (size_t)T * S);
        return SSMQ_OK;
    }
    hipStream_t s = stream();
    DevBuf ws, out;
    if ((rc = ws.alloc(sizeof(double) * pcrlb_ws_doubles(D, T, B))) || (rc = out.alloc(sizeof(double) * (size_t)T * S))) return rc;
    std::vector<double> steps((size_t)T);
    for (int j = 0; j < T; ++j) steps[j] = (double)j;
    SSMQ_HIP(hipMemcpyAsync(ws.p, steps.data(), sizeof(double) * (size_t)T, hipMemcpyHostToDevice, s));
    h.B = B; h.ld = ld; h.T = T; h.x = d_x; h.ws = ws.d(); h.sums = out.d();
    rc = launch_pcrlb(h, s, nullptr, nullptr, false);
    std::vector<double> host((size_t)T * S);
    if (!rc) rc = hip_fail(hipMemcpyAsync(host.data(), out.p, sizeof(double) * host.size(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
    hipError_t e = hipStreamSynchronize(s);
    if (rc) return rc;
    SSMQ_HIP(e);
    memcpy(sums, host.data(), sizeof(double) * host.size());
    return SSMQ_OK;
}

extern "C" int ssmq_pcrlb_finalize(int D, int T, int64_t B_total, const double *sums, const double *P0, const ssmq_rv *q, const double *G,
                                   double *info, double *bound, double *rmse_bound, int32_t *status) {
    if (!sums || !P0 || !q || !status || T < 1 || B_total < 1 || D < 1) {
        set_error("ssmq_pcrlb_finalize: bad argument (non-null sums, P0, q and status, T >= 1, B_total >= 1, D >= 1)");
        return SSMQ_E_ARG;
    }
    if (D > kPcrlbHostMaxD) {
        set_error(std::string("ssmq_pcrlb_finalize: D = ") + std::to_string(D) + " is outside the range: " + kRange);
        return SSMQ_E_UNSUPPORTED;
    }
    double Qi[kMaxN * kMaxN];
    int rc = noise_check("ssmq_pcrlb_finalize", D, q->dim, q, G, Qi);
    if (rc) return rc;
    const int tri = D * (D + 1) / 2, S = pcrlb_sums_width(D), DD = D * D;
    const double nan = std::nan(""), inv_n = 1.0 / (double)B_total;
    double Jp[kMaxN * kMaxN], L[kMaxN * kMaxN], M[kMaxN * kMaxN], D12[kMaxN * kMaxN], D22[kMaxN * kMaxN], X[kMaxN * kMaxN], Jn[kMaxN * kMaxN] = {},
        Bn[kMaxN * kMaxN] = {};
    int failed = 0;                                   // 0, or 1 + the step that failed
    if (chol_host(P0, D, L)) inv_from_chol(L, D, Jp);   // J_{-1} = P0^-1
    else failed = 1;
    for (int j = 0; j < T; ++j) {
        const double *row = sums + (size_t)j * S;
        if (!failed) {
            bool finite = true;
            for (int i = 0; i < S; ++i) finite = finite && std::isfinite(row[i]);
            if (!finite) failed = 1 + j;
        }
        if (!failed) {
            // M = J_{j-1} + D11,  D12 = -(mean F)' Qi,  D22 = Qi + mean H' Ri H
            for (int i = 0; i < D; ++i)
                for (int k = 0; k <= i; ++k) {
                    M[i * D + k] = M[k * D + i] = Jp[i * D + k] + row[i * (i + 1) / 2 + k] * inv_n;
                    D22[i * D + k] = D22[k * D + i] = Qi[i * D + k] + row[tri + DD + i * (i + 1) / 2 + k] * inv_n;
                }
            for (int i = 0; i < D; ++i)
                for (int k = 0; k < D; ++k) {
                    double s = 0.0;
                    for (int m = 0; m < D; ++m) s += (row[tri + m * D + i] * inv_n) * Qi[m * D + k];
                    D12[i * D + k] = -s;
                }
            if (!chol_host(M, D, L)) failed = 1 + j;
        }
        if (!failed) {
            // X = M^-1 D12 column by column (forward, then backward substitution);  J_j = D22 - D12' X, the lower triangle mirrored
            for (int c = 0; c < D; ++c) {
                double v[kMaxN];
                for (int i = 0; i < D; ++i) {
                    double s = D12[i * D + c];
                    for (int k = 0; k < i; ++k) s -= L[i * D + k] * v[k];
                    v[i] = s / L[i * D + i];
                }
                for (int i = D - 1; i >= 0; --i) {
                    double s = v[i];
                    for (int k = i + 1; k < D; ++k) s -= L[k * D + i] * v[k];
                    v[i] = s / L[i * D + i];
                }
                for (int i = 0; i < D; ++i) X[i * D + c] = v[i];
            }
            for (int i = 0; i < D; ++i)
                for (int k = 0; k <= i; ++k) {
                    double s = 0.0;
                    for (int m = 0; m < D; ++m) s += D12[m * D + i] * X[m * D + k];
                    Jn[i * D + k] = Jn[k * D + i] = D22[i * D + k] - s;
                }
            if (chol_host(Jn, D, L)) inv_from_chol(L, D, Bn);
            else failed = 1 + j;
        }
        double tr = 0.0;
        for (int i = 0; i < D; ++i) tr += Bn[i * D + i];
        for (int i = 0; i < DD; ++i) {
            if (info) info[(size_t)j * DD + i] = failed ? nan : Jn[i];
            if (bound) bound[(size_t)j * DD + i] = failed ? nan : Bn[i];
        }
        if (rmse_bound) rmse_bound[j] = failed ? nan : sqrt(tr);
        if (!failed)
            for (int i = 0; i < DD; ++i) Jp[i] = Jn[i];
    }
    *status = failed;
    return SSMQ_OK;
}
