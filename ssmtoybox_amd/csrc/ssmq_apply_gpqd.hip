// GPQ with derivative observations at the sigma points (SSMQ_FORM_GPQD): the handle with its expanded constant block, the
// instantiations of k_apply_gpqd / k_apply_gpqd_lds (ssmq_apply_gpqd_kernel.h, where the transform is described) for the built-in
// models that have a Jacobian and additive noise, and the launcher of both routes.  A user model's kernels are compiled for it at
// run time (ssmq_rtc.hip: rtc_launch_gpqd).
#include <cmath>
#include "ssmq_device.h"
#include "ssmq_host.h"
#include "ssmq_math.h"
#include "ssmq_apply_gpqd_kernel.h"

namespace ssmq {

int refuse_gpqd(const char *what) {
    set_error(std::string(what) + ": not implemented for the GPQ+D transform (SSMQ_FORM_GPQD runs through ssmq_apply_batch[_dev], "
              "ssmq_apply_kernel_name and the launch loop of ssmq_filter_forward_dev / ssmq_filter_smooth_dev)");
    return SSMQ_E_UNSUPPORTED;
}

bool gpqd_range_ok(int D, int E, int N) {
    return D >= 1 && D <= SSMQ_USER_MAX_D && E >= 1 && E <= std::max(D, SSMQ_USER_MAX_Y) && N >= 2 && N <= 2 * D + 1;
}

namespace {
const char kRange[] = "the GPQ+D transform supports D <= 6, 2 <= N <= 2 D + 1 points, outputs <= max(D, 4) and a strictly increasing "
                      "which_der within the points";

template <int D, int E>
void launch_reg(const GpqdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_apply_gpqd<-1, D, E, D>), dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, s, a);
}
template <int D, int E>
void launch_lds(const GpqdArgs &a, hipStream_t s) {
    constexpr int ipw = gpqd_lds_items(D, E);
    hipLaunchKernelGGL((k_apply_gpqd_lds<-1, D, E, D>), dim3((unsigned)((a.B + ipw - 1) / ipw)), dim3(kGpqdLdsBlock), 0, s, a);
}

// the handle's block in the full layout from the compact arrays: wm [M], Wc [M][M], Wcc [D][M], M = N + Nd D
int expand(ssmq_transform *h, const double *xi, int Nd, const int32_t *which_der, const double *wm, const double *Wc, const double *Wcc,
           double model_var, std::vector<double> *blk, uint32_t *mask) {
    const int D = h->D, N = h->N;
    if (Nd < 0 || Nd > N || (Nd > 0 && !which_der) || !wm || !Wc || !Wcc) {
        set_error(std::string("GPQ+D: bad argument; ") + kRange);
        return SSMQ_E_ARG;
    }
    *mask = 0;
    for (int j = 0; j < Nd; ++j) {
        if (which_der[j] < 0 || which_der[j] >= N || (j > 0 && which_der[j] <= which_der[j - 1])) {
            set_error(std::string("GPQ+D: which_der out of range; ") + kRange);
            return SSMQ_E_ARG;
        }
        *mask |= 1u << which_der[j];
    }
    const GpqdLayout cl = gpqd_layout(D);
    const int M = N + Nd * D;
    std::vector<int> slot(M);
    for (int n = 0; n < N; ++n) slot[n] = n;
    for (int j = 0; j < Nd; ++j)
        for (int k = 0; k < D; ++k) slot[N + j * D + k] = cl.nmax + which_der[j] * D + k;
    blk->assign((size_t)cl.total, 0.0);
    double *p = blk->data();
    if (xi)
        for (int n = 0; n < N; ++n)
            for (int d = 0; d < D; ++d) p[cl.xi + n * D + d] = xi[d * N + n];
    for (int i = 0; i < M; ++i) {
        p[cl.wm + slot[i]] = wm[i];
        for (int d = 0; d < D; ++d) p[cl.Wcc + d * cl.mx + slot[i]] = Wcc[d * M + i];
        for (int j = 0; j < M; ++j) p[cl.Wc + slot[i] * cl.mx + slot[j]] = Wc[(size_t)i * M + j];
    }
    p[cl.emv] = model_var;
    for (double v : *blk)
        if (!std::isfinite(v)) {
            set_error("GPQ+D: points, weights and the model variance must be finite");
            return SSMQ_E_ARG;
        }
    return SSMQ_OK;
}

int upload(ssmq_transform *h, const std::vector<double> &blk, uint32_t mask) {
    // `generation` carries a hash of the constants: part of the launch loop's graph key (key_of_pair, ssmq_host.h)
    std::vector<uint64_t> words;
    key_bytes(words, blk.data(), sizeof(double) * blk.size());
    uint64_t hash = 1469598103934665603ull ^ (uint64_t)mask ^ ((uint64_t)h->N << 32);
    for (uint64_t w : words) hash = (hash ^ w) * 1099511628211ull;
    h->generation = (uint32_t)(hash ^ (hash >> 32));
    h->gq_mask = mask;
    SSMQ_HIP(hipMemcpyAsync(h->d_gpqd, blk.data(), sizeof(double) * blk.size(), hipMemcpyHostToDevice, stream()));
    SSMQ_HIP(hipStreamSynchronize(stream()));
    return SSMQ_OK;
}
}  // namespace

int launch_apply_gpqd(const ssmq_transform *h, int din, const ssmq_integrand *f, const LinArgs &planes, hipStream_t s, const char **name,
                      bool dry_run) {
    if (!is_gpqd(h) || !h->d_gpqd || !gpqd_range_ok(h->D, h->E, h->N)) {
        set_error("apply (GPQ+D): not a GPQ+D handle");
        return SSMQ_E_ARG;
    }
    const int D = h->D, E = h->E;
    GpqdArgs a;
    static_cast<LinArgs &>(a) = planes;
    a.D = D; a.E = E; a.din = din; a.fid = f->id; a.bcast = (f->n_idx == 0 && din == 1 && D > 1) ? 1 : 0;
    a.consts = h->d_gpqd; a.N = h->N; a.der_mask = h->gq_mask;
    const bool lds = D > kGpqdRegMaxD;
    if (is_user_integrand(f)) return rtc_launch_gpqd(f, a, lds, s, name, dry_run);      // (makes the checks of that route)
    if (name) *name = lds ? "k_apply_gpqd_lds" : "k_apply_gpqd";
    if (!integrand_has_jacobian(f->id) || f->id == SSMQ_F_UNGMNA_DYN || f->id == SSMQ_F_UNGMNA_MEAS) {
        set_error("GPQ+D: built-in models with a Jacobian and additive noise only (UNGM, pendulum, constant velocity, coordinated turn, "
                  "radar, bearings)");
        return SSMQ_E_UNSUPPORTED;
    }
    // (a Jacobian of 1 < din < D columns without a state index lands in the leading din columns, as jac_front_builtin places it)
    if (!jacobian_fits(f->id, D, E)) {
        set_error("GPQ+D: this model's Jacobian does not fit the shape (D, E) = (" + std::to_string(D) + ", " + std::to_string(E) + ")");
        return SSMQ_E_UNSUPPORTED;
    }
    const bool have = (D == 1 && E == 1) || (D == 2 && (E == 1 || E == 2)) || (D == 4 && (E == 2 || E == 4)) ||
                      (D == 5 && (E == 2 || E == 4 || E == 5));
    if (!have) {
        set_error("GPQ+D: no kernel for a built-in model of this shape (D, E) = (" + std::to_string(D) + ", " + std::to_string(E) + ")");
        return SSMQ_E_UNSUPPORTED;
    }
    if (dry_run) return SSMQ_OK;
    if (D == 1) launch_reg<1, 1>(a, s);
    else if (D == 2 && E == 1) launch_reg<2, 1>(a, s);
    else if (D == 2) launch_reg<2, 2>(a, s);
    else if (D == 4 && E == 2) launch_lds<4, 2>(a, s);
    else if (D == 4) launch_lds<4, 4>(a, s);
    else if (E == 2) launch_lds<5, 2>(a, s);
    else if (E == 4) launch_lds<5, 4>(a, s);
    else launch_lds<5, 5>(a, s);
    return hip_fail(hipGetLastError(), lds ? "k_apply_gpqd_lds" : "k_apply_gpqd");
}

}  // namespace ssmq

using namespace ssmq;

extern "C" ssmq_transform *ssmq_transform_create_gpqd(int D, int E, int N, const double *xi, int Nd, const int32_t *which_der,
                                                      const double *wm, const double *Wc, const double *Wcc, double model_var) {
    if (!gpqd_range_ok(D, E, N) || !xi) {
        set_error(std::string("transform_create_gpqd: ") + kRange);
        return nullptr;
    }
    if (ensure_device()) return nullptr;
    ssmq_transform *h = new ssmq_transform();
    h->D = D; h->E = E; h->N = N; h->form = SSMQ_FORM_GPQD; h->emv_mode = SSMQ_EMV_DIAG; h->tp_nu = 0.0;
    h->opt_mask = 0;
    hipGetDevice(&h->device);
    h->d_small = h->d_wide = nullptr;
    h->xi.assign(xi, xi + D * N);
    std::vector<double> blk;
    uint32_t mask = 0;
    if (expand(h, xi, Nd, which_der, wm, Wc, Wcc, model_var, &blk, &mask) != SSMQ_OK ||
        hipMalloc((void **)&h->d_gpqd, sizeof(double) * blk.size()) != hipSuccess || upload(h, blk, mask) != SSMQ_OK) {
        if (!*ssmq_last_error()) set_error("transform_create_gpqd: device allocation or upload failed");
        ssmq_transform_destroy(h);
        return nullptr;
    }
    return h;
}

extern "C" int ssmq_transform_gpqd_set(ssmq_transform *h, int Nd, const int32_t *which_der, const double *wm, const double *Wc,
                                       const double *Wcc, double model_var) {
    SSMQ_HANDLE_LOCK(h);
    if (!is_gpqd(h)) {
        set_error("transform_gpqd_set: not a GPQ+D handle");
        return SSMQ_E_ARG;
    }
    std::vector<double> blk;
    uint32_t mask = 0;
    int rc = expand(h, h->xi.data(), Nd, which_der, wm, Wc, Wcc, model_var, &blk, &mask);
    if (rc) return rc;
    // on the library's stream: an application queued there may still be reading the old block
    return upload(h, blk, mask);
}
