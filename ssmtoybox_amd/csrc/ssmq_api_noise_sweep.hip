// C ABI of libssmq (include/ssmq.h), the noise sweep of a Gaussian filter by measurement likelihood: the refusals, the row arrays
// (G Q G', R, m0 | P0 per row or shared) and the one launch of k_noise_sweep<> (ssmq_noise_sweep.hip) on the constant blocks of the
// two transform handles.
#include <cmath>
#include <string>
#include <vector>
#include "ssmq_noise_sweep_kernel.h"
#include "ssmq_host.h"

namespace ssmq {

const char *find_noise_sweep_kernel(const FilterShape &shape);
int launch_noise_sweep(const FilterShape &shape, const NoiseSweepArgs &a, hipStream_t s);

static const char kNoiseSweepRange[] =
    "filter_noise_sweep: two transform handles of one form - both sigma-point rules, both GP / Bayes-Sard (BQ) or both t-process BQ "
    "transforms - on the built-in additive-noise model pairs of the fused time loop, D <= 6, Y <= 4, the point counts the fused time "
    "loop is instantiated for (the same count for both transforms), Gaussian recursion";

static int noise_refuse(int code, const std::string &why) {
    set_error(why + " - " + kNoiseSweepRange);
    return code;
}

// What both entry points check, in this order, before anything else happens; *shape: the key of the kernel's table.  (Also the
// route of the IMM filter over noise modes, ssmq_api_imm.hip: the same range.)
int noise_sweep_route(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                             int recursion, FilterShape *shape, const char **name) {
    if (!h_dyn || !h_obs || !f_dyn || !f_obs) return noise_refuse(SSMQ_E_ARG, "filter_noise_sweep: bad argument");
    if (recursion != SSMQ_RECURSION_GAUSS && recursion != SSMQ_RECURSION_STUDENT) return noise_refuse(SSMQ_E_ARG, "filter_noise_sweep: bad recursion");
    const int D = h_dyn->D, Y = h_obs->E;
    auto handles = [&]() {
        if (recursion == SSMQ_RECURSION_STUDENT) return noise_refuse(SSMQ_E_UNSUPPORTED, "filter_noise_sweep: the Studentian recursion is not implemented");
        for (const ssmq_transform *h : {h_dyn, h_obs}) {
            if (is_mo(h)) return noise_refuse(SSMQ_E_UNSUPPORTED, "filter_noise_sweep: multi-output transforms are not implemented");
            if (is_trunc(h)) return noise_refuse(SSMQ_E_UNSUPPORTED, "filter_noise_sweep: truncated sigma-point transforms are not implemented");
            if (is_gpqd(h)) return noise_refuse(SSMQ_E_UNSUPPORTED, "filter_noise_sweep: GPQ+D transforms are not implemented");
            if (is_taylor_gpqd(h) || h->form == SSMQ_FORM_TAYLOR1)
                return noise_refuse(SSMQ_E_UNSUPPORTED, "filter_noise_sweep: linearisation and Taylor-GPQD transforms are not implemented");
        }
        if (h_dyn->form != h_obs->form || (h_dyn->tp_nu > 0.0) != (h_obs->tp_nu > 0.0) || (h_dyn->form != SSMQ_FORM_BQ && h_dyn->form != SSMQ_FORM_SIGMA))
            return noise_refuse(SSMQ_E_UNSUPPORTED, "filter_noise_sweep: the two transforms are of different forms");
        if (h_dyn->E != D || h_obs->D != D) return noise_refuse(SSMQ_E_ARG, "filter_noise_sweep: needs dyn (D -> D) and obs (D -> Y) transforms");
        return (int)SSMQ_OK;
    };
    int selo = 0;
    if (int rc = additive_pair_route(noise_refuse, "filter_noise_sweep", f_dyn, f_obs, D, handles, &selo)) return rc;
    if (D > 6 || Y > 4) return noise_refuse(SSMQ_E_UNSUPPORTED, "filter_noise_sweep: dimension out of range");
    *shape = {f_dyn->id, f_obs->id, D, Y, h_dyn->N, h_obs->N, h_dyn->form, h_dyn->tp_nu > 0.0 ? 1 : 0, selo, 0};
    const char *kn = selo < 0 || !h_dyn->d_small || !h_obs->d_small ? nullptr : find_noise_sweep_kernel(*shape);
    if (!kn) return noise_refuse(SSMQ_E_UNSUPPORTED, "filter_noise_sweep: no kernel for this pair of models and point sets");
    if (name) *name = kn;
    return SSMQ_OK;
}

// One row array: `rows` rows of n doubles (stride 0: one row; else stride == n and P rows), every entry finite.  Null is allowed
// where `optional` (zeros).  (Also the mode rows of ssmq_api_imm.hip.)
int noise_rows_ok(const char *what, const double *a, int64_t stride, int n, int P, bool optional) {
    if (!a) return optional ? SSMQ_OK : noise_refuse(SSMQ_E_ARG, std::string("filter_noise_sweep: ") + what + " is null");
    if (stride != 0 && stride != n)
        return noise_refuse(SSMQ_E_ARG, std::string("filter_noise_sweep: the row stride of ") + what + " is 0 (shared) or the row size " + std::to_string(n));
    const int rows = stride ? P : 1;
    for (int p = 0; p < rows; ++p)
        for (int i = 0; i < n; ++i)
            if (!std::isfinite(a[(size_t)p * n + i]))
                return noise_refuse(SSMQ_E_ARG, std::string("filter_noise_sweep: row ") + std::to_string(p) + " of " + what + " is not finite");
    return SSMQ_OK;
}

}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_filter_noise_sweep_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                                   const ssmq_integrand *f_obs, int recursion, char *buf, int len) {
    if (!buf || len <= 0) return noise_refuse(SSMQ_E_ARG, "filter_noise_sweep: bad argument");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    FilterShape shape;
    const char *name = nullptr;
    if (int rc = noise_sweep_route(h_dyn, f_dyn, h_obs, f_obs, recursion, &shape, &name)) return rc;
    snprintf(buf, len, "%s", name);
    return SSMQ_OK;
}

extern "C" int ssmq_filter_noise_sweep_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                                           int recursion, int64_t B, int64_t ld, int T, const double *d_y, int P, const double *gqg,
                                           int64_t gqg_stride, const double *rr, int64_t rr_stride, const double *x0, int64_t x0_stride,
                                           double *d_loglik_total, double *d_nis_mean, double *d_loglik, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    FilterShape shape;
    if (int rc = noise_sweep_route(h_dyn, f_dyn, h_obs, f_obs, recursion, &shape, nullptr)) return rc;
    const int D = shape.D, Y = shape.Y;
    if (P < 1 || B < 0 || ld < B || ld % kSmallBlock != 0 || T < 0 || !d_y || !d_loglik_total || !d_nis_mean || !d_status)
        return noise_refuse(SSMQ_E_ARG, "filter_noise_sweep: bad argument (P >= 1, ld a multiple of 64 and >= B)");
    if ((int64_t)P * (ld / kSmallBlock) >= (int64_t)1 << 31) return noise_refuse(SSMQ_E_ARG, "filter_noise_sweep: P * ld / 64 must stay below 2^31");
    const int nq = D * D, nr = Y * Y, nx = D + D * D;
    int rc;
    if ((rc = noise_rows_ok("gqg", gqg, gqg_stride, nq, P, true)) || (rc = noise_rows_ok("rr", rr, rr_stride, nr, P, true)) ||
        (rc = noise_rows_ok("x0", x0, x0_stride, nx, P, false)))
        return rc;
    if ((rc = ensure_device())) return rc;
    if (B == 0) return SSMQ_OK;
    if (T == 0) return score_empty("filter_noise_sweep", P, ld, nullptr, d_loglik_total, d_nis_mean, d_status);
    // ---- one host image: gqg rows | rr rows | x0 rows | ttab_dyn [T] | ttab_obs [T]; a null array is one row of zeros -----------
    const size_t rows_q = gqg && gqg_stride ? P : 1, rows_r = rr && rr_stride ? P : 1, rows_x = x0_stride ? P : 1;
    const size_t o_r = (rows_q * nq + 1) / 2 * 2, o_x = o_r + (rows_r * nr + 1) / 2 * 2, o_tt = o_x + (rows_x * nx + 1) / 2 * 2;
    std::vector<double> host(o_tt + (size_t)2 * T, 0.0);
    if (gqg) std::copy(gqg, gqg + rows_q * nq, host.begin());
    if (rr) std::copy(rr, rr + rows_r * nr, host.begin() + o_r);
    std::copy(x0, x0 + rows_x * nx, host.begin() + o_x);
    const bool ttd = time_table(f_dyn->id, T, host.data() + o_tt), tto = time_table(f_obs->id, T, host.data() + o_tt + T);
    DeviceImage img;
    if ((rc = img.alloc(host.size()))) return rc;
    double *const dev = img.dev;
    hipStream_t s = stream();
    NoiseSweepArgs a;
    memset(&a, 0, sizeof(a));
    a.y = d_y; a.c_dyn = h_dyn->d_small; a.c_obs = h_obs->d_small;
    a.gqg = dev; a.rr = dev + o_r; a.x0 = dev + o_x;
    a.gqg_stride = rows_q > 1 ? nq : 0; a.rr_stride = rows_r > 1 ? nr : 0; a.x0_stride = rows_x > 1 ? nx : 0;
    a.ll_total = d_loglik_total; a.nis_mean = d_nis_mean; a.ll_steps = d_loglik; a.status = d_status;
    a.B = B; a.ld = ld; a.T = T; a.P = P; a.nblk = (int32_t)(ld / kSmallBlock);
    a.emv_dyn = h_dyn->emv_mode; a.emv_obs = h_obs->emv_mode; a.nu_dyn = h_dyn->tp_nu; a.nu_obs = h_obs->tp_nu;
    fill_fpar(f_dyn, &a.fd);
    fill_fpar(f_obs, &a.fo);
    a.fd.ttab = ttd ? dev + o_tt : nullptr;
    a.fo.ttab = tto ? dev + o_tt + T : nullptr;
    rc = img.upload(host, "filter_noise_sweep: upload");
    if (!rc) rc = launch_noise_sweep(shape, a, s);
    const int rs = hip_fail(hipStreamSynchronize(s), "filter_noise_sweep");
    return rc ? rc : rs;
}
