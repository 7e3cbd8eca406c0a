// C ABI of libssmq (include/ssmq.h), the interacting multiple-model filter over noise modes: the refusals - those of the noise sweep
// (ssmq_api_noise_sweep.hip), plus the mode count, the transition matrix and the initial mode probabilities -, the mode rows (G Q G', R,
// m0 | P0 per mode or shared) and the one launch of k_imm_loop<> (ssmq_imm.hip) on the constant blocks of the two transform handles.
#include <cmath>
#include <string>
#include <vector>
#include "ssmq_imm_kernel.h"
#include "ssmq_host.h"

namespace ssmq {

const char *find_imm_kernel(const FilterShape &shape);
int launch_imm(const FilterShape &shape, const ImmArgs &a, hipStream_t s);
// ssmq_api_noise_sweep.hip: the range check and the row check of the noise sweep
int noise_sweep_route(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                      int recursion, FilterShape *shape, const char **name);
int noise_rows_ok(const char *what, const double *a, int64_t stride, int n, int P, bool optional);

static const char kImmRange[] =
    "filter_imm: the range of filter_noise_sweep - two transform handles of one form on the built-in additive-noise model pairs of the "
    "fused time loop, D <= 6, Y <= 4, Gaussian recursion - with 1 <= M <= 8 modes, a row-stochastic transition matrix and initial mode "
    "probabilities that sum to 1";

static int imm_refuse(int code, const std::string &why) {
    set_error(why + " - " + kImmRange);
    return code;
}

// A refusal of the noise sweep's checks under this entry point's name.
static int imm_renamed(int rc) {
    if (rc) {
        std::string msg = ssmq_last_error();
        const std::string from = "filter_noise_sweep", to = "filter_imm";
        for (size_t at = msg.find(from); at != std::string::npos; at = msg.find(from, at + to.size())) msg.replace(at, from.size(), to);
        set_error(msg);
    }
    return rc;
}

static int imm_route(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs, int recursion,
                     FilterShape *shape, const char **name) {
    if (int rc = imm_renamed(noise_sweep_route(h_dyn, f_dyn, h_obs, f_obs, recursion, shape, nullptr))) return rc;
    const char *kn = find_imm_kernel(*shape);
    if (!kn) return imm_refuse(SSMQ_E_UNSUPPORTED, "filter_imm: no kernel for this pair of models and point sets");
    if (name) *name = kn;
    return SSMQ_OK;
}

// One probability row: n entries, finite, non-negative, summing (ascending) to 1 within 1e-12.
static int imm_row_ok(const std::string &what, const double *row, int n) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(row[i]) || row[i] < 0.0) return imm_refuse(SSMQ_E_ARG, "filter_imm: " + what + " has an entry that is not finite or is negative");
        sum += row[i];
    }
    if (!(std::fabs(sum - 1.0) <= 1e-12)) return imm_refuse(SSMQ_E_ARG, "filter_imm: " + what + " does not sum to 1 within 1e-12");
    return SSMQ_OK;
}

}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_filter_imm_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                           const ssmq_integrand *f_obs, int recursion, char *buf, int len) {
    if (!buf || len <= 0) return imm_refuse(SSMQ_E_ARG, "filter_imm: bad argument");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    FilterShape shape;
    const char *name = nullptr;
    if (int rc = imm_route(h_dyn, f_dyn, h_obs, f_obs, recursion, &shape, &name)) return rc;
    snprintf(buf, len, "%s", name);
    return SSMQ_OK;
}

extern "C" int ssmq_filter_imm_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs, int recursion,
                                   int64_t B, int64_t ld, int T, const double *d_y, int M, const double *gqg, int64_t gqg_stride, const double *rr,
                                   int64_t rr_stride, const double *x0, int64_t x0_stride, const double *pi, const double *mu0, double *d_fm,
                                   double *d_fP, double *d_mode_prob, double *d_loglik, double *d_loglik_total, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    FilterShape shape;
    if (int rc = imm_route(h_dyn, f_dyn, h_obs, f_obs, recursion, &shape, nullptr)) return rc;
    const int D = shape.D, Y = shape.Y;
    if (M < 1 || M > kImmMaxModes) return imm_refuse(SSMQ_E_ARG, "filter_imm: bad argument (1 <= M <= 8 modes)");
    if (B < 0 || ld < B || ld % kSmallBlock != 0 || T < 0 || !d_y || !pi || !mu0 || !d_fm || !d_fP || !d_mode_prob || !d_loglik || !d_loglik_total || !d_status)
        return imm_refuse(SSMQ_E_ARG, "filter_imm: bad argument (ld a multiple of 64 and >= B)");
    if (ld / kSmallBlock >= (int64_t)1 << 31) return imm_refuse(SSMQ_E_ARG, "filter_imm: ld / 64 must stay below 2^31");
    const int nq = D * D, nr = Y * Y, nx = D + D * D;
    int rc;
    if ((rc = imm_renamed(noise_rows_ok("gqg", gqg, gqg_stride, nq, M, true))) || (rc = imm_renamed(noise_rows_ok("rr", rr, rr_stride, nr, M, true))) ||
        (rc = imm_renamed(noise_rows_ok("x0", x0, x0_stride, nx, M, false))))
        return rc;
    for (int i = 0; i < M; ++i)
        if ((rc = imm_row_ok("row " + std::to_string(i) + " of pi", pi + (size_t)i * M, M))) return rc;
    if ((rc = imm_row_ok("mu0", mu0, M))) return rc;
    if ((rc = ensure_device())) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    if (T == 0) {   // no step: an empty sum (as ssmq_filter_noise_sweep_dev)
        SSMQ_HIP(hipMemsetAsync(d_loglik_total, 0, sizeof(double) * ld, s));
        SSMQ_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t) * ld, s));
        return hip_fail(hipStreamSynchronize(s), "filter_imm");
    }
    // ---- one host image: gqg rows | rr rows | x0 rows | pi [M*M] | mu0 [M] | ttab_dyn [T] | ttab_obs [T]; a null array is one row of zeros
    const size_t rows_q = gqg && gqg_stride ? M : 1, rows_r = rr && rr_stride ? M : 1, rows_x = x0_stride ? M : 1;
    const size_t o_r = (rows_q * nq + 1) / 2 * 2, o_x = o_r + (rows_r * nr + 1) / 2 * 2, o_pi = o_x + (rows_x * nx + 1) / 2 * 2,
                 o_mu = o_pi + ((size_t)M * M + 1) / 2 * 2, o_tt = o_mu + ((size_t)M + 1) / 2 * 2;
    std::vector<double> host(o_tt + (size_t)2 * T, 0.0);
    if (gqg) std::copy(gqg, gqg + rows_q * nq, host.begin());
    if (rr) std::copy(rr, rr + rows_r * nr, host.begin() + o_r);
    std::copy(x0, x0 + rows_x * nx, host.begin() + o_x);
    std::copy(pi, pi + (size_t)M * M, host.begin() + o_pi);
    std::copy(mu0, mu0 + M, host.begin() + o_mu);
    const bool ttd = time_table(f_dyn->id, T, host.data() + o_tt), tto = time_table(f_obs->id, T, host.data() + o_tt + T);
    DeviceImage img;
    if ((rc = img.alloc(host.size()))) return rc;
    double *const dev = img.dev;
    ImmArgs a;
    memset(&a, 0, sizeof(a));
    a.y = d_y; a.c_dyn = h_dyn->d_small; a.c_obs = h_obs->d_small;
    a.gqg = dev; a.rr = dev + o_r; a.x0 = dev + o_x; a.pi = dev + o_pi; a.mu0 = dev + o_mu;
    a.gqg_stride = rows_q > 1 ? nq : 0; a.rr_stride = rows_r > 1 ? nr : 0; a.x0_stride = rows_x > 1 ? nx : 0;
    a.fm = d_fm; a.fP = d_fP; a.mode_prob = d_mode_prob; a.ll_steps = d_loglik; a.ll_total = d_loglik_total; a.status = d_status;
    a.B = B; a.ld = ld; a.T = T; a.M = M;
    a.emv_dyn = h_dyn->emv_mode; a.emv_obs = h_obs->emv_mode; a.nu_dyn = h_dyn->tp_nu; a.nu_obs = h_obs->tp_nu;
    fill_fpar(f_dyn, &a.fd);
    fill_fpar(f_obs, &a.fo);
    a.fd.ttab = ttd ? dev + o_tt : nullptr;
    a.fo.ttab = tto ? dev + o_tt + T : nullptr;
    rc = img.upload(host, "filter_imm: upload");
    if (!rc) rc = launch_imm(shape, a, s);
    const int rs = hip_fail(hipStreamSynchronize(s), "filter_imm");
    return rc ? rc : rs;
}
