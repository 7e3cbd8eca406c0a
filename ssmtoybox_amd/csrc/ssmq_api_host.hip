// C ABI of libssmq (include/ssmq.h), the entry points that take HOST arrays: the pinned staging arena of the calling thread's
// context, the plane upload / download, and the transform with its split variants (sigma points out, integrand values in).
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>
#include "ssmq_host.h"

using namespace ssmq;

namespace ssmq {
StagingArena &stage_of_ctx() {
    Ctx &c = ssmq::ctx();
    if (!c.stage) c.stage = new StagingArena;
    return *(StagingArena *)c.stage;
}
}  // namespace ssmq
namespace {
#define g_stage (stage_of_ctx())

// memcpy between caller memory and the pinned blocks; large blocks on several threads (one core moves ~8 GB/s, which
// would cost more than the PCIe transfer it feeds)
void fast_copy(void *dst, const void *src, size_t bytes) {
    constexpr size_t kChunk = size_t(2) << 20;
    if (bytes < 2 * kChunk) {
        memcpy(dst, src, bytes);
        return;
    }
    const size_t nt = std::min<size_t>(8, bytes / kChunk);
    const size_t per = (bytes / nt + 63) / 64 * 64;
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; ++t) {
        const size_t lo = t * per, n = lo < bytes ? std::min(per, bytes - lo) : 0;
        if (n) th.emplace_back([=] { memcpy((char *)dst + lo, (const char *)src + lo, n); });
    }
    memcpy(dst, src, std::min(per, bytes));
    for (auto &t : th) t.join();
}
}  // namespace
namespace ssmq {
void drop_staging_arena() { g_stage.drop(); }
}

// ---- host arrays in the reference's study layout <-> time-major planes in HBM, through the pinned staging blocks --------
// The filters' device buffers are [n_outer][n_elem][ld] (time step, element, trajectory); the reference's arrays are
// (n_elem..., n_outer, B): dim_y x T x B measurements in, D x T x B means and D x D x T x B covariances out
// (ssinf.py:66-118).  Rows of B doubles are contiguous on both sides, so the permutation is a row copy: done on the host
// between the caller's array and the pinned block (several threads), one contiguous transfer per chunk.
namespace {
void copy_rows(bool to_planes, double *host, double *pinned, int64_t t0, int64_t t1, int n_outer, int n_elem, int64_t B,
               int64_t ld) {
    // planes row (t - t0, e) of the chunk <-> host row (e, t)
    const int64_t rows = (t1 - t0) * n_elem;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(8, (rows * B) / (256 * 1024)));
    auto work = [=](int64_t r0, int64_t r1) {
        for (int64_t r = r0; r < r1; ++r) {
            const int64_t t = t0 + r / n_elem, e = r % n_elem;
            double *pl = pinned + r * ld, *hs = host + (e * n_outer + t) * B;
            if (to_planes) {
                memcpy(pl, hs, sizeof(double) * B);
                if (ld > B) memset(pl + B, 0, sizeof(double) * (ld - B));
            } else {
                memcpy(hs, pl, sizeof(double) * B);
            }
        }
    };
    std::vector<std::thread> th;
    const int64_t per = (rows + nt - 1) / nt;
    for (int k = 1; k < nt; ++k)
        if (k * per < rows) th.emplace_back(work, k * per, std::min(rows, (k + 1) * per));
    work(0, std::min(rows, per));
    for (auto &t : th) t.join();
}
constexpr size_t kPlaneChunkBytes = size_t(128) << 20;
}  // namespace

extern "C" {

int ssmq_upload_planes(const double *host, int n_outer, int n_elem, int64_t B, int64_t ld, double *d_planes) {
    if (!host || !d_planes || n_outer < 0 || n_elem < 1 || B < 0 || ld < B) {
        set_error("upload_planes: bad argument");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (n_outer == 0 || B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    const size_t step_bytes = sizeof(double) * (size_t)n_elem * ld;
    const int64_t tc = std::max<int64_t>(1, std::min<int64_t>(n_outer, (int64_t)(kPlaneChunkBytes / step_bytes)));
    if ((rc = g_stage.reserve(0, step_bytes * tc, 0))) return rc;
    for (int64_t t0 = 0; t0 < n_outer; t0 += tc) {
        const int64_t t1 = std::min<int64_t>(n_outer, t0 + tc);
        copy_rows(true, const_cast<double *>(host), (double *)g_stage.hin, t0, t1, n_outer, n_elem, B, ld);
        SSMQ_HIP(hipMemcpyAsync(d_planes + (size_t)t0 * n_elem * ld, g_stage.hin, step_bytes * (t1 - t0), hipMemcpyHostToDevice, s));
        SSMQ_HIP(hipStreamSynchronize(s));       // the pinned block is refilled for the next chunk
    }
    return SSMQ_OK;
}

int ssmq_download_planes(const double *d_planes, int n_outer, int n_elem, int64_t B, int64_t ld, double *host) {
    if (!host || !d_planes || n_outer < 0 || n_elem < 1 || B < 0 || ld < B) {
        set_error("download_planes: bad argument");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (n_outer == 0 || B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    const size_t step_bytes = sizeof(double) * (size_t)n_elem * ld;
    const int64_t tc = std::max<int64_t>(1, std::min<int64_t>(n_outer, (int64_t)(kPlaneChunkBytes / step_bytes)));
    if ((rc = g_stage.reserve(0, 0, step_bytes * tc))) return rc;
    for (int64_t t0 = 0; t0 < n_outer; t0 += tc) {
        const int64_t t1 = std::min<int64_t>(n_outer, t0 + tc);
        SSMQ_HIP(hipMemcpyAsync(g_stage.hout, d_planes + (size_t)t0 * n_elem * ld, step_bytes * (t1 - t0), hipMemcpyDeviceToHost, s));
        SSMQ_HIP(hipStreamSynchronize(s));
        copy_rows(false, host, (double *)g_stage.hout, t0, t1, n_outer, n_elem, B, ld);
    }
    return SSMQ_OK;
}

int ssmq_apply_batch(ssmq_transform *h, const ssmq_integrand *f, int64_t B, const double *mean, const double *cov,
                     const double *time, int time_stride, double *mean_f, double *cov_f, double *cov_fx,
                     int32_t *status) {
    SSMQ_HANDLE_LOCK(h);
    if (!h || !f || B < 0 || !mean || !cov || !mean_f || !cov_f || !cov_fx) {
        set_error("apply_batch: null argument");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    const int D = h->D, E = h->E;
    const int64_t ld = (B + 63) / 64 * 64;
    const size_t n_in = (size_t)D + (size_t)D * D, n_out = (size_t)E + (size_t)E * E + (size_t)E * D;
    const size_t n_time = time && time_stride ? (size_t)B : 1;
    // Small batches - the drop-in apply() is B = 1 - convert the layout on the host and move one pinned block each way:
    // one upload, one kernel, one download (the reference needs 60-120 us per apply(); six allocations, five layout
    // kernels and seven copies per call took longer than that).  Large batches transpose on the device.
    const bool host_layout = (size_t)B * (n_in + n_out) <= 65536;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    // device: [planes in | time] [planes out | status] and, for the device-side conversion, [AoS in | time] [AoS out | status]
    const size_t pin_bytes = sizeof(double) * (n_in * ld + n_time), pout_bytes = sizeof(double) * n_out * ld + sizeof(int32_t) * ld;
    const size_t ain_bytes = sizeof(double) * ((size_t)B * n_in + n_time), aout_bytes = sizeof(double) * B * n_out + sizeof(int32_t) * ld;
    const size_t off_in = 0, off_out = al(pin_bytes), off_ai = off_out + al(pout_bytes),
                 off_ao = off_ai + (host_layout ? 0 : al(ain_bytes)), total = off_ao + (host_layout ? 0 : al(aout_bytes));
    // every transfer goes through the pinned blocks: copies from / to pageable caller memory stalled for 20-30 ms at some
    // sizes (the runtime pins fresh pages on the fly)
    if ((rc = g_stage.reserve(total, host_layout ? pin_bytes : ain_bytes, host_layout ? pout_bytes : aout_bytes))) return rc;
    hipStream_t s = stream();
    char *dev = (char *)g_stage.dev;
    double *soa_in = (double *)(dev + off_in), *d_time = soa_in + n_in * ld;
    double *o_mf = (double *)(dev + off_out), *o_cf = o_mf + ld * E, *o_cfx = o_cf + ld * E * E;
    int32_t *d_st = (int32_t *)(o_cfx + ld * E * D);
    const double tzero = 0.0;
    double *hin = (double *)g_stage.hin;
    if (host_layout) {
        for (int e = 0; e < D; ++e) {
            double *pl = hin + (size_t)e * ld;
            for (int64_t i = 0; i < B; ++i) pl[i] = mean[(size_t)i * D + e];
            for (int64_t i = B; i < ld; ++i) pl[i] = 0.0;
        }
        for (int e = 0; e < D * D; ++e) {
            double *pl = hin + (size_t)(D + e) * ld;
            for (int64_t i = 0; i < B; ++i) pl[i] = cov[(size_t)i * D * D + e];
            for (int64_t i = B; i < ld; ++i) pl[i] = 0.0;
        }
        memcpy(hin + n_in * ld, time ? time : &tzero, sizeof(double) * n_time);
        SSMQ_HIP(hipMemcpyAsync(soa_in, hin, pin_bytes, hipMemcpyHostToDevice, s));
    } else {
        double *aos_in = (double *)(dev + off_ai);
        fast_copy(hin, mean, sizeof(double) * B * D);
        fast_copy(hin + (size_t)B * D, cov, sizeof(double) * B * D * D);
        memcpy(hin + (size_t)B * n_in, time ? time : &tzero, sizeof(double) * n_time);
        SSMQ_HIP(hipMemcpyAsync(aos_in, hin, ain_bytes, hipMemcpyHostToDevice, s));
        SSMQ_HIP(hipMemcpyAsync(d_time, aos_in + (size_t)B * n_in, sizeof(double) * n_time, hipMemcpyDeviceToDevice, s));
        if ((rc = ssmq_aos_to_soa(aos_in, soa_in, D, B, ld))) return rc;
        if ((rc = ssmq_aos_to_soa(aos_in + B * D, soa_in + ld * D, D * D, B, ld))) return rc;
    }
    rc = apply_dev_impl(h, f, B, ld, soa_in, soa_in + ld * D, d_time, time && time_stride ? 1 : 0, o_mf, o_cf, o_cfx, d_st,
                        nullptr, nullptr, false);
    if (rc) return rc;
    const int32_t *hst;
    const double *ho = (const double *)g_stage.hout;
    if (host_layout) {
        SSMQ_HIP(hipMemcpyAsync(g_stage.hout, o_mf, pout_bytes, hipMemcpyDeviceToHost, s));
        SSMQ_HIP(hipStreamSynchronize(s));
        for (int e = 0; e < E; ++e)
            for (int64_t i = 0; i < B; ++i) mean_f[(size_t)i * E + e] = ho[(size_t)e * ld + i];
        const double *hc = ho + (size_t)E * ld;
        for (int e = 0; e < E * E; ++e)
            for (int64_t i = 0; i < B; ++i) cov_f[(size_t)i * E * E + e] = hc[(size_t)e * ld + i];
        const double *hx = hc + (size_t)E * E * ld;
        for (int e = 0; e < E * D; ++e)
            for (int64_t i = 0; i < B; ++i) cov_fx[(size_t)i * E * D + e] = hx[(size_t)e * ld + i];
        hst = (const int32_t *)(hx + (size_t)E * D * ld);
    } else {
        double *a_mf = (double *)(dev + off_ao), *a_cf = a_mf + B * E, *a_cfx = a_cf + B * E * E;
        if ((rc = ssmq_soa_to_aos(o_mf, a_mf, E, B, ld))) return rc;
        if ((rc = ssmq_soa_to_aos(o_cf, a_cf, E * E, B, ld))) return rc;
        if ((rc = ssmq_soa_to_aos(o_cfx, a_cfx, E * D, B, ld))) return rc;
        SSMQ_HIP(hipMemcpyAsync(a_mf + (size_t)B * n_out, d_st, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, s));
        SSMQ_HIP(hipMemcpyAsync(g_stage.hout, a_mf, aout_bytes, hipMemcpyDeviceToHost, s));
        SSMQ_HIP(hipStreamSynchronize(s));
        fast_copy(mean_f, ho, sizeof(double) * B * E);
        fast_copy(cov_f, ho + (size_t)B * E, sizeof(double) * B * E * E);
        fast_copy(cov_fx, ho + (size_t)B * (E + E * E), sizeof(double) * B * E * D);
        hst = (const int32_t *)(ho + (size_t)B * n_out);
    }
    int first = 0;
    for (int64_t i = 0; i < B; ++i) {
        if (status) status[i] = hst[i];
        if (hst[i] && !first) first = (int)std::min<int64_t>(i + 1, 0x7fffffff);
    }
    return first;
}

int ssmq_sigma_points_batch(ssmq_transform *h, int64_t B, const double *mean, const double *cov, double *x,
                            double *chol, int32_t *status) {
    SSMQ_HANDLE_LOCK(h);
    if (h && h->form == SSMQ_FORM_TAYLOR1) {
        set_error("the linearisation transform has no sigma points");
        return SSMQ_E_UNSUPPORTED;
    }
    if (is_taylor_gpqd(h)) return refuse_taylor_gpqd("ssmq_sigma_points_batch");
    if (is_trunc(h)) return refuse_trunc("ssmq_sigma_points_batch");
    if (is_gpqd(h)) return refuse_gpqd("ssmq_sigma_points_batch");
    if (!h || B < 0 || !mean || !cov || !x || !chol) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    const int D = h->D, N = h->N;
    if (!is_mo(h) && wide_lds_bytes(D, h->E, N) > 160 * 1024 - 64) return SSMQ_E_UNSUPPORTED;
    // staging arena: [mean | cov] up, [x | chol | status] down, one transfer each way through the pinned blocks
    const size_t nb = (size_t)B, n_in = nb * ((size_t)D + (size_t)D * D), n_x = nb * D * N, n_l = nb * D * D;
    const size_t in_bytes = sizeof(double) * n_in, out_bytes = sizeof(double) * (n_x + n_l) + sizeof(int32_t) * nb;
    const size_t off_out = (in_bytes + 255) / 256 * 256;
    if ((rc = g_stage.reserve(off_out + out_bytes, in_bytes, out_bytes))) return rc;
    hipStream_t s = stream();
    double *dm = (double *)g_stage.dev, *dc = dm + nb * D;
    double *dx = (double *)((char *)g_stage.dev + off_out), *dl = dx + n_x;
    int32_t *ds = (int32_t *)(dl + n_l);
    double *hin = (double *)g_stage.hin;
    fast_copy(hin, mean, sizeof(double) * nb * D);
    fast_copy(hin + nb * D, cov, sizeof(double) * n_l);
    SSMQ_HIP(hipMemcpyAsync(dm, hin, in_bytes, hipMemcpyHostToDevice, s));
    if (is_mo(h)) {
        MoArgs m;
        memset(&m, 0, sizeof(m));
        m.D = D; m.E = h->E; m.N = N; m.mode = SSMQ_MO_POINTS; m.consts = h->d_mo; m.cov_scale = m.ccov_scale = 1.0;
        m.mean = dm; m.cov = dc; m.es_in = 1; m.bs_mean = D; m.bs_cov = D * D; m.status = ds; m.x_out = dx; m.chol_out = dl;
        if ((rc = launch_apply_mo(m, B, s))) return rc;
    } else {
        WideArgs a;
        memset(&a, 0, sizeof(a));
        a.D = D; a.E = h->E; a.N = N; a.form = h->form; a.mode = SSMQ_WIDE_POINTS; a.consts = h->d_wide;
        a.cov_scale = a.ccov_scale = 1.0;
        a.mean = dm; a.cov = dc; a.es_in = 1; a.bs_mean = D; a.bs_cov = D * D; a.status = ds;
        a.x_out = dx; a.chol_out = dl;
        if ((rc = hip_fail(launch_apply_wide(a, B, s), "k_apply_wide(points)"))) return rc;
    }
    SSMQ_HIP(hipMemcpyAsync(g_stage.hout, dx, out_bytes, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    const double *ho = (const double *)g_stage.hout;
    fast_copy(x, ho, sizeof(double) * n_x);
    fast_copy(chol, ho + n_x, sizeof(double) * n_l);
    const int32_t *st = (const int32_t *)(ho + n_x + n_l);
    int first = 0;
    for (int64_t i = 0; i < B; ++i) {
        if (status) status[i] = st[i];
        if (st[i] && !first) first = (int)std::min<int64_t>(i + 1, 0x7fffffff);
    }
    return first;
}

int ssmq_apply_fx_batch(ssmq_transform *h, int64_t B, const double *chol, const double *mean, const double *x,
                        const double *fx, double *mean_f, double *cov_f, double *cov_fx) {
    SSMQ_HANDLE_LOCK(h);
    if (h && h->form == SSMQ_FORM_TAYLOR1) {
        set_error("the linearisation transform has no sigma points");
        return SSMQ_E_UNSUPPORTED;
    }
    if (is_taylor_gpqd(h)) return refuse_taylor_gpqd("ssmq_apply_fx_batch");
    if (is_trunc(h)) return refuse_trunc("ssmq_apply_fx_batch");
    if (is_gpqd(h)) return refuse_gpqd("ssmq_apply_fx_batch");
    if (!h || B < 0 || !chol || !fx || !mean_f || !cov_f || !cov_fx) return SSMQ_E_ARG;
    if (h->form == SSMQ_FORM_SIGMA && (!mean || !x)) {
        set_error("apply_fx_batch: the centred form needs mean and x");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    const int D = h->D, E = h->E, N = h->N;
    if (is_mo(h)) {
        // the multi-output form: [chol | fx] up, the reductions of k_apply_mo, [mean_f | cov_f | cov_fx] down
        const size_t nb = (size_t)B, n_l = nb * D * D, n_fx = nb * E * N, n_out = nb * ((size_t)E + (size_t)E * E + (size_t)E * D);
        const size_t in_bytes = sizeof(double) * (n_l + n_fx), out_bytes = sizeof(double) * n_out, off_out = (in_bytes + 255) / 256 * 256;
        if ((rc = g_stage.reserve(off_out + out_bytes, in_bytes, out_bytes))) return rc;
        hipStream_t s = stream();
        double *dl = (double *)g_stage.dev, *dfx = dl + n_l, *omf = (double *)((char *)g_stage.dev + off_out);
        double *hin = (double *)g_stage.hin;
        fast_copy(hin, chol, sizeof(double) * n_l);
        fast_copy(hin + n_l, fx, sizeof(double) * n_fx);
        SSMQ_HIP(hipMemcpyAsync(dl, hin, in_bytes, hipMemcpyHostToDevice, s));
        MoArgs m;
        memset(&m, 0, sizeof(m));
        m.D = D; m.E = E; m.N = N; m.mode = SSMQ_MO_FX; m.tp_nu = h->tp_nu; m.cov_scale = m.ccov_scale = 1.0; m.consts = h->d_mo;
        m.chol_in = dl; m.fx_in = dfx; m.mean_f = omf; m.cov_f = omf + nb * E; m.cov_fx = m.cov_f + nb * E * E;
        m.es_out = 1; m.bs_mf = E; m.bs_cf = E * E; m.bs_cfx = E * D;
        if ((rc = launch_apply_mo(m, B, s))) return rc;
        SSMQ_HIP(hipMemcpyAsync(g_stage.hout, omf, out_bytes, hipMemcpyDeviceToHost, s));
        SSMQ_HIP(hipStreamSynchronize(s));
        const double *ho = (const double *)g_stage.hout;
        fast_copy(mean_f, ho, sizeof(double) * nb * E);
        fast_copy(cov_f, ho + nb * E, sizeof(double) * nb * E * E);
        fast_copy(cov_fx, ho + nb * (E + (size_t)E * E), sizeof(double) * nb * E * D);
        return SSMQ_OK;
    }
    const bool wide_fits = wide_lds_bytes(D, E, N) <= 160 * 1024 - 64;
    const bool centred = h->form == SSMQ_FORM_SIGMA;
    // point sets beyond the wave kernels without a fused matrix-core instantiation (as apply_dev_impl): blocked GEMM + rest
    const bool big = N > 64 && ((!centred && h->d_wc_blk && (B * E >= kGemmMinRows || !wide_fits) && (h->tp_nu <= 0.0 || h->d_ik_blk)) ||
                                (centred && !wide_fits));
    if (!big && !wide_fits) {
        set_error("apply_fx_batch: shape too large for the LDS-resident generic kernel");
        return SSMQ_E_UNSUPPORTED;
    }
    // staging arena: [chol | fx | mean | x] up, [mean_f | cov_f | cov_fx] down through the pinned blocks; the padded copies
    // of the matrix-core route behind them
    const bool gemm = !big && h->d_wc_pad && h->form == SSMQ_FORM_BQ && B * E >= kGemmMinRows;
    const size_t nb = (size_t)B, n_l = nb * D * D, n_fx = nb * E * N, n_m = centred ? nb * D : 0, n_x = centred ? nb * D * N : 0;
    const size_t n_out = nb * ((size_t)E + (size_t)E * E + (size_t)E * D);
    const size_t in_bytes = sizeof(double) * (n_l + n_fx + n_m + n_x), out_bytes = sizeof(double) * n_out;
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    const int big_kb = (N + 15) / 16, big_lda = big_kb * 16, big_ldt = (big && !centred) ? h->big_ncb * kBigCols : 0;
    const int big_nt = (big && !centred) ? (h->tp_nu > 0.0 ? 2 : 1) : 0;
    const size_t pad_bytes = gemm ? sizeof(double) * nb * E * h->np_pad : big ? sizeof(double) * nb * E * big_lda : 0;
    const size_t t_bytes = gemm ? pad_bytes : sizeof(double) * nb * E * (size_t)big_ldt * big_nt;
    const size_t off_out = al(in_bytes), off_fxp = off_out + al(out_bytes), off_tt = off_fxp + al(pad_bytes);
    if ((rc = g_stage.reserve(off_tt + al(t_bytes), in_bytes, out_bytes))) return rc;
    hipStream_t s = stream();
    char *dev = (char *)g_stage.dev;
    double *dl = (double *)dev, *dfx = dl + n_l, *dm = dfx + n_fx, *dx = dm + n_m;
    double *omf = (double *)(dev + off_out), *ocf = omf + nb * E, *ocfx = ocf + nb * E * E;
    double *hin = (double *)g_stage.hin;
    fast_copy(hin, chol, sizeof(double) * n_l);
    fast_copy(hin + n_l, fx, sizeof(double) * n_fx);
    if (centred) {
        fast_copy(hin + n_l + n_fx, mean, sizeof(double) * n_m);
        fast_copy(hin + n_l + n_fx + n_m, x, sizeof(double) * n_x);
    }
    SSMQ_HIP(hipMemcpyAsync(dl, hin, in_bytes, hipMemcpyHostToDevice, s));
    WideArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.E = E; a.N = N; a.form = h->form; a.mode = SSMQ_WIDE_FX; a.emv_mode = h->emv_mode; a.tp_nu = h->tp_nu;
    a.cov_scale = a.ccov_scale = 1.0;
    a.consts = h->d_wide; a.mean = dm; a.chol_in = dl; a.fx_in = dfx; a.x_in = dx;
    a.mean_f = omf; a.cov_f = ocf; a.cov_fx = ocfx; a.es_out = 1; a.bs_mf = E; a.bs_cf = E * E;
    a.bs_cfx = E * D;
    if (big) {
        const int64_t M = B * E;
        double *fxp = (double *)(dev + off_fxp), *ttp = (double *)(dev + off_tt);
        SSMQ_HIP(hipMemsetAsync(fxp, 0, sizeof(double) * M * big_lda, s));
        SSMQ_HIP(hipMemcpy2DAsync(fxp, sizeof(double) * big_lda, dfx, sizeof(double) * N, sizeof(double) * N, M,
                                  hipMemcpyDeviceToDevice, s));
        const WideLayout wl = wide_layout(D, E, N, h->form);
        if ((rc = launch_row_means(fxp, h->d_wide + wl.wm, M, big_lda, N, omf, s))) return rc;
        if (!centred && (rc = launch_fxwc_blocks(fxp, h->d_wc_blk, ttp, M, big_lda, big_ldt, big_kb, h->big_ncb, s))) return rc;
        if (big_nt == 2 && (rc = launch_fxwc_blocks(fxp, h->d_ik_blk, ttp + (size_t)M * big_ldt, M, big_lda, big_ldt, big_kb,
                                                    h->big_ncb, s)))
            return rc;
        BigRest r;
        memset(&r, 0, sizeof(r));
        r.D = D; r.E = E; r.N = N; r.form = h->form; r.emv_mode = h->emv_mode; r.tp_nu = h->tp_nu; r.cov_scale = r.ccov_scale = 1.0;
        r.consts = h->d_wide; r.fx = fxp; r.t = centred ? nullptr : ttp; r.t2 = big_nt == 2 ? ttp + (size_t)M * big_ldt : nullptr;
        r.lda = big_lda; r.ldt = big_ldt; r.p_col = 16 * big_kb; r.mean_rows = omf; r.chol = dl;
        r.cov_f = ocf; r.cov_fx = ocfx; r.es = 1; r.bs_cf = (int64_t)E * E; r.bs_cfx = (int64_t)E * D;
        if ((rc = launch_big_rest(r, B, s))) return rc;
        a.mode = -1;   // done
    } else if (gemm) {
        // matrix-core route: rows re-pitched to the padded column count, T = FX Wc for the whole batch, then the rest
        const int NP = h->np_pad;
        const int64_t M = B * E;
        double *fxp = (double *)(dev + off_fxp), *ttp = (double *)(dev + off_tt);
        SSMQ_HIP(hipMemsetAsync(fxp, 0, sizeof(double) * M * NP, s));
        SSMQ_HIP(hipMemcpy2DAsync(fxp, sizeof(double) * NP, dfx, sizeof(double) * N, sizeof(double) * N, M,
                                  hipMemcpyDeviceToDevice, s));
        if (h->tp_nu <= 0.0 && h->d_wcx_pad && fxwc_cov_supported(E) && D <= 16 && !ssmq::sw("SSMQ_NO_FUSED_COV")) {
            // means of the supplied values, then the GEMM whose epilogue forms both covariances (no T in memory)
            const WideLayout wl = wide_layout(D, E, N, h->form);
            if ((rc = launch_row_means(fxp, h->d_wide + wl.wm, M, NP, N, omf, s))) return rc;
            if ((rc = launch_fxwc_cov_mfma(NP, fxp, h->d_wcx_pad, M, NP, omf, dl, h->d_wide + wl.emv,
                                           h->emv_mode == SSMQ_EMV_BROADCAST ? 1 : 0, nullptr, 1.0, 1.0, E, D, ocf, ocfx, 1,
                                           (int64_t)E * E, (int64_t)E * D, s)))
                return rc;
            a.mode = -1;   // done
        } else {
            if ((rc = launch_fxwc_mfma(NP, fxp, h->d_wc_pad, ttp, M, NP, NP, s))) return rc;
            a.fx_ld = NP; a.fx_in = fxp; a.t_in = ttp;
        }
    }
    if (a.mode != -1 && (rc = hip_fail(launch_apply_wide(a, B, s), "k_apply_wide(fx)"))) return rc;
    SSMQ_HIP(hipMemcpyAsync(g_stage.hout, omf, out_bytes, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    const double *ho = (const double *)g_stage.hout;
    fast_copy(mean_f, ho, sizeof(double) * nb * E);
    fast_copy(cov_f, ho + nb * E, sizeof(double) * nb * E * E);
    fast_copy(cov_fx, ho + nb * (E + (size_t)E * E), sizeof(double) * nb * E * D);
    return SSMQ_OK;
}

// T = FX Wc on the matrix cores for device-resident integrand values (the GEMM-shaped stage of a large-N BQ transform)
int ssmq_fxwc_batch_dev(ssmq_transform *h, int64_t M, const double *d_fx, int64_t ld_fx, double *d_t, int64_t ld_t,
                        int *n_padded) {
    SSMQ_HANDLE_LOCK(h);
    if (is_mo(h)) return refuse_mo("ssmq_fxwc_batch_dev");
    if (h && h->form == SSMQ_FORM_TAYLOR1) {
        set_error("the linearisation transform has no sigma points");
        return SSMQ_E_UNSUPPORTED;
    }
    if (is_taylor_gpqd(h)) return refuse_taylor_gpqd("ssmq_fxwc_batch_dev");
    if (is_trunc(h)) return refuse_trunc("ssmq_fxwc_batch_dev");
    if (is_gpqd(h)) return refuse_gpqd("ssmq_fxwc_batch_dev");
    if (!h || M < 0 || (M > 0 && (!d_fx || !d_t))) {
        set_error("fxwc_batch: bad argument");
        return SSMQ_E_ARG;
    }
    if (n_padded) *n_padded = h->np_pad;
    if (!h->d_wc_pad) {
        set_error("fxwc_batch: this transform has no matrix-core instantiation (BQ form, N in 113..128, 193..208, 241..256)");
        return SSMQ_E_UNSUPPORTED;
    }
    if (M == 0) return SSMQ_OK;
    if (ld_fx < h->np_pad || ld_t < h->np_pad || ld_fx > 0x7fffffff || ld_t > 0x7fffffff || (ld_fx & 1)) {
        set_error("fxwc_batch: row pitches must be even and at least the padded point count");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    return launch_fxwc_mfma(h->np_pad, d_fx, h->d_wc_pad, d_t, M, (int)ld_fx, (int)ld_t, stream());
}

}  // extern "C"
