// The truncated sigma-point transform (SSMQ_FORM_TRUNC_SIGMA; mtran.py:588-658: TruncatedSigmaPointTransform - the measurement
// transform of the Truncated*Kalman filters, ssinf.py:844-901) for an integrand that reads the DE leading of its D inputs:
//
//   L = chol(cov),  m_e = mean[:DE],  L_e = L[:DE, :DE]  (= chol(cov[:DE, :DE]): one factorisation serves both point sets)
//   x_eff_i = m_e + L_e xi_eff_i  (NE points),   x_j = mean + L xi_j  (N points)
//   mean_f = sum_i wm_i f(x_eff_i),  cov_f = sum_i wc_i (f(x_eff_i) - mean_f)(..)' [+ cov_add],
//   cov_fx = sum_j wcc_j (f(x_j) - mean_f)(x_j - mean)'                                      (E, D)
//
// k_apply_trunc<D, E>: one transform per lane, element planes in and out (element e of item b at ptr[e ld + b]), everything in
// registers.  D and E are compile-time - they size the factor and the three accumulators and make every register index static; the
// effective dimension and both point counts are run-time: DE only guards rows (a wave-uniform test) and pitches the effective
// points.  The constants sit in the handle's block [xi_eff [NE][DE] | wm [NE] | wc [NE] | xi [N][D] | wcc [N]]; every lane
// reads the same address, so they come through the constant address space as scalar loads.  The integrand is reached through
// eval_integrand as in k_linearize.  One point loop runs three times - mean (effective set), covariance (effective set again: up
// to 729 values per output cannot wait in registers, and the centred sum needs the finished mean), cross-covariance (full set) - so
// the 16-way integrand switch is in the code once.  Nothing is reused between the full and the effective set: every value is a
// fresh evaluation.  The factorisation is chol_packed's, column by column from the top-left corner: L_e, and with it mean_f and
// cov_f, depend on mean[:DE] and cov[:DE, :DE] alone, bit for bit.  A pivot that is not positive: status 1, NaN outputs.
#include "ssmq_device.h"
#include "ssmq_host.h"
#include "ssmq_math.h"
#include "ssmq_jacobian_kernel.h"   // LinArgs: the planes of one application

namespace ssmq {

constexpr int kTruncMaxD = 6, kTruncMaxE = 4, kTruncMaxN = 729;   // Gauss-Hermite of degree 3 at six dimensions

struct TruncArgs {
    int32_t DE, NE, N, fid, time_stride;
    const double *consts;                            // trunc_layout block
    const double *mean, *cov, *time, *cov_add;       // planes [D][ld], [D*D][ld] (lower triangle read); time [B] or [1]; cov_add [E*E] or null
    double *mean_f, *cov_f, *cov_fx;                 // planes [E][ld], [E*E][ld], [E*D][ld]
    int32_t *status;                                 // [B]
    int64_t B, ld;
    double cov_scale, ccov_scale;
    FPar fp;
};

// offsets (doubles) into the constant block
struct TruncLayout {
    int xi_eff, wm, wc, xi, wcc, total;
};
__host__ __device__ constexpr inline TruncLayout trunc_layout(int D, int DE, int NE, int N) {
    TruncLayout c{};
    c.xi_eff = 0;
    c.wm = NE * DE;
    c.wc = c.wm + NE;
    c.xi = c.wc + NE;
    c.wcc = c.xi + N * D;
    c.total = c.wcc + N;
    return c;
}

template <int D, int E>
__global__ __launch_bounds__(256) void k_apply_trunc(const TruncArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    const int64_t ld = a.ld;
    double m[D], L[D * (D + 1) / 2];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = a.mean[d * ld + b];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[SSMQ_PK(i, j)] = a.cov[(int64_t)(i * D + j) * ld + b];
    const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
    const bool ok = chol_packed<D>(L);

    const int DE = a.DE;
    const TruncLayout cl = trunc_layout(D, DE, a.NE, a.N);
    const cdouble_p c = (cdouble_p)a.consts;
    double mf[E], cf[E * (E + 1) / 2], cx[E * D];
#pragma unroll
    for (int e = 0; e < E; ++e) mf[e] = 0.0;
#pragma unroll
    for (int i = 0; i < E * (E + 1) / 2; ++i) cf[i] = 0.0;
#pragma unroll
    for (int i = 0; i < E * D; ++i) cx[i] = 0.0;
    if (ok) {
        // pass 0: mean over the effective set; pass 1: covariance over it; pass 2: cross-covariance over the full set
#pragma unroll 1
        for (int pass = 0; pass < 3; ++pass) {
            const bool full = pass == 2;
            const int dim = full ? D : DE, cnt = full ? a.N : a.NE;
            const int pts = full ? cl.xi : cl.xi_eff, wts = pass == 0 ? cl.wm : (pass == 1 ? cl.wc : cl.wcc);
#pragma unroll 1
            for (int n = 0; n < cnt; ++n) {
                double dx[D], x[D];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    double s = 0.0;
                    if (d < dim) {
#pragma unroll
                        for (int k = 0; k <= d; ++k) s += L[SSMQ_PK(d, k)] * c[pts + n * dim + k];
                    }
                    dx[d] = s;
                    x[d] = d < dim ? m[d] + s : 0.0;       // (the integrand reads no entry behind dim: launch_apply_trunc)
                }
                double xs[kMaxIntegrandIn], o[SSMQ_MAX_DIM];
#pragma unroll
                for (int k = 0; k < kMaxIntegrandIn; ++k) {
                    const int src = a.fp.n_idx > 0 ? (k < a.fp.n_idx ? a.fp.idx[k] : 0) : (k < D ? k : 0);
                    double v = x[0];                        // static register indices: a select chain over the D candidates
#pragma unroll
                    for (int q = 1; q < D; ++q) v = (src == q) ? x[q] : v;
                    xs[k] = k < D ? v : 0.0;
                }
#pragma unroll
                for (int e = 0; e < SSMQ_MAX_DIM; ++e) o[e] = 0.0;
                eval_integrand(a.fid, xs, t, a.fp, o);
                const double w = c[wts + n];
                if (pass == 0) {
#pragma unroll
                    for (int e = 0; e < E; ++e) mf[e] += w * o[e];
                } else if (pass == 1) {
#pragma unroll
                    for (int e = 0; e < E; ++e)
#pragma unroll
                        for (int e2 = 0; e2 <= e; ++e2) cf[SSMQ_PK(e, e2)] += w * (o[e] - mf[e]) * (o[e2] - mf[e2]);
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e)
#pragma unroll
                        for (int d = 0; d < D; ++d) cx[e * D + d] += w * (o[e] - mf[e]) * dx[d];
                }
            }
        }
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int e = 0; e < E; ++e) a.mean_f[e * ld + b] = ok ? mf[e] : nan;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            double s = cf[e2 <= e ? SSMQ_PK(e, e2) : SSMQ_PK(e2, e)] * a.cov_scale;
            if (a.cov_add) s += a.cov_add[e * E + e2];
            a.cov_f[(int64_t)(e * E + e2) * ld + b] = ok ? s : nan;
        }
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) a.cov_fx[(int64_t)(e * D + d) * ld + b] = ok ? cx[e * D + d] * a.ccov_scale : nan;
    a.status[b] = ok ? 0 : 1;
}

int refuse_trunc(const char *what) {
    set_error(std::string(what) + ": not implemented for the truncated sigma-point transform (SSMQ_FORM_TRUNC_SIGMA runs through "
              "ssmq_apply_batch[_dev] and, as the measurement transform next to a sigma-point dynamics transform, through "
              "ssmq_filter_forward_dev and ssmq_filter_smooth_dev)");
    return SSMQ_E_UNSUPPORTED;
}

bool trunc_range_ok(int D, int D_eff, int E, int N_eff, int N) {
    return D_eff >= 1 && D_eff <= D && D <= kTruncMaxD && E >= 1 && E <= kTruncMaxE && N_eff >= 1 && N_eff <= kTruncMaxN && N >= 1 &&
           N <= kTruncMaxN;
}

namespace {
template <int D, int E>
void launch_shape(const TruncArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_apply_trunc<D, E>), dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, s, a);
}
template <int D>
void launch_outputs(int E, const TruncArgs &a, hipStream_t s) {
    switch (E) {
        case 1: launch_shape<D, 1>(a, s); break;
        case 2: launch_shape<D, 2>(a, s); break;
        case 3: launch_shape<D, 3>(a, s); break;
        default: launch_shape<D, 4>(a, s); break;
    }
}
}  // namespace

int launch_apply_trunc(const ssmq_transform *h, const ssmq_integrand *f, const LinArgs &p, hipStream_t s) {
    if (!is_trunc(h) || !h->d_trunc || !trunc_range_ok(h->D, h->tr_deff, h->E, h->tr_neff, h->N)) {
        set_error("apply (truncated): not a truncated sigma-point handle");
        return SSMQ_E_ARG;
    }
    if (is_user_integrand(f)) return refuse_user_integrand("truncated sigma-point transform (k_apply_trunc)");
    FInfo fi;
    if (!integrand_info(f->id, &fi)) {
        set_error("unknown integrand id");
        return SSMQ_E_ARG;
    }
    // the effective points have DE entries: an integrand that reads behind them has no truncated transform
    bool reads_ok = f->n_idx > 0 ? f->n_idx >= fi.din : fi.din <= h->tr_deff;
    for (int k = 0; k < f->n_idx && k < SSMQ_MAX_FIDX; ++k) reads_ok = reads_ok && f->idx[k] >= 0 && f->idx[k] < h->tr_deff;
    if (!reads_ok) {
        set_error("apply (truncated): the integrand reads state entries behind the effective dimension " + std::to_string(h->tr_deff) +
                  " (supported: models that read at most D_eff leading inputs, every state-index entry < D_eff)");
        return SSMQ_E_UNSUPPORTED;
    }
    TruncArgs a;
    memset(&a, 0, sizeof(a));
    a.DE = h->tr_deff; a.NE = h->tr_neff; a.N = h->N; a.fid = f->id; a.time_stride = p.time_stride; a.consts = h->d_trunc;
    a.mean = p.mean; a.cov = p.cov; a.time = p.time; a.cov_add = p.cov_add; a.mean_f = p.mean_f; a.cov_f = p.cov_f; a.cov_fx = p.cov_fx;
    a.status = p.status; a.B = p.B; a.ld = p.ld; a.cov_scale = p.cov_scale; a.ccov_scale = p.ccov_scale; a.fp = p.fp;
    switch (h->D) {
        case 1: launch_outputs<1>(h->E, a, s); break;
        case 2: launch_outputs<2>(h->E, a, s); break;
        case 3: launch_outputs<3>(h->E, a, s); break;
        case 4: launch_outputs<4>(h->E, a, s); break;
        case 5: launch_outputs<5>(h->E, a, s); break;
        default: launch_outputs<6>(h->E, a, s); break;
    }
    return hip_fail(hipGetLastError(), "k_apply_trunc");
}

}  // namespace ssmq

using namespace ssmq;

extern "C" ssmq_transform *ssmq_transform_create_truncated(int D, int D_eff, int E, int N_eff, const double *xi_eff, const double *wm,
                                                           const double *wc, int N, const double *xi, const double *wcc) {
    if (!trunc_range_ok(D, D_eff, E, N_eff, N)) {
        set_error("transform_create_truncated: the truncated sigma-point transform supports 1 <= D_eff <= D <= 6, 1 <= E <= 4 and "
                  "1 <= N_eff, N <= 729");
        return nullptr;
    }
    if (!xi_eff || !wm || !wc || !xi || !wcc) {
        set_error("transform_create_truncated: null argument");
        return nullptr;
    }
    // the block in the kernel's layout: points point-major, as the other constant blocks keep them
    const TruncLayout cl = trunc_layout(D, D_eff, N_eff, N);
    std::vector<double> blk((size_t)cl.total);
    for (int n = 0; n < N_eff; ++n) {
        for (int d = 0; d < D_eff; ++d) blk[cl.xi_eff + n * D_eff + d] = xi_eff[d * N_eff + n];
        blk[cl.wm + n] = wm[n];
        blk[cl.wc + n] = wc[n];
    }
    for (int n = 0; n < N; ++n) {
        for (int d = 0; d < D; ++d) blk[cl.xi + n * D + d] = xi[d * N + n];
        blk[cl.wcc + n] = wcc[n];
    }
    for (double v : blk)
        if (!std::isfinite(v)) {
            set_error("transform_create_truncated: points and weights must be finite");
            return nullptr;
        }
    if (ensure_device()) return nullptr;
    ssmq_transform *h = new ssmq_transform();
    h->D = D; h->E = E; h->N = N; h->form = SSMQ_FORM_TRUNC_SIGMA; h->emv_mode = SSMQ_EMV_DIAG; h->tp_nu = 0.0;
    h->opt_mask = 0;
    h->tr_deff = D_eff; h->tr_neff = N_eff;
    hipGetDevice(&h->device);
    h->d_small = h->d_wide = nullptr;
    // `generation` carries a hash of the constants: a handle that a later allocation puts at the address of a destroyed one must not
    // find the launch loop captured for the old constants (key_of_pair, ssmq_host.h)
    std::vector<uint64_t> words;
    key_bytes(words, blk.data(), sizeof(double) * blk.size());
    uint64_t hash = 1469598103934665603ull ^ (uint64_t)D_eff ^ ((uint64_t)N_eff << 16);
    for (uint64_t w : words) hash = (hash ^ w) * 1099511628211ull;
    h->generation = (uint32_t)(hash ^ (hash >> 32));
    if (hipMalloc((void **)&h->d_trunc, sizeof(double) * blk.size()) != hipSuccess ||
        hipMemcpyAsync(h->d_trunc, blk.data(), sizeof(double) * blk.size(), hipMemcpyHostToDevice, ssmq::stream()) != hipSuccess ||
        hipStreamSynchronize(ssmq::stream()) != hipSuccess) {
        set_error("transform_create_truncated: device allocation or upload failed");
        ssmq_transform_destroy(h);
        return nullptr;
    }
    return h;
}
