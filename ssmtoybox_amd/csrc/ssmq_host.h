// Host-side internals of libssmq shared between translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <functional>
#include <vector>
#include "ssmq_device.h"
#include "ssmq_wide.h"

struct ssmq_transform {
    int D, E, N, form, emv_mode, device;
    double tp_nu;
    // host copies in the reference's natural layout
    std::vector<double> xi, wm, Wc, Wcc, emv, iK;
    // device constant blocks: `small` = transposed layout of ssmq_apply_small.h, `wide` = natural layout
    double *d_small, *d_wide;
    int opt_mask;   // SSMQ_OPT_* fast paths this handle's constants qualify for (decided in upload_consts)
    // matrix-core route for large point sets (ssmq_gemm_mfma.hip): Wc zero-padded to np_pad x np_pad, or null
    double *d_wc_pad = nullptr;
    int np_pad = 0;
    // ... and [Wc | Wcc'] as np_pad x (np_pad + 16) for the route whose GEMM epilogue forms both covariances, or null
    double *d_wcx_pad = nullptr;
    // ... and [S | Wcc' | wm] with S = tril(sym(Wc)), half the diagonal (Wc = S + S'): the one-launch routes skip the zero blocks
    double *d_sx_pad = nullptr;
    // ... and for point sets beyond that route's instantiations (208 < N): S in fragment order by panels of 256 columns, then the G tile
    // (ssmq_bq_stream.hip: bq_stream_pack), or null
    double *d_sx_pan = nullptr;
    // point sets without an instantiation of that route (N > 64): Wc (and iK for the t-process) as column blocks of
    // kBigCols columns, each [big_kb 16][kBigCols] zero-padded (ssmq_apply_big.hip); null = not built
    double *d_wc_blk = nullptr, *d_ik_blk = nullptr;
    int big_kb = 0, big_ncb = 0;   // k blocks of 16 points; column blocks of [Wc | pad to 16 big_kb | Wcc'] (big_ncb)
    // multi-output form (SSMQ_FORM_BQ_MO, ssmq_apply_mo.hip): the host vectors above hold wm [E][N], Wc as the blocks (i, j), i >= j,
    // in packed order [i (i + 1) / 2 + j][N][N], Wcc [E][D][N], emv [E], iK [E][N][N]; d_mo is the one constant block (mo_layout),
    // d_small / d_wide stay null
    double *d_mo = nullptr;
    // Taylor-GPQD form (SSMQ_FORM_TAYLOR_GPQD, ssmq_jacobian_kernel.h): the RBF kernel's scale and length-scales, which travel to the
    // kernel by value, and the two optional planes [B] the next applications write model_var / integ_var of every item to
    // (ssmq_taylor_gpqd_variance_planes; null: not written)
    double tg_alpha = 0.0, tg_ell[SSMQ_MAX_DIM] = {};
    double *d_tg_mvar = nullptr, *d_tg_ivar = nullptr;
    // truncated sigma-point form (SSMQ_FORM_TRUNC_SIGMA, ssmq_apply_trunc.hip): D inputs of which the integrand reads the tr_deff
    // leading ones, N points of the full-dimension rule, tr_neff of the effective one; d_trunc is the one constant block
    // (trunc_layout), d_small / d_wide stay null and no host copies are kept (the handle is recreated when its constants change)
    int tr_deff = 0, tr_neff = 0;
    double *d_trunc = nullptr;
    // GPQ+D form (SSMQ_FORM_GPQD, ssmq_apply_gpqd_kernel.h): N points of which those in gq_mask carry a derivative observation;
    // d_gpqd is the one constant block (gpqd_layout: the weights expanded to the full layout), xi the host copy of the points,
    // d_small / d_wide stay null
    double *d_gpqd = nullptr;
    uint32_t gq_mask = 0;
    uint32_t generation = 0;   // bumped by every upload of constants (create / update)
    // Threads (include/ssmq.h, conventions): every entry point that takes this handle holds `mu` for its duration; `owner` /
    // `owner_epoch` name the thread context (its stream) that used the handle last - another context waits for that stream
    // before it touches the handle's device blocks (ssmq::HandleGuard).
    mutable std::recursive_mutex mu;
    mutable void *owner = nullptr;
    mutable unsigned owner_epoch = 0;
};

namespace ssmq {

void set_error(const std::string &msg);

// User-defined integrands (ssmq_rtc.hip).  Only the two routes below run them; every other entry point that takes an integrand
// refuses a user id at its top (SSMQ_E_UNSUPPORTED) instead of reaching a generic kernel, whose eval_integrand() has no case for it.
inline bool is_user_integrand(int id) { return id >= SSMQ_F_USER_FIRST && id < SSMQ_F_USER_FIRST + SSMQ_F_USER_SLOTS; }
inline bool is_user_integrand(const ssmq_integrand *f) { return f && is_user_integrand(f->id); }
int refuse_user_integrand(const char *what);   // sets the error text, returns SSMQ_E_UNSUPPORTED
struct FusedArgs;   // ssmq_fused.h
struct ApplyArgs;   // ssmq_apply_small.h
struct UpdArgs;     // ssmq_update.h
// Whole-pass filter kernel k_filter_fused<> for a pair of models of which at least one is a user integrand: 1 launched (or, with
// dry_run, the name set), < 0 error - never 0, so that no caller falls back to the launch loop.
struct FilterPass;   // below, with the launchers of the fused time loop
int rtc_launch_fused(const FilterPass &p);
// k_apply_small<> for a user integrand: SSMQ_OK (launched, or with dry_run the name set) or < 0.
int rtc_launch_apply(const ssmq_transform *h, const ssmq_integrand *f, int sel, const ApplyArgs &a, hipStream_t s,
                     const char **name, bool dry_run);
// k_mc_moments<> (ssmq_mc_moments.h) for a user integrand, launched with the AOT route's arguments: SSMQ_OK or < 0.
struct McMomArgs;
int rtc_launch_mc(const ssmq_integrand *f, int D, int E, const McMomArgs &a, unsigned grid, hipStream_t s);
bool mc_range_ok(int D, int E, int64_t n);   // ssmq_mc_transform.hip: 1 <= D, E <= 6, 2 <= n < 2^31
// Threads.  Every calling thread has its own CONTEXT: a HIP stream and the caches that belong to a stream (grow-only workspaces,
// pinned staging blocks, captured launch graphs).  Calls of different threads on different handles run concurrently - on the
// host and, stream by stream, on the device.  Contexts are pooled: a thread that ends hands its context (stream and caches
// intact) to the next new thread.  A handle is locked for the duration of every entry point that takes it (HandleGuard; two
// handles in address order), and a context that picks up a handle last used by another one waits for that context's stream
// first, so that constants uploaded or buffers built there are complete.  Device buffers the CALLER passes between threads are
// the caller's to order (ssmq_sync() in the thread that queued the work), as with any per-thread stream.  The communicator entry
// points (ssmq_comm_*) belong to one thread.
struct Ctx {
    hipStream_t stream = nullptr;
    int dev = -1;
    unsigned epoch = 0;                      // unique per (context, device binding): per-device function attributes, cached graphs
    void *gemm_ws = nullptr;                 // scratch of the matrix-core routes (ssmq_api_transform.hip)
    size_t gemm_ws_bytes = 0;
    void *stage = nullptr;                   // ssmq_api_host.hip: StagingArena
    void *fc = nullptr;                      // ssmq_api_filter.hip: FilterCache
    void *theta_graphs = nullptr;            // ssmq_api_theta.hip: captured graphs of the theta-batched step
    void *pinned_flags = nullptr;            // 64 bytes of pinned host memory the device rounds report through (ssmq_marginal_device.hip)
    void *strip_buf = nullptr;               // flags + hand-over buffer of the strip schedule (ssmq_filter_chunked.hip), grow-only
    size_t strip_bytes = 0;
    void *multi = nullptr;                   // ssmq_api_study.hip: MultiCache (side streams, events, constants and captured graph of
                                             // ssmq_filter_forward_multi_dev)
    void *pipe = nullptr;                    // ssmq_api_study.hip: PipeCache (copy streams and events of ssmq_filter_forward_piped)
    bool no_strips = false;                  // set while a multi-filter launch is being built: the strip schedule owns ONE buffer
                                             // per context and its jobs run concurrently
};
Ctx &ctx();
struct HandleGuard {
    const ssmq_transform *a, *b;
    explicit HandleGuard(const ssmq_transform *h0, const ssmq_transform *h1 = nullptr);
    ~HandleGuard();
    HandleGuard(const HandleGuard &) = delete;
    HandleGuard &operator=(const HandleGuard &) = delete;
};
#define SSMQ_HANDLE_LOCK(...) ssmq::HandleGuard ssmq_handle_guard_(__VA_ARGS__)
// ... for any number of handles (ssmq_filter_forward_multi_dev): unique handles, locked in address order
struct MultiHandleGuard {
    std::vector<const ssmq_transform *> hs;
    explicit MultiHandleGuard(std::vector<const ssmq_transform *> handles);
    ~MultiHandleGuard();
    MultiHandleGuard(const MultiHandleGuard &) = delete;
    MultiHandleGuard &operator=(const MultiHandleGuard &) = delete;
};
int hip_fail(hipError_t e, const char *what);
hipStream_t stream();
int ensure_device();
// The calling thread's context epoch: a new value whenever the context binds to a device (reset_device_caches); per-function
// attributes (hipFuncAttributeMaxDynamicSharedMemorySize) are per device and are set again when a thread sees a new value
// (the `static thread_local unsigned attr_epoch` of the launchers).
unsigned device_epoch();
// What the calling thread's context caches on ONE device, each piece dropped by the unit that owns it when the context binds to
// another device (ssmq_api_runtime.hip: reset_device_caches, in this order).
void drop_filter_cache();        // ssmq_api_filter.hip: workspace, constants and captured launch loop of the filter time loop
void drop_theta_step_graphs();   // ssmq_api_theta.hip
void drop_gemm_scratch();        // ssmq_api_transform.hip
void drop_staging_arena();       // ssmq_api_host.hip
void reset_wide_attributes();    // ssmq_apply_wide.hip: the dynamic-LDS limits are set again on the new device
void drop_multi_cache();         // ssmq_api_study.hip
void drop_pipe_cache();          // ssmq_api_study.hip

// Device arena + pinned staging blocks of the host-buffer entry points (ssmq_api_host.hip, ssmq_api_theta.hip,
// ssmq_api_study.hip): one per context.
struct StagingArena;
StagingArena &stage_of_ctx();

#define SSMQ_HIP(call)                                        \
    do {                                                      \
        hipError_t e__ = (call);                              \
        if (e__ != hipSuccess) return ssmq::hip_fail(e__, #call); \
    } while (0)

// Raises the dynamic-LDS limit of `kernels` to `bytes` once per device binding of the calling thread; `seen` is the call
// site's `static thread_local unsigned`, left as it is on failure so that the next call tries again.
inline int set_max_dynamic_lds(unsigned &seen, std::initializer_list<const void *> kernels, size_t bytes) {
    if (seen == device_epoch()) return SSMQ_OK;
    for (const void *k : kernels) SSMQ_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    seen = device_epoch();
    return SSMQ_OK;
}

// Device arena + pinned staging blocks of the host-buffer entry points that are called in tight loops with small batches
// (ssmq_apply_batch: the drop-in apply(); ssmq_gp_theta_step), grow-only, dropped when the device changes.  The calls are
// synchronous on the library's one stream, so one arena serves them all.
struct StagingArena {
    void *dev = nullptr, *hin = nullptr, *hout = nullptr;
    size_t dev_bytes = 0, hin_bytes = 0, hout_bytes = 0;
    static int grow(void **p, size_t *have, size_t need, bool host) {
        if (*have >= need) return SSMQ_OK;
        if (*p) {
            SSMQ_HIP(hipStreamSynchronize(stream()));
            if (host) hipHostFree(*p); else hipFree(*p);
        }
        *p = nullptr;
        *have = 0;
        const size_t want = need + need / 4;       // a little head room: consecutive calls differ by a few items
        if (host) SSMQ_HIP(hipHostMalloc(p, want, hipHostMallocDefault)); else SSMQ_HIP(hipMalloc(p, want));
        *have = want;
        return SSMQ_OK;
    }
    int reserve(size_t d, size_t hi, size_t ho) {
        int rc;
        if ((rc = grow(&dev, &dev_bytes, d, false)) || (rc = grow(&hin, &hin_bytes, hi, true)) ||
            (rc = grow(&hout, &hout_bytes, ho, true)))
            return rc;
        return SSMQ_OK;
    }
    void drop() {
        if (dev) hipFree(dev);
        if (hin) hipHostFree(hin);
        if (hout) hipHostFree(hout);
        dev = hin = hout = nullptr;
        dev_bytes = hin_bytes = hout_bytes = 0;
    }
};

// transform handles and the route selection of one transform (ssmq_api_transform.hip)
void fill_fpar(const ssmq_integrand *f, FPar *fp);
int sel_pattern(const ssmq_integrand *f, int din);   // 0: the integrand reads the leading entries, 1: (0, 2, 4, ...), -1: anything else
int check_integrand(const ssmq_transform *h, const ssmq_integrand *f, FInfo *fi);
constexpr int64_t kGemmMinRows = 256;                // rows B E from which a batch takes the matrix-core routes
int apply_dev_impl(ssmq_transform *h, const ssmq_integrand *f, int64_t B, int64_t ld, const double *d_mean, const double *d_cov,
                   const double *d_time, int time_stride, double *d_mean_f, double *d_cov_f, double *d_cov_fx, int32_t *d_status,
                   const double *d_cov_add, const char **kernel_name, bool dry_run, double cov_scale = 1.0, double ccov_scale = 1.0,
                   const double *ttab = nullptr, bool stream_out = true);

// the multi-output form (ssmq_apply_mo.hip): one kernel for the whole transform, the sigma points alone (x_out / chol_out) or the
// reductions alone (chol_in / fx_in); element e of trajectory b at ptr[e * es + b * bs]
inline bool is_mo(const ssmq_transform *h) { return h && h->form == SSMQ_FORM_BQ_MO; }
int refuse_mo(const char *what);   // sets the error text, returns SSMQ_E_UNSUPPORTED
// the Taylor-GPQD form (ssmq_jacobian_kernel.h): no points, no weights - every entry point that reads a handle's constants refuses it
inline bool is_taylor_gpqd(const ssmq_transform *h) { return h && h->form == SSMQ_FORM_TAYLOR_GPQD; }
int refuse_taylor_gpqd(const char *what);   // sets the error text, returns SSMQ_E_UNSUPPORTED
// the truncated sigma-point form (ssmq_apply_trunc.hip): two point sets in a block of its own - it runs through ssmq_apply_batch[_dev]
// and as the measurement transform of the launch-loop filter and smoother, every other entry point refuses it
inline bool is_trunc(const ssmq_transform *h) { return h && h->form == SSMQ_FORM_TRUNC_SIGMA; }
int refuse_trunc(const char *what);   // sets the error text, returns SSMQ_E_UNSUPPORTED
bool trunc_range_ok(int D, int D_eff, int E, int N_eff, int N);   // 1 <= D_eff <= D <= 6, 1 <= E <= 4, 1 <= N_eff, N <= 729
struct TruncArgs;                     // ssmq_apply_trunc.hip
// the GPQ+D form (ssmq_apply_gpqd.hip): a block of its own - it runs through ssmq_apply_batch[_dev] and the launch loop of the
// additive-noise filter and smoother, every other entry point refuses it
inline bool is_gpqd(const ssmq_transform *h) { return h && h->form == SSMQ_FORM_GPQD; }
int refuse_gpqd(const char *what);   // sets the error text, returns SSMQ_E_UNSUPPORTED
bool gpqd_range_ok(int D, int E, int N);   // D <= 6, E <= max(D, 4), 2 <= N <= 2 D + 1
struct GpqdArgs;                      // ssmq_apply_gpqd_kernel.h
struct LinArgs;                       // ssmq_jacobian_kernel.h
// `planes` as for launch_jacobian; a built-in model runs k_apply_gpqd<> / k_apply_gpqd_lds<>, a user integrand registered with a
// Jacobian the same kernels compiled for it at run time (ssmq_rtc.hip: rtc_launch_gpqd; rtc_prepare_gpqd compiles and loads without
// launching, for a stream that is about to be captured).  SSMQ_OK (launched, or with dry_run the name set) or < 0.
int launch_apply_gpqd(const ssmq_transform *h, int din, const ssmq_integrand *f, const LinArgs &planes, hipStream_t s,
                      const char **name = nullptr, bool dry_run = false);
int rtc_launch_gpqd(const ssmq_integrand *f, const GpqdArgs &a, bool lds, hipStream_t s, const char **name, bool dry_run);
int rtc_prepare_gpqd(const ssmq_transform *h, const ssmq_integrand *f);
// `planes`: the planes, the time argument, cov_add, B, ld and the hooks of one application (a LinArgs, as for launch_jacobian); the
// rest of the argument block comes from the handle and the integrand.  SSMQ_OK or < 0.
struct LinArgs;
int launch_apply_trunc(const ssmq_transform *h, const ssmq_integrand *f, const LinArgs &planes, hipStream_t s);
enum { SSMQ_MO_FULL = 0, SSMQ_MO_POINTS = 1, SSMQ_MO_FX = 2 };
struct MoArgs {
    int D, E, N, mode, fid, time_stride;
    double tp_nu, cov_scale, ccov_scale;
    const double *consts;          // mo_layout block
    const double *cov_add;         // [E*E] or null
    const double *mean, *cov, *time;
    int64_t es_in, bs_mean, bs_cov;
    double *mean_f, *cov_f, *cov_fx;
    int64_t es_out, bs_mf, bs_cf, bs_cfx;
    int32_t *status;               // [B] or null
    double *x_out, *chol_out;      // SSMQ_MO_POINTS: [B][D][N], [B][D][D]
    const double *chol_in, *fx_in; // SSMQ_MO_FX: [B][D][D], [B][E][N]
    FPar fp;
};
int launch_apply_mo(const MoArgs &a, int64_t B, hipStream_t s);

// dispatch table of the register-resident kernels (ssmq_small_*.hip)
typedef hipError_t (*small_launch_fn)(const ApplyArgs &, hipStream_t);
struct SmallEntry {
    int fid, D, E, N, form, tp, sel, opt;
    small_launch_fn fn;
    const char *name;
};
const SmallEntry *find_small(int fid, int D, int E, int N, int form, int tp, int sel, int opt);
const SmallEntry *small_table_a(int *n);
const SmallEntry *small_table_b(int *n);
const SmallEntry *small_table_c(int *n);
const SmallEntry *small_table_d(int *n);

// batch GEMM fx Wc on the matrix cores (ssmq_gemm_mfma.hip)
int gemm_mfma_padded(int N);
int launch_fxwc_mfma(int NP, const double *A, const double *Bm, double *T, int64_t M, int lda, int ldt, hipStream_t s);
// ... with the covariance of every trajectory formed in the epilogue (no T in memory)
bool fxwc_cov_supported(int E);
// whole BQ transform in one launch, integrand values LDS-resident (ssmq_bq_fused.hip); WideArgs: ssmq_wide.h
struct WideArgs;
bool bq_fused_supported(int D, int E, int N);
int launch_bq_fused(const WideArgs &a, const double *X, const double *emv, int emv_broadcast, int64_t B, hipStream_t s);
// ... the same for any larger point set, the point axis tiled (ssmq_bq_stream.hip)
bool bq_stream_supported(int D, int E, int N);
int bq_stream_tpw(int E);          // trajectories per 64-row block of FX (fragment order, WideArgs::fx_frag)
size_t bq_stream_x_doubles(int N);
void bq_stream_pack(int D, int N, const double *Wc, const double *Wcc, const double *wm, double *X);
// linearisation transform (mean_f = f(mean), cov_fx = J cov, cov_f = cov_fx J' with the model's own Jacobian) and Taylor-GPQD
// transform (its moments calibrated by the RBF kernel in the handle) - ssmq_jacobian_kernel.h; one launcher for both forms and
// both kinds of model (ssmq_linear.hip): `planes` holds the planes, the time argument, B, ld and the hooks, the rest of the
// argument block comes from the handle and the integrand.  A built-in model runs k_linearize<> / k_taylor_gpqd<>; a user
// integrand that was registered with a Jacobian (ssmq_integrand_define_dx) is handed to rtc_launch_jacobian: k_linearize_fn<> /
// k_taylor_gpqd_fn<> compiled for the model and its shape at run time (ssmq_rtc.hip), launched with the same argument block, grid
// and block.  SSMQ_OK (launched, or with dry_run the name set) or < 0; an integrand without a Jacobian is SSMQ_E_UNSUPPORTED.
// rtc_prepare_jacobian compiles and loads the kernel of (h, f) without launching it: a stream that is being captured must not
// meet a compile or a module load.
struct LinArgs;          // ssmq_jacobian_kernel.h
struct TaylorGpqdArgs;
int launch_jacobian(const ssmq_transform *h, int din, const ssmq_integrand *f, const LinArgs &planes, hipStream_t s,
                    const char **name = nullptr, bool dry_run = false);
bool user_integrand_has_jacobian(int id);
int rtc_launch_jacobian(int form, const ssmq_integrand *f, const TaylorGpqdArgs &a, hipStream_t s, const char **name, bool dry_run);
int rtc_prepare_jacobian(const ssmq_transform *h, const ssmq_integrand *f);
size_t bq_stream_parts_doubles(int E, int N, int64_t B, int cus);   // scratch for the panel-wise tail of a batch (0: no tail is cut)
int launch_bq_stream(const WideArgs &a, const double *X, const double *emv, int emv_broadcast, int64_t B, const double *fx,
                     const double *chol, int64_t lda, int cus, double *parts, hipStream_t s);
int launch_fxwc_cov_mfma(int NP, const double *A, const double *X, int64_t M, int lda, const double *mean_rows,
                         const double *chol, const double *emv, int emv_broadcast, const double *cov_add,
                         double cov_scale, double ccov_scale, int E, int D, double *cov_f, double *cov_fx, int64_t es,
                         int64_t bs, int64_t bs_fx, hipStream_t s);
int launch_row_means(const double *A, const double *wm, int64_t M, int lda, int N, double *mean_rows, hipStream_t s);
// ... and for any point count, by column blocks (ssmq_gemm_mfma.hip); the per-trajectory rest (ssmq_apply_big.hip)
constexpr int kBigCols = 256;
int launch_fxwc_blocks(const double *A, const double *Wblk, double *T, int64_t M, int lda, int ldt, int KB, int ncb,
                       hipStream_t s);
struct BigRest {
    int D, E, N, form, emv_mode;
    double tp_nu, cov_scale, ccov_scale;
    const double *consts;          // WideLayout block (wm, Wc diagonal for the centred form, Wcc, xiT, emv)
    const double *fx, *t, *t2;     // rows b E + e: integrand values [lda], fx Wc [ldt] (null: centred form), fx iK [ldt] or null
    int64_t lda, ldt;
    int p_col;                     // BQ: column of T where the D columns fx Wcc' start (the GEMM's extra columns)
    const double *mean_rows;       // [B E]
    const double *chol;            // [B][D][D]
    const double *cov_add;         // [E*E] or null
    double *cov_f, *cov_fx;        // element e of trajectory b at ptr[e * es + b * bs_*]
    int64_t es, bs_cf, bs_cfx;
    const int32_t *status;         // [B] or null: nonzero -> NaN outputs
};
int launch_big_rest(const BigRest &r, int64_t B, hipStream_t s);

// theta-batched step on items that are already on the device, their number read from device memory (ssmq_api_theta.hip; used by the
// device-resident rounds of ssmq_gp_marginal_filter_batch, ssmq_marginal_device.hip)
struct ThetaDev {
    int Din, D, Y, Nd, No;
    int64_t cap, ld;                                     // items the arena holds; plane pitch
    double *pard, *paro, *mean, *cov, *ysoa, *tt;        // per item, filled by the caller: kernel parameters [cap][1 + Din] / [cap][1 + D],
                                                         // state moments [cap][Din] / [cap][Din Din], measurement planes [Y][ld], time [ld]
    double *m_fi, *P_fi, *ll;                            // results: planes [D][ld], [D D][ld], log-likelihood [ld]
    int32_t *st_all;                                     // merged status flags [ld]
    double *xid, *xio, *gq, *rr, *cd, *co, *mid;         // internal: unit points, noise terms, constant blocks, work planes
    int32_t *st5;
};
bool theta_dev_supported(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs);
size_t theta_dev_bytes(const ssmq_transform *h_dyn, const ssmq_transform *h_obs, int64_t cap);
size_t theta_dev_carve(ThetaDev &t, const ssmq_transform *h_dyn, const ssmq_transform *h_obs, int64_t cap, void *base);
int theta_dev_upload_static(const ThetaDev &t, const ssmq_transform *h_dyn, const ssmq_transform *h_obs, const double *GQG, const double *R,
                            hipStream_t s);
int theta_dev_enqueue(const ThetaDev &t, const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                      const ssmq_integrand *f_obs, double jitter, int64_t bound, const int32_t *d_count, hipStream_t s);

// One call of ssmq_gp_marginal_filter_batch as its routes take it: the entry point's arguments under their names (include/ssmq.h).
struct MarginalCall {
    ssmq_transform *h_dyn;
    const ssmq_integrand *f_dyn;
    ssmq_transform *h_obs;
    const ssmq_integrand *f_obs;
    int64_t B;
    int T;
    double jitter;
    const double *y, *x0_mean, *x0_cov, *q_mean, *q_cov, *GQG, *R, *prior_mean, *prior_cov, *upts, *uwts;
    int NP;
    double fd_step, param_jitter;
    double *fm, *fP;
    int32_t *failed;
    double *theta_last, *pcov_last;
    int64_t *stats;
};
// The state machines on the device (ssmq_marginal_device.hip): SSMQ_OK having produced everything, SSMQ_E_UNSUPPORTED if this shape
// has no device-resident route (the caller, ssmq_marginal.hip, then runs the host rounds), or an error.
int marginal_filter_batch_device(const MarginalCall &c);

// trajectory / measurement simulator (ssmq_simulate.hip)
struct SimRv {
    int kind, dim, ncomp, off;      // off: doubles into the constants block (alpha | mean | chol)
    double dof;
};
struct SimLaunch {
    int mode, D, Y, dq, dr, dyn_additive, obs_additive, T, continuous, g_off;
    double dt;
    int64_t B, ld;
    uint64_t seed, traj_offset;
    SimRv rv[3];                    // initial state, process noise, measurement noise
    const ssmq_integrand *f_dyn, *f_obs;
    const double *d_consts;
    double *d_x, *d_y;
};
int launch_simulate(const SimLaunch &h, hipStream_t s);
bool has_continuous_dynamics(int fid);

// measurement update, moment augmentation, log-density and backward pass (ssmq_filter.hip)
int launch_kalman_update(int D, int Y, int64_t B, int64_t ld, const double *m_pr, const double *P_pr,
                         const double *y_mean, const double *P_y, const double *P_yx, const double *y, double *m_fi,
                         double *P_fi, int32_t *status, hipStream_t s);
int launch_kalman_update_ex(int D, int Y, int64_t B, int64_t ld, const double *m_pr, const double *P_pr, const double *y_mean,
                            const double *P_y, const double *P_yx, const double *y, double *m_fi, double *P_fi, int32_t *status,
                            const int32_t *st_a, const int32_t *st_b, int step, hipStream_t s, double student_dof, double *smat_out,
                            int Dx);
int launch_augment(const double *m, const double *P, const double *nmean, const double *ncov, double *ma, double *Pa, int D, int Dn,
                   int64_t B, int64_t ld, hipStream_t s);
int launch_gauss_logpdf(int Y, int64_t B, int64_t ld, const double *y, const double *y_mean, const double *P_y, double *out,
                        hipStream_t s, const int32_t *merge = nullptr, int32_t *merge_out = nullptr);
int launch_rts_backward(int D, int64_t B, int64_t ld, int T, const double *fm, const double *fP, const double *pm, const double *pP,
                        const double *pC, double *sm, double *sP, int32_t *status, hipStream_t s, int c_cols);

// the filter time loop of the entry points (ssmq_api_filter.hip).  sscale (host, [T]) / student_dof: Studentian recursion, null / 0
// for the Gaussian filters; d_pm / d_pP / d_pC (all or none): the predictive moments of every step are kept for a backward pass.
int filter_forward_impl(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                        int64_t B, int64_t ld, int T, const double *d_y, const double *d_m0, const double *d_P0, const double *GQG,
                        const double *R, double *d_fm, double *d_fP, int32_t *d_status, const double *sscale, double student_dof,
                        double *d_pm = nullptr, double *d_pP = nullptr, double *d_pC = nullptr);

// One pass of the additive-noise filter time loop, as every launcher of the fused time loop takes it.  Pointers are device
// pointers.  A default-constructed pass with the handles, the integrands, sel_obs and B set is a valid dry-run query (dry_run = true).
struct FilterPass {
    const ssmq_transform *hd = nullptr;
    const ssmq_integrand *fd = nullptr;
    const ssmq_transform *ho = nullptr;
    const ssmq_integrand *fo = nullptr;
    int sel_obs = 0;                                              // sel_pattern() of the measurement integrand
    int64_t B = 0, ld = 0;
    int T = 0;
    const double *y = nullptr, *m0 = nullptr, *P0 = nullptr;      // [T][Y][ld], [D][ld], [D*D][ld]
    double *fm = nullptr, *fP = nullptr;                          // [T][D][ld], [T][D*D][ld]
    int32_t *status = nullptr;                                    // [B]
    const double *gqg = nullptr, *rr = nullptr;                   // [D*D], [Y*Y]
    const double *sscale = nullptr;                               // Studentian recursion: scale [T] and the filter's dof (null / 0: Gaussian)
    double student_dof = 0.0;
    const double *ttab_dyn = nullptr, *ttab_obs = nullptr;        // time tables [T] of the integrands that have one (has_time_table)
    hipStream_t s = nullptr;
    const char **name = nullptr;                                  // receives the kernel's name, or null
    bool dry_run = false;                                         // only say whether a kernel exists (and its name)
};
// The one place that builds a pass: looks the measurement integrand up (sel_obs; an id unknown to integrand_info() is
// SSMQ_E_ARG - the transforms of a launch loop would refuse it all the same) and sets every field, the constants (below), the
// Studentian dof, name and dry_run at their defaults.  ssmq_api_filter.hip.
int make_filter_pass(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                     int64_t B, int64_t ld, int T, const double *y, const double *m0, const double *P0, double *fm, double *fP,
                     int32_t *status, hipStream_t stream, FilterPass *out);
// The small per-pass constants of the time loop, ONE layout for every route:
//     gqg [D*D] | rr [Y*Y] | scale [T] | ttab_dyn [T] | ttab_obs [T] | steps [T]        (rounded up to 8 doubles)
// steps holds 0 .. T-1, the time argument of the launch loops (both transforms of step k + 1 use time index k, ssinf.py:104).
// The single-filter routes keep one block per context (ssmq_api_filter.hip: FilterCache), the multi-filter entry one per job
// side by side (MultiCache), the piped pass sends it as the third part of its m0 | P0 | constants transfer.
struct PassConsts {
    size_t rr, scale, ttab_dyn, ttab_obs, steps;   // where the segments start, in doubles (gqg at 0)
    bool has_scale, has_ttab_dyn, has_ttab_obs;    // the caller passed a scale; time_table() filled that table (T > 0)
};
inline size_t pass_consts_doubles(int D, int Y, int T) { return ((size_t)D * D + (size_t)Y * Y + 4 * (size_t)T + 7) / 8 * 8; }
// ... its host image: null GQG / R are zeros, a null scale is ones, an absent table and the padding are zeros
inline PassConsts fill_pass_consts(double *host, const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int T,
                                   const double *GQG, const double *R, const double *sscale) {
    PassConsts c;
    c.rr = (size_t)D * D; c.scale = c.rr + (size_t)Y * Y; c.ttab_dyn = c.scale + T; c.ttab_obs = c.ttab_dyn + T; c.steps = c.ttab_obs + T;
    std::fill(host, host + pass_consts_doubles(D, Y, T), 0.0);
    if (GQG) std::copy(GQG, GQG + c.rr, host);
    if (R) std::copy(R, R + (size_t)Y * Y, host + c.rr);
    for (int k = 0; k < T; ++k) {
        host[c.scale + k] = sscale ? sscale[k] : 1.0;
        host[c.steps + k] = (double)k;
    }
    c.has_scale = sscale != nullptr;
    c.has_ttab_dyn = T > 0 && time_table(f_dyn->id, T, host + c.ttab_dyn);
    c.has_ttab_obs = T > 0 && time_table(f_obs->id, T, host + c.ttab_obs);
    return c;
}
// ... and the pass's pointers into the block at `dev`; the kernels branch on a null scale / table
inline void wire_pass_consts(FilterPass &p, const double *dev, const PassConsts &c) {
    p.gqg = dev; p.rr = dev + c.rr; p.sscale = c.has_scale ? dev + c.scale : nullptr;
    p.ttab_dyn = c.has_ttab_dyn ? dev + c.ttab_dyn : nullptr; p.ttab_obs = c.has_ttab_obs ? dev + c.ttab_obs : nullptr;
}
// What a captured launch depends on, as words of a graph key: raw bytes of a struct ...
inline void key_bytes(std::vector<uint64_t> &key, const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i += 8) { uint64_t v = 0; memcpy(&v, b + i, std::min<size_t>(8, n - i)); key.push_back(v); }
}
// ... and everything about the two handles and the two integrands of a filter.  ssmq_transform_update keeps a handle's block
// addresses but may change the fast paths its constants qualify for (opt_mask) - and bumps `generation`.
inline void key_of_pair(std::vector<uint64_t> &key, const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                        const ssmq_integrand *f_obs) {
    for (const ssmq_transform *h : {h_dyn, h_obs}) {
        for (const void *p : {(const void *)h, (const void *)h->d_small, (const void *)h->d_mo, (const void *)h->d_trunc, (const void *)h->d_gpqd}) key.push_back((uint64_t)(uintptr_t)p);
        for (int v : {h->D, h->E, h->N, h->form, h->emv_mode, h->opt_mask, h->np_pad, (int)h->generation, (int)h->gq_mask}) key.push_back((uint64_t)(uint32_t)v);
        key_bytes(key, &h->tp_nu, 8);
    }
    key_bytes(key, f_dyn, sizeof(ssmq_integrand));
    key_bytes(key, f_obs, sizeof(ssmq_integrand));
}
// The one place that fills the kernels' argument block from a pass: everything zero but the pass's fields, lpw = 64
// (ssmq_filter_fused.hip).  A route states what it sets differently next to its launch.
FusedArgs fused_args(const FilterPass &p);
// both transforms of one form (sigma-point, BQ or t-process BQ), a measurement index pattern the kernels know, no state index list;
// the Taylor-GPQD, the truncated sigma-point and the GPQ+D form are no family by name: no time-loop kernel (fused, strips, quad, wave split,
// time blocks) reads their parameters
inline bool same_family(const FilterPass &p) {
    return !is_gpqd(p.hd) && !is_gpqd(p.ho) && !is_taylor_gpqd(p.hd) && !is_taylor_gpqd(p.ho) && !is_trunc(p.hd) && !is_trunc(p.ho) && p.hd->form == p.ho->form && (p.hd->tp_nu > 0.0) == (p.ho->tp_nu > 0.0) && p.sel_obs >= 0 && p.fd->n_idx <= 0;
}
// Integrands whose time dependence the fused loops read from a per-step table (time_table() in ssmq_device.h fills it); the kernels'
// HasTimeTable<> (ssmq_fused.h) is checked against this function id by id in ssmq_filter_shapes.h.
constexpr bool has_time_table(int fid) { return fid == SSMQ_F_UNGM_DYN || fid == SSMQ_F_UNGMNA_DYN; }
// What the tables of the time-loop kernels are keyed by (the template arguments of an instantiation)
struct FilterShape {
    int fd, fo, D, Y, ND, NO, form, tp, selo, opt;
    bool operator==(const FilterShape &o) const {
        return fd == o.fd && fo == o.fo && D == o.D && Y == o.Y && ND == o.ND && NO == o.NO && form == o.form && tp == o.tp &&
               selo == o.selo && opt == o.opt;
    }
};
// ... of k_filter_score<> (ssmq_filter_score.hip): the shape and the recursion (stu 1: Studentian)
struct ScoreShape : FilterShape {
    int stu;
    bool operator==(const ScoreShape &o) const { return FilterShape::operator==(o) && stu == o.stu; }
};
// ... and the key of a pass (same_family) with fast path `opt`
inline FilterShape shape_of(const FilterPass &p, int opt) {
    return {p.fd->id, p.fo->id, p.hd->D, p.ho->E, p.hd->N, p.ho->N, p.hd->form, p.hd->tp_nu > 0.0 ? 1 : 0, p.sel_obs, opt};
}

// the whole time loop in one kernel: 1 launched (dry_run: a kernel exists, its name set), 0 no kernel for this combination, < 0 error
// (ssmq_filter_fused.hip, which tries the schedules of ssmq_filter_quad.hip, ssmq_filter_wsplit.hip and ssmq_filter_chunked.hip;
// cus: compute units of the device)
int try_launch_fused(const FilterPass &p);
int try_launch_quad(const FilterPass &p, int cus);
int try_launch_ungm_quad(const FilterPass &p, int64_t waves);      // (try_launch_quad's entry for the scalar UNGM shapes: ssmq_filter_ungm_quad.hip)
int try_launch_wsplit(const FilterPass &p, int cus);
int try_launch_chunked(const FusedArgs &a0, const FilterShape &shape, int cus, hipStream_t s, bool dry_run, const char **name);
// ... for models that take their noise as an argument, and for the smoother (p.gqg / p.rr are not read)
struct AugExtras {
    int D, dq, dr;                            // state dimension; dimensions of the noise inputs (0: that model is additive)
    const double *add_dyn, *add_obs;          // [D*D] / [Y*Y]: G Q G' / R for an additive model, zeros otherwise
    const double *noise;                      // q_mean[dq] | q_cov[dq*dq] | r_mean[dr] | r_cov[dr*dr]
    double *pm, *pP, *pC;                     // all or none: predictive moments of every step, kept for the backward pass
};
int try_launch_fused_aug(const FilterPass &p, const AugExtras &x);
// ... and for the extended Kalman filter of a pair of built-in models (both handles a linearisation; ssmq_filter_ekf.hip: k_ekf_loop),
// which try_launch_fused asks first; pm / pP / pC (all or none): the predictive moments of every step are kept for the smoother
int try_launch_ekf_loop(const FilterPass &p, double *pm, double *pP, double *pC);
// ... several filters of one model family as one launch (ssmq_filter_fused.hip; ssmq_filter_forward_multi_dev)
int multi_family_table(int n, const ssmq_transform *const *hd, const ssmq_integrand *const *fd, const ssmq_transform *const *ho,
                       const ssmq_integrand *const *fo, const FusedArgs *args, std::vector<char> *table, int *blocks);
int multi_family_launch(const char *table, int blocks, hipStream_t s);
// ... and the steps [kb, ke) of every trajectory (ssmq_filter_piped.hip; ssmq_filter_forward_piped); hand: range_hand_doubles(D)
// doubles per block of 64 trajectories
int try_launch_range(const FilterPass &p, int kb, int ke, double *hand);
size_t range_hand_doubles(int D);

// Innovation scores of a pass whose fm / fP hold the FILTERED moments (inputs here; ssmq_innovation.hip, ssmq_filter_innovations_dev):
// the planes of all T steps, ymean / S null = not stored
struct InnovOut {
    double *ymean, *S;                        // [T][Y][ld], [T][Y*Y][ld] or null
    double *nis, *ll;                         // [T][ld]
};
struct InnovArgs;                             // ssmq_innovation_kernel.h (k_innovation<>: ssmq_score_step.h)
InnovArgs innov_args(const FilterPass &p, const InnovOut &o);
// all T B items in one launch of k_innovation<>: 1 launched (dry_run: a kernel exists, its name set), 0 no kernel for this pair,
// < 0 error; a pair with a user integrand runs the instantiation compiled for it at run time (ssmq_rtc.hip) or is an error
int try_launch_innovation(const FilterPass &p, const InnovOut &o);
int rtc_launch_innovation(const FilterPass &p, const InnovOut &o);
// one step of the launch-loop route: scores from the planes the step's two transforms left (st_a / st_b: their status planes,
// m_in: the mean the step started from); ymean / S / nis / ll: the planes of this step
int launch_innovation_score(int D, int Y, int64_t B, int64_t ld, const double *y, const double *y_mean, const double *P_y,
                            const double *m_in, const int32_t *st_a, const int32_t *st_b, double *ymean, double *S, double *nis,
                            double *ll, hipStream_t s);
// total [2][ld]: sum of ll, mean of nis over the steps in ascending order; status [B]: 1 + first step with NaN scores, or 0
int launch_innovation_total(int64_t B, int64_t ld, int T, const double *nis, const double *ll, double *total, int32_t *status,
                            hipStream_t s);

// The likelihood-scoring entry points (ssmq_api_sweep.hip, ssmq_api_score.hip, ssmq_api_noise_sweep.hip, ssmq_api_imm.hip).
// The model checks their routes share, in the order every one of them makes them: no user-defined integrand; own() - the entry
// point's checks that come next (nonzero: its refusal, already reported); known integrand ids; additive noise, D -> D dynamics
// without an index list.  refuse(code, text) is the entry point's refusal, w the name it reports under.  *selo: sel_pattern() of the
// measurement integrand (< 0: no kernel reads that pattern).
template <class Refuse, class Own>
int additive_pair_route(Refuse refuse, const std::string &w, const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, Own own, int *selo) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs))
        return refuse(SSMQ_E_UNSUPPORTED, w + ": user-defined models (device_code) are not implemented");
    if (int rc = own()) return rc;
    FInfo fid, fio;
    if (!integrand_info(f_dyn->id, &fid) || !integrand_info(f_obs->id, &fio)) return refuse(SSMQ_E_ARG, w + ": unknown integrand id");
    if (f_dyn->id == SSMQ_F_UNGMNA_DYN || f_dyn->id == SSMQ_F_CTRS_DYN || f_obs->id == SSMQ_F_UNGMNA_MEAS || fid.din != D || fid.dout != D ||
        f_dyn->n_idx > 0)
        return refuse(SSMQ_E_UNSUPPORTED, w + ": models that take their noise as an argument (non-additive noise) are not implemented");
    *selo = sel_pattern(f_obs, fio.din);
    return SSMQ_OK;
}
// T == 0, the row entry points: nothing to score - empty sums, status 0; a failed row is still a failed row (theta_status: host [P]
// or null; NaN, -1).  Synchronous.  (ssmq_api_score.hip)
int score_empty(const char *who, int P, int64_t ld, const int32_t *theta_status, double *d_ll_total, double *d_nis_mean, int32_t *d_status);
// A host image on the device for the length of one call: uploaded asynchronously on stream(), so the launch that follows on that
// stream reads the copy; freed when the scope ends, on every path - the caller synchronises the stream before that.
struct DeviceImage {
    double *dev = nullptr;
    DeviceImage() = default;
    DeviceImage(const DeviceImage &) = delete;
    DeviceImage &operator=(const DeviceImage &) = delete;
    ~DeviceImage() {
        if (dev) hipFree(dev);
    }
    int alloc(size_t doubles) {
        SSMQ_HIP(hipMalloc((void **)&dev, sizeof(double) * doubles));
        return SSMQ_OK;
    }
    int upload(const std::vector<double> &host, const char *what) {
        return hip_fail(hipMemcpyAsync(dev, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, stream()), what);
    }
};

// The measurement-update variants of the additive-noise Gaussian filters - the iterated posterior linearisation pass
// (ssmq_filter_iterated.hip: `iterations` updates per step, each re-linearised around the current posterior), the outlier-robust pass
// (ssmq_filter_robust.hip: Student-t noise of scale R and `dof` degrees of freedom, `iterations` - 1 rounds of its fixed point per
// step) and the masked pass (ssmq_filter_masked.hip: the components a bit mask marks as observed, behind a chi-square gate).  The
// robust and the masked pass are built WITHOUT R (p.rr: zeros - the measurement transform adds no noise); R | R^-1 and R | gate travel
// in their own structs, device pointers.  try_launch_*: the whole pass in one launch of k_*_loop<>: 1 launched (dry_run: a kernel
// exists, its name set), 0 no kernel for this pair, < 0 error; a pair with a user integrand runs the instantiation compiled for it at
// run time (rtc_launch_pass) or is an error.  *_launch_loop: every other pair, through update_launch_loop.
struct IplfPass {
    int iterations;
    double *delta;                            // [T][ld] or null
};
struct RobustPass {
    int iterations;
    double dof;
    const double *rr, *ir;                    // [Y*Y] each
    double *lam, *delta;                      // [T][ld] each
};
struct MaskedPass {
    const uint32_t *mask;                     // [T][ld] or null: NaN = missing
    const double *rr, *gate;                  // [Y*Y], [Y+1]
    uint32_t *used;                           // [T][ld]
    double *nis, *ll;                         // [T][ld] each
};
int try_launch_iterated(const FilterPass &p, const IplfPass &r);
int try_launch_robust(const FilterPass &p, const RobustPass &r);
int try_launch_masked(const FilterPass &p, const MaskedPass &r);
int iterated_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, const IplfPass &r, const double *tvec, void *ws);
int robust_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, const RobustPass &r, const double *tvec, void *ws);
int masked_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, const MaskedPass &r, const double *tvec, void *ws);
// What the three share.  The launch loop (ssmq_filter.hip): per step apply dyn, then `napply` x (apply obs | item).  The first
// application of the measurement transform is at the prior, every later one at the iterate planes the item before it wrote; the last
// item writes plane k of p.fm / p.fP.  item(c, last): fills its per-item arguments from c (launch_item_update, ssmq_filter_shapes.h)
// and launches its kernel.  ws: update_ws_bytes() bytes, tvec: device [T] holding 0 .. T-1 (the pass's constants).  Plain launches
// on p.s, no graph.
struct ItemPlanes {
    const double *m_pr, *P_pr;        // the prior of the step
    const double *m_at, *P_at;        // where the measurement transform was applied: the prior, or the iterate
    const double *y_mean, *P_y, *P_yx, *y;
    double *m_out, *P_out;
    int32_t *status;
    const int32_t *st_dyn, *st_obs;
    int64_t B, ld;
    int32_t step, D, Y;
};
size_t update_ws_bytes(int D, int Y, int64_t ld);
int update_launch_loop(ssmq_transform *h_dyn, ssmq_transform *h_obs, const FilterPass &p, int napply, const double *tvec, void *ws,
                       const std::function<int(const ItemPlanes &c, bool last)> &item);
// A whole-pass kernel for a pair with a user member, compiled at run time (ssmq_rtc.hip): kind SSMQ_RTC_ITERATED, _ROBUST, _MASKED or
// _SMOOTHER_ITERATED; args: the kernel's argument block (fd, fo: its FPar members, B: its batch), the grid ceil(B / 64) of the AOT
// launchers.  Returns as try_launch_*.
int rtc_launch_pass(const FilterPass &p, int kind, void *args, FPar *fd, FPar *fo, int64_t B);
// k_detection_mask (ssmq_filter_masked.hip): p_detect host [Y], Y <= SSMQ_MAX_DIM
int launch_detection_mask(int64_t B, int64_t ld, int T, int Y, const double *p_detect, uint64_t seed, uint64_t traj_offset, int per_component,
                          uint32_t *d_mask, hipStream_t s);

// Iterated posterior linearisation smoother (ssmq_filter_ipls.hip, ssmq_smoother_iterated_dev): ONE iteration - the forward sweep and
// the backward sweep - is one launch of k_ipls_pass<> (ssmq_ipls_kernel.h).  The planes of an iteration besides those of the pass
// (p.fm / p.fP: its filtered moments, p.status: read and written): the linearisation moments it reads (both null: the running
// moments), the workspace the two sweeps share, the smoothed moments it writes, delta [ld] or null.  try_launch_ipls: 1 launched
// (dry_run: a kernel exists, its name set), 0 no kernel for this pair, < 0 error; a pair with a user integrand runs the
// instantiation compiled for it at run time (ssmq_rtc.hip) or is an error
struct IplsPlanes {
    const double *lin_m, *lin_P;   // [T+1][D][ld], [T+1][D*D][ld]
    double *pm, *pP, *pC;          // [T][D][ld], [T][D(D+1)/2][ld], [T][D*D][ld]
    double *sm0, *sP0, *sm, *sP;   // [D][ld], [D*D][ld], [T][D][ld], [T][D*D][ld]
    double *delta;
};
struct IplsArgs;                              // ssmq_ipls_kernel.h
IplsArgs ipls_args(const FilterPass &p, const IplsPlanes &q);
int try_launch_ipls(const FilterPass &p, const IplsPlanes &q);

// error sums over a batch of filtered trajectories (ssmq_metrics.hip)
int metrics_values_per_step(int D);
int metrics_chunks(int64_t B);
int metrics_left_bytes();      // per (step, chunk): the record of the entries left to the second pass
int launch_metrics(int phase, int D, int64_t B, int64_t ld, int T, const double *x, const double *fm, const double *fP,
                   const int32_t *status, const double *mse, double *partial, uint8_t *left, double *out, hipStream_t s);
int launch_metrics_indef(int phase, int D, int64_t B, int64_t ld, int T, const double *x, const double *fm, const double *fP,
                         const int32_t *status, const double *mse, double *partial, uint8_t *left, double *out, hipStream_t s);

// time-averaged scores of every trajectory (ssmq_metrics.hip: k_traj_scores); mse: device [T][D*D] or null
int launch_traj_scores(int D, int64_t B, int64_t ld, int T, int k0, const double *x, const double *fm, const double *fP,
                       const int32_t *status, const double *mse, double *scores, hipStream_t s);
// bootstrap variance of the mean of the rows of a [R][ld] block (ssmq_bootstrap.hip); the range the entry points accept
bool bootstrap_range_ok(int64_t n, int S, int R);

// the stages of the theta-batched step (ssmq_api_theta.hip): GP weights of every item as its own constant block
// (ssmq_weights.hip) ...
size_t gp_weights_wide_ws_bytes(int D, int N, int64_t P);
int gp_weights_wide_consts(int D, int E, int N, const double *d_xi, const double *d_par, int P, double jitter, double *d_consts,
                           int32_t *d_status, void *ws, size_t ws_bytes);
// ... or the two-launch route: both transforms' weights (ssmq_weights.hip: k_theta_weights), then transform -> transform -> update
// -> log-likelihood by the wave that owns the item (ssmq_apply_wide.hip: k_theta_chain) ...
bool gp_theta_weights_fits(int D0, int N0, int D1, int N1);
int gp_theta_weights_pair(const int D[2], const int E[2], const int N[2], const double *const d_xi[2], const double *const d_par[2],
                          int P, double jitter, double *const d_consts[2], int32_t *const d_status[2],
                          const int32_t *d_count = nullptr);
bool theta_chain_supported(int Din, int D, int Y, int Nd, int No);
hipError_t launch_theta_chain(const WideArgs &dyn, const WideArgs &obs, const UpdArgs &upd, const double *y, double *loglik,
                              const int32_t *merge, int32_t *merge_out, int64_t B, hipStream_t s, const int32_t *d_count = nullptr);
// ... and for the small systems one lane per item, everything in registers (ssmq_theta_item.hip)
bool theta_item_supported(int Din, int D, int Y, int Nd, int No);
int launch_theta_item(int Din, int D, int Y, int Nd, int No, const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int emv_dyn,
                      int emv_obs, const double *xid, const double *xio, const double *pard, const double *paro, const double *mean,
                      const double *cov, int64_t bs_mean, int64_t bs_cov, const double *ysoa, const double *time, int time_stride,
                      const double *gq, const double *rr, double jitter, double *m_fi, double *P_fi, double *ll, int32_t *st_all,
                      int64_t ld, int64_t bound, const int32_t *d_count, hipStream_t s);

}  // namespace ssmq
