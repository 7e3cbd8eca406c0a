/*
 * ssmq.h - C ABI of the MI355X-native sigma-point / Bayesian-quadrature moment-transform library (libssmq.so).
 *
 * This is the drop-in boundary for ONE path of jacobnzw/SSMToybox: the moment transform that the filters in
 * ssmtoybox/ssinf.py call twice per time step, plus the quadrature-weight construction that feeds it.  The reference
 * is pure Python and has no FFI; the entry points below are what a ctypes binding for that path would bind, and each
 * cites the reference interface (file:line under the reference tree) it replaces.  INTEGRATION.md shows the
 * reference-side stub.
 *
 * Conventions
 *   - plain C types only; all floating point is IEEE fp64 (`double`); integers are int32 unless stated.
 *   - host arrays are C-contiguous in the reference's NumPy layout ("AoS": trajectory-major, e.g. cov[b][i][j]).
 *   - device arrays handed to the *_dev entry points are in the library's HBM layout ("SoA planes"): element e of
 *     trajectory b lives at ptr[e * ld + b]; ld >= B is the plane pitch in doubles.  Matrices are row-major in e
 *     (e = i * ncol + j).  ssmq_aos_to_soa / ssmq_soa_to_aos convert on the device.
 *   - return value: 0 ok; > 0 = 1 + index of the first batch item whose input covariance is not positive definite
 *     (the reference raises numpy.linalg.LinAlgError there: bq/bqmtran.py:98, mtran.py:139); < 0 error
 *     (SSMQ_E_*); ssmq_last_error() gives the text.  No exception crosses the ABI.
 *   - a transform handle is bound to the device that was current when it was created.
 *     Threads (round 5): every calling thread has a CONTEXT of its own - one HIP stream and the caches that belong to a stream
 *     (grow-only workspaces, pinned staging blocks, captured launch graphs).  Calls of different threads on different handles
 *     run concurrently, on the host and - stream by stream - on the device.  A handle is locked for the duration of every
 *     entry point that takes it (two handles in address order), so calls of several threads on the SAME handle are safe and
 *     run one after the other; a thread that picks up a handle last used by another thread first waits for that thread's
 *     stream, so constants uploaded or buffers built there are complete.  The *_dev entry points queue on the CALLING
 *     thread's stream and return; ssmq_sync() / events / copies act on that stream.  Device buffers the caller hands from one
 *     thread to another are the caller's to order (ssmq_sync() in the thread that queued the work), as with any per-thread
 *     stream.  A thread that ends returns its context (stream and caches intact) to a pool for the next new thread.  The
 *     ssmq_comm_* entry points belong to one thread.  One process per GPU is the intended deployment: HIP's
 *     current device is per thread and starts at 0, so a thread's first call moves it to the device of the last
 *     ssmq_set_device(); a context that finds its thread on another device drops its caches and binds there.
 *   - there is NO CPU fallback anywhere behind this ABI: without a usable gfx950 device every compute entry point
 *     returns SSMQ_E_HIP.
 */
#ifndef SSMQ_H
#define SSMQ_H

#ifndef __HIPCC_RTC__   /* the run-time compiler (csrc/ssmq_rtc.hip) supplies these itself */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SSMQ_VERSION 102

#define SSMQ_OK 0
#define SSMQ_E_ARG (-1)          /* bad argument (null pointer, size out of range, unknown id) */
#define SSMQ_E_HIP (-2)          /* HIP runtime error / no device */
#define SSMQ_E_UNSUPPORTED (-3)  /* combination not implemented */
#define SSMQ_E_NOMEM (-4)

#define SSMQ_MAX_FPAR 16 /* doubles of integrand constants */
#define SSMQ_MAX_FIDX 16 /* state-index entries (= SSMQ_MAX_DIM: any sub-state of any state) */
#define SSMQ_MAX_DIM 16  /* D, E (input / output dimension of a transform) */
#define SSMQ_MAX_PTS 4096 /* N (sigma points) */

/* Integrands: closed-form dynamics / measurement functions of ssmtoybox/ssmod.py evaluated on the device so sigma
 * points never leave the GPU (bq/bqmtran.py:132-156 evaluates a Python callable column by column). */
enum ssmq_integrand_id {
    SSMQ_F_UNGM_DYN = 1,          /* ssmod.py:268-269   par: -            in 1 out 1, uses time          */
    SSMQ_F_UNGM_MEAS = 2,         /* ssmod.py:1060-1061 par: -            in 1 out 1                     */
    SSMQ_F_UNGMNA_DYN = 3,        /* ssmod.py:299-300   input [x, q]      in 2 out 1, uses time          */
    SSMQ_F_UNGMNA_MEAS = 4,       /* ssmod.py:1085-1086 input [x, r]      in 2 out 1                     */
    SSMQ_F_PENDULUM_DYN = 5,      /* ssmod.py:357-358   par: dt           in 2 out 2                     */
    SSMQ_F_PENDULUM_MEAS = 6,     /* ssmod.py:1114-1115                   in 1 out 1                     */
    SSMQ_F_REENTRY1D_DYN = 7,     /* ssmod.py:424-427   par: dt           in 3 out 3                     */
    SSMQ_F_RANGE_MEAS = 8,        /* ssmod.py:1147-1149                   in 1 out 1                     */
    SSMQ_F_REENTRY2D_DYN = 9,     /* ssmod.py:530-564   par: dt           in 5 out 5                     */
    SSMQ_F_RADAR2D_MEAS = 10,     /* ssmod.py:1227-1252 par: loc_x loc_y  in 2 out 2                     */
    SSMQ_F_CT_DYN = 11,           /* ssmod.py:675-690   par: dt           in 5 out 5                     */
    SSMQ_F_BEARING_MEAS = 12,     /* ssmod.py:1189-1195 par: S x (sx, sy) in 2 out S (S = n_par / 2 <= 8) */
    SSMQ_F_CTRS_DYN = 13,         /* ssmod.py:755-774   par: dt, input [x(5), q(2)]  in 7 out 5          */
    SSMQ_F_CV_DYN = 14,           /* ssmod.py:839-846   par: dt           in 4 out 4                     */
    SSMQ_F_REENTRY2D_BIAS_DYN = 15, /* this build's synthetic 6-D case: reentry-2D + pass-through state, in 6 out 6 */
    SSMQ_F_SMOOTH10D_DYN = 16      /* this build's synthetic 10-D case (the reference has no model above 7 inputs; Bayes-Sard
                                      quadrature at D = 10 is BASELINE config 5): out[i] = sin(x[i]) + x[5+i]^2,
                                      out[5+i] = x[5+i] cos(x[i]), i = 0..4; in 10 out 10; no state index */
};

/*
 * User-defined integrands, compiled for the device at run time (csrc/ssmq_rtc.hip, ROCm's hiprtc).  A model's function body
 * is registered once and gets an id in [SSMQ_F_USER_FIRST, SSMQ_F_USER_FIRST + SSMQ_F_USER_SLOTS); the body is placed inside
 *     template <int E> __device__ void eval(const double *x, double *o) const { const double t = ..; const double *p = ..; { BODY } }
 * with x the `din` inputs, o the `dout` outputs, t the time index the built-in integrands receive and p the n_par constants of
 * ssmq_integrand.par; it may call the helpers of csrc/ssmq_math.h / ssmq_device.h (sin_nr, sincos_nr, atan2_nr, exp_nr, div_nr,
 * sqrt_rsqrt) and the device math functions.  At most SSMQ_USER_BODY_MAX characters, braces balanced, no preprocessor lines.
 * Idempotent: the same (body, din, dout) returns the same id.  1 <= din, dout <= SSMQ_MAX_DIM.
 * User ids run on: ssmq_filter_forward_dev / ssmq_student_filter_forward_dev (additive noise; the whole-pass kernel compiled for
 * the pair of models, D <= 6, Y <= 4, ND, NO <= 2 D + 1, no state index) and ssmq_apply_batch[_dev] / ssmq_apply_kernel_name
 * (k_apply_small, the same shape range), and ssmq_mc_transform_dev (k_mc_moments, D <= 6, E <= 6, no state index).  Every other
 * entry point that takes an ssmq_integrand returns SSMQ_E_UNSUPPORTED.
 * Compiled kernels are cached in the process (key: body hashes, kernel, template arguments, device architecture).
 */
#define SSMQ_F_USER_FIRST 1024
#define SSMQ_F_USER_SLOTS 64
#define SSMQ_USER_BODY_MAX 8192
#define SSMQ_USER_MAX_D 6
#define SSMQ_USER_MAX_Y 4
int ssmq_integrand_define(const char *body, int din, int dout, int uses_time, int32_t *id);
/* The same with the model's Jacobian: `jac_body` is placed inside
 *     __device__ void jac(const double *x, double *J, const int ldj) const { const double t = ..; const double *p = ..; { JAC_BODY } }
 * and sets J[e * ldj + k] = d o_e / d x_k for the `din` inputs; all dout x din entries are zero on entry, so a sparse Jacobian
 * writes its non-zeros only.  The same rules as `body`.  Idempotent on (body, jac_body, din, dout); the ids differ from the id
 * ssmq_integrand_define gives the same body, and between two Jacobians of one body.  Pass uses_time != 0 if either body reads t.
 * Such an id runs everywhere a user id runs and, in addition, on linearisation (ssmq_transform_create_linear) and Taylor-GPQD
 * handles: ssmq_apply_batch[_dev] (k_linearize_fn / k_taylor_gpqd_fn, compiled for (id, D, E, din), D <= 6, E <= max(D, 4), no
 * state index; ssmq_taylor_gpqd_variance_planes applies) and ssmq_filter_forward_dev with both handles of these forms (the
 * launch loop; the other member may be a built-in integrand that has a Jacobian).  The Jacobian lands in the `din` leading
 * columns of the E x D matrix, the other columns are zero - the broadcast of a one-column Jacobian into every column that the
 * built-in pendulum measurement inherits from the reference is not applied to user integrands.  A user id without a Jacobian
 * is SSMQ_E_UNSUPPORTED on these handles. */
int ssmq_integrand_define_dx(const char *body, const char *jac_body, int din, int dout, int uses_time, int32_t *id);
/* Compile only (no device needed): kind SSMQ_RTC_FILTER instantiates k_filter_fused<D, E (= Y), N, N_obs, id, id_obs, form, tp,
 * 0, opt> (id_obs: any integrand id), SSMQ_RTC_APPLY k_apply_small<D, E, N, id, form, tp, 0, opt> (id_obs, N_obs ignored), for
 * `arch` (e.g. "gfx950").  On success `log` gets the lowered kernel name on its first line, then the compiler's resource
 * remarks (registers, spills); on failure the compiler log.  Returns SSMQ_OK, SSMQ_E_ARG or SSMQ_E_UNSUPPORTED (compile error). */
/* SSMQ_RTC_MC instantiates the streaming Monte-Carlo kernel k_mc_moments<id, D, E, 0> (N, N_obs, form, tp, opt ignored). */
/* SSMQ_RTC_LINEAR / SSMQ_RTC_TAYLOR_GPQD instantiate k_linearize_fn / k_taylor_gpqd_fn<id, D, E, din> for an id that has a
 * Jacobian (N, N_obs, form, tp, opt ignored); an id without one is SSMQ_E_UNSUPPORTED. */
/* SSMQ_RTC_GPQD instantiates the GPQ+D kernel of a user id that has a Jacobian: k_apply_gpqd<id, D, E, din> for D <= 2,
 * k_apply_gpqd_lds<id, D, E, din> beyond (D <= 6, E <= max(D, 4); N, N_obs, form, tp, opt ignored). */
/* SSMQ_RTC_INNOVATION instantiates the innovation-score kernel k_innovation<D, E (= Y), N, N_obs, id, id_obs, form, tp, 0, opt>
 * (arguments as SSMQ_RTC_FILTER). */
/* SSMQ_RTC_ITERATED instantiates the iterated-pass kernel k_iplf_loop<D, E (= Y), N, N_obs, id, id_obs, form, tp, 0, 0> (arguments as
 * SSMQ_RTC_FILTER; opt must be 0: the dense kernel is the only one). */
/* SSMQ_RTC_SMOOTHER_ITERATED instantiates the iterated-smoother kernel k_ipls_pass<D, E (= Y), N, N_obs, id, id_obs, form, tp, 0>
 * (arguments as SSMQ_RTC_FILTER; opt must be 0: the dense transforms are the only ones). */
/* SSMQ_RTC_PCRLB_DYN / SSMQ_RTC_PCRLB_OBS instantiate the two kernels of the posterior Cramer-Rao sums (ssmq_pcrlb_sums_dev) for a
 * user id that has a Jacobian: k_pcrlb_dyn_fn<id, D, din> (a D -> D model: E is not read) and k_pcrlb_obs_fn<id, D, E, din> (N, N_obs, form,
 * tp, opt ignored); an id without a Jacobian, D > 6 or E > 4 (measurement) is SSMQ_E_UNSUPPORTED. */
/* SSMQ_RTC_IMM instantiates the IMM kernel k_imm_loop<D, E (= Y), N, N_obs, id, id_obs, SELO, form, tp> of two built-in integrands
 * (ssmq_filter_imm_dev); `opt` carries SELO (0: the measurement reads the leading states, 1: states 0, 2, 4, ...). */
/* SSMQ_RTC_ROBUST instantiates the outlier-robust kernel k_robust_loop<D, E (= Y), N, N_obs, id, id_obs, form, tp, 0, 0> (arguments as
 * SSMQ_RTC_FILTER; opt must be 0: the dense kernel is the only one). */
/* SSMQ_RTC_MASKED instantiates the masked-pass kernel k_masked_loop<..> with the same arguments (opt must be 0). */
enum ssmq_rtc_kind { SSMQ_RTC_FILTER = 0, SSMQ_RTC_APPLY = 1, SSMQ_RTC_MC = 2, SSMQ_RTC_LINEAR = 3, SSMQ_RTC_TAYLOR_GPQD = 4, SSMQ_RTC_GPQD = 5,
                     SSMQ_RTC_INNOVATION = 6, SSMQ_RTC_ITERATED = 7, SSMQ_RTC_SMOOTHER_ITERATED = 8, SSMQ_RTC_PCRLB_DYN = 9,
                     SSMQ_RTC_PCRLB_OBS = 10, SSMQ_RTC_IMM = 11, SSMQ_RTC_ROBUST = 12, SSMQ_RTC_MASKED = 13 };
int ssmq_rtc_compile_check(int32_t id, int32_t id_obs, int kind, int D, int E, int N, int N_obs, int form, int tp, int opt,
                           const char *arch, char *log, int len);
/* Process-wide counters of the run-time compiler: programs compiled, kernel lookups served from the cache, compile wall time. */
int ssmq_rtc_stats(int64_t *compiles, int64_t *cache_hits, double *compile_seconds);

/* One integrand = id + constants + optional sub-state selection (MeasurementModel.state_index, ssmod.py:990-991):
 * if n_idx > 0 the integrand sees x[idx[0]], x[idx[1]], ... of the D-dimensional sigma point. */
typedef struct ssmq_integrand {
    int32_t id;
    int32_t n_par;
    int32_t n_idx;
    int32_t reserved;
    double par[SSMQ_MAX_FPAR];
    int32_t idx[SSMQ_MAX_FIDX];
} ssmq_integrand;

/* Form of the moment equations. */
enum ssmq_form {
    SSMQ_FORM_BQ = 0,    /* bq/bqmtran.py:158-223: mean = fx wm; cov = fx Wc fx' - mean mean' + emv; ccov = fx Wcc' L' */
    SSMQ_FORM_SIGMA = 1, /* mtran.py:141-149: centred, diagonal Wc: cov = dfx diag(wc) dfx'; ccov = dfx diag(wc) (x-m)' */
    SSMQ_FORM_TAYLOR1 = 2, /* mtran.py:49-59 (LinearizationTransform): mean = f(m); J = df/dx(m); ccov = J cov; cov = ccov J'.
                             Handles of this form come from ssmq_transform_create_linear only */
    SSMQ_FORM_BQ_MO = 3, /* multi-output BQ (bq/bqmtran.py:425-602): one weight set per output and output pair -
                            mean_i = fx_i wm_i; cov_ij = fx_i Wc_ij fx_j' - mean_i mean_j + delta_ij emv_i; ccov_i = fx_i Wcc_i' L'.
                            Handles of this form come from ssmq_transform_create_mo only */
    SSMQ_FORM_TAYLOR_GPQD = 4, /* mtran.py:668-701 (TaylorGPQDTransform): the linearisation read as single-point GP quadrature with
                            derivative observations and an RBF kernel - mean = wm f(m); cov = wc (f f' + J Wc J') - mean mean' +
                            model_var; ccov = J cov (Lam + cov)^-1 Lam.  Handles of this form come from
                            ssmq_transform_create_taylor_gpqd only */
    SSMQ_FORM_TRUNC_SIGMA = 5, /* mtran.py:588-658 (TruncatedSigmaPointTransform): mean and cov from a sigma-point rule of the effective
                            dimension on the leading block of the input moments, ccov from the rule of the full dimension.  Handles
                            of this form come from ssmq_transform_create_truncated only */
    SSMQ_FORM_GPQD = 6 /* research/gpqd/gpqd_base.py (GaussianProcessDerTransform): the BQ moment equations on the integrand's values
                            at all sigma points and the rows of J(x_n) L at a subset of them.  Handles of this form come from
                            ssmq_transform_create_gpqd only */
};

/* How the expected model variance enters the covariance (bq/bqmtran.py:198 `model_var * I_out`). */
enum ssmq_emv_mode {
    SSMQ_EMV_DIAG = 0,      /* I_out = eye(E): only the diagonal of the (E, E) emv matrix is added            */
    SSMQ_EMV_BROADCAST = 1  /* I_out = eye(1) with E > 1 (ssinf.py StudentProcessKalman builds its transforms so):
                               the whole (E, E) matrix is added                                                 */
};

typedef struct ssmq_transform ssmq_transform; /* opaque; replaces the attribute carriers BQTransform / Model
                                                 (bq/bqmtran.py:11-58, bq/bqmod.py:15-106) on the device side */

/* ---- library / device ------------------------------------------------------------------------------------- */
int ssmq_version(void);
const char *ssmq_last_error(void);
int ssmq_device_count(int *n);
int ssmq_set_device(int device);
/* The device the library's stream and caches live on (the calling thread's current device on first use), -1 on error.
 * The HIP current device is PER THREAD: a caller that enters the library from a second thread selects this device there
 * first (ssmq_set_device), otherwise the library would move to that thread's default device. */
int ssmq_current_device(void);
int ssmq_device_name(char *buf, int len);
/* PCI bus id ("0000:c1:00.0", len >= 13) of that device: what tells N ranks of one node apart in a scaling record. */
int ssmq_device_pci_bus_id(char *buf, int len);

/* ---- device memory, layout conversion, timing (plumbing) ---------------------------------------------------- */
int ssmq_malloc(void **dptr, size_t bytes);
int ssmq_free(void *dptr);
int ssmq_memcpy_h2d(void *dst, const void *src, size_t bytes);
int ssmq_memcpy_d2h(void *dst, const void *src, size_t bytes);
int ssmq_memcpy_d2d(void *dst, const void *src, size_t bytes);
int ssmq_memset(void *dptr, int value, size_t bytes);
int ssmq_sync(void);
/* AoS [B][n] (reference layout) <-> SoA planes [n][ld] (HBM layout), both on the device. */
int ssmq_aos_to_soa(const double *d_aos, double *d_soa, int n, int64_t B, int64_t ld);
int ssmq_soa_to_aos(const double *d_soa, double *d_aos, int n, int64_t B, int64_t ld);
/* Host arrays in the reference's study layout (n_elem..., n_outer, B) - dim_y x T x B measurements, D x T x B means,
 * D x D x T x B covariances of forward_pass / the Monte-Carlo loops (ssinf.py:66-118, research/tpq/tpq_base.py:175-192) -
 * to / from the filters' time-major planes [n_outer][n_elem][ld] in HBM.  Transfers go through the library's pinned
 * staging block in chunks; padding lanes (B .. ld) are zero-filled on upload.  Synchronous. */
int ssmq_upload_planes(const double *host, int n_outer, int n_elem, int64_t B, int64_t ld, double *d_planes);
int ssmq_download_planes(const double *d_planes, int n_outer, int n_elem, int64_t B, int64_t ld, double *host);
/* HIP events on the library's stream (bench.py times kernels with these). */
int ssmq_event_create(void **ev);
int ssmq_event_destroy(void *ev);
int ssmq_event_record(void *ev);
int ssmq_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */
/* index of the first non-zero entry of a device status vector, or -1 */
int ssmq_status_first(const int32_t *d_status, int64_t B, int64_t *first);

/* ---- quadrature weights (theta-batched, computed on the device) --------------------------------------------- */
/*
 * GP quadrature weights for P kernel-parameter rows at once.
 * Replaces GaussianProcessModel.bq_weights (bq/bqmod.py:495-523) together with RBFGauss.eval / exp_x_kx / exp_x_xkx /
 * exp_x_kxkx / exp_x_kxx / exp_xy_kxy (bq/bqkern.py:329-424), utils.maha (utils.py:385-409) and
 * Kernel.eval_inv_dot / _cho_inv (bq/bqkern.py:38-64, 96-120).
 *   xi  [D*N]      unit sigma points, row-major (D, N)            (host)
 *   par [P*(1+D)]  rows [alpha, ell_1..ell_D]                     (host)
 * outputs (host; any may be NULL): wm [P*N], Wc [P*N*N], Wcc [P*D*N], iK [P*N*N] (scaling=False inverse),
 *   q [P*N], Q [P*N*N], R [P*D*N], model_var [P], integral_var [P], status [P] (1 = K + jitter I not PD).
 */
int ssmq_weights_gp(int D, int N, const double *xi, const double *par, int P, double jitter,
                    double *wm, double *Wc, double *Wcc, double *iK, double *q, double *Q, double *R,
                    double *model_var, double *integral_var, int32_t *status);
/*
 * The kernel-level methods of the reference as entry points of their own (the weights entry points build K, its inverse
 * and the expectations in one kernel and need none of these):
 *   ssmq_rbf_eval      RBFGauss.eval (bq/bqkern.py:329-343, utils.maha utils.py:385-409): K [P][N1][N2] between the
 *                      point sets x1 [D*N1], x2 [D*N2] (NULL: x1); scaling = use alpha; diag: N1 values k(x1_i, x2_i)
 *                      through the difference form of the reference's diag branch.
 *   ssmq_rbf_factor    Kernel.eval_chol (bq/bqkern.py:122-142): chol [P][N][N], lower factor of K + jitter I, and / or
 *                      Kernel.eval_inv_dot / _cho_inv (:38-64, 96-120): iK [P][N][N] = sym((K + jitter I)^-1 rhs), rhs [N][N]
 *                      or NULL (= I; the reference symmetrises whatever it solved for, so a right-hand side is square);
 *                      chol or iK may be NULL; status [P] / return value as ssmq_weights_gp.
 *   ssmq_rbf_exp_kxkx  RBFGauss.exp_x_kxkx for two (possibly different) parameter rows (:366-415): Q [N][N].
 */
int ssmq_rbf_eval(int D, int N1, const double *x1, int N2, const double *x2, const double *par, int P, int scaling,
                  int diag, double *K);
int ssmq_rbf_factor(int D, int N, const double *x, const double *par, int P, int scaling, double jitter,
                    const double *rhs, double *chol, double *iK, int32_t *status);
int ssmq_rbf_exp_kxkx(int D, int N, const double *x, const double *par0, const double *par1, int scaling, double *Q);

/*
 * The 'rbf-student' kernel (RBFStudent, bq/bqkern.py:457-536): the RBF kernel with its expectations under a standard
 * multivariate Student-t density with dof degrees of freedom, estimated by Monte Carlo on the device.  Sample s is x = z /
 * sqrt(u), z ~ N(0, I_D), u ~ Gamma(dof / 2, scale 2 / dof) (utils.py:349-382), drawn by the counter-based generator of the
 * simulator as a function of (seed, s) alone.
 *   ssmq_rbf_student_expect  exp_x_kx, exp_x_xkx and exp_x_kxkx (scaling=False) from ONE set of num_samples samples (the
 *                            reference draws three): q [N] = E[k0], R [D][N] = E[x k0'], Q [N][N] with Q[i][j] = E[k1_i k0_j],
 *                            k0 / k1 the kernel at par0 / par1 [1 + D] (par1 NULL or equal to par0: one kernel; Q is then
 *                            symmetric bit for bit).  Any output may be NULL.
 *   ssmq_rbf_student_kxy     exp_xy_kxy as the reference estimates it (:529-536): 10 000 batches of 200 samples, per batch the
 *                            sum of alpha^2 k(x_a, x_b) over all 200 x 200 pairs (diagonal included), the total divided by
 *                            num_samples - about 200 E[k(x, y)] at the default 2e6 samples, a quirk kept as it is.  out [1];
 *                            batch_sums [10000] (may be NULL): the per-batch sums.
 *   ssmq_weights_gp_given    GaussianProcessModel.bq_weights (bq/bqmod.py:495-523) from expectations the caller supplies: iK =
 *                            sym((K + jitter I)^-1), scaling=False, then wm = q iK, Wc = sym(iK Q iK), Wcc = R iK, model_var =
 *                            alpha^2 (1 - tr(Q iK)), integral_var = kbar - q'iK q - the code path of ssmq_weights_gp with q, R,
 *                            Q, kbar given instead of the Gaussian closed forms.  One parameter row; status / return value as
 *                            ssmq_weights_gp.
 * Samples are summed in slots of 8192 (at most 1024 slots, then multiples of 8192) in sample order and the slots in index order,
 * without atomics: the same bits from run to run, whatever the launch grid.
 * Supported: D <= 16, N <= 128, 1 <= num_samples < 2^31, dof > 0 (else SSMQ_E_UNSUPPORTED, outputs untouched).  Host arrays;
 * synchronous.
 */
int ssmq_rbf_student_expect(int D, int N, const double *x, const double *par0, const double *par1, double dof,
                            int64_t num_samples, uint64_t seed, double *q, double *R, double *Q);
int ssmq_rbf_student_kxy(int D, const double *par, double dof, int64_t num_samples, uint64_t seed, double *out,
                         double *batch_sums);
int ssmq_weights_gp_given(int D, int N, const double *xi, const double *par, double jitter, const double *q, const double *R,
                          const double *Q, double kbar, double *wm, double *Wc, double *Wcc, double *iK, double *model_var,
                          double *integral_var, int32_t *status);

/*
 * Type-II maximum likelihood of the RBF kernel's parameters [alpha, ell_1 .. ell_D] (P = D + 1), B independent rows in
 * one launch, one workgroup each.
 *   ssmq_gp_nlml_batch  GaussianProcessModel.neg_log_marginal_likelihood (bq/bqmod.py:537-596), nu = 0, and
 *                       StudentTProcessModel.neg_log_marginal_likelihood (bq/bqmod.py:1191-1245), nu > 2, with the
 *                       kernel derivatives of RBFGauss.der_par (bq/bqkern.py:426-436): nlml [B] and grad [B][P] at the
 *                       log-parameters log_par [B][P].  K = eval(exp(log_par), x) + jitter; der_par uses K without the
 *                       jitter and differentiates with respect to alpha (not log alpha) and log ell_d: grad[b][0] is the
 *                       derivative with respect to log alpha divided by alpha, as in the reference.  status[b] = 1 (nlml and
 *                       grad NaN) where K is not positive definite; the return value is then the first such row + 1.
 *   ssmq_gp_ml2_batch   Model.optimize (bq/bqmod.py:250-285): scipy.optimize.minimize(nlml, log_par_0, method='BFGS',
 *                       jac=True, options={gtol, maxiter}) per row (maxiter < 0: 200 P), the whole optimisation inside
 *                       the launch.  x [B][P] minimisers, fun [B], jac [B][P] at them, hess_inv [B][P*P] (may be NULL),
 *                       status[b] = scipy's warnflag (0, SSMQ_BFGS_MAXITER, _PRECISION_LOSS, _NAN), nit [B] and nfev [B]
 *                       (may be NULL; the gradient comes with every evaluation: njev = nfev).  A point where K is not
 *                       positive definite is a value of +inf there (the reference raises LinAlgError).
 * x_obs [D][N] shared, or [B][D][N] with x_per_fit; fcn_obs [B][N][E]; jitter [N][N] added to K, of which only the
 * upper triangle is read (entry (i, j), j >= i, of K + jitter), as the reference's cho_factor(lower=False) reads it: a
 * jitter that is not symmetric (a per-point nugget jitter[i][j] = v[j], a triangle) gives the reference's answer.
 * Supported: D <= 16, N <= 128, E <= 16 (else SSMQ_E_UNSUPPORTED).  Host arrays; synchronous.
 */
int ssmq_gp_nlml_batch(int D, int N, int E, int64_t B, const double *x_obs, int x_per_fit, const double *fcn_obs,
                       const double *jitter, double nu, const double *log_par, double *nlml, double *grad, int32_t *status);
int ssmq_gp_ml2_batch(int D, int N, int E, int64_t B, const double *x_obs, int x_per_fit, const double *fcn_obs,
                      const double *jitter, double nu, double gtol, int maxiter, const double *log_par_0, double *x,
                      double *fun, double *jac, double *hess_inv, int32_t *status, int32_t *nit, int32_t *nfev);
/*
 * Prediction with the fitted models: GaussianProcessModel.predict (bq/bqmod.py:454-493), StudentTProcessModel.predict
 * (:1090-1130) and BayesSardModel.predict (:840-891), B independent fits with M test points each.  With iK = sym((K(x_obs)
 * + jitter I)^-1) at the NATURAL parameters par [B][1 + D] (rows [alpha, ell_1 .. ell_D]; scaling=True), kx = K(test,
 * x_obs) and kxx = alpha^2:
 *   GP (nu = 0, NB = 0)   mean = kx iK Y, var = kxx - diag(kx iK kx')
 *   TP (nu > 2, E = 1)    the GP's, the variance times (nu - 2 + y'iK y) / (nu - 2 + tp_num_pts); tp_num_pts is the MODEL's
 *                         point count, which the reference uses whatever x_obs holds
 *   Bayes-Sard (NB > 0)   V = vandermonde(mulind, x_obs), Z = V'iK, iG = (Z V)^-1 by Cholesky, A = iG V', b = Z kx' - vx',
 *                         mean = (kx - b'A) iK Y, var = kxx - diag(kx iK kx') + diag(b'iG b); mulind [D][NB], NB <= N
 * Layouts (host arrays, row-major): x_obs [D][N] shared, or [B][D][N] with x_per_fit; fcn_obs [B][N][E]; test [D][M] shared,
 * or [B][D][M] with test_per_fit; jitter: the scalar added to the diagonal of K.  Outputs: mean [B][M][E], var [B][M],
 * status [B]: 0 ok, 1 = K + jitter I not positive definite, 2 = Z V not positive definite; the mean and variance of a row
 * with a non-zero status are NaN, other rows are unaffected, and the return value is the first such row + 1.  Row b depends
 * on row b's data alone: a batch and B single calls give the same bits.
 * Supported: D <= 16, N <= 128, E <= 16, NB <= N, 1 <= M <= 2^31 - 1 (else SSMQ_E_UNSUPPORTED, outputs untouched).
 * Synchronous; rows are processed in chunks so that the device workspace stays within 512 MiB.
 */
int ssmq_gp_predict_batch(int D, int N, int E, int64_t B, const double *x_obs, int x_per_fit, const double *fcn_obs,
                          double jitter, double nu, int tp_num_pts, const double *par, const int32_t *mulind, int NB,
                          int64_t M, const double *test, int test_per_fit, double *mean, double *var, int32_t *status);
/*
 * Student-t process model: the same weights as ssmq_weights_gp (StudentTProcessModel inherits bq_weights,
 * bq/bqmod.py:1060-1130); model_var / integral_var are the GP values, which the t-process rescales with the integrand
 * values at transform time (bq/bqmod.py:1132-1190; tp_nu / tp_iK of ssmq_transform_create).
 */
int ssmq_weights_tp(int D, int N, const double *xi, const double *par, int P, double jitter, double *wm, double *Wc,
                    double *Wcc, double *iK, double *q, double *Q, double *R, double *model_var, double *integral_var,
                    int32_t *status);
/*
 * Bayes-Sard quadrature weights.  Replaces BayesSardModel.bq_weights (bq/bqmod.py:893-992) with _exp_x_px / _exp_x_xpx
 * / _exp_x_pxpx / _exp_x_kxpx (bq/bqmod.py:635-797) and utils.vandermonde (utils.py:478-502).
 *   mulind [D*NB]  multi-indices, row-major (D, NB), NB <= N; NB == N selects the unisolvent branch (:952-961).
 * outputs as ssmq_weights_gp (iK, q, Q, R as there; Q / R are only produced in the NB < N branch).
 */
int ssmq_weights_bs(int D, int N, const double *xi, const double *par, int P, double jitter,
                    const int32_t *mulind, int NB,
                    double *wm, double *Wc, double *Wcc, double *iK, double *q, double *Q, double *R,
                    double *model_var, double *integral_var, int32_t *status);

/*
 * The polynomial expectations behind the Bayes-Sard weights as entry points of their own (ssmq_weights_bs forms them
 * inline), for multi-indices mulind [D*NB] (row-major (D, NB)); any output may be NULL:
 *   px [NB]       BayesSardModel._exp_x_px   (bq/bqmod.py:635-662)   E[p_q(x)]
 *   xpx [D*NB]    BayesSardModel._exp_x_xpx  (:664-698)              E[x_e p_q(x)], with the reference's alpha_e factor
 *   pxpx [NB*NB]  BayesSardModel._exp_x_pxpx (:700-731)              E[p_r(x) p_q(x)]
 *   kxpx [N*NB]   BayesSardModel._exp_x_kxpx (:733-797)              E[k(x, x_n) p_q(x)] for the points x [D*N], kernel
 *                 parameters par [1+D] (the reference's `ell = sqrt_inv_lam ** -2` kept as written)
 *   vand [N*NB]   utils.vandermonde (utils.py:478-502)               p_q(x_n)
 * px / xpx / pxpx are integer arithmetic on the multi-indices (host code, no device needed); kxpx / vand run on the
 * device.
 */
int ssmq_bs_moments(int D, int N, const double *x, const double *par, const int32_t *mulind, int NB, double *px,
                    double *xpx, double *pxpx, double *kxpx, double *vand);

/*
 * Expected model variance and integral variance of the Bayes-Sard model as BayesSardModel.exp_model_variance /
 * integral_variance compute them (bq/bqmod.py:995-1050; the length-scale sweeps of research/bsq/bsq_ungm.py:244-282):
 * the general formulas  alpha^2 (1 - tr(Q iK) + tr(B (V' iK V)^-1)),  kbar - q' iK q + b' (V' iK V)^-1 b  for every
 * point set, with NO jitter on V' iK V - which is not what bq_weights() returns beside the weights (ssmq_weights_bs).
 * theta-batched: par [P][1+D], outputs model_var [P], integral_var [P] (either may be NULL), status [P] as above.
 */
int ssmq_variances_bs(int D, int N, const double *xi, const double *par, int P, double jitter, const int32_t *mulind,
                      int NB, double *model_var, double *integral_var, int32_t *status);

/*
 * Multi-output GP quadrature weights: one kernel-parameter row per output of the integrand.  Replaces
 * MultiOutputModel.bq_weights (bq/bqmod.py:1254-1315) with GaussianProcessMO.exp_model_variance / integral_variance
 * (:1532-1548).  par [E][1+D]; for output e everything comes from row e as in ssmq_weights_gp (stage one: the same per-row
 * code, P = E); stage two, one workgroup per pair i > j: Q_ij = exp_x_kxkx(par_i, par_j) (not symmetric), W = iK_i Q_ij iK_j,
 * both blocks [i][j] and [j][i] of Wc get sym(W) - what the reference's `0.5 * (w_c + w_c.swapaxes(0, 1).swapaxes(2, 3))`
 * leaves - and both blocks of Q get Q_ij untransposed, as the reference stores them.
 * outputs (host, output-major; any may be NULL): wm [E][N], Wcc [E][D][N], iK [E][N][N], q [E][N], R [E][D][N],
 *   Wc [E][E][N][N], Q [E][E][N][N], model_var [E] = alpha_e^2 (1 - tr(Q_ee iK_e)) with alpha_e from `par`,
 *   integral_var [E], status [E] (1 = K_e + jitter I not positive definite; the return value is then the first such row + 1
 *   and the pair blocks are not written).
 * Supported: D <= SSMQ_MAX_DIM, E <= SSMQ_MO_MAX_OUT, N <= SSMQ_MO_MAX_PTS (else SSMQ_E_UNSUPPORTED, outputs untouched).
 * Host arrays; synchronous.
 */
#define SSMQ_MO_MAX_OUT 8
#define SSMQ_MO_MAX_PTS 64
int ssmq_weights_gp_mo(int D, int N, int E, const double *xi, const double *par, double jitter, double *wm, double *Wcc,
                       double *iK, double *q, double *R, double *Wc, double *Q, double *model_var, double *integral_var,
                       int32_t *status);

/* ---- transform handle --------------------------------------------------------------------------------------- */
/*
 * Upload the constants of one moment transform (what BQTransform.__init__ / SigmaPointTransform.__init__ keep as
 * tf.wm / tf.Wc / tf.Wcc / tf.model.points / tf.model.model_var / tf.model.iK / tf.model.nu: bq/bqmtran.py:55-58,
 * 306-310, 387-392; mtran.py:165-168, 226-232).
 *   xi [D*N]; wm [N]; Wc: [N*N] (BQ form) or the diagonal [N] (SIGMA form); Wcc [D*N] (BQ form; NULL for SIGMA);
 *   emv [E*E] expected model variance as an (E, E) matrix (scalar model_var -> model_var * ones; NULL = 0);
 *   tp_nu > 0 selects the Student-t process covariance (bq/bqmtran.py:394-415, bq/bqmod.py:1132-1160) and needs
 *   tp_iK [N*N].
 * Returns NULL on error.
 */
ssmq_transform *ssmq_transform_create(int D, int E, int N, int form, const double *xi, const double *wm,
                                      const double *Wc, const double *Wcc, const double *emv, int emv_mode,
                                      double tp_nu, const double *tp_iK);
/* Replace the constants in place (research code overwrites tf.wm / tf.Wc / tf.Wcc / model_var:
 * research/tpq/tpq_ungm.py:114-124, research/bsq/bsq_tracking.py:276-281).  Any pointer may be NULL = keep. */
int ssmq_transform_update(ssmq_transform *h, const double *xi, const double *wm, const double *Wc, const double *Wcc,
                          const double *emv, int emv_mode, double tp_nu, const double *tp_iK);
/* The linearisation transform of ExtendedKalman (mtran.py:49-59: LinearizationTransform.apply; ssinf.py:347-357): no points and
 * no weights - mean_f = f(mean), cov_fx = J cov, cov_f = cov_fx J' with the model's own Jacobian (the seven models whose
 * dyn_fcn_dx / meas_fcn_dx the reference implements: UNGM, UNGM with non-additive noise, pendulum, constant velocity; every
 * other integrand: SSMQ_E_UNSUPPORTED at apply time, where the reference's Jacobian is None).  The handle goes wherever a
 * transform handle goes (ssmq_apply_batch[_dev], the filter / smoother entry points: time loop as a launch loop). */
ssmq_transform *ssmq_transform_create_linear(int D, int E);
/*
 * The Taylor-GPQD transform of ExtendedKalmanGPQD (SSMQ_FORM_TAYLOR_GPQD; mtran.py:668-701, ssinf.py:1302-1319): the linearisation
 * transform calibrated by an RBF kernel with scale alpha and length-scales ell [D], Lam = diag(ell^2).  With f = f(mean) and J the
 * model's own Jacobian (the models of ssmq_transform_create_linear; every other integrand, and every user integrand:
 * SSMQ_E_UNSUPPORTED at apply time):
 *   wm = det(Lam^-1 cov + I)^-1/2, wc = det(2 Lam^-1 cov + I)^-1/2, Wc = Lam/2 (Lam/2 + cov)^-1 cov,
 *   model_var = alpha^2 - alpha^2 wc (1 + tr(Wc Lam^-1)), integ_var = alpha^2 wc - wm^2,
 *   mean_f = wm f, cov_f = wc (f f' + J Wc J') - mean_f mean_f' + model_var (the scalar on every entry, as the reference adds it),
 *   cov_fx = J cov (Lam + cov)^-1 Lam - (E, D) as every transform of this library; the reference returns the transpose (D, E).
 * One launch of k_taylor_gpqd per batch; status 1 and NaN outputs for an item whose Lam + cov or Lam/2 + cov has a pivot that is
 * not positive (cov not positive semi-definite).  alpha, ell finite, ell > 0, D <= SSMQ_MAX_DIM (else NULL, SSMQ_E_ARG semantics:
 * ssmq_last_error() names the argument).  The handle runs through ssmq_apply_batch[_dev], ssmq_apply_kernel_name and the filter /
 * smoother entry points that take the linearisation transform (time loop as a launch loop); ssmq_filter_forward_multi_dev, the
 * marginalised filter, the theta-step, the sigma-point entry points and ssmq_transform_update[_mo] return SSMQ_E_UNSUPPORTED.
 */
ssmq_transform *ssmq_transform_create_taylor_gpqd(int D, int E, double alpha, const double *ell);
/* Where the following applications of a Taylor-GPQD handle (ssmq_apply_batch[_dev]) write model_var and integ_var of item b:
 * d_model_var[b], d_integ_var[b] - device arrays of at least B doubles each that the caller keeps alive; either may be NULL
 * (not written; the state of a new handle).  A filter pass does not need them. */
int ssmq_taylor_gpqd_variance_planes(ssmq_transform *h, double *d_model_var, double *d_integ_var);
/*
 * The truncated sigma-point transform (SSMQ_FORM_TRUNC_SIGMA; mtran.py:588-658, the measurement transform of the Truncated*Kalman
 * filters, ssinf.py:844-901) for an integrand that reads the D_eff leading of its D inputs: xi_eff [D_eff*N_eff], wm [N_eff],
 * wc [N_eff] - points (element d of point n at xi_eff[d * N_eff + n], as xi of ssmq_transform_create) and mean / covariance weights
 * of the rule of the effective dimension; xi [D*N], wcc [N] - points and cross-covariance weights of the rule of the full dimension.
 * With L = chol(cov) (lower; its leading D_eff x D_eff block L_e is the factor of the leading block of cov), m_e = mean[:D_eff]:
 *   x_eff_i = m_e + L_e xi_eff_i,  x_j = mean + L xi_j,
 *   mean_f = sum_i wm_i f(x_eff_i),  cov_f = sum_i wc_i (f(x_eff_i) - mean_f)(..)',  cov_fx = sum_j wcc_j (f(x_j) - mean_f)(x_j - mean)'.
 * mean_f and cov_f are functions of mean[:D_eff] and cov[:D_eff, :D_eff] alone, bit for bit.  One launch of k_apply_trunc per
 * batch; an item whose cov is not positive definite has status 1 and NaN outputs.  1 <= D_eff <= D <= 6, 1 <= E <= 4,
 * 1 <= N_eff, N <= 729, finite constants (else NULL, ssmq_last_error() names the range).  Built-in integrands that read at most
 * D_eff inputs, every state-index entry < D_eff (else SSMQ_E_UNSUPPORTED at apply time).  The handle runs through
 * ssmq_apply_batch[_dev], ssmq_apply_kernel_name and, as the MEASUREMENT handle next to an SSMQ_FORM_SIGMA dynamics handle, through
 * ssmq_filter_forward_dev, ssmq_filter_smooth_dev and ssmq_filter_kernel_name[_batch] (the launch loop apply dyn | k_apply_trunc |
 * k_kalman_update); every other entry point that takes a transform handle - and these as the dynamics handle - returns
 * SSMQ_E_UNSUPPORTED for it before it writes to an output.  There is no update: recreate the handle when its constants change.
 */
ssmq_transform *ssmq_transform_create_truncated(int D, int D_eff, int E, int N_eff, const double *xi_eff, const double *wm,
                                                const double *wc, int N, const double *xi, const double *wcc);
/*
 * GP quadrature with derivative observations at the sigma points (SSMQ_FORM_GPQD; research/gpqd/gpqd_base.py:
 * GaussianProcessDerTransform): xi [D*N] as for ssmq_transform_create; which_der [Nd], strictly increasing indices into the points
 * (Nd = 0: none); the weights in the compact layout of M = N + Nd D observations per output,
 *     [f(x_0) .. f(x_N-1) | (J L)[e, :] at which_der[0] | (J L)[e, :] at which_der[1] | ..],   L = chol(cov), x_n = mean + L xi_n:
 * wm [M], Wc [M*M], Wcc [D*M], and the scalar model variance, added to the diagonal of the covariance.
 *   mean_f = obs wm,  cov_f = obs Wc obs' - mean_f mean_f' + model_var I,  cov_fx = (obs Wcc') L'      - (E, D).
 * 1 <= D <= 6, 1 <= E <= max(D, 4), 2 <= N <= 2 D + 1, finite constants (else NULL, ssmq_last_error() names the range).  Integrands:
 * the built-in models that have a Jacobian and additive noise (UNGM, pendulum, constant velocity and their measurement models; the
 * Jacobian placed as for ssmq_transform_create_linear) and user ids registered with ssmq_integrand_define_dx; everything else is
 * SSMQ_E_UNSUPPORTED at apply time.  One launch per batch: k_apply_gpqd (D <= 2, observations in registers) or k_apply_gpqd_lds
 * (observations in LDS); an item whose cov is not positive definite has status 1 and NaN outputs.  The handle runs through
 * ssmq_apply_batch[_dev], ssmq_apply_kernel_name and, both handles of this form, the launch loop of ssmq_filter_forward_dev and
 * ssmq_filter_smooth_dev (built-in models; the forward pass also for user ids); every other entry point that takes a transform
 * handle returns SSMQ_E_UNSUPPORTED for it before it writes to an output.  ssmq_transform_gpqd_set replaces the subset, the weights
 * and the model variance of a handle (same D, E, N and points).
 * ssmq_weights_gpqd computes the weights on the device (ssmq_weights_gpqd.hip, one workgroup, the joint kernel matrix in LDS): the
 * RBF kernel par = [alpha, ell_1 .. ell_D], jitter on the whole diagonal of the M x M joint kernel matrix of values and derivatives;
 * `scaling` != 0 evaluates the joint kernel matrix with alpha^2 (K_out, L_out, iK_out: what eval / eval_chol / eval_inv_dot of the
 * reference return by default); the weights and variances are the reference's bq_weights for scaling = 0 only.  Outputs (host, each may be NULL): wm [M], Wc [M*M] symmetrised, Wcc [D*M], model_var, integral_var, the joint
 * kernel matrix without jitter K_out [M*M], its lower Cholesky factor with jitter L_out [M*M], the symmetrised inverse iK_out [M*M],
 * and the joint kernel expectations q_out [M], Q_out [M*M], R_out [D*M].  Returns 1 if the matrix is not positive definite (NaN
 * outputs), SSMQ_OK otherwise.
 */
ssmq_transform *ssmq_transform_create_gpqd(int D, int E, int N, const double *xi, int Nd, const int32_t *which_der, const double *wm,
                                           const double *Wc, const double *Wcc, double model_var);
int ssmq_transform_gpqd_set(ssmq_transform *h, int Nd, const int32_t *which_der, const double *wm, const double *Wc, const double *Wcc,
                            double model_var);
int ssmq_weights_gpqd(int D, int N, const double *xi, const double *par, int Nd, const int32_t *which_der, double jitter, int scaling,
                      double *wm, double *Wc, double *Wcc, double *model_var, double *integral_var, double *K_out, double *L_out,
                      double *iK_out, double *q_out, double *Q_out, double *R_out);
/*
 * The multi-output BQ transform (SSMQ_FORM_BQ_MO; MultiOutputGaussianProcessTransform / MultiOutputStudentTProcessTransform,
 * bq/bqmtran.py:425-602): xi [D*N]; wm [E][N]; Wc [E][E][N][N], of which the blocks [i][j] with i >= j are read; Wcc [E][D][N];
 * emv [E] model variance per output, added to the DIAGONAL of the covariance (NULL = 0); tp_nu > 0 selects the t-process scale
 * emv_i (tp_nu - 2 + fx_i iK_i fx_i') / (tp_nu - 2 + N) and needs tp_iK [E][N][N].
 * D <= SSMQ_MAX_DIM, E <= SSMQ_MO_MAX_OUT, N <= SSMQ_MO_MAX_PTS (else NULL, ssmq_last_error() names the range).  Every point set
 * with N >= 2 D is inside the range; with fewer points the kernel packs 64 / N trajectories into a wave, and the few shapes whose
 * work space then exceeds the LDS of a CU (D = 16, E = 8, N = 8; D = 12, E = 8, N = 4; ...) are refused here as well.
 * The handle runs through ssmq_apply_batch[_dev], ssmq_apply_kernel_name, ssmq_sigma_points_batch, ssmq_apply_fx_batch (one
 * kernel, k_apply_mo; built-in integrands) and ssmq_filter_forward_dev / ssmq_filter_kernel_name[_batch] (the launch loop);
 * every other entry point that takes a transform handle returns SSMQ_E_UNSUPPORTED for it and leaves its outputs untouched.
 * ssmq_transform_update_mo replaces constants in place (any pointer NULL = keep; tp_nu <= 0 = keep).
 */
ssmq_transform *ssmq_transform_create_mo(int D, int E, int N, const double *xi, const double *wm, const double *Wc,
                                         const double *Wcc, const double *emv, double tp_nu, const double *tp_iK);
int ssmq_transform_update_mo(ssmq_transform *h, const double *xi, const double *wm, const double *Wc, const double *Wcc,
                             const double *emv, double tp_nu, const double *tp_iK);
void ssmq_transform_destroy(ssmq_transform *h);
int ssmq_transform_dims(const ssmq_transform *h, int *D, int *E, int *N);

/* ---- the moment transform, batched over independent trajectories --------------------------------------------- */
/*
 * B moment transforms in one launch.  Replaces BQTransform.apply (bq/bqmtran.py:60-109) / SigmaPointTransform.apply
 * (mtran.py:105-149) for the built-in integrands: Cholesky of each cov, sigma points x = mean + L xi, integrand,
 * weighted mean / covariance / cross-covariance.
 * Host version, reference layout: mean [B*D], cov [B*D*D], time [B] or [1] (time_stride 1 or 0; the reference passes
 * np.atleast_1d(k - 1): ssinf.py:276-277), outputs mean_f [B*E], cov_f [B*E*E], cov_fx [B*E*D], status [B] (may be NULL).
 * B == 1 serves the drop-in apply().
 */
int ssmq_apply_batch(ssmq_transform *h, const ssmq_integrand *f, int64_t B, const double *mean, const double *cov,
                     const double *time, int time_stride, double *mean_f, double *cov_f, double *cov_fx,
                     int32_t *status);
/* Device version, SoA planes with pitch ld; d_time [B] or [1]; d_status [B] int32 (required).  Asynchronous on the
 * library stream.  Only the lower triangle of each input covariance is read (as LAPACK dpotrf 'L' does). */
int ssmq_apply_batch_dev(ssmq_transform *h, const ssmq_integrand *f, int64_t B, int64_t ld, const double *d_mean,
                         const double *d_cov, const double *d_time, int time_stride, double *d_mean_f,
                         double *d_cov_f, double *d_cov_fx, int32_t *d_status);
/* Which kernel ssmq_apply_batch_dev would run for this (transform, integrand): writes its name (for profiles). */
int ssmq_apply_kernel_name(const ssmq_transform *h, const ssmq_integrand *f, char *buf, int len);

/*
 * Arbitrary Python integrand f: the sigma points are formed on the device, f is evaluated by the caller, and the
 * weighted reductions run on the device (bq/bqmtran.py:97-101 and :104-107 around the `_fcn_eval` call at :102).
 *   ssmq_sigma_points_batch: x [B*D*N] (each (D, N) row-major), chol [B*D*D] lower factors.
 *   ssmq_apply_fx_batch:     fx [B*E*N]; `mean` / `x` are only read for the SIGMA form (centred cross-covariance).
 */
int ssmq_sigma_points_batch(ssmq_transform *h, int64_t B, const double *mean, const double *cov, double *x,
                            double *chol, int32_t *status);
int ssmq_apply_fx_batch(ssmq_transform *h, int64_t B, const double *chol, const double *mean, const double *x,
                        const double *fx, double *mean_f, double *cov_f, double *cov_fx);

/*
 * T = FX Wc for M = B E rows of integrand values that are already on the device: the GEMM-shaped stage of
 * fx Wc fx' (bq/bqmtran.py:199) for large point sets, on the matrix cores (v_mfma_f64_16x16x4_f64).  Row r of d_fx is
 * the integrand output e of trajectory b with r = b E + e, pitch ld_fx >= NP doubles (even), columns N..NP-1 ZERO,
 * NP = N rounded up to 16; d_t gets the same shape with pitch ld_t.  *n_padded (may be NULL) returns NP, 0 when the
 * handle has no instantiation (then SSMQ_E_UNSUPPORTED; ssmq_apply_batch* fall back to the generic kernel themselves).
 * Asynchronous on the library stream.
 */
int ssmq_fxwc_batch_dev(ssmq_transform *h, int64_t M, const double *d_fx, int64_t ld_fx, double *d_t, int64_t ld_t,
                        int *n_padded);

/* ---- callers of the path kept on the device (filter recursion) ------------------------------- */
/*
 * Gaussian measurement update for B trajectories (ssinf.py:297-323): gain = (P_y^-1 P_yx)' by Cholesky,
 * m = m_pr + gain (y - y_mean), P = P_pr - gain P_y gain' (left unsymmetrised as the reference does, :323).
 * SoA planes, pitch ld.  P_yx is (Y, D) as returned by the obs transform.  In-place (m_fi == m_pr etc.) is allowed.
 * P_y must be symmetric (its lower triangle is factored).  D, Y <= SSMQ_MAX_DIM, else SSMQ_E_UNSUPPORTED and nothing is written.
 * Asynchronous on the library stream: ssmq_sync() before the results are read.  The call clears d_status[0..B) (lanes B..ld-1 of
 * every output stay untouched) and then writes 1 to d_status[b], and NaN to every entry of that item's m_fi and P_fi, where P_y is
 * not positive definite (a pivot that is zero, negative or NaN).
 */
int ssmq_kalman_update_dev(int D, int Y, int64_t B, int64_t ld, const double *d_m_pr, const double *d_P_pr,
                           const double *d_y_mean, const double *d_P_y, const double *d_P_yx, const double *d_y,
                           double *d_m_fi, double *d_P_fi, int32_t *d_status);
/*
 * Forward pass of an additive-noise Gaussian filter for B trajectories and T steps (ssinf.py:66-118, 254-323):
 * per step k = 1..T: dyn transform at time k-1, += GQG', obs transform at time k-1, += R, measurement update.
 *   d_y [T][Y][ld]; d_m0 [D][ld], d_P0 [D*D][ld] (read only); GQG [D*D], R [Y*Y] host;
 *   outputs d_fm [T][D][ld], d_fP [T][D*D][ld]; d_status [ld] (0 ok, else 1 + first failing step).
 * Asynchronous on the library stream.  Common (models, shape, form) combinations run as ONE fused kernel with the
 * filter state in registers; every other combination replays the 3 T launches of the loop as a hipGraph.
 */
int ssmq_filter_forward_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                            const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y,
                            const double *d_m0, const double *d_P0, const double *GQG, const double *R,
                            double *d_fm, double *d_fP, int32_t *d_status);

/*
 * Forward pass of a Gaussian filter whose transition and / or measurement model takes its noise as an argument
 * (ssinf.py:271-272 and 282-283: mean <- [mean; noise_mean], cov <- blockdiag(cov, noise_cov) before each transform;
 * ssinf.py:294-295: cross-covariances trimmed to the first dim_state columns).
 *   dq > 0: non-additive dynamics, q_mean [dq], q_cov [dq*dq] host, h_dyn is a (dim_state + dq -> dim_state) transform;
 *   dq = 0: additive dynamics, q_cov is G Q G' [dim_state^2] (or NULL for none), q_mean ignored.
 *   dr likewise for the measurement model (h_obs: dim_state + dr -> Y; dr = 0: r_cov is R [Y*Y]).
 * Buffers and status as ssmq_filter_forward_dev.  Synchronous; one fused kernel where this (models, shapes, form)
 * combination has an instantiation (UNGMNA with 4 / 5 points, CTRS + radar with unscented points), else a launch loop
 * of 5 T launches.
 */
int ssmq_filter_forward_aug_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                const ssmq_integrand *f_obs, int dim_state, int64_t B, int64_t ld, int T,
                                const double *d_y, const double *d_m0, const double *d_P0, const double *q_mean,
                                const double *q_cov, int dq, const double *r_mean, const double *r_cov, int dr,
                                double *d_fm, double *d_fP, int32_t *d_status);

/*
 * Forward pass + Rauch-Tung-Striebel backward pass (ssinf.py:120-147, 325-344): as ssmq_filter_forward_dev, and
 * additionally d_sm [T][D][ld], d_sP [T][D*D][ld] smoothed moments.  The reference's indexing is kept: the recursion
 * starts at the last filtered estimate and leaves the last two smoothed steps equal to the filtered ones.  Synchronous.
 * The forward pass that keeps the predictive moments is one kernel for the UNGM / pendulum / reentry (5, 2, 11) shapes,
 * else the launch loop (hipGraph).
 */
/* The backward pass alone (ssinf.py:120-147, 325-344) over moments the caller kept from its own forward pass (the
 * marginalised filter drives its forward pass from the host): filtered d_fm [T][D][ld], d_fP [T][D*D][ld], predictive
 * d_pm, d_pP (element k = the prediction INTO step k), dynamics cross-covariance d_pC [T][D*D][ld]; outputs d_sm, d_sP;
 * d_status [ld] gets bit 30 set where a predictive covariance is not positive definite: the bit is OR-ed into the word the caller
 * passes in, nothing is cleared.  Every d_pP[k] must be symmetric (its lower triangle is read and mirrored); d_fP and d_pC are taken
 * as they are.  Elements 0 and T - 1 of d_pm, d_pP, d_pC are never read.  D <= 7.  Synchronous. */
int ssmq_rts_backward_dev(int D, int64_t B, int64_t ld, int T, const double *d_fm, const double *d_fP, const double *d_pm,
                          const double *d_pP, const double *d_pC, double *d_sm, double *d_sP, int32_t *d_status);

int ssmq_filter_smooth_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                           const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y,
                           const double *d_m0, const double *d_P0, const double *GQG, const double *R, double *d_fm,
                           double *d_fP, double *d_sm, double *d_sP, int32_t *d_status);
/*
 * The same for models that take their noise as an argument (arguments as ssmq_filter_forward_aug_dev): backward_pass of
 * the reference does not look at the model (ssinf.py:120-147, 325-344); the cross-covariance it uses is the one that
 * _time_update cut back to the state columns (ssinf.py:294-295).  Synchronous.
 */
int ssmq_filter_smooth_aug_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                               const ssmq_integrand *f_obs, int dim_state, int64_t B, int64_t ld, int T,
                               const double *d_y, const double *d_m0, const double *d_P0, const double *q_mean,
                               const double *q_cov, int dq, const double *r_mean, const double *r_cov, int dr,
                               double *d_fm, double *d_fP, double *d_sm, double *d_sP, int32_t *d_status);

/*
 * theta-batched filter step for GP-quadrature transforms whose kernel parameters are re-drawn per item - the inner
 * evaluation of the marginalised filter (ssinf.py:1117-1151 _state_posterior_moments, :1153-1198 _param_log_likelihood;
 * re-weighting bq/bqmtran.py:93-95).  For item i = 0..P-1:
 *   weights(par_dyn[i]) -> dyn transform at `time` (+ GQG) -> weights(par_obs[i]) -> obs transform at `time` (+ R)
 *   -> Kalman update with y -> post_mean[i][D], post_cov[i][D*D], loglik[i] = log N(y | y_mean, P_y).
 * h_dyn / h_obs supply shapes, sigma points and the emv mode (their own weights are not used; GP models only).
 * par_dyn: host [P][1+Din], par_obs [P][1+D] = [alpha, ell_1..] (already exponentiated), Din = input dimension of h_dyn.
 * Additive dynamics: Din = D.  Dynamics that take their noise as an argument: h_dyn is a (D + dq) -> D transform and the
 * caller passes the augmented moments [mean; q_mean], blockdiag(cov, Q) (ssinf.py:1174-1176) with GQG = NULL; the
 * measurement model is additive in either case (the reference builds that transform on dim_state inputs, ssinf.py:1288).
 * mean [Din] / cov [Din*Din] when shared_state = 1, else [P][Din] / [P][Din*Din]; y [Y] when shared_y = 1, else [P][Y].
 * GQG [D*D], R [Y*Y] host or NULL.
 * status[i] (may be NULL): bit 0 K_dyn not positive definite, bit 1 K_obs, bit 2 cov (Cholesky in the dyn transform),
 * bit 3 predictive cov, bit 4 P_y.  Returns 0, or 1 + index of the first item with a nonzero status.  Synchronous;
 * the weights never leave the device (k_weights writes per-item constant blocks that the generic transform kernel reads in place).
 */
int ssmq_gp_theta_step(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                       const ssmq_integrand *f_obs, int64_t P, const double *par_dyn, const double *par_obs,
                       double jitter, const double *mean, const double *cov, int shared_state, const double *y,
                       int shared_y, double time, const double *GQG, const double *R, double *post_mean,
                       double *post_cov, double *loglik, int32_t *status);

/* ssmq_gp_theta_step with a time of its own per item (times [P]): items of different time steps in one call. */
int ssmq_gp_theta_step_times(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                             const ssmq_integrand *f_obs, int64_t P, const double *par_dyn, const double *par_obs,
                             double jitter, const double *mean, const double *cov, int shared_state, const double *y,
                             int shared_y, const double *times, const double *GQG, const double *R, double *post_mean,
                             double *post_cov, double *loglik, int32_t *status);

/*
 * Batched Laplace step of the marginalised filter (ssinf.py:1243-1273 _param_posterior_moments: one scipy BFGS run per
 * trajectory and time step in the reference; research/tpq/tpq_base.py:175-192 loops over trajectories): B independent
 * minimisations of  -log N(y_b | theta-conditioned step)  -  log N(theta | prior_mean_b, prior_cov_b)  in lock step - every
 * round ONE ssmq_gp_theta_step of (unfinished trajectories) x (param_dim + 1) items (objective + forward-difference gradient,
 * step fd_step as scipy's default 1.4901161193847656e-08).  The optimiser restates SciPy 1.15's BFGS with its first line
 * search (MINPACK-2 DCSRCH, c1 = 1e-4, c2 = 0.9, gtol 1e-5 on the max-norm, maxiter 200 param_dim).
 * mean [B][Din], cov [B][Din*Din] (augmented as for ssmq_gp_theta_step), y [B][Y], prior_mean [B][P], prior_cov [B][P*P],
 * theta [B][P]: start points in (normally the prior means), minimisers out; hess_inv [B][P*P] the BFGS inverse Hessian.
 * status[b]: 0 converged, SSMQ_BFGS_MAXITER / _PRECISION_LOSS / _NAN = scipy's warnflag 1 / 2 / 3 (theta / hess_inv as scipy
 * leaves them), SSMQ_BFGS_PRIOR_NOT_PD.  (SSMQ_BFGS_FALLBACK is kept for binary compatibility and no longer returned: where
 * scipy switches to its second line search, scalar_search_wolfe2 / _zoom, the state machine follows it.)  An objective point
 * that the reference's objective would RAISE on (kernel matrix or covariance not positive definite: LinAlgError out of
 * scipy.optimize.minimize, ssinf.py:1153-1241) is a value of +inf here and the search continues; NaN is tested before maxiter
 * (scipy: the other way round).  iters[b] (may be NULL): BFGS iterations; *rounds (may be NULL): device calls made.  Host
 * arrays; synchronous.
 */
enum { SSMQ_BFGS_MAXITER = 1, SSMQ_BFGS_PRECISION_LOSS = 2, SSMQ_BFGS_NAN = 3, SSMQ_BFGS_FALLBACK = 100, SSMQ_BFGS_PRIOR_NOT_PD = 101 };
/*
 * The same optimiser on a host objective (no device): fn(ctx, n, P, traj, rows, vals) fills vals[i] with the objective of
 * trajectory traj[i] at the parameter row rows[i][P] and returns 0 (< 0: abort with that code).  What the tests pin against
 * scipy.optimize.minimize(method='BFGS') on the CPU.
 */
typedef int (*ssmq_objective_fn)(void *ctx, int64_t n, int P, const int64_t *traj, const double *rows, double *vals);
int ssmq_bfgs_lockstep_host(ssmq_objective_fn fn, void *ctx, int64_t B, int P, double fd_step, double *theta, double *hess_inv,
                            int32_t *status, int32_t *iters, int64_t *rounds);
/*
 * The analytic-gradient mode of the same optimiser (scipy.optimize.minimize(method='BFGS', jac=True), options gtol and
 * maxiter; maxiter < 0: 200 P): fn(ctx, n, P, traj, rows, vals, grads) fills vals[i] and grads[i][P] with the objective
 * and its gradient of run traj[i] at rows[i][P] and returns 0 (< 0: abort with that code).  theta [B][P]: start points in,
 * minimisers out; fun [B], jac [B][P], hess_inv [B][P*P]; status[b] as scipy's warnflag (0, SSMQ_BFGS_MAXITER,
 * _PRECISION_LOSS, _NAN); nit[b], nfev[b] (may be NULL): iterations, objective evaluations.  No device.
 */
typedef int (*ssmq_objective_grad_fn)(void *ctx, int64_t n, int P, const int64_t *traj, const double *rows, double *vals,
                                      double *grads);
int ssmq_bfgs_jac_lockstep_host(ssmq_objective_grad_fn fn, void *ctx, int64_t B, int P, double gtol, int maxiter,
                                double *theta, double *fun, double *jac, double *hess_inv, int32_t *status, int32_t *nit,
                                int32_t *nfev);
int ssmq_gp_marginal_laplace_batch(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                   const ssmq_integrand *f_obs, int64_t B, double jitter, const double *mean,
                                   const double *cov, const double *y, double time, const double *GQG, const double *R,
                                   const double *prior_mean, const double *prior_cov, double fd_step, double *theta,
                                   double *hess_inv, int32_t *status, int32_t *iters, int64_t *rounds);

/*
 * The whole marginalised filter (ssinf.py:66-118 around :1083-1273) for B trajectories, every trajectory at its own pace: each
 * walks Laplace step (BFGS as above) -> mixture over the NP parameter sigma points -> next time step by itself, and every device
 * round (ONE theta step) serves whatever the unfinished trajectories wait for.  Rounds = the longest trajectory's total, not
 * the sum over the time steps of the slowest one's.  Where the theta step has its two-launch route and P <= 16 the trajectories'
 * state machines live ON THE DEVICE (round 5: pack | theta step | advance are five launches per round, nothing is copied or
 * waited for per round; every eighth round one integer comes back); SSMQ_MARGINAL_HOST_ROUNDS=1 keeps them on the host.
 * y [B][T][Y]; x0_mean [D], x0_cov [D*D]; q_mean [dq] / q_cov [dq*dq] for dynamics that take their noise as an argument (h_dyn is
 * then a (D + dq) -> D transform, GQG = NULL), else NULL; prior_mean [P], prior_cov [P*P] of the log-parameters at step 1 (each
 * step's posterior is the next step's prior); upts [P][NP] unit sigma points and uwts [NP] weights of the parameter mixture
 * (the reference: spherical-radial, NP = 2 P); time index of step k is k (ssinf.py:1088-1122 as called from :101-110).
 * fm [B][T][D], fP [B][T][D*D] filtered moments (NaN from the step at which a trajectory failed); failed [B]: 0, or
 * step + 65536 reason (T < 65536) for the step at which the reference would raise numpy.linalg.LinAlgError - reason 1: the
 * step's parameter prior is not positive definite (_param_log_prior); 2 / 3: the Laplace posterior hess_inv + jitter is not
 * finite / not positive definite (the Cholesky factor of _measurement_update's parameter sigma points, ssinf.py:1103-1106);
 * 4: a parameter sigma point's filter step failed (kernel matrix or covariance not positive definite); 5: the mixture moments
 * are not finite.  Reasons 2-3 depend on the path BFGS took through a noisy objective (forward-difference gradients): a
 * trajectory that fails so in one implementation of the same optimiser may pass in another (tests/test_gpu_parity.py:
 * test_marginal_filter_failures_are_the_reference_s_linalg_errors);
 * theta_last [B][P], pcov_last [B][P*P] (may be NULL): the last parameter posterior; stats [3] (may be NULL): device rounds,
 * BFGS iterations, theta items.  Host arrays; synchronous.
 */
int ssmq_gp_marginal_filter_batch(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                  const ssmq_integrand *f_obs, int64_t B, int T, double jitter, const double *y,
                                  const double *x0_mean, const double *x0_cov, const double *q_mean, const double *q_cov,
                                  const double *GQG, const double *R, const double *prior_mean, const double *prior_cov,
                                  const double *upts, const double *uwts, int NP, double fd_step, double param_jitter,
                                  double *fm, double *fP, int32_t *failed, double *theta_last, double *pcov_last,
                                  int64_t *stats);

/*
 * Unit sigma-point sets and classical quadrature weights, host code (no device needed):
 *   SSMQ_PTS_UT  unscented, 2D+1 points    mtran.py:234-293   par = [kappa, alpha, beta]   (NaN / missing: max(3-D,0), 1, 2)
 *   SSMQ_PTS_SR  spherical-radial, 2D      mtran.py:171-204   par = []
 *   SSMQ_PTS_GH  Gauss-Hermite, degree^D   mtran.py:315-360   par = [degree]               (default 3)
 *   SSMQ_PTS_FS  fully symmetric Student   mtran.py:405-578   par = [degree 3|5, kappa, dof] (defaults 3, max(3-D,0), 4);
 *                degree 7: NOT in the reference (mtran.py:392 stops at 5) - this build's rule for BASELINE configs[4],
 *                generators [0], [v1], [v2], [u,u], [u,u,u], 1 + 4D + 2D(D-1) + 4D(D-1)(D-2)/3 points (1181 at D = 10), exact
 *                for all monomials of total degree <= 7 under St(0, I, max(dof, 7)); parity-unpinned, property-tested
 * BQ models use the points only (bq/bqmod.py:340-382).  ssmq_points_count returns N (or < 0); ssmq_points fills
 * xi [D*N] (row-major (D, N), the reference's column order), wm [N] mean weights, wc [N] covariance weights (any may be
 * NULL) and returns N.
 */
enum ssmq_point_kind { SSMQ_PTS_UT = 0, SSMQ_PTS_SR = 1, SSMQ_PTS_GH = 2, SSMQ_PTS_FS = 3 };
int ssmq_points_count(int kind, int D, const double *par, int n_par);
int ssmq_points(int kind, int D, const double *par, int n_par, double *xi, double *wm, double *wc);

/*
 * Synthetic trajectories and measurements generated on the device, in the filter's plane layout
 * (TransitionModel.simulate_discrete ssmod.py:168-199, MeasurementModel.simulate_measurements ssmod.py:1011-1039):
 *   x[0] = x0_mean + x0_chol z;  x[k] = dyn_fcn(x[k-1], q[k-1], k-1);  y[k] = meas_fcn(x[k], r[k], k+1),
 *   q = q_mean + q_chol z, r = r_mean + r_chol z (lower Cholesky factors, host arrays; means may be NULL = 0).
 * Additive dynamics add G q (G [D*dq] host, NULL = eye(D, dq)); non-additive models get the noise as integrand input.
 * Outputs d_x [T][D][ld], d_y [T][Y][ld].  Random numbers: Philox4x32-10 keyed by `seed`, counter = (traj_offset + b,
 * step, purpose, pair) + Box-Muller, so a trajectory depends on its GLOBAL index only (shard with traj_offset).
 * f_obs = NULL: states only (d_y unused); f_dyn = NULL: measurements of the GIVEN states d_x (simulate_measurements(x)).
 * Parity with np.random is statistical; the generator itself is restated in oracle/ (known-answer vectors).  Synchronous.
 */
int ssmq_simulate_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int dr,
                      int dyn_additive, int obs_additive, int64_t B, int64_t ld, int T, const double *x0_mean,
                      const double *x0_chol, const double *q_mean, const double *q_chol, const double *G,
                      const double *r_mean, const double *r_chol, uint64_t seed, uint64_t traj_offset, double *d_x,
                      double *d_y);

/*
 * The same with any of the reference's random variables for the initial state, the process noise and the measurement
 * noise, and optionally the continuous-time dynamics:
 *   SSMQ_RV_GAUSS    mean + chol z                                  GaussRV     utils.py:580-625
 *   SSMQ_RV_STUDENT  mean + chol z / sqrt(u), u ~ Gamma(dof/2, 2/dof) StudentRV   utils.py:349-382, 628-674 (chol = factor
 *                    of the SCALE matrix)
 *   SSMQ_RV_MIXTURE  component k with probability alpha[k], then Gaussian (mean[k], chol[k])   utils.py:254-299,
 *                    research/tpq/tpq_base.py:13-32; n_comp <= 8
 * mean [n_comp][dim] (NULL = 0), chol [n_comp][dim*dim] lower factors, alpha [n_comp]: host arrays.
 * continuous != 0: Euler-Maruyama of TransitionModel.simulate_continuous (ssmod.py:201-244) -
 *   x[k] = x[k-1] + dt dyn_fcn_cont(x[k-1], (sqrt(dt)/dt) q[k-1], k-1), T = floor(duration / dt) columns, the initial
 *   state not among them - for the models that define dyn_fcn_cont: SSMQ_F_REENTRY1D_DYN (ssmod.py:429-432),
 *   SSMQ_F_REENTRY2D_DYN (:569-585), SSMQ_F_CTRS_DYN (:779-780); SSMQ_E_UNSUPPORTED otherwise (the reference's other models
 *   return None there).  Measurements (f_obs) are taken of the returned columns, column k at time k + 1.
 * Gamma variates: Marsaglia-Tsang on the same counter-based stream (attempt t of (trajectory, step, purpose) has its own
 * counter), so every draw is a pure function of (seed, global trajectory index, step).
 */
enum ssmq_rv_kind { SSMQ_RV_GAUSS = 0, SSMQ_RV_STUDENT = 1, SSMQ_RV_MIXTURE = 2 };
typedef struct ssmq_rv {
    int32_t kind, dim, n_comp, reserved;
    double dof;
    const double *mean, *chol, *alpha;
} ssmq_rv;
int ssmq_simulate_rv_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, const ssmq_rv *x0,
                         const ssmq_rv *q, const ssmq_rv *r, const double *G, int dyn_additive, int obs_additive,
                         int64_t B, int64_t ld, int T, int continuous, double dt, uint64_t seed, uint64_t traj_offset,
                         double *d_x, double *d_y);

/*
 * Error statistics of B filtered trajectories against the true states, summed over the Monte-Carlo axis on the device
 * (utils.py:18-38 squared_error, :41-64 mse_matrix, :123-148 neg_log_likelihood; aggregated per time step as
 * research/tpq/tpq_base.py:154-160 does).  d_x, d_fm [T][D][ld], d_fP [T][D*D][ld] (the filter's output buffers),
 * d_status [ld] or NULL (nonzero = trajectory excluded).  sums: host [T][W], W = ssmq_error_sums_width(D) = D*D+D+4:
 *   se[D] sum (x-m)^2 | rmse sum ||x-m|| | nll sum | mse[D*D] sum (x-m)(x-m)' | n_ok | n_pd
 * n_ok = trajectories counted (status 0), n_pd = those that entered the nll sum: every trajectory whose P is nonsingular.
 * A P that is not positive definite does not stop the reference (inv(P), sign * logdet of slogdet, utils.py:143-148):
 * such entries are handled by a second pass with an LU factorisation, so n_pd < n_ok only for a singular P (where
 * numpy.linalg.inv raises).  Sums, not means: ranks add them (one all-reduce) before dividing.  Deterministic summation
 * order.  Synchronous.
 */
int ssmq_error_sums_width(int D);
int ssmq_error_sums_dev(int D, int64_t B, int64_t ld, int T, const double *d_x, const double *d_fm, const double *d_fP,
                        const int32_t *d_status, double *sums);
/*
 * Second phase: sums of the log credibility ratio 10 (log10 dx'P^-1 dx - log10 dx'M^-1 dx) (utils.py:66-120) against
 * the GLOBAL per-step MSE matrices mse [T][D*D] (host; regularisation, e.g. + 1e-6 I of research/tpq/tpq_base.py:161,
 * already added).  sums: host [T][2] = lcr sum | n counted (status 0).  A P that is not positive definite goes through
 * the reference's fallback, mat_sqrt = u sqrt(s) of an SVD (utils.py:426-432), i.e. the quadratic form with |P|: a second
 * pass with a Jacobi eigen-decomposition handles those entries.  A singular P is counted in n and its term is +inf (a zero
 * eigenvalue of |P|), and with it the step's sum.
 */
int ssmq_lcr_sums_dev(int D, int64_t B, int64_t ld, int T, const double *d_x, const double *d_fm, const double *d_fP,
                      const int32_t *d_status, const double *mse, double *sums);

/*
 * The time-averaged scores of every trajectory - what the reference's studies hand to bootstrap_var (utils.py:223-244) for their
 * "+- 2 sqrt(var)" columns.  Inputs as for ssmq_error_sums_dev; the steps k0 .. T-1 enter (0 <= k0 < T; the studies skip step 0).
 * d_scores: device [D + 3][ld], R = ssmq_traj_scores_rows(D) = D + 3 rows, for trajectory b:
 *   rows 0 .. D-1  sqrt(mean_k (x - m)_d^2)   per-dimension RMSE (research/bsq/bsq_ungm.py:32)
 *   row  D         mean_k ||x - m||           (research/tpq/tpq_base.py:154-160; the convention of the `rmse` sum above)
 *   row  D + 1     mean_k of the negative log-likelihood
 *   row  D + 2     mean_k of the log credibility ratio against mse [T][D*D] (host, regularisation already added); NaN if mse == NULL
 * A P that is not positive definite takes the fallbacks of the sums (LU for the NLL, the quadratic form with |P| for the LCR); a
 * singular P leaves NaN in row D + 1, an mse[k] that is not positive definite NaN in row D + 2.  Excluded trajectories (nonzero
 * status) and the padding lanes B .. ld-1 are NaN in every row.  Synchronous.
 */
int ssmq_traj_scores_rows(int D);
int ssmq_traj_scores_dev(int D, int64_t B, int64_t ld, int T, int k0, const double *d_x, const double *d_fm, const double *d_fP,
                         const int32_t *d_status, const double *mse, double *d_scores);

/*
 * Bootstrap variance of the mean (utils.py:223-244 bootstrap_var) of each of the R rows of a device block d_data [R][ld], without
 * the reference's (S, n) matrix of draws: S resamples of n entries, drawn with replacement from the n included entries d_idx [n]
 * (device; values in 0 .. ld-1; NULL = the entries 0 .. n-1), mean_s = (1 / n) sum_i data[idx[j(s, i)]], var[r] = numpy.var
 * (ddof 0, two-pass) of the S means of row r.  The draw (csrc/ssmq_bootstrap.hip states it in full):
 *   (o0, o1, o2, o3) = Philox4x32-10(counter (i >> 1, 0, s, 0xB0075747), key (seed lo, seed hi));
 *   word = o0 | o1 << 32 for even i, o2 | o3 << 32 for odd i;   j(s, i) = (word * n) >> 64.
 * The draws are shared by the rows (row r of an R-row call is the one-row call on that row, bit for bit), and the summation order
 * depends on n alone: the same (data, idx, S, seed) gives the same bits on every device.  A NaN among the included values
 * propagates.  d_means: device [R][S], receives the resample means, or NULL.  var: host [R].
 * 1 <= n < 2^31, n <= ld, 1 <= S <= 2^20, 1 <= R <= 19 (SSMQ_E_ARG otherwise, before the device is touched).  Synchronous.
 * ssmq_bootstrap_var: one row of n entries in a host array.
 */
int ssmq_bootstrap_var_dev(const double *d_data, int64_t ld, int R, const int32_t *d_idx, int64_t n, int S, uint64_t seed,
                           double *var, double *d_means);
int ssmq_bootstrap_var(const double *data, int64_t n, int S, uint64_t seed, double *var);

/*
 * Monte-Carlo moment transform of any sample count (mtran.py:62-94 MonteCarloTransform.apply), streamed: the n unit samples are
 * drawn where they are used and no (D, n) point matrix exists.  For item b with moments (m_b, P_b), x_j = m_b + L_b z_j:
 *   mean_f = sum f(x_j) / n,  cov_f = sum (f - mean_f)(f - mean_f)' / (n - 1),  cov_fx = sum (f - mean_f)(x_j - m_b)' / (n - 1).
 * The draw (csrc/ssmq_mc_moments.h states it in full): (z_j[2 p], z_j[2 p + 1]) = Box-Muller of the two 53-bit uniforms of
 *   Philox4x32-10(counter (j, 0, p, 0x4D435446), key (seed lo, seed hi)) - the same unit samples for every item of a batch.
 * The sums are taken in one pass around the pivot f(m_b), in chunks of 2048 samples in a fixed order: an item's bits depend on
 * (seed, n, its own inputs) alone, not on B or the launch (n <= 2048: a second pass around the mean of the first).
 * Takes an integrand, not a transform handle: built-in ids in the (D, E, state index) combinations of csrc/ssmq_mc_transform.hip's table, and user ids (no state index).  Device buffers in the
 * conventions of ssmq_apply_batch_dev: SoA planes with pitch ld, d_time [B] or [1], d_status [B] (1: covariance not positive
 * definite, that item's outputs NaN).  1 <= D, E <= 6 and 2 <= n < 2^31, else SSMQ_E_UNSUPPORTED before an output is touched.
 * Synchronous.
 * ssmq_mc_unit_points: the unit samples first .. first + count - 1 as a host array z [D][count], by the same device code.
 */
int ssmq_mc_transform_dev(const ssmq_integrand *f, int D, int E, int64_t n, uint64_t seed, int64_t B, int64_t ld,
                          const double *d_mean, const double *d_cov, const double *d_time, int time_stride, double *d_mean_f,
                          double *d_cov_f, double *d_cov_fx, int32_t *d_status);
int ssmq_mc_unit_points(int D, uint64_t seed, int64_t first, int64_t count, double *z);

/*
 * KL divergence of Gaussian pairs (utils.py:151-182 kl_divergence, as written there:
 *   0.5 (tr(P1^-1 P0) + (m0 - m1)' P1^-1 (m0 - m1) + log(det P0 / det P1) - E) ), or with `symmetrized`
 *   0.5 (KL(0, 1) + KL(1, 0)) (utils.py:185-220), one pair per lane, through the two Cholesky factors (in double-double arithmetic):
 *   tr(P1^-1 P0) = |L1^-1 L0|_F^2, the quadratic term |L1^-1 (m0 - m1)|^2, log(det P0 / det P1) = 2 sum (log L0_ii - log L1_ii).
 * SoA planes d_m1 [E][ld], d_P1 [E*E][ld] (lower triangle read); d_m0 / d_P0 likewise, or with bcast0 one pair [E], [E*E] used
 * for every item.  d_kl [B], d_status [B]: a pair with a factor that fails gets status 1 and NaN (the reference returns NaN or a
 * number without meaning from log(det / det) there).  1 <= E <= 6, else SSMQ_E_UNSUPPORTED.  Asynchronous on the library stream.
 */
int ssmq_kl_divergence_dev(int E, int64_t B, int64_t ld, const double *d_m0, const double *d_P0, int bcast0, const double *d_m1,
                           const double *d_P1, int symmetrized, double *d_kl, int32_t *d_status);

/*
 * Forward pass of a Studentian filter (ssinf.py:555-736: StudentianInference._time_update / _measurement_update) for B
 * trajectories.  Same loop as ssmq_filter_forward_dev with the reference's scale-matrix bookkeeping:
 *   transforms are fed the SCALE matrix; scale[k] * cov_f (+ G q_smat G') and scale[k] * (cov_f, cov_fx) (+ r_smat)
 *   replace the Gaussian predictive covariances; after the Kalman-form update P = S_pr - K S_y K' the next step's scale
 *   matrix is (dof + delta'delta) / (dof + Y) * P with delta = chol(S_y)^-1 (y - y_mean).
 *   d_S0 [D*D][ld] initial scale matrix ((dof - 2) / dof * x0_cov); GqG [D*D], r_smat [Y*Y], scale [T] host arrays
 *   (scale[k] = (dof_pr - 2) / dof_pr of step k - it depends on the degrees of freedom only, not on the data);
 *   outputs as above: d_fm filtered means, d_fP the reference's `x_cov_fi` (ssinf.py:726).
 */
int ssmq_student_filter_forward_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                    const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y,
                                    const double *d_m0, const double *d_S0, const double *GqG, const double *r_smat,
                                    const double *scale, double dof, double *d_fm, double *d_fP, int32_t *d_status);

/*
 * A independent filters in ONE launch (round 6; ABI 102).  The reference's studies run several filters over the same
 * measurements one after the other (research/bsq/bsq_ungm.py:132-137, research/tpq/tpq_base.py:175-192); a pass of 1e4
 * trajectories occupies a sixth of the device, so the passes of a study fit side by side.  Each job is one call of
 * ssmq_filter_forward_dev (scale == NULL, dof == 0) or of ssmq_student_filter_forward_dev (scale [T] host, dof > 0) with
 * the same argument meaning; jobs may share d_y / d_m0 / d_P0 (read only) but not their outputs.  The calling thread's
 * stream forks into one branch per job inside a captured launch graph and joins again: the jobs run concurrently on the
 * device, every job is its own fused time-loop kernel (the results are the bits of the single calls), and a repeated call
 * with the same job list is one graph launch.  Jobs whose (models, shapes, form) have no fused kernel run after the graph,
 * one by one, through the ordinary path.  Asynchronous on the calling thread's stream; d_status as for the single calls.
 * At most 64 jobs.  The strip schedule (k_filter_chunked) is not used for the jobs of a multi-launch.
 */
typedef struct ssmq_filter_job {
    ssmq_transform *h_dyn;
    const ssmq_integrand *f_dyn;
    ssmq_transform *h_obs;
    const ssmq_integrand *f_obs;
    int64_t B, ld;
    int32_t T, reserved;
    const double *d_y, *d_m0, *d_P0; /* device: [T][Y][ld], [D][ld], [D*D][ld] */
    const double *GQG, *R;           /* host: [D*D], [Y*Y] (NULL = zeros) */
    double *d_fm, *d_fP;             /* device: [T][D][ld], [T][D*D][ld] */
    int32_t *d_status;               /* device: [ld] */
    const double *scale;             /* host [T]: Studentian recursion (with dof > 0), NULL for the Gaussian filters */
    double dof;
} ssmq_filter_job;
int ssmq_filter_forward_multi_dev(int n_jobs, const ssmq_filter_job *jobs);

/*
 * The drop-in forward pass with HOST arrays in the reference's layout (ssinf.py:66-118: forward_pass takes the measurements
 * as an ndarray and returns ndarrays), pipelined (round 6; ABI 102): the pass runs as K launches over consecutive time blocks
 * (k_filter_range: the whole-pass kernel's bits), the measurements of block k + 1 are uploaded and the filtered moments of
 * block k - 1 downloaded while block k runs.
 *   y (Y, T, B) host; m0 (D) and P0 (D, D) host, or (B, D) and (B, D, D) with SSMQ_PIPED_X0_PER_TRAJECTORY; GQG (D, D), R (Y, Y)
 *   host or NULL; outputs fm (D, T, B), fP (D, D, T, B), status [B] host.  With SSMQ_PIPED_OUT_PINNED fm and fP are page-locked
 *   (ssmq_pinned_alloc): the copy engine writes them in place, no staging copy.  n_blocks = 0: the library chooses K.
 * Synchronous.  Gaussian recursion, additive noise; SSMQ_E_UNSUPPORTED when the (models, shapes, form) combination has no
 * time-block kernel (UNGM with 2 / 3 / 5 points, the reentry and coordinated-turn shapes with unscented points have one) -
 * the caller then uses ssmq_upload_planes / ssmq_filter_forward_dev / ssmq_download_planes.
 */
#define SSMQ_PIPED_OUT_PINNED 1
#define SSMQ_PIPED_X0_PER_TRAJECTORY 2
int ssmq_filter_forward_piped(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                              const ssmq_integrand *f_obs, int64_t B, int T, const double *y, const double *m0,
                              const double *P0, const double *GQG, const double *R, double *fm, double *fP,
                              int32_t *status, int flags, int n_blocks);
/* Page-locked host memory from a process-wide pool (blocks are reused; at most 1 GiB is kept idle).  ssmq_pinned_is_block:
 * 1 if p is the start of a live block. */
int ssmq_pinned_alloc(size_t bytes, void **p);
int ssmq_pinned_free(void *p);
int ssmq_pinned_is_block(const void *p);

/* Name of the kernel(s) ssmq_filter_forward_dev would run for this pair of transforms (for profiles). */
int ssmq_filter_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                            const ssmq_integrand *f_obs, char *buf, int len);
/* ... for a batch of B trajectories: batches that leave most of the device idle run the time loop with the sigma points of every
 * transform shared out over the waves of a workgroup (k_filter_wsplit, csrc/ssmq_filter_wsplit.hip); B = 0: the kernel of
 * saturated batches. */
int ssmq_filter_kernel_name_batch(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                  const ssmq_integrand *f_obs, int64_t B, char *buf, int len);
/* ... and for planes of pitch ld and T steps (0, 0: not given - the answer for the batch alone): routes whose kernels address a
 * pass with 32-bit offsets are bounded by its size (k_filter_ungm_quad: 8 ld T < 2^31).  Nothing is allocated or launched. */
int ssmq_filter_kernel_name_shape(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                  const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, char *buf, int len);

/*
 * Innovation scores of a filter pass, from the measurements and the FILTERED moments alone (no true states): for step k = 0 .. T-1
 * with (m, P) = (m0, P0) for k = 0, else (fm[k-1], fP[k-1]; the lower triangle of fP is read, as the filters read it),
 *     m_pr, P_pr = dynamics transform of (m, P) + G Q G';   y_mean, S = measurement transform of (m_pr, P_pr) + R;   e = y_k - y_mean;
 *     nis[k] = e' S^-1 e (Cholesky of S);   ll[k] = -(Y log 2 pi + log det S + nis[k]) / 2 = log p(y_k | y_1..k-1)
 * (additive-noise Gaussian recursion, ssinf.py:254-323; both transforms use time index k).  Per trajectory, summed in ascending k:
 * d_total[b] = sum_k ll[k], d_total[ld + b] = sum_k nis[k] / T.
 * Buffers: d_y, d_m0, d_P0, d_fm, d_fP, GQG, R as ssmq_filter_forward_dev takes and leaves them; d_nis, d_ll [T][ld]; d_total
 * [2][ld]; d_status [ld] int32; d_ymean [T][Y][ld] and d_S [T][Y*Y][ld] (both triangles) are optional: NULL = not stored.
 * Failures: an item whose inputs are NaN (the filter failed earlier) or one of whose Cholesky factorisations fails (input
 * covariance, predictive covariance, S) is NaN in nis, ll, y_mean and S; d_status[b] = 1 + the first such k, 0 if there is none,
 * and the totals are NaN from there on.  A trajectory's results do not depend on the batch around it.
 * One launch of k_innovation<> over all T B items where the fused time loop has an instantiation for the pair (and for a pair
 * with a user integrand in the range of ssmq_filter_forward_dev, compiled at run time); every other pair the Gaussian launch loop
 * of ssmq_filter_forward_dev accepts - and every pair under SSMQ_NO_FUSED=1 - runs apply dyn | apply obs | k_innovation_score per
 * step.  The Studentian recursion has no entry point here; transforms of models that take their noise as an argument (D -> D and
 * D -> Y is required) return SSMQ_E_UNSUPPORTED before an output is touched.  B == 0: nothing happens; T == 0: status and totals
 * are zero.  Asynchronous on the library stream.
 */
int ssmq_filter_innovations_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                const ssmq_integrand *f_obs, int64_t B, int64_t ld, int T, const double *d_y, const double *d_m0,
                                const double *d_P0, const double *d_fm, const double *d_fP, const double *GQG, const double *R,
                                double *d_ymean, double *d_S, double *d_nis, double *d_ll, double *d_total, int32_t *d_status);
/* Name of the kernel(s) ssmq_filter_innovations_dev would run for this pair (the dry-run twin of ssmq_filter_kernel_name_batch). */
int ssmq_innovations_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                 const ssmq_integrand *f_obs, int64_t B, char *buf, int len);

/*
 * Iterated posterior linearisation pass (IPLF, Garcia-Fernandez et al. 2015; with linearisation transforms the iterated EKF) of the
 * additive-noise Gaussian filters: the time update of ssmq_filter_forward_dev, (m-, P-) = dynamics transform of (m, P) + G Q G', then
 * with (m_0, P_0) = (m-, P-), for i = 0 .. iterations - 1 (both transforms use time index k at every iteration):
 *     y^, S_y, C = measurement transform of (m_i, P_i)          A = C P_i^-1     b = y^ - A m_i     Omega = S_y - A P_i A'
 *     S = A P- A' + Omega + R      K = P- A' S^-1      m_{i+1} = m- + K (y_k - A m- - b)      P_{i+1} = P- - K S K'
 * and (fm[k], fP[k]) = (m_J, P_J).  iterations = 1 is ssmq_filter_forward_dev up to rounding; 1 <= iterations <= SSMQ_ITERATED_MAX,
 * else SSMQ_E_ARG.  d_delta [T][ld] or NULL: max_d |m_J[d] - m_{J-1}[d]| / sqrt(P_J[d][d]) of every step (against m- for one
 * iteration), the convergence diagnostic - there is no stopping rule.  Only P_i and S are factored; P is read through its lower
 * triangle and both triangles of fP are written from one value.
 * Buffers as ssmq_filter_forward_dev.  Failures: a step with a failed factorisation or NaN inputs makes the trajectory's outputs
 * (delta included) NaN from that step on, d_status[b] = 1 + that step.  A trajectory's results do not depend on the batch around it.
 * One launch of k_iplf_loop<> where the fused time loop has an instantiation for the pair (the dense kernels), and for a pair with a
 * user integrand in the range of ssmq_filter_forward_dev, compiled at run time; every other pair that ssmq_filter_innovations_dev
 * accepts - and every pair under SSMQ_NO_FUSED=1 or with flags bit 0 set - runs apply dyn | iterations x (apply obs | k_iplf_update)
 * per step.  What ssmq_filter_innovations_dev refuses is refused here, SSMQ_E_UNSUPPORTED before an output is touched.
 * Asynchronous on the library stream.
 */
#define SSMQ_ITERATED_MAX 64
#define SSMQ_ITERATED_LAUNCH_LOOP 1 /* flags bit 0 */
int ssmq_filter_iterated_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                             int64_t B, int64_t ld, int T, int iterations, int flags, const double *d_y, const double *d_m0,
                             const double *d_P0, const double *GQG, const double *R, double *d_fm, double *d_fP,
                             double *d_delta /* [T][ld] or NULL */, int32_t *d_status);
/* Name of the kernel(s) ssmq_filter_iterated_dev would run for this pair, iteration count and flags. */
int ssmq_iterated_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                              const ssmq_integrand *f_obs, int64_t B, int iterations, int flags, char *buf, int len);

/*
 * Outlier-robust pass of the additive-noise Gaussian filters (Agamennoni, Nieto, Nebot 2012; Piche, Sarkka, Hartikainen 2012): the
 * measurement noise is Student-t, r_k | lambda_k ~ N(0, R / lambda_k), lambda_k ~ Gamma(dof / 2, rate dof / 2), R its SCALE matrix.
 * Per step the time update of ssmq_filter_forward_dev, ONE measurement transform at the prior,
 *     y^, P_h (no noise), C = measurement transform of (m-, P-)          e = y_k - y^          lambda_0 = 1,
 * the variational fixed point in measurement space, i = 0 .. iterations - 2,
 *     S_i = P_h + R / lambda_i      r^ = (R / lambda_i) S_i^-1 e      Psi = r^ r^' + P_h - P_h S_i^-1 P_h
 *     gamma = sum_ab (R^-1)[a][b] Psi[a][b]      lambda_{i+1} = (dof + Y) / (dof + gamma)
 * and one state update with the last weight: S = P_h + R / lambda, K = C' S^-1, m = m- + K e, P = P- - K S K' (both triangles of fP
 * from one value).  d_lam [T][ld]: the weight the update used (the outlier indicator: 1 for an unsurprising measurement, towards 0
 * for an outlier); d_delta [T][ld]: |lambda_{J-1} - lambda_{J-2}| / lambda_{J-1}, 0 for iterations = 1 - there is no stopping rule.
 * iterations = 1 is ssmq_filter_forward_dev up to rounding.  1 <= iterations <= SSMQ_ITERATED_MAX, dof a positive finite number
 * (1e300: every weight is exactly 1), R symmetric positive definite (its inverse is taken on the host by Cholesky), flags: bit 0
 * alone - else SSMQ_E_ARG.  Buffers as ssmq_filter_forward_dev.
 * Failures: a factorisation that fails (P by the transforms, S_i, S), a weight that is not a positive finite number or an updated mean
 * that is not finite (a NaN measurement) makes the trajectory's outputs (lam and delta included) NaN from that step on,
 * d_status[b] = 1 + that step.  A trajectory's results do not depend on the batch around it.
 * One launch of k_robust_loop<> where the fused time loop has an instantiation for the pair (the dense kernels), and for a pair with a
 * user integrand in the range of ssmq_filter_forward_dev, compiled at run time; every other pair that ssmq_filter_innovations_dev
 * accepts - and every pair under SSMQ_NO_FUSED=1 or with flags bit 0 set - runs apply dyn | apply obs | k_robust_update per step.  What
 * ssmq_filter_innovations_dev refuses is refused here; every refusal comes before an output is touched.  Asynchronous on the library
 * stream.
 */
#define SSMQ_ROBUST_LAUNCH_LOOP 1 /* flags bit 0 */
int ssmq_filter_robust_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                           int64_t B, int64_t ld, int T, int iterations, int flags, const double *d_y, const double *d_m0,
                           const double *d_P0, const double *GQG, const double *R /* scale, [Y*Y] */, double dof, double *d_fm,
                           double *d_fP, double *d_lam /* [T][ld] */, double *d_delta /* [T][ld] */, int32_t *d_status);
/* Name of the kernel(s) ssmq_filter_robust_dev would run for this pair, iteration count and flags. */
int ssmq_robust_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                            const ssmq_integrand *f_obs, int64_t B, int iterations, int flags, char *buf, int len);

/*
 * Masked pass of the additive-noise Gaussian filters: missing components of y_k and a chi-square gate in front of the update.
 * d_mask [T][ld], uint32: bit i of mask[k][b] set = component i of y_k was observed (bits at or above Y are ignored); NULL: component
 * i is observed iff y_k[i] is not a NaN.  Per step the time update of ssmq_filter_forward_dev, ONE measurement transform at the prior
 * - at every step, whatever the mask -
 *     y^, P_h (no noise), C = measurement transform of (m-, P-)          S = P_h + R          e = y_k - y^
 * and with o = popcount(mask) and the subscript o selecting the observed rows and columns
 *     d2 = e_o' S_oo^-1 e_o          ll = -(o log 2 pi + log det S_oo + d2) / 2          (both 0 for o = 0)
 *     take = (o > 0) and not (d2 > gate[o])
 *     take:  K = C_o' S_oo^-1,  m = m- + K e_o,  P = P- - K S_oo K'          else:  m = m-,  P = P-  (bit for bit the prior)
 * (both triangles of fP from one value).  The observed rows are not compressed: the unobserved components are decoupled in place by
 * selects (e_i = 0, S_ii = 1, S_ij = S_ji = 0, C_i. = 0) and the Y x Y update runs; every term they contribute is an exact zero.  The
 * value under a cleared bit is never an operand: it may be anything, NaN and Inf included.
 * gate: HOST [Y + 1], entry o = the threshold for o observed components (the chi-square quantile with o degrees of freedom, say),
 * entry 0 ignored, +inf = no gate for that o; NULL: no gate.  An entry 1 .. Y that is NaN or <= 0, an R that is not finite and
 * symmetric, flags other than bit 0: SSMQ_E_ARG.
 * d_used [T][ld], uint32: the mask the update applied - 0 when nothing was offered or the gate rejected; d_nis [T][ld] = d2 and
 * d_loglik [T][ld] = ll: the scores of the OFFERED components, whether or not the gate then rejected them.  Other buffers as
 * ssmq_filter_forward_dev.
 * Failures: a factorisation that fails (P by the transforms - the measurement transform's counts at a fully masked step too, so the
 * status does not depend on the mask - or S_oo) or a mean that is not finite (an OBSERVED component that is NaN; a NaN d2 does not
 * gate, so the update runs and fails) makes the trajectory's outputs NaN and d_used 0 from that step on, d_status[b] = 1 + that step.
 * A trajectory's results do not depend on the batch around it.
 * One launch of k_masked_loop<> where the fused time loop has an instantiation for the pair (the dense kernels), and for a pair with a
 * user integrand in the range of ssmq_filter_forward_dev, compiled at run time; every other pair that ssmq_filter_innovations_dev
 * accepts - and every pair under SSMQ_NO_FUSED=1 or with flags bit 0 set - runs apply dyn | apply obs | k_masked_update per step.  What
 * ssmq_filter_innovations_dev refuses is refused here; every refusal comes before an output is touched.  Asynchronous on the library
 * stream.
 */
#define SSMQ_MASKED_LAUNCH_LOOP 1 /* flags bit 0 */
int ssmq_filter_masked_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                           int64_t B, int64_t ld, int T, int flags, const double *d_y, const uint32_t *d_mask /* [T][ld] or NULL */,
                           const double *d_m0, const double *d_P0, const double *GQG, const double *R /* [Y*Y] */,
                           const double *gate /* host [Y+1] or NULL */, double *d_fm, double *d_fP, uint32_t *d_used /* [T][ld] */,
                           double *d_nis /* [T][ld] */, double *d_loglik /* [T][ld] */, int32_t *d_status);
/* Name of the kernel(s) ssmq_filter_masked_dev would run for this pair and flags. */
int ssmq_masked_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                            const ssmq_integrand *f_obs, int64_t B, int flags, char *buf, int len);
/*
 * Detection masks for ssmq_filter_masked_dev, drawn on the device: bit i of d_mask[k][b] (uint32 [T][ld]) is set iff u < p_detect[i]
 * (host [Y], each in [0, 1]; 1 <= Y <= SSMQ_MAX_DIM), u a 53-bit uniform in (0, 1) from Philox4x32-10 keyed by `seed`, counter
 * (traj_offset + b lo, hi, k, 15 << 28 | i), its first two output words.  per_component = 0: one draw per (k, b) with i = 0 against
 * p_detect[0], and all Y bits go together (a scan is detected or it is not).  The bits depend on (seed, traj_offset + b, k, i) alone.
 * Asynchronous on the library stream.
 */
int ssmq_detection_mask_dev(int64_t B, int64_t ld, int T, int Y, const double *p_detect, uint64_t seed, uint64_t traj_offset,
                            int per_component, uint32_t *d_mask);

/*
 * Iterated posterior linearisation smoother (IPLS; Garcia-Fernandez, Svensson, Sarkka, IEEE TAC 2017) of the additive-noise Gaussian
 * filters, properly indexed: x_{-1} ~ N(m0, P0), step k = 0 .. T-1: x_k = f(x_{k-1}, k) + G q, y_k = h(x_k, k) + r.  One iteration
 * takes linearisation moments (ml_j, Pl_j), j = -1 .. T-1 (lower triangle read), and runs
 *   forward, k = 0 .. T-1, (m, P) the filtered moments of step k - 1 ((m0, P0) for k = 0):
 *     z, S_z, C_f = dynamics transform of (ml_{k-1}, Pl_{k-1})     F = C_f Pl_{k-1}^-1     Lambda = S_z - F Pl_{k-1} F'
 *     m- = z + F (m - ml_{k-1})     P- = F P F' + Lambda + G Q G'     C_k = P F'
 *     y^, S_y, C_h = measurement transform of (ml_k, Pl_k)         H = C_h Pl_k^-1         Omega = S_y - H Pl_k H'
 *     S = H P- H' + Omega + R     K = P- H' S^-1     m_k = m- + K (y_k - y^ - H (m- - ml_k))     P_k = P- - K S K'
 *   backward, k = T-1 .. 0, from (ms_{T-1}, Ps_{T-1}) = (m_{T-1}, P_{T-1}), the same bits:
 *     G_k = C_k (P-_k)^-1     ms_{k-1} = m_{k-1} + G_k (ms_k - m-_k)     Ps_{k-1} = P_{k-1} + G_k (Ps_k - P-_k) G_k'
 * down to the smoothed initial state (d_sm0, d_sP0).  Iteration 1 linearises at d_lin_m / d_lin_P (plane 0: the initial state, plane
 * 1 + k: step k) or, when both are NULL, at its own running moments - the plain filter step, so that iterations = 1 is
 * ssmq_filter_forward_dev up to rounding followed by an RTS pass; iteration i > 1 linearises at the smoothed moments of iteration
 * i - 1.  Outputs: the filtered (d_fm, d_fP) and smoothed (d_sm, d_sP, d_sm0, d_sP0) moments of the LAST iteration, both triangles
 * written from one value; d_delta [ld] or NULL: max over k = -1 .. T-1 and d of |ms_k[d] - ref_k[d]| / sqrt(Ps_k[d][d]) with ref the
 * smoothed means of the iteration before (d_lin_m in iteration 1; the filtered means without it) - there is no stopping rule.
 * 1 <= iterations <= SSMQ_ITERATED_MAX and flags == 0 (reserved), else SSMQ_E_ARG.
 * Failures: a factorisation that fails (Pl by the transforms, S, P-_k) or a filtered mean that is not finite, in any step of any
 * iteration, makes EVERY output of the trajectory NaN (delta included); d_status[b] = 1 + that step in the first iteration that
 * fails (forward sweep first), 0 otherwise.  A trajectory's results do not depend on the batch around it.
 * One launch of k_ipls_pass<> per iteration, for the pairs the fused time loop has a dense instantiation for and, compiled at run
 * time, for pairs with a user integrand (sigma-point and BQ forms, 2 .. 2 D + 1 points).  Everything else - other point counts,
 * linearisation, Taylor-GPQD, GPQ+D, truncated and multi-output transforms, models that take their noise as an argument - is
 * SSMQ_E_UNSUPPORTED, like every refusal before an output or d_status is touched.  The workspace (the planes the two sweeps share,
 * two sets of smoothed moments) is allocated per call.  Synchronous.
 */
int ssmq_smoother_iterated_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                               int64_t B, int64_t ld, int T, const double *d_y, const double *d_m0, const double *d_P0,
                               const double *GQG, const double *R, int iterations, int flags,
                               const double *d_lin_m /* [T+1][D][ld] or NULL */, const double *d_lin_P /* [T+1][D*D][ld] or NULL */,
                               double *d_fm, double *d_fP, double *d_sm, double *d_sP, double *d_sm0 /* [D][ld] */,
                               double *d_sP0 /* [D*D][ld] */, double *d_delta /* [ld] or NULL */, int32_t *d_status);
/* Name of the kernel ssmq_smoother_iterated_dev would run for this pair (SSMQ_E_UNSUPPORTED where it has none). */
int ssmq_smoother_iterated_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                       const ssmq_integrand *f_obs, int iterations, char *buf, int len);

/*
 * Kernel-parameter sweep of a BQ filter by measurement likelihood: the additive-noise Gaussian recursion of ssmq_filter_forward_dev for
 * P rows of kernel parameters ("theta") on B measurement sequences in ONE launch (k_filter_sweep<>), of which only the scores are kept.
 * Row p pairs par_dyn[p] with par_obs[p] (not Cartesian).  Per item (p, b), with (m, P) = (x0_mean, x0_cov) and the weights of row p,
 * for k = 0 .. T-1 (both transforms use time index k):
 *     m-, P-  = dynamics transform of (m, P) + G Q G';      y^, S, C = measurement transform of (m-, P-) + R;      e = y_k - y^
 *     nis_k = e' S^-1 e (Cholesky of S);   ll_k = -(Y log 2 pi + log det S + nis_k) / 2 = log p(y_k | y_1..k-1)
 *     K = C' S^-1;   m = m- + K e;   P = P- - K S K'
 * - step by step what ssmq_filter_forward_dev followed by ssmq_filter_innovations_dev computes with the dense kernels -, and
 *     d_loglik_total[p][b] = sum_k ll_k,   d_nis_mean[p][b] = sum_k nis_k / T   (ascending k),   d_loglik_steps[p][k][b] = ll_k.
 * The filtered moments are never stored.
 *   kind_dyn / kind_obs        SSMQ_SWEEP_GP (ssmq_weights_gp) or SSMQ_SWEEP_BS (ssmq_weights_bs, with mulind_* [D*NB_*]; NULL / 0 for GP)
 *   xi_dyn [D*N_dyn], xi_obs [D*N_obs]   unit sigma points, row-major (host);  jitter_*: as the weights entry points take it
 *   par_dyn, par_obs [P][1+D]  rows [alpha, ell_1 .. ell_D] (host)
 *   d_y [T][Y][ld] (device);  x0_mean [D], x0_cov [D*D], GQG [D*D], R [Y*Y] (host; NULL GQG / R = zeros)
 *   d_loglik_total, d_nis_mean [P][ld];  d_loglik_steps [P][T][ld] or NULL;  d_status [P][ld] int32 (device);  theta_status [P] (host)
 * ld is a multiple of 64 (every wave belongs to one row).  Failures: theta_status[p] = (status of the dynamics weights) + 4 (status of
 * the measurement weights), as ssmq_weights_gp / ssmq_weights_bs report them; a row with a non-zero value is NaN and has d_status -1.
 * An item's d_status is otherwise 1 + the first step whose scores are not numbers (a factorisation failed, a measurement is not
 * finite) - the totals and the remaining steps are then NaN - or 0.  An item's results do not depend on the items around it.
 * Range: the 'rbf' kernel, the built-in additive-noise model pairs the fused time loop is instantiated for, D <= 6, Y <= 4,
 * 2 <= N_dyn = N_obs <= 2 D + 1; user-defined integrands, models that take their noise as an argument, other kinds and point counts
 * beyond 2 D + 1 return SSMQ_E_UNSUPPORTED (bad arguments SSMQ_E_ARG) with the range in ssmq_last_error(), before any output is
 * touched.  B == 0: only theta_status is written; T == 0: the totals are zero.  Synchronous.
 */
#define SSMQ_SWEEP_GP 0
#define SSMQ_SWEEP_BS 1
int ssmq_filter_sweep_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int kind_dyn, int kind_obs, const double *xi_dyn,
                          int N_dyn, const double *xi_obs, int N_obs, const int32_t *mulind_dyn, int NB_dyn, const int32_t *mulind_obs,
                          int NB_obs, const double *par_dyn, const double *par_obs, int P, double jitter_dyn, double jitter_obs, int D,
                          int Y, int64_t B, int64_t ld, int T, const double *d_y, const double *x0_mean, const double *x0_cov,
                          const double *GQG, const double *R, double *d_loglik_total, double *d_nis_mean, double *d_loglik_steps,
                          int32_t *d_status, int32_t *theta_status);
/* Name of the kernel ssmq_filter_sweep_dev would run for this pair (the same refusals). */
int ssmq_filter_sweep_kernel_name(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int kind_dyn, int kind_obs, int N_dyn,
                                  int N_obs, int D, int Y, char *buf, int len);

/*
 * Student-t measurement likelihood of a Studentian pass: the recursion of ssmq_student_filter_forward_dev for B measurement
 * sequences in ONE launch (k_filter_score<>), of which only the scores are kept.  Every trajectory starts from (x0_mean, x0_smat).
 * Per step k = 0 .. T-1, with the weights in the two handles (dense kernels, no fast path) and (m, S) the running mean and scale matrix:
 *     m-, S-  = scale[k] * (dynamics transform of (m, S)) + GqG;    y^, S_y, S_yx = scale[k] * (measurement transform of (m-, S-)) + r_smat
 *     e = y_k - y^;   nis_k = Delta^2 = e' S_y^-1 e (Cholesky of S_y)
 *     ll_k = lgamma((dof + Y) / 2) - lgamma(dof / 2) - Y / 2 log(dof pi) - 1/2 log det S_y - (dof + Y) / 2 log1p(Delta^2 / dof)
 *     K = S_yx' S_y^-1;   m = m- + K e;   S = (dof + Delta^2) / (dof + Y) * (S- - K S_y K')
 * The update is the conditional of a joint Student t with `dof` degrees of freedom and these scale blocks; ll_k is the log-density of
 * the marginal of y_k under the same joint, t_dof(y^, S_y) - so `dof` is the filter's dof, the one in the update factor, not the
 * dof_pr behind scale[k].  The expected value of nis_k under that density is Y dof / (dof - 2).
 *   x0_mean [D], x0_smat [D*D], GqG [D*D], r_smat [Y*Y], scale [T]: host arrays as for ssmq_student_filter_forward_dev (NULL GqG / r_smat
 *   = zeros);  d_y [T][Y][ld] (device);  d_nis, d_loglik [T][ld] or NULL;  d_loglik_total, d_nis_mean [ld];  d_status [ld] int32:
 *   1 + the first step whose scores are not numbers (a factorisation failed, a measurement is not finite) - the totals and the
 *   remaining steps are then NaN - or 0.  ld is a multiple of 64.  A trajectory's results do not depend on the trajectories around it.
 * Range: both handles t-process BQ transforms (tp_nu > 0) or both sigma-point rules, on the built-in additive-noise model pairs of the
 * fused time loop with D <= 4, Y <= 2 and 2 <= N_dyn = N_obs <= 2 D + 1 points; dof > 2.  User-defined integrands, models that take
 * their noise as an argument, truncated / multi-output / GPQ+D / Taylor-GPQD / plain GP or Bayes-Sard handles and shapes without an
 * instantiation return SSMQ_E_UNSUPPORTED (bad arguments SSMQ_E_ARG) with the range in ssmq_last_error(), before any launch.
 * T == 0: the totals are zero.  Synchronous.
 */
int ssmq_student_scores_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                            int64_t B, int64_t ld, int T, const double *d_y, const double *x0_mean, const double *x0_smat,
                            const double *GqG, const double *r_smat, const double *scale, double dof, double *d_nis, double *d_loglik,
                            double *d_loglik_total, double *d_nis_mean, int32_t *d_status);
/* Name of the kernel ssmq_student_scores_dev would run for this pair (the same refusals). */
int ssmq_student_scores_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                    const ssmq_integrand *f_obs, char *buf, int len);

/*
 * Sweep of a t-process filter by measurement likelihood: ssmq_filter_sweep_dev for the filters whose transforms are t-process
 * quadratures, over P rows of (par_dyn[p], par_obs[p], nu_dyn[p], nu_obs[p], dof[p]) in ONE launch of k_filter_score<>.
 *   recursion  SSMQ_RECURSION_GAUSS: the Gaussian recursion and score of ssmq_filter_sweep_dev (StudentProcessKalmanSweep); dof and scale
 *              are not read.  SSMQ_RECURSION_STUDENT: the recursion and Student-t score of ssmq_student_scores_dev
 *              (StudentProcessStudent) with dof[p] > 2 and the scale table scale[p][0 .. T-1].
 *   The weights of both transforms come from one theta-batched ssmq_weights_gp call each ('rbf' kernel), with its iK output: the
 *   model variance of a transform is (nu - 2 + fx iK fx') / (nu - 2 + N) * model_var, added as the whole matrix where the transform
 *   has more than one output (the t-process filters build their transforms with one output).
 *   x0_mean [D] is shared; x0_mat [P][D*D], GQG [P][D*D], R [P][Y*Y] are PER ROW (host; NULL GQG / R = zeros): in the Studentian
 *   recursion they are scale matrices and change with (dof[p] - 2) / dof[p].
 *   Everything else - xi_*, par_*, jitter_*, d_y, the outputs, d_status and theta_status - as ssmq_filter_sweep_dev.
 * Range and refusals: as ssmq_student_scores_dev; P <= 65535.  B == 0: only theta_status is written; T == 0: the totals are zero.
 * Synchronous.
 */
#define SSMQ_RECURSION_GAUSS 0
#define SSMQ_RECURSION_STUDENT 1
int ssmq_filter_sweep_t_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int recursion, const double *xi_dyn, int N_dyn,
                            const double *xi_obs, int N_obs, const double *par_dyn, const double *par_obs, const double *nu_dyn,
                            const double *nu_obs, const double *dof, int P, double jitter_dyn, double jitter_obs, int D, int Y, int64_t B,
                            int64_t ld, int T, const double *d_y, const double *x0_mean, const double *x0_mat, const double *GQG,
                            const double *R, const double *scale, double *d_loglik_total, double *d_nis_mean, double *d_loglik_steps,
                            int32_t *d_status, int32_t *theta_status);
/* Name of the kernel ssmq_filter_sweep_t_dev would run for this pair and recursion (the same refusals). */
int ssmq_filter_sweep_t_kernel_name(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int recursion, int N_dyn, int N_obs, int D,
                                    int Y, char *buf, int len);

/*
 * Noise sweep of a Gaussian filter by measurement likelihood: the sibling of ssmq_filter_sweep_dev that keeps the weights - the two
 * transform handles, as ssmq_filter_forward_dev takes them - shared and varies the process-noise term G Q G', the measurement-noise
 * covariance R and the initial moments per row, for P rows on B measurement sequences in ONE launch (k_noise_sweep<>), of which only
 * the scores are kept.  Per item (p, b), with (m, P) = row p of x0 and the recursion of ssmq_filter_sweep_dev,
 *     m-, P- = dynamics transform of (m, P) + gqg[p];   y^, S, C = measurement transform of (m-, P-) + rr[p];   nis_k, ll_k;   update
 * - step by step what ssmq_filter_forward_dev followed by ssmq_filter_innovations_dev computes with the dense kernels for a filter
 * whose noise covariances and initial moments are those of row p -, and
 *     d_loglik_total[p][b] = sum_k ll_k,   d_nis_mean[p][b] = sum_k nis_k / T   (ascending k),   d_loglik[p][k][b] = ll_k.
 * The filtered moments are never stored.
 *   recursion      SSMQ_RECURSION_GAUSS; SSMQ_RECURSION_STUDENT (a Studentian pass) is refused
 *   d_y [T][Y][ld] (device), ld a multiple of 64 (every wave belongs to one row)
 *   gqg [P or 1][D*D], rr [P or 1][Y*Y], x0 [P or 1][D + D*D] = m0 | P0 (lower triangle read): host arrays, each with its own row stride
 *   in doubles - the row size, or 0 for ONE row shared by all P (NULL gqg / rr = zeros).  Every entry is finite; whether a row is
 *   positive definite is not checked: an indefinite row fails in its first factorisation and shows up in d_status.
 *   d_loglik_total, d_nis_mean [P][ld];  d_loglik [P][T][ld] or NULL;  d_status [P][ld] int32 (device): 1 + the first step whose scores
 *   are not numbers - the totals and the remaining steps of that item are then NaN - or 0.  An item's results do not depend on the
 *   items around it.
 * Range: both handles sigma-point rules, both GP / Bayes-Sard transforms or both t-process BQ transforms, on the built-in
 * additive-noise model pairs and point counts the fused time loop is instantiated for (D <= 6, Y <= 4, N_dyn = N_obs).  User-defined
 * integrands, handles of two different forms, linearisation / Taylor-GPQD / GPQ+D / truncated / multi-output handles, a Studentian pass,
 * models that take their noise as an argument and shapes without an instantiation return SSMQ_E_UNSUPPORTED; null or ill-sized
 * arguments, a stride that is neither 0 nor the row size, a non-finite entry of a row array and P < 1 return SSMQ_E_ARG - both with the
 * range in ssmq_last_error(), before any output is touched.  T == 0: the totals are zero.  Synchronous.
 */
int ssmq_filter_noise_sweep_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs,
                                int recursion, int64_t B, int64_t ld, int T, const double *d_y, int P, const double *gqg,
                                int64_t gqg_stride, const double *rr, int64_t rr_stride, const double *x0, int64_t x0_stride,
                                double *d_loglik_total, double *d_nis_mean, double *d_loglik, int32_t *d_status);
/* Name of the kernel ssmq_filter_noise_sweep_dev would run for this pair (the same range check; no launch). */
int ssmq_filter_noise_sweep_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                        const ssmq_integrand *f_obs, int recursion, char *buf, int len);

/*
 * Interacting multiple-model (IMM) filter over noise modes (Blom & Bar-Shalom 1988), the whole pass in ONE launch (k_imm_loop<>): M
 * mode-matched filters of the two transform handles - mode j is the filter with the rows gqg[j], rr[j], x0[j], as a row of
 * ssmq_filter_noise_sweep_dev - exchange moments every step through the Markov mixing probabilities and are weighted by the per-step
 * measurement likelihood.  Everything fp64, the time convention of ssmq_filter_forward_dev.  Per trajectory and step k, every sum over
 * modes in ascending mode index, with mu = mu0 before step 0:
 *     c_j = sum_i pi[i][j] mu_i;   w_ij = pi[i][j] mu_i / c_j   (c_j == 0: w_ij = delta_ij, a mode nobody can reach keeps its moments)
 *     m0_j = sum_i w_ij m_i;       P0_j = sum_i w_ij (P_i + (m_i - m0_j)(m_i - m0_j)')
 *     (m_j, P_j, ll_j) = the step of ssmq_filter_noise_sweep_dev for row j from (m0_j, P0_j)
 *     a_j = log c_j + ll_j (-inf when c_j == 0);   amax = max_j a_j;   loglik[k] = amax + log sum_j exp(a_j - amax);
 *     mu_j = exp(a_j - loglik[k]);   fm[k] = sum_j mu_j m_j;   fP[k] = sum_j mu_j (P_j + (m_j - fm)(m_j - fm)')
 *   pi [M][M] (host): pi[i][j] the probability of going from mode i to mode j; mu0 [M] (host): the initial mode probabilities.  Every
 *   entry finite and non-negative, every row of pi and mu0 summing to 1 within 1e-12 (else SSMQ_E_ARG, the row named), 1 <= M <= 8.
 *   d_y, gqg, rr, x0 and their strides: as ssmq_filter_noise_sweep_dev, with M for P.
 *   d_fm [T][D][ld], d_fP [T][D*D][ld] (both triangles from the one value), d_mode_prob [T][M][ld], d_loglik [T][ld],
 *   d_loglik_total [ld] (ascending k), d_status [ld] int32 (device).  A trajectory fails as a whole: the first step at which a mode's
 *   scores or a mixed quantity is not a finite number sets status = 1 + k; from that step on every output of the trajectory, and its
 *   total, is NaN.  A trajectory's results do not depend on the batch around it.
 * Range and refusals: those of ssmq_filter_noise_sweep_dev (SSMQ_E_UNSUPPORTED / SSMQ_E_ARG with the range in ssmq_last_error(), before
 * any output is touched).  T == 0: the totals are zero.  Synchronous.
 */
int ssmq_filter_imm_dev(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs, const ssmq_integrand *f_obs, int recursion,
                        int64_t B, int64_t ld, int T, const double *d_y, int M, const double *gqg, int64_t gqg_stride, const double *rr,
                        int64_t rr_stride, const double *x0, int64_t x0_stride, const double *pi, const double *mu0, double *d_fm, double *d_fP,
                        double *d_mode_prob, double *d_loglik, double *d_loglik_total, int32_t *d_status);
/* Name of the kernel ssmq_filter_imm_dev would run for this pair (the same range check; no launch). */
int ssmq_filter_imm_kernel_name(const ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, const ssmq_transform *h_obs,
                                const ssmq_integrand *f_obs, int recursion, char *buf, int len);

/*
 * Bootstrap particle filter (sequential Monte Carlo; Gordon, Salmond, Smith 1993) of the additive-noise models: the ground truth the
 * moment-matching filters are measured against.  N weighted particles per trajectory, in the time convention of
 * ssmq_filter_forward_dev (both models of step j, 0-based, are evaluated at time j):
 *     x_{-1,i} = m0_b + chol(P0_b) z                                            initial particles, log w_{-1,i} = -log N
 *     x_{j,i}  = f(x_{j-1,a(i)}, j) + G (q_mean + L_q z)                        j = 0 .. T-1, a(i) the ancestors chosen after step j-1
 *     log w_{j,i} = log w_{j-1,a(i)} + log p(y_j | h(x_{j,i}, j))               Gaussian noise: N(y; h + r_mean, R);  Student-t noise:
 *                                                                               const - (dof + Y) / 2 log(1 + delta^2 / dof), scale R
 * Per step, in this order: log-sum-exp normalisation with the maximum subtracted; ll[j] = log sum_i w~_{j-1,i} p(y_j | x_{j,i}) with w~ the
 * normalised weights before the step; fm[j] = sum w~ x; fP[j] = sum w~ (x - fm)(x - fm)' by a second pass around the mean (both
 * triangles written from one value); ess[j] = 1 / sum w~^2; then systematic resampling - always if ess_threshold >= 1, never if
 * ess_threshold <= 0, else when ess[j] < ess_threshold N: one uniform u_j, positions p_i = (i + u_j) / N, the CDF the inclusive prefix
 * sum of w~ with its last entry forced to 1, a(i) the smallest m with cdf[m] > p_i, the weights reset to 1 / N.  Without resampling
 * a(i) = i.
 * Random numbers: Philox4x32-10 keyed by `seed`, counter (traj_offset + b lo, hi, step, tag), tag = purpose << 28 | particle << 4 | pair,
 * normals by Box-Muller, two per counter (pair p gives z[2 p], z[2 p + 1]).  Purpose 8: the initial particles (step 0); 9: the process
 * noise of step j; 10: the resampling uniform of step j (particle 0, pair 0).  These tags lie above every tag of ssmq_simulate*_dev, so
 * a filter run with the seed of its data is independent of the data.  Every sum and the prefix sum run in an order fixed by N alone:
 * a trajectory's bits depend on seed, its global index traj_offset + b, N, ess_threshold and its own inputs - not on B or the device.
 * Buffers: d_y [T][Y][ld], d_m0 [D][ld], d_P0 [D*D][ld] (lower triangle read) as for ssmq_filter_forward_dev; outputs d_fm [T][D][ld],
 * d_fP [T][D*D][ld], d_status [ld] in the layout of the Gaussian filters (ssmq_error_sums_dev and ssmq_traj_scores_dev take them
 * unchanged); d_loglik [T+1][ld], row T the total (summed in ascending j); d_ess [T][ld].  Host arrays: q_mean [dq] (NULL = 0), q_chol
 * [dq*dq] lower factor, G [D*dq] (NULL = eye(D, dq)); r: SSMQ_RV_GAUSS or SSMQ_RV_STUDENT of dimension Y with n_comp <= 1, chol the lower
 * factor of R (the scale matrix for Student-t; dof > 0), mean NULL = 0.  Optional outputs, each may be NULL - together the weighted
 * posterior sample: d_part [T][D][B][N] the particles of step j after propagation; d_logw [T][B][N] their normalised log-weights after
 * the measurement of step j, before resampling; d_anc [T][B][N] int32 the ancestors chosen after step j (the identity without resampling).
 * Failures: a step whose largest log-weight is not finite (a NaN measurement, a NaN among the weights, every particle at zero
 * likelihood) fails the trajectory: d_status[b] = 1 + j, and fm, fP, loglik (the total included) and ess are NaN from step j on (d_logw
 * NaN and d_anc -1 from step j, d_part NaN from step j + 1); other trajectories are unaffected.
 * Range: built-in integrands with additive noise, the transition without a state index; 1 <= D <= 6, 1 <= Y <= 4, 1 <= dq <= 6; N a
 * multiple of 64, 64 <= N <= 4096, (2 D + 1) N <= 13312 (the cloud lives in LDS: 104 KB).  User integrands, SSMQ_F_UNGMNA_*,
 * SSMQ_F_CTRS_DYN (noise as an argument), SSMQ_RV_MIXTURE noise and larger shapes are SSMQ_E_UNSUPPORTED; an N that is no multiple of
 * 64 or below 64, T < 1, a NaN ess_threshold, null pointers and mismatched dimensions SSMQ_E_ARG - both before the device, an output or
 * d_status is touched.  B == 0: nothing happens.  One launch of k_particle_filter<D> (one trajectory per workgroup of 256 threads,
 * particle i on thread i mod 256, the time loop inside).  Synchronous.
 */
int ssmq_particle_filter_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N, int64_t B, int64_t ld,
                             int T, const double *d_y, const double *d_m0, const double *d_P0, const double *q_mean,
                             const double *q_chol, const double *G, const ssmq_rv *r, double ess_threshold, uint64_t seed,
                             uint64_t traj_offset, double *d_fm, double *d_fP, double *d_loglik, double *d_ess, int32_t *d_status,
                             double *d_part, double *d_logw, int32_t *d_anc);
/* Name of the kernel ssmq_particle_filter_dev would run, with the LDS it requests: the range check of that call without a device
 * (the same return codes; T is not part of it). */
int ssmq_particle_kernel_name(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N, const ssmq_rv *r,
                              char *buf, int len);

/*
 * Particle smoothers over the cloud ssmq_particle_filter_dev wrote (d_part, d_logw, d_anc of one call, with its d_fm, d_fP, d_ess and
 * d_status): the ground truth the Gaussian smoothers are measured against, E[x_k | y_0..T-1] and the covariance.  Per trajectory, in the
 * filter's time convention: x_k^i the particles of step k after propagation, lw_k^i their normalised log-weights after the measurement
 * of step k (before resampling), a_k(i) the ancestors chosen after step k.
 *
 * SSMQ_PS_MARGINAL - the marginal forward-filter backward-smoother (FFBSm; Doucet, Godsill, Andrieu 2000), for process noise of full
 * rank: dq == D and Sigma = G Q G' positive definite, Ls = chol(Sigma).  With
 *     alpha_k^i = Ls^-1 (f(x_k^i, k + 1) + G q_mean),   beta_{k+1}^j = Ls^-1 x_{k+1}^j,   d2_ij = |beta_{k+1}^j - alpha_k^i|^2
 * (the Gaussian normalising constant cancels), entirely in the log domain:
 *     ls_{T-1}^i = lw_{T-1}^i
 *     lv_j       = logsumexp_i ( lw_k^i - d2_ij / 2 )                         for every j of step k + 1
 *     ls_k^i     = lw_k^i + logsumexp_j ( ls_{k+1}^j - lv_j - d2_ij / 2 )     for every i of step k,  k = T-2 .. 0
 * and ls_k is then normalised (in exact arithmetic its log-sum-exp is already 0).  Every log-sum-exp is a sweep for the maximum followed
 * by a sweep for the sum of exp(. - max), both in ascending order of the index summed over.  Terms with a log-weight of -inf contribute
 * nothing; a lv_j of -inf is skipped (it can only belong to a particle whose own smoothed weight is -inf).  sm[k], sP[k] are the mean
 * and the covariance (second pass around the mean, both triangles from one value) of the cloud x_k under exp(ls_k), as the filter's;
 * ess_s[k] = 1 / sum exp(2 ls_k).  O(N^2) transition densities per step and trajectory; deterministic given the forward pass - no
 * random numbers.
 *
 * SSMQ_PS_GENEALOGY - ancestor tracing, for every model the filter covers (singular G Q G' included, where the transition has no
 * density on the state space and FFBSm does not exist):
 *     idx_{T-1}(j) = j,   idx_k(j) = a_k(idx_{k+1}(j)),   k = T-2 .. 0
 * sm[k], sP[k] are the moments of x_k[:, idx_k(j)], j = 0 .. N-1, under the final weights exp(lw_{T-1}^j); ess_s[k] = 1 / sum
 * exp(2 lw_{T-1}^j) for every k; d_unique[k] is the number of distinct idx_k(j) - the path-degeneracy diagnostic: where it has fallen to
 * a few, the estimate of step k has collapsed.  A gather, not a scatter-add: the sums run over j in the filter's fixed order.
 *
 * Both: step T-1 is the filter's - fm, fP and ess of that step are copied, bit for bit.  The smoothed initial state x_{-1} is not
 * computed (the filter does not keep its initial cloud).  All sums run in the filter's order, fixed by N alone: a trajectory's bits
 * depend on its own cloud and N, not on B or on how a batch is split over calls.
 * Buffers: d_part [T][D][B][N], d_logw [T][B][N], d_anc [T][B][N] int32 (read by SSMQ_PS_GENEALOGY only; may be NULL otherwise), d_fm
 * [T][D][ld], d_fP [T][D*D][ld], d_ess [T][ld], d_status [ld] as the filter left them; outputs d_sm [T][D][ld], d_sP [T][D*D][ld] in
 * the layout of the Gaussian smoothers (with d_status the triple ssmq_error_sums_dev and ssmq_traj_scores_dev take), d_ess_s [T][ld].
 * Optional outputs, each may be NULL: d_logw_s [T][B][N] the normalised smoothed log-weights ls_k (genealogy: the final weights,
 * repeated); genealogy only: d_lineage [T][B][N] int32 idx_k(j), d_unique [T][ld] int32.  Host arrays: q_mean [dq] (NULL = 0), q_chol
 * [dq*dq] lower factor of Q, G [D*dq] (NULL = eye(D, dq)) - the filter's; SSMQ_PS_GENEALOGY reads none of the three.
 * Failures: a trajectory whose d_status is not 0 gets NaN in d_sm, d_sP, d_ess_s and d_logw_s (-1 in d_lineage and d_unique) at every
 * step; its status stays, other trajectories are untouched.
 * Range: the filter's (built-in integrand with additive noise, no state index, 1 <= D <= 6, 1 <= dq <= 6, N a multiple of 64 in
 * 64 .. 4096 with (2 D + 1) N <= 13312).  SSMQ_E_UNSUPPORTED, the reason named: SSMQ_PS_MARGINAL with dq != D or with G Q G' not
 * positive definite (use SSMQ_PS_GENEALOGY), and what the filter refuses.  SSMQ_E_ARG: a condition number of G Q G' above 1e12, an
 * unknown method, T < 1, ld < B, null pointers, an N that is no multiple of 64 - all before the device, an output or d_status is
 * touched.  B == 0: nothing happens.  One launch of k_particle_smooth<D> (LDS: alpha, beta [D][N] and two [N] rows, (2 D + 2) N doubles
 * and the reduction scratch - at most 128 KB + 768 B) or k_particle_lineage<D>: one trajectory per workgroup of 256 threads, particle i
 * on thread i mod 256, the loop over k inside.  Synchronous.
 */
enum { SSMQ_PS_MARGINAL = 0, SSMQ_PS_GENEALOGY = 1 };
int ssmq_particle_smoother_dev(const ssmq_integrand *f_dyn, int D, int dq, int N, int64_t B, int64_t ld, int T, const double *q_mean,
                               const double *q_chol, const double *G, int method, const double *d_part, const double *d_logw,
                               const int32_t *d_anc, const double *d_fm, const double *d_fP, const double *d_ess,
                               const int32_t *d_status, double *d_sm, double *d_sP, double *d_ess_s, double *d_logw_s,
                               int32_t *d_lineage, int32_t *d_unique);
/* Name of the kernel ssmq_particle_smoother_dev would run, with the LDS it requests: the range check of that call without a device
 * (the same return codes; B, T and the device buffers are not part of it). */
int ssmq_particle_smoother_kernel_name(const ssmq_integrand *f_dyn, int D, int dq, int N, const double *q_mean, const double *q_chol,
                                       const double *G, int method, char *buf, int len);

/*
 * The particle filter and its smoothers with a heavy-tailed initial state and process noise: the four entry points above, except that
 * the initial state x0 and the process noise q are described by ssmq_rv, as in ssmq_simulate_rv_dev.  Kinds: SSMQ_RV_GAUSS, or
 * SSMQ_RV_STUDENT with one component - a draw is v = mean + chol z / sqrt(u), u ~ Gamma(dof / 2, scale 2 / dof), the construction of
 * ssmq_simulate_rv_dev - in any combination of the two sides.
 *   x0: only kind and dof are read.  The per-trajectory planes d_m0 / d_P0 keep their role: x_{-1,i} = m0_b + chol(P0_b) z / sqrt(u);
 *       for a Student-t initial state d_P0 holds the SCALE matrix, not the covariance.
 *   q:  kind, dim (= dq), n_comp (<= 1), dof, mean [dq] (NULL = 0) and chol [dq*dq], the lower factor of Q (Student-t: of the scale
 *       matrix) - what q_mean / q_chol are above.
 * Random numbers: z from the counters of ssmq_particle_filter_dev (purposes 8 and 9); u by Marsaglia-Tsang, one per particle and draw,
 * attempt t = 0 .. 15 in the low four bits of the tag (the pair field): purpose 11 the normal and 12 the uniform of attempt t for the
 * initial particle (step 0), 13 the normal and 14 the uniform for the process noise of step j.  No counter is used twice; a side that
 * is Gaussian draws no u.  A trajectory's bits depend on seed, its global index, N, ess_threshold and its own inputs, as above.
 * Smoothers: SSMQ_PS_GENEALOGY reads no density and is unchanged.  SSMQ_PS_MARGINAL with Student-t process noise of full rank (dq == D,
 * G Q G' positive definite, Q the scale matrix): x_{k+1} | x_k is Student-t with location f(x_k, k + 1) + G q_mean, scale G Q G' and
 * q's dof, so with the whitened d2_ij above  log p = const - (dof + D) / 2 log1p(d2_ij / dof)  takes the place of -d2_ij / 2 in both
 * log-sum-exps (the constant cancels in the normalisation); everything else is the recursion above.
 * With SSMQ_RV_GAUSS on both sides the entries launch the kernels of the four entry points above on the same arguments and return
 * their bits; otherwise k_particle_filter<D, QK=1> / k_particle_smooth<D, QK=1>, the same mapping and LDS.
 * Range: that of the entry points above, and SSMQ_RV_STUDENT with dof >= 2 (the Gamma sampler needs the shape dof / 2 >= 1):
 * SSMQ_RV_MIXTURE for x0 or q and 0 < dof < 2 are SSMQ_E_UNSUPPORTED, the range named; a null descriptor, an unknown kind, q->dim != dq,
 * q->n_comp > 1, a null q->chol, a dof that is not finite and positive SSMQ_E_ARG - before the device or an output is touched.
 */
int ssmq_particle_filter_rv_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N, int64_t B,
                                int64_t ld, int T, const double *d_y, const double *d_m0, const double *d_P0, const ssmq_rv *x0,
                                const ssmq_rv *q, const double *G, const ssmq_rv *r, double ess_threshold, uint64_t seed,
                                uint64_t traj_offset, double *d_fm, double *d_fP, double *d_loglik, double *d_ess, int32_t *d_status,
                                double *d_part, double *d_logw, int32_t *d_anc);
int ssmq_particle_kernel_name_rv(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int N, const ssmq_rv *x0,
                                 const ssmq_rv *q, const ssmq_rv *r, char *buf, int len);
int ssmq_particle_smoother_rv_dev(const ssmq_integrand *f_dyn, int D, int dq, int N, int64_t B, int64_t ld, int T, const ssmq_rv *q,
                                  const double *G, int method, const double *d_part, const double *d_logw, const int32_t *d_anc,
                                  const double *d_fm, const double *d_fP, const double *d_ess, const int32_t *d_status, double *d_sm,
                                  double *d_sP, double *d_ess_s, double *d_logw_s, int32_t *d_lineage, int32_t *d_unique);
int ssmq_particle_smoother_kernel_name_rv(const ssmq_integrand *f_dyn, int D, int dq, int N, const ssmq_rv *q, const double *G, int method,
                                          char *buf, int len);

/*
 * Posterior Cramer-Rao lower bound (Tichavsky, Muravchik, Nehorai 1998) of the additive-Gaussian-noise models: the floor no filter of
 * a study can get under, E[(x_j - m_j)(x_j - m_j)'] >= J_j^-1 for every estimator m_j of x_j from y_0 .. y_j.  Input: the true states,
 * planes p_0 .. p_T as ssmq_simulate*_dev with T + 1 steps writes them (p_0 ~ the initial state, p_{j+1} the state the filters call x_j).
 * In the filters' time convention (both models of step j at time j), per trajectory
 *     F_j = df/dx (p_j, j)  (D x D),     H_j = dh/dx (p_{j+1}, j)  (Y x D, placed into the state's columns as the linearisation
 *     transform places it: through the state index, or - a built-in one-column Jacobian without one - into every column),
 * and with Qi = (G Q G')^-1, Ri = R^-1, for j = 0 .. T-1:
 *     D11_j = mean_b F_j' Qi F_j,     D12_j = -(mean_b F_j)' Qi,     D22_j = Qi + mean_b H_j' Ri H_j,
 *     J_j = D22_j - D12_j' (J_{j-1} + D11_j)^-1 D12_j,     J_{-1} = P0^-1.
 * Two phases, as the error sums: ssmq_pcrlb_sums_dev adds over this rank's B trajectories, the sums of all ranks are added (one
 * all-reduce), ssmq_pcrlb_finalize divides by the total count and runs the recursion on the host.
 *
 * ssmq_pcrlb_sums_dev: d_x [T+1][D][ld] device planes; q: the process noise, r: the measurement noise - SSMQ_RV_GAUSS with chol the
 * lower factor of Q [dq*dq] / R [Y*Y] (their means are not read); G [D*dq] (NULL = eye(D, dq)); host arrays.  sums: host [T][S],
 * S = ssmq_pcrlb_sums_width(D) = D (D + 1) / 2 + D D + D (D + 1) / 2, row j:
 *     sum_b F_j' Qi F_j, lower triangle packed (entry (i, k), k <= i, at i (i + 1) / 2 + k)  |  sum_b F_j, row-major [D][D]  |
 *     sum_b H_j' Ri H_j, lower triangle packed.
 * Sums, not means.  Summation order (fixed: the bits depend on B and the states alone, not on ld, the grid or the device): the
 * trajectories of a step in groups of 256 consecutive ones; inside a group the 64 lanes of a wave by a butterfly (l ^ 32, 16, .. 1),
 * then the four waves as (w0 + w1) + (w2 + w3); then the groups in ascending order.  Lanes b >= B contribute exact zeros and their
 * columns are not read.  A non-finite term is not masked: it makes the sums of its step non-finite, which the finaliser reports.
 * Kernels: k_pcrlb_dyn<D, D> / k_pcrlb_obs<D, Y> for the built-in models that have a Jacobian, k_pcrlb_dyn_fn / k_pcrlb_obs_fn compiled
 * at run time for a user integrand registered with one (ssmq_integrand_define_dx) - one kernel per model, so the two kinds pair freely;
 * one trajectory per lane, one row of partial sums per (step, group) in a workspace; k_pcrlb_rows adds the rows of a step.  No atomics.
 * Refusals, all before a device is looked for or `sums` is touched.  SSMQ_E_UNSUPPORTED, the range named: a model that takes its noise
 * as an argument; a model without a Jacobian on the device; Student-t or mixture noise; D > 6 or Y > 4; dq != D or G Q G' not positive
 * definite.  SSMQ_E_ARG: a condition number of G Q G' above 1e12, a factor of R without a positive diagonal, T < 1, ld < B, B < 0, null
 * pointers, mismatched dimensions.  B == 0: the sums are zeros.  Synchronous.
 */
int ssmq_pcrlb_sums_width(int D);
int ssmq_pcrlb_sums_dev(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, int64_t B, int64_t ld, int T,
                        const double *d_x, const ssmq_rv *q, const double *G, const ssmq_rv *r, double *sums);
/* Names of the two kernels ssmq_pcrlb_sums_dev would run: the range check of that call without a device (the same return codes; B, ld, T
 * and d_x are not part of it). */
int ssmq_pcrlb_kernel_name(const ssmq_integrand *f_dyn, const ssmq_integrand *f_obs, int D, int Y, int dq, const ssmq_rv *q,
                           const double *G, const ssmq_rv *r, char *buf, int len);
/* The recursion from the (all-reduced) sums of B_total trajectories, on the host in double; no device.  P0 [D*D] the covariance of the
 * initial state (lower triangle read), q / G as above (Qi is formed from them again; dq must equal D).  Per step a Cholesky
 * factorisation of J_{j-1} + D11_j and one of J_j.  Outputs, each may be NULL: info [T][D*D] J_j, bound [T][D*D] J_j^-1 (both symmetric,
 * both triangles from one value), rmse_bound [T] sqrt(trace J_j^-1).  *status: 0, or 1 + j for the first step j with a non-finite sum
 * or a non-positive pivot - the outputs of the steps before it stand, those from step j on are NaN; a P0 that is not positive definite
 * is status 1.  Returns SSMQ_OK also then; SSMQ_E_ARG / SSMQ_E_UNSUPPORTED for the arguments as ssmq_pcrlb_sums_dev. */
int ssmq_pcrlb_finalize(int D, int T, int64_t B_total, const double *sums, const double *P0, const ssmq_rv *q, const double *G,
                        double *info, double *bound, double *rmse_bound, int32_t *status);

/*
 * The path's only collective: independent Monte-Carlo trajectories shard across ranks, one process per
 * GPU, and only the per-time-step error sums are added at the end (the reference loops `for imc in range(mc)` in one
 * process and averages with numpy: research/tpq/tpq_base.py:154-172, utils.py:113-120).  RCCL over xGMI, opened at run
 * time; nothing else in this library depends on it.
 *   ssmq_comm_unique_id  rank 0: 128-byte id (ncclGetUniqueId) to be handed to every rank out of band
 *   ssmq_comm_init       every rank, after ssmq_set_device: joins the communicator (world = 1 with id = NULL: no RCCL)
 *   ssmq_comm_abandon_init   for a caller that ran ssmq_comm_init on a helper thread and stopped waiting for it (a peer
 *                        never arrived): puts the process's stdout back (ssmq_comm_init parks it on stderr while RCCL
 *                        prints its banner); harmless at any other time
 *   ssmq_allreduce_sum / _max   host buffer of n doubles, reduced in place over all ranks (synchronous)
 *   ssmq_comm_barrier    drains this rank's stream, then a one-element all-reduce
 * One communicator per process; calls are collective and must be issued in the same order on every rank.
 */
int ssmq_comm_unique_id(char *id, int len);
int ssmq_comm_init(int rank, int world, const char *id, int len);
int ssmq_comm_abandon_init(void);
int ssmq_comm_rank(void);
int ssmq_comm_world(void);
int ssmq_allreduce_sum(double *buf, int64_t n);
int ssmq_allreduce_max(double *buf, int64_t n);
int ssmq_comm_barrier(void);
int ssmq_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* SSMQ_H */
