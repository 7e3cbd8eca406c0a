// The multi-output BQ moment transform (SSMQ_FORM_BQ_MO; bq/bqmtran.py:425-602 with the model variance on the diagonal):
//   mean_i = fx_i wm_i;  cov_ij = fx_i Wc_ij fx_j' - mean_i mean_j + delta_ij emv_i;  ccov_i = fx_i Wcc_i' L'
// with a weight set of its own per output and per output pair, E (E + 1) / 2 quadratic forms in N points where the
// single-output transform has one matrix product.  One kernel, k_apply_mo, correct for D <= 16, E <= 8, N <= 64 (of the point
// sets with fewer than 2 D points, those whose work space fits the LDS: mo_range_ok):
//
//   a wave takes G = 64 / GL trajectories at a time, GL = N rounded up to a power of two; lane (g, n) owns sigma point n of
//   trajectory g.  Per trajectory: the lower triangle of cov -> LDS, Cholesky column by column (left-looking, the order of
//   LAPACK dpotf2 'L'), x_n = m + L xi_n and f(x_n) in registers, the values into the trajectory's [E][N] tile in LDS.
//   Quadratic form (i, j): lane n forms t_n = sum_m Wc_ij[n][m] fx_j[m] - fx_j[m] is an LDS broadcast, the weight words of
//   the lanes of a group are consecutive (the blocks are stored transposed), lanes of different groups read the same word -
//   then fx_i[n] t_n is summed over the group by xor shuffles.  The same for the mean (wm), the t-process scale (iK_i) and
//   P_i = fx_i Wcc_i'; ccov_i = P_i L' by the lanes over its entries.  Every sum runs in an order that depends on (D, E, N)
//   alone: a trajectory's results are the same bits whatever the batch around it.
//   Outputs are collected in the wave's LDS slice and written plane by plane, G neighbouring trajectories by neighbouring lanes.
//
// The constant block (mo_layout) - E (E + 1) / 2 N^2 doubles of pair weights, 28 KB at D = E = 6, N = 13 - is staged in LDS once
// per workgroup when it fits next to the waves' slices (template argument WLDS), otherwise read through L2.
// Modes: the whole transform; the sigma points and factors alone (ssmq_sigma_points_batch); the reductions alone on integrand
// values the caller supplies (ssmq_apply_fx_batch).
#include <algorithm>
#include <cstring>
#include <vector>
#include "ssmq_host.h"

namespace ssmq {
namespace {

constexpr int kMoWaves = 4;

// Offsets (in doubles) into the constant block: xi [D][N] | wm [E][N] | Wcc [E][D][N] | emv [E] | pair blocks [E (E + 1) / 2][N][N],
// block (i, j), i >= j, at i (i + 1) / 2 + j and TRANSPOSED (entry [m][n] = Wc_ij[n][m]) | iK [E][N][N], transposed likewise
struct MoLayout {
    int xi, wm, Wcc, emv, Wp, iK, total;
};
__host__ __device__ constexpr inline MoLayout mo_layout(int D, int E, int N) {
    MoLayout l{};
    l.xi = 0;
    l.wm = l.xi + D * N;
    l.Wcc = l.wm + E * N;
    l.emv = l.Wcc + E * D * N;
    l.Wp = (l.emv + E + 1) & ~1;
    l.iK = l.Wp + E * (E + 1) / 2 * N * N;
    l.total = l.iK + E * N * N;
    return l;
}
// the wave's LDS slice: per trajectory  L [D][D] | mean [D] | fx [E][N] | P [E][D] | t-process scale [E] | outputs [E + E E + E D]
struct MoGeom {
    int GL, G, o_m, o_fx, o_p, o_s, o_out, n_out, per_traj, wave_doubles;
};
__host__ __device__ constexpr inline MoGeom mo_geom(int D, int E, int N) {
    MoGeom g{};
    g.GL = 1;
    while (g.GL < N) g.GL *= 2;
    g.G = 64 / g.GL;
    g.o_m = D * D;
    g.o_fx = g.o_m + D;
    g.o_p = g.o_fx + E * N;
    g.o_s = g.o_p + E * D;
    g.o_out = g.o_s + E;
    g.n_out = E + E * E + E * D;
    g.per_traj = g.o_out + g.n_out;
    g.wave_doubles = (g.G * g.per_traj + 1) & ~1;
    return g;
}

#define SSMQ_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// sum over the GL lanes of a group (GL a power of two, groups aligned): every lane gets the total
__device__ __forceinline__ double group_sum(double v, int GL) {
    for (int s = GL >> 1; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// DM: compile-time bound on D; WLDS: the constant block is staged in LDS
template <int DM, bool WLDS>
__global__ __launch_bounds__(64 * kMoWaves) void k_apply_mo(const MoArgs a, int64_t B) {
    extern __shared__ __align__(16) double lds[];
    const int D = a.D, E = a.E, N = a.N;
    const bool tp = a.tp_nu > 0.0;
    const MoLayout ml = mo_layout(D, E, N);
    const MoGeom mg = mo_geom(D, E, N);
    const int GL = mg.GL, G = mg.G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_const = tp ? ml.total : ml.iK;
    if (WLDS) {
        for (int i = threadIdx.x; i < n_const; i += 64 * kMoWaves) lds[i] = a.consts[i];
        __syncthreads();
    }
    const double *C = WLDS ? (const double *)lds : a.consts;
    double *wbase = lds + (WLDS ? ((n_const + 1) & ~1) : 0) + (size_t)wave * mg.wave_doubles;
    const int gi = lane / GL, gl = lane - gi * GL;
    const bool valid = gl < N;
    const int nn = valid ? gl : N - 1;                 // every lane reads a valid column; what is not its own counts as zero
    const double nan = __builtin_nan("");
    const double tp_den = tp ? 1.0 / (a.tp_nu - 2.0 + (double)N) : 0.0;
    const int64_t n_groups = (B + G - 1) / G;
    double *sL = wbase + gi * mg.per_traj, *sm = sL + mg.o_m, *sfx = sL + mg.o_fx, *sP = sL + mg.o_p, *ss = sL + mg.o_s,
           *so = sL + mg.o_out;
    for (int64_t grp = (int64_t)blockIdx.x * kMoWaves + wave; grp < n_groups; grp += (int64_t)gridDim.x * kMoWaves) {
        const int64_t b0 = grp * G;
        const bool active = b0 + gi < B;
        const int64_t b = active ? b0 + gi : B - 1;     // a group beyond the batch repeats the last trajectory and stores nothing
        bool ok = true;
        if (a.mode != SSMQ_MO_FX) {
            // ---- 1. inputs and Cholesky: lane i of the group owns rows i, i + GL, ... --------------------------------------------
            for (int idx = gl; idx < D * D; idx += GL) {
                const int i = idx / D, j = idx - i * D;
                sL[idx] = j <= i ? a.cov[(int64_t)idx * a.es_in + b * a.bs_cov] : 0.0;
            }
            for (int d = gl; d < D; d += GL) sm[d] = a.mean[(int64_t)d * a.es_in + b * a.bs_mean];
            SSMQ_WAVE_SYNC();
            for (int j = 0; j < D; ++j) {
                for (int i = j + gl; i < D; i += GL) {
                    double s = sL[i * D + j];
                    for (int k = 0; k < j; ++k) s -= sL[i * D + k] * sL[j * D + k];
                    sL[i * D + j] = s;
                }
                SSMQ_WAVE_SYNC();
                const double ajj = sL[j * D + j];
                ok = ok && (ajj > 0.0);
                double ljj, rinv;
                sqrt_rsqrt(ajj, ljj, rinv);
                SSMQ_WAVE_SYNC();                       // every lane has read the pivot before it is replaced
                for (int i = j + gl; i < D; i += GL) sL[i * D + j] = i == j ? ljj : sL[i * D + j] * rinv;
                SSMQ_WAVE_SYNC();
            }
            if (active && gl == 0 && a.status) a.status[b] = ok ? 0 : 1;
            // ---- 2. lane (g, n): sigma point and integrand -------------------------------------------------------------------------
            double x[DM];
#pragma unroll
            for (int d = 0; d < DM; ++d) {
                double acc = 0.0;
                if (d < D) {
                    acc = sm[d];
#pragma unroll
                    for (int k = 0; k < DM; ++k)
                        if (k <= d) acc += sL[d * D + k] * C[ml.xi + k * N + nn];
                }
                x[d] = acc;
            }
            if (a.mode == SSMQ_MO_POINTS) {
                if (active) {
                    if (valid) {
#pragma unroll
                        for (int d = 0; d < DM; ++d)
                            if (d < D) a.x_out[(b * D + d) * N + gl] = x[d];
                    }
                    for (int idx = gl; idx < D * D; idx += GL) a.chol_out[b * D * D + idx] = sL[idx];
                }
                SSMQ_WAVE_SYNC();
                continue;
            }
            double xs[kMaxIntegrandIn], o[SSMQ_MAX_DIM];
#pragma unroll
            for (int k = 0; k < kMaxIntegrandIn; ++k) {
                double v = k < DM ? x[k < DM ? k : 0] : 0.0;
                if (a.fp.n_idx > 0) {                   // state-index selection (MeasurementModel.state_index)
                    const int src = k < a.fp.n_idx ? a.fp.idx[k] : 0;
                    v = x[0];
#pragma unroll
                    for (int q = 1; q < DM; ++q) v = (src == q) ? x[q] : v;
                }
                xs[k] = v;
            }
#pragma unroll
            for (int e = 0; e < SSMQ_MAX_DIM; ++e) o[e] = 0.0;
            const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
            eval_integrand(a.fid, xs, t, a.fp, o);
            if (valid) {
#pragma unroll
                for (int e = 0; e < SSMQ_MO_MAX_OUT; ++e)   // a covariance that is not positive definite poisons every output
                    if (e < E) sfx[e * N + gl] = ok ? o[e] : nan;
            }
        } else {
            for (int idx = gl; idx < D * D; idx += GL) sL[idx] = a.chol_in[b * D * D + idx];
            for (int idx = gl; idx < E * N; idx += GL) sfx[idx] = a.fx_in[b * E * N + idx];
        }
        SSMQ_WAVE_SYNC();
        // ---- 3. the reductions; lane n contributes point n ----------------------------------------------------------------------------
        for (int i = 0; i < E; ++i) {
            const double fi = valid ? sfx[i * N + nn] : 0.0;
            const double m = group_sum(fi * C[ml.wm + i * N + nn], GL);
            double sc = 1.0;
            if (tp) {
                const double *K = C + ml.iK + i * N * N;
                double tt = 0.0;
                for (int k = 0; k < N; ++k) tt = fma(K[k * N + nn], sfx[i * N + k], tt);
                sc = (a.tp_nu - 2.0 + group_sum(fi * tt, GL)) * tp_den;
            }
            if (gl == 0) {
                so[i] = m;
                ss[i] = sc * C[ml.emv + i];
            }
            for (int d = 0; d < D; ++d) {
                const double p = group_sum(fi * C[ml.Wcc + (i * D + d) * N + nn], GL);
                if (gl == 0) sP[i * D + d] = p;
            }
        }
        SSMQ_WAVE_SYNC();
        for (int i = 0, pr = 0; i < E; ++i) {
            const double fi = valid ? sfx[i * N + nn] : 0.0;
            for (int j = 0; j <= i; ++j, ++pr) {
                const double *W = C + ml.Wp + pr * N * N, *fj = sfx + j * N;
                double tt = 0.0;
                for (int k = 0; k < N; ++k) tt = fma(W[k * N + nn], fj[k], tt);
                const double qf = group_sum(fi * tt, GL);
                if (gl == 0) {
                    double v = qf - so[i] * so[j];
                    if (i == j) v += ss[i];
                    v = v * a.cov_scale + (a.cov_add ? a.cov_add[i * E + j] : 0.0);
                    so[E + i * E + j] = v;              // both triangles from the one value
                    so[E + j * E + i] = v;
                }
            }
        }
        for (int idx = gl; idx < E * D; idx += GL) {    // ccov_i = P_i L'
            const int i = idx / D, c = idx - i * D;
            double v = 0.0;
            for (int d = 0; d <= c; ++d) v += sP[i * D + d] * sL[c * D + d];
            so[E + E * E + idx] = v * a.ccov_scale;
        }
        SSMQ_WAVE_SYNC();
        // ---- 4. stores: plane by plane, the wave's G trajectories by neighbouring lanes ---------------------------------------------
        for (int id = lane; id < mg.n_out * G; id += 64) {
            const int p = id / G, g = id - p * G;
            const int64_t bb = b0 + g;
            if (bb >= B) continue;
            const double v = wbase[g * mg.per_traj + mg.o_out + p];
            if (p < E) a.mean_f[(int64_t)p * a.es_out + bb * a.bs_mf] = v;
            else if (p < E + E * E) a.cov_f[(int64_t)(p - E) * a.es_out + bb * a.bs_cf] = v;
            else a.cov_fx[(int64_t)(p - E - E * E) * a.es_out + bb * a.bs_cfx] = v;
        }
        SSMQ_WAVE_SYNC();                               // the next group overwrites the slice
    }
}

template <int DM>
int launch_mo_dm(const MoArgs &a, int64_t B, hipStream_t s) {
    const MoLayout ml = mo_layout(a.D, a.E, a.N);
    const MoGeom mg = mo_geom(a.D, a.E, a.N);
    const size_t n_const = a.tp_nu > 0.0 ? ml.total : ml.iK;
    const size_t slices = sizeof(double) * (size_t)kMoWaves * mg.wave_doubles;
    const size_t with_consts = slices + sizeof(double) * ((n_const + 1) & ~(size_t)1);
    const bool wlds = with_consts <= 160 * 1024 - 64 && !ssmq::sw("SSMQ_MO_NO_LDS");
    const size_t lds = wlds ? with_consts : slices;
    static thread_local unsigned attr_epoch = ~0u;
    int rc = set_max_dynamic_lds(attr_epoch, {(const void *)k_apply_mo<DM, true>, (const void *)k_apply_mo<DM, false>}, 160 * 1024 - 64);
    if (rc) return rc;
    const int64_t groups = (B + mg.G - 1) / mg.G, blocks = (groups + kMoWaves - 1) / kMoWaves;
    // a few workgroups per CU, each walking its share of the batch: the constants are staged once per workgroup
    const int64_t cap = 256 * 4;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, cap)), block(64 * kMoWaves);
    if (wlds) hipLaunchKernelGGL((k_apply_mo<DM, true>), grid, block, lds, s, a, B);
    else hipLaunchKernelGGL((k_apply_mo<DM, false>), grid, block, lds, s, a, B);
    return hip_fail(hipGetLastError(), "k_apply_mo");
}

// The waves' LDS slices (64 / GL trajectories each) must fit the 160 KiB of a CU by themselves: every point set of the package
// (N >= 2 D) does; a few points in many dimensions - D = 16, E = 8, N = 8 would need 172 KB - do not and are refused at creation.
bool mo_range_ok(int D, int E, int N) {
    if (!(D >= 1 && D <= SSMQ_MAX_DIM && E >= 1 && E <= SSMQ_MO_MAX_OUT && N >= 1 && N <= SSMQ_MO_MAX_PTS)) return false;
    return sizeof(double) * (size_t)kMoWaves * mo_geom(D, E, N).wave_doubles <= 160 * 1024 - 64;
}

// the handle's host copies -> its constant block
int mo_upload(ssmq_transform *h) {
    ++h->generation;
    const int D = h->D, E = h->E, N = h->N;
    const MoLayout ml = mo_layout(D, E, N);
    std::vector<double> c(ml.total, 0.0);
    std::copy(h->xi.begin(), h->xi.end(), c.begin() + ml.xi);
    std::copy(h->wm.begin(), h->wm.end(), c.begin() + ml.wm);
    std::copy(h->Wcc.begin(), h->Wcc.end(), c.begin() + ml.Wcc);
    std::copy(h->emv.begin(), h->emv.end(), c.begin() + ml.emv);
    for (int p = 0; p < E * (E + 1) / 2; ++p)
        for (int n = 0; n < N; ++n)
            for (int m = 0; m < N; ++m) c[ml.Wp + ((size_t)p * N + m) * N + n] = h->Wc[((size_t)p * N + n) * N + m];
    if (h->tp_nu > 0.0)
        for (int e = 0; e < E; ++e)
            for (int n = 0; n < N; ++n)
                for (int m = 0; m < N; ++m) c[ml.iK + ((size_t)e * N + m) * N + n] = h->iK[((size_t)e * N + n) * N + m];
    SSMQ_HIP(hipMemcpyAsync(h->d_mo, c.data(), sizeof(double) * ml.total, hipMemcpyHostToDevice, stream()));
    SSMQ_HIP(hipStreamSynchronize(stream()));
    return SSMQ_OK;
}

// the blocks (i, j), i >= j, of a full [E][E][N][N] array in packed order
void mo_pack_pairs(int E, int N, const double *Wc, std::vector<double> &out) {
    out.resize((size_t)E * (E + 1) / 2 * N * N);
    for (int i = 0, p = 0; i < E; ++i)
        for (int j = 0; j <= i; ++j, ++p)
            std::copy(Wc + ((size_t)i * E + j) * N * N, Wc + ((size_t)i * E + j + 1) * N * N, out.begin() + (size_t)p * N * N);
}

}  // namespace

int refuse_mo(const char *what) {
    set_error(std::string(what) + ": not implemented for the multi-output transform (SSMQ_FORM_BQ_MO runs through ssmq_apply_batch[_dev], "
              "ssmq_sigma_points_batch, ssmq_apply_fx_batch and ssmq_filter_forward_dev)");
    return SSMQ_E_UNSUPPORTED;
}

int launch_apply_mo(const MoArgs &a, int64_t B, hipStream_t s) {
    if (B <= 0) return SSMQ_OK;
    if (a.D <= 4) return launch_mo_dm<4>(a, B, s);
    if (a.D <= 8) return launch_mo_dm<8>(a, B, s);
    return launch_mo_dm<SSMQ_MAX_DIM>(a, B, s);
}

}  // namespace ssmq

using namespace ssmq;

extern "C" {

ssmq_transform *ssmq_transform_create_mo(int D, int E, int N, const double *xi, const double *wm, const double *Wc,
                                         const double *Wcc, const double *emv, double tp_nu, const double *tp_iK) {
    if (D < 1 || E < 1 || N < 1 || !xi || !wm || !Wc || !Wcc || (tp_nu > 0.0 && !tp_iK)) {
        set_error("transform_create_mo: bad argument");
        return nullptr;
    }
    if (!mo_range_ok(D, E, N)) {
        set_error("transform_create_mo: the multi-output transform supports D <= 16, E <= 8, N <= 64, and point sets of fewer than "
                  "2 D points only while (64 / N) trajectories' work space fits the LDS of a CU");
        return nullptr;
    }
    if (ensure_device()) return nullptr;
    ssmq_transform *h = new ssmq_transform();
    h->D = D; h->E = E; h->N = N; h->form = SSMQ_FORM_BQ_MO; h->emv_mode = SSMQ_EMV_DIAG; h->tp_nu = tp_nu > 0.0 ? tp_nu : 0.0;
    h->opt_mask = 0;
    hipGetDevice(&h->device);
    h->xi.assign(xi, xi + D * N);
    h->wm.assign(wm, wm + E * N);
    mo_pack_pairs(E, N, Wc, h->Wc);
    h->Wcc.assign(Wcc, Wcc + E * D * N);
    h->emv.assign(E, 0.0);
    if (emv) h->emv.assign(emv, emv + E);
    if (tp_iK) h->iK.assign(tp_iK, tp_iK + (size_t)E * N * N);
    h->d_small = h->d_wide = nullptr;
    if (hipMalloc((void **)&h->d_mo, sizeof(double) * mo_layout(D, E, N).total) != hipSuccess || mo_upload(h) != SSMQ_OK) {
        if (!*ssmq_last_error()) set_error("transform_create_mo: device allocation failed");
        ssmq_transform_destroy(h);
        return nullptr;
    }
    return h;
}

int ssmq_transform_update_mo(ssmq_transform *h, const double *xi, const double *wm, const double *Wc, const double *Wcc,
                             const double *emv, double tp_nu, const double *tp_iK) {
    SSMQ_HANDLE_LOCK(h);
    if (!h) return SSMQ_E_ARG;
    if (is_taylor_gpqd(h)) return refuse_taylor_gpqd("ssmq_transform_update_mo");
    if (is_trunc(h)) return refuse_trunc("ssmq_transform_update_mo");
    if (is_gpqd(h)) return refuse_gpqd("ssmq_transform_update_mo");
    if (!is_mo(h)) {
        set_error("transform_update_mo: not a multi-output transform");
        return SSMQ_E_ARG;
    }
    const int D = h->D, E = h->E, N = h->N;
    if (tp_nu > 0.0 && !tp_iK && h->iK.empty()) {
        set_error("transform_update_mo: tp_nu > 0 needs tp_iK");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (xi) h->xi.assign(xi, xi + D * N);
    if (wm) h->wm.assign(wm, wm + E * N);
    if (Wc) mo_pack_pairs(E, N, Wc, h->Wc);
    if (Wcc) h->Wcc.assign(Wcc, Wcc + E * D * N);
    if (emv) h->emv.assign(emv, emv + E);
    if (tp_iK) h->iK.assign(tp_iK, tp_iK + (size_t)E * N * N);
    if (tp_nu > 0.0) h->tp_nu = tp_nu;
    return mo_upload(h);
}

}  // extern "C"
