// Particle smoothers over the cloud of k_particle_filter<D> (include/ssmq.h ssmq_particle_smoother_dev states both recursions).
//
// Mapping, both kernels: the filter's - one trajectory per workgroup of 256 threads (4 waves), particle i on thread i mod 256, the loop
// over k = T-2 .. 0 inside the kernel.
//
// k_particle_smooth<D> (marginal forward-filter backward-smoother).  LDS per step:
//     al [D][N] | be [D][N] | lw [N] | rr [N] | red [96]                          ((2 D + 2) N + 96 doubles, at most 128 KB + 768 B)
// al holds alpha_k = Ls^-1 (f(x_k, k + 1) + G q_mean), be holds beta_{k+1} = Ls^-1 x_{k+1}, lw the filter's log-weights of step k and rr
// ls_{k+1}, which the first sweep turns into ls_{k+1} - lv.  Both sweeps are "a thread owns a row and walks the other index in
// ascending order": in the first a thread owns particle j of step k + 1 (be[:, j] in registers) and walks i, reading al[:, i] and lw[i]
// at addresses that are the same in every lane (LDS broadcasts, no bank conflicts); in the second it owns particle i of step k and
// walks j over be[:, j] and rr[j].  A log-sum-exp is one walk for the maximum and one for the sum of exp(. - max): one fp64 exp per
// pair and sweep, which is the cost of the kernel; the second evaluation of d2 is D subtractions and D fused multiply-adds.  The second
// sweep leaves the unnormalised ls_k^i in lw[i] (only its owner reads lw then); the normalisation and the moments are the filter's:
// maximum, sum of exp(ls - max), mean and sum of squared weights, covariance around the mean - through pf_block_max / pf_block_sum, in
// the order stated at the top of ssmq_particle.hip.  No other sum crosses threads, so a trajectory's bits depend on its cloud and N.
//
// Noise kind QK of k_particle_smooth (compile time): 0 - Gaussian process noise, log p(x' | x) = const - d2 / 2, the kernel as it always
// was; 1 - Student-t process noise of full rank: x' | x is Student-t with location f(x) + G q_mean, scale G Q G' and the noise's nu, so
// log p = const - (nu + D) / 2 log1p(d2 / nu) with the same whitened d2 (Ls the factor of the scale matrix); the constant cancels in the
// normalisation.  One more fp64 log1p and division per pair and sweep.
//
// k_particle_lineage<D> (ancestor tracing): LDS w [N] doubles (the final weights) | idx [N] | mark [N] int32 | red [96].  idx_k(j) =
// a_k(idx_{k+1}(j)) is a gather by the owner of j; the moments are sums over j of w[j] x_k[:, idx_k(j)] in the filter's order; the
// number of distinct idx_k(j) is counted through marks (every writer of a mark writes 1).
#include <cmath>
#include "ssmq_particle.h"

namespace ssmq {
namespace {

struct PsArgs {
    int32_t N, T, fid_dyn, pad;
    int64_t B, ld;
    double Li[kPfMaxD * kPfMaxD], gq[kPfMaxD];
    const double *part, *logw, *fm, *fP, *ess;
    const int32_t *anc, *status;
    double *sm, *sP, *ess_s, *logw_s;
    int32_t *lineage, *unique;
    FPar fd;
    double nuq, hk;                        // QK = 1: the process noise's degrees of freedom nu and (nu + D) / 2
};

// a failed trajectory: NaN (-1) at every step; uniform over the workgroup, before its first barrier
template <int D>
__device__ __forceinline__ void ps_fail(const PsArgs &a, int64_t b) {
    const int N = a.N, T = a.T, tid = threadIdx.x;
    const double qnan = __builtin_nan("");
    for (int k = tid; k < T * D; k += kPfBlock) a.sm[(int64_t)k * a.ld + b] = qnan;
    for (int k = tid; k < T * D * D; k += kPfBlock) a.sP[(int64_t)k * a.ld + b] = qnan;
    for (int k = tid; k < T; k += kPfBlock) {
        a.ess_s[(int64_t)k * a.ld + b] = qnan;
        if (a.unique) a.unique[(int64_t)k * a.ld + b] = -1;
    }
    for (int k = 0; k < T; ++k)
        for (int i = tid; i < N; i += kPfBlock) {
            if (a.logw_s) a.logw_s[((int64_t)k * a.B + b) * N + i] = qnan;
            if (a.lineage) a.lineage[((int64_t)k * a.B + b) * N + i] = -1;
        }
}

// step T-1 is the filter's: its moments and its effective sample size, bit for bit
template <int D>
__device__ __forceinline__ void ps_copy_last(const PsArgs &a, int64_t b) {
    const int T = a.T, tid = threadIdx.x;
    for (int k = (T - 1) * D + tid; k < T * D; k += kPfBlock) a.sm[(int64_t)k * a.ld + b] = a.fm[(int64_t)k * a.ld + b];
    for (int k = (T - 1) * D * D + tid; k < T * D * D; k += kPfBlock) a.sP[(int64_t)k * a.ld + b] = a.fP[(int64_t)k * a.ld + b];
    if (tid == 0) a.ess_s[(int64_t)(T - 1) * a.ld + b] = a.ess[(int64_t)(T - 1) * a.ld + b];
}

// mean, covariance (lower triangle, row-major packed, second pass around the mean) of one step to global memory, by thread 0
template <int D>
__device__ __forceinline__ void ps_store_moments(const PsArgs &a, int64_t b, int k, const double *mean, const double *cv) {
#pragma unroll
    for (int d = 0; d < D; ++d) a.sm[((int64_t)k * D + d) * a.ld + b] = mean[d];
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            const double val = cv[r * (r + 1) / 2 + c];
            a.sP[((int64_t)k * D * D + r * D + c) * a.ld + b] = val;
            a.sP[((int64_t)k * D * D + c * D + r) * a.ld + b] = val;
        }
}

// v <- Li v (the lower-triangular inverse factor, stride kPfMaxD)
template <int D>
__device__ __forceinline__ void ps_whiten(const PsArgs &a, const double *v, double *out) {
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c <= r; ++c) s += a.Li[r * kPfMaxD + c] * v[c];
        out[r] = s;
    }
}

template <int D, int QK>
__global__ __launch_bounds__(kPfBlock) void k_particle_smooth(const PsArgs a) {
    extern __shared__ __align__(16) double lds[];
    const int N = a.N, T = a.T, tid = threadIdx.x;
    const int64_t b = blockIdx.x, B = a.B;
    double *al = lds, *be = lds + (size_t)D * N, *lw = lds + (size_t)2 * D * N, *rr = lw + N, *red = rr + N;
    constexpr int NC = D * (D + 1) / 2;
    if (a.status[b] != 0) {
        ps_fail<D>(a, b);
        return;
    }
    ps_copy_last<D>(a, b);
    for (int i = tid; i < N; i += kPfBlock) {
        const double v = a.logw[((int64_t)(T - 1) * B + b) * N + i];
        rr[i] = v;
        if (a.logw_s) __builtin_nontemporal_store(v, &a.logw_s[((int64_t)(T - 1) * B + b) * N + i]);
    }

    for (int k = T - 2; k >= 0; --k) {
        const double t = (double)(k + 1);
        // ---- alpha_k, beta_{k+1} and the filter's log-weights of step k (own particles) ----
        for (int i = tid; i < N; i += kPfBlock) {
            double xs[kMaxIntegrandIn], o[SSMQ_MAX_DIM], v[D], wv[D];
#pragma unroll
            for (int d = 0; d < kMaxIntegrandIn; ++d) xs[d] = a.part[(((int64_t)k * D + (d < D ? d : 0)) * B + b) * N + i];
#pragma unroll
            for (int e = 0; e < SSMQ_MAX_DIM; ++e) o[e] = 0.0;
            eval_integrand(a.fid_dyn, xs, t, a.fd, o);
#pragma unroll
            for (int d = 0; d < D; ++d) v[d] = o[d] + a.gq[d];
            ps_whiten<D>(a, v, wv);
#pragma unroll
            for (int d = 0; d < D; ++d) al[d * N + i] = wv[d];
#pragma unroll
            for (int d = 0; d < D; ++d) v[d] = a.part[(((int64_t)(k + 1) * D + d) * B + b) * N + i];
            ps_whiten<D>(a, v, wv);
#pragma unroll
            for (int d = 0; d < D; ++d) be[d * N + i] = wv[d];
            lw[i] = a.logw[((int64_t)k * B + b) * N + i];
        }
        __syncthreads();
        // ---- first sweep: lv_j = logsumexp_i (lw_i - d2_ij / 2), rr[j] <- ls_{k+1}^j - lv_j ----
        for (int j = tid; j < N; j += kPfBlock) {
            double bj[D];
#pragma unroll
            for (int d = 0; d < D; ++d) bj[d] = be[d * N + j];
            double m = -INFINITY;
            for (int i = 0; i < N; ++i) {
                double d2 = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double df = bj[d] - al[d * N + i];
                    d2 += df * df;
                }
                const double v = QK == 1 ? lw[i] - a.hk * log1p(d2 / a.nuq) : lw[i] - 0.5 * d2;
                m = v > m ? v : m;
            }
            double lv = -INFINITY;
            if (m > -INFINITY) {
                double s = 0.0;
                for (int i = 0; i < N; ++i) {
                    double d2 = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const double df = bj[d] - al[d * N + i];
                        d2 += df * df;
                    }
                    s += QK == 1 ? exp((lw[i] - a.hk * log1p(d2 / a.nuq)) - m) : exp((lw[i] - 0.5 * d2) - m);
                }
                lv = m + log(s);
            }
            const double ls = rr[j];
            rr[j] = (lv > -INFINITY && ls > -INFINITY) ? ls - lv : -INFINITY;
        }
        __syncthreads();
        // ---- second sweep: ls_k^i = lw_i + logsumexp_j (rr_j - d2_ij / 2), left in lw[i] ----
        for (int i = tid; i < N; i += kPfBlock) {
            double ai[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ai[d] = al[d * N + i];
            double m = -INFINITY;
            for (int j = 0; j < N; ++j) {
                double d2 = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double df = be[d * N + j] - ai[d];
                    d2 += df * df;
                }
                const double v = QK == 1 ? rr[j] - a.hk * log1p(d2 / a.nuq) : rr[j] - 0.5 * d2;
                m = v > m ? v : m;
            }
            double lt = -INFINITY;
            if (m > -INFINITY) {
                double s = 0.0;
                for (int j = 0; j < N; ++j) {
                    double d2 = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const double df = be[d * N + j] - ai[d];
                        d2 += df * df;
                    }
                    s += QK == 1 ? exp((rr[j] - a.hk * log1p(d2 / a.nuq)) - m) : exp((rr[j] - 0.5 * d2) - m);
                }
                lt = m + log(s);
            }
            lw[i] = lw[i] + lt;
        }
        // ---- normalisation and moments, as the filter's (the reductions' barriers end the second sweep's reads of rr) ----
        double vmax = -INFINITY;
        for (int i = tid; i < N; i += kPfBlock) vmax = pf_max(vmax, lw[i]);
        const double m = pf_block_max(vmax, red);
        double s1[1] = {0.0};
        for (int i = tid; i < N; i += kPfBlock) {
            const double e = exp(lw[i] - m);
            rr[i] = e;
            s1[0] += e;
        }
        pf_block_sum<1>(s1, red);
        const double S = s1[0], lse = m + log(S);
        double acc[D + 1];
#pragma unroll
        for (int d = 0; d <= D; ++d) acc[d] = 0.0;
        for (int i = tid; i < N; i += kPfBlock) {
            const double wt = rr[i] / S, lsn = lw[i] - lse;
            lw[i] = wt;
            rr[i] = lsn;
            if (a.logw_s) __builtin_nontemporal_store(lsn, &a.logw_s[((int64_t)k * B + b) * N + i]);
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += wt * a.part[(((int64_t)k * D + d) * B + b) * N + i];
            acc[D] += wt * wt;
        }
        pf_block_sum<D + 1>(acc, red);
        double cv[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) cv[q] = 0.0;
        for (int i = tid; i < N; i += kPfBlock) {
            const double wt = lw[i];
            double dx[D];
#pragma unroll
            for (int d = 0; d < D; ++d) dx[d] = a.part[(((int64_t)k * D + d) * B + b) * N + i] - acc[d];
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) cv[r * (r + 1) / 2 + c] += wt * (dx[r] * dx[c]);
        }
        pf_block_sum<NC>(cv, red);
        if (tid == 0) {
            ps_store_moments<D>(a, b, k, acc, cv);
            a.ess_s[(int64_t)k * a.ld + b] = 1.0 / acc[D];
        }
        __syncthreads();                   // the next step overwrites al and be
    }
}

template <int D>
__global__ __launch_bounds__(kPfBlock) void k_particle_lineage(const PsArgs a) {
    extern __shared__ __align__(16) double lds[];
    const int N = a.N, T = a.T, tid = threadIdx.x;
    const int64_t b = blockIdx.x, B = a.B;
    double *w = lds, *red = lds + (size_t)2 * N;
    int32_t *idx = (int32_t *)(lds + N), *mark = idx + N;
    constexpr int NC = D * (D + 1) / 2;
    if (a.status[b] != 0) {
        ps_fail<D>(a, b);
        return;
    }
    ps_copy_last<D>(a, b);
    double s2[1] = {0.0};
    for (int j = tid; j < N; j += kPfBlock) {
        const double lwj = a.logw[((int64_t)(T - 1) * B + b) * N + j], wt = exp(lwj);
        w[j] = wt;
        idx[j] = j;
        s2[0] += wt * wt;
        if (a.logw_s) __builtin_nontemporal_store(lwj, &a.logw_s[((int64_t)(T - 1) * B + b) * N + j]);
        if (a.lineage) a.lineage[((int64_t)(T - 1) * B + b) * N + j] = j;
    }
    pf_block_sum<1>(s2, red);
    const double ess = 1.0 / s2[0];
    if (tid == 0 && a.unique) a.unique[(int64_t)(T - 1) * a.ld + b] = N;

    for (int k = T - 2; k >= 0; --k) {
        for (int j = tid; j < N; j += kPfBlock) mark[j] = 0;
        __syncthreads();
        double acc[D + 1];
#pragma unroll
        for (int d = 0; d <= D; ++d) acc[d] = 0.0;
        for (int j = tid; j < N; j += kPfBlock) {
            int id = a.anc[((int64_t)k * B + b) * N + idx[j]];
            id = id < 0 ? 0 : (id >= N ? N - 1 : id);          // (a cloud of status 0 holds ancestors in range)
            idx[j] = id;
            mark[id] = 1;
            if (a.lineage) a.lineage[((int64_t)k * B + b) * N + j] = id;
            if (a.logw_s) __builtin_nontemporal_store(a.logw[((int64_t)(T - 1) * B + b) * N + j], &a.logw_s[((int64_t)k * B + b) * N + j]);
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += w[j] * a.part[(((int64_t)k * D + d) * B + b) * N + id];
        }
        __syncthreads();
        for (int j = tid; j < N; j += kPfBlock) acc[D] += (double)mark[j];       // whole numbers: exact in any order
        pf_block_sum<D + 1>(acc, red);
        double cv[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) cv[q] = 0.0;
        for (int j = tid; j < N; j += kPfBlock) {
            const int id = idx[j];
            double dx[D];
#pragma unroll
            for (int d = 0; d < D; ++d) dx[d] = a.part[(((int64_t)k * D + d) * B + b) * N + id] - acc[d];
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) cv[r * (r + 1) / 2 + c] += w[j] * (dx[r] * dx[c]);
        }
        pf_block_sum<NC>(cv, red);
        if (tid == 0) {
            ps_store_moments<D>(a, b, k, acc, cv);
            a.ess_s[(int64_t)k * a.ld + b] = ess;
            if (a.unique) a.unique[(int64_t)k * a.ld + b] = (int32_t)acc[D];
        }
    }
}

typedef void (*ps_kernel)(const PsArgs);
template <int D, int QK> constexpr ps_kernel ps_smooth_of() { return k_particle_smooth<D, QK>; }
template <int D> constexpr ps_kernel ps_lineage_of() { return k_particle_lineage<D>; }

}  // namespace

int launch_particle_smoother(const PsLaunch &h, hipStream_t s) {
    PsArgs a;
    memset(&a, 0, sizeof(a));
    a.N = h.N; a.T = h.T; a.fid_dyn = h.f_dyn->id; a.B = h.B; a.ld = h.ld;
    memcpy(a.Li, h.Li, sizeof(a.Li)); memcpy(a.gq, h.gq, sizeof(a.gq));
    a.nuq = h.nuq; a.hk = 0.5 * (h.nuq + (double)h.D);
    a.part = h.part; a.logw = h.logw; a.fm = h.fm; a.fP = h.fP; a.ess = h.ess; a.anc = h.anc; a.status = h.status;
    a.sm = h.sm; a.sP = h.sP; a.ess_s = h.ess_s; a.logw_s = h.logw_s; a.lineage = h.lineage; a.unique = h.unique;
    fill_fpar(h.f_dyn, &a.fd);
    static const ps_kernel table[3][kPfMaxD] = {
        {ps_smooth_of<1, 0>(), ps_smooth_of<2, 0>(), ps_smooth_of<3, 0>(), ps_smooth_of<4, 0>(), ps_smooth_of<5, 0>(), ps_smooth_of<6, 0>()},
        {ps_lineage_of<1>(), ps_lineage_of<2>(), ps_lineage_of<3>(), ps_lineage_of<4>(), ps_lineage_of<5>(), ps_lineage_of<6>()},
        {ps_smooth_of<1, 1>(), ps_smooth_of<2, 1>(), ps_smooth_of<3, 1>(), ps_smooth_of<4, 1>(), ps_smooth_of<5, 1>(), ps_smooth_of<6, 1>()}};
    if (!pf_shape_ok(h.D, 1, 1, h.N) || h.N < kPfMinN || h.N % 64 != 0 || h.B < 1 || h.B > 0x7fffffff ||
        (h.method != SSMQ_PS_MARGINAL && h.method != SSMQ_PS_GENEALOGY) || (h.method == SSMQ_PS_GENEALOGY && !h.anc) || !pf_dof_ok(h.nuq)) {
        set_error("particle smoother: shape or method outside the kernels' range");
        return SSMQ_E_UNSUPPORTED;
    }
    const size_t lds = ps_lds_bytes(h.method, h.D, h.N);
    static thread_local unsigned attr_epoch = 0;
    int rc = set_max_dynamic_lds(attr_epoch, {(const void *)table[0][0], (const void *)table[0][1], (const void *)table[0][2],
                                              (const void *)table[0][3], (const void *)table[0][4], (const void *)table[0][5],
                                              (const void *)table[1][0], (const void *)table[1][1], (const void *)table[1][2],
                                              (const void *)table[1][3], (const void *)table[1][4], (const void *)table[1][5],
                                              (const void *)table[2][0], (const void *)table[2][1], (const void *)table[2][2],
                                              (const void *)table[2][3], (const void *)table[2][4], (const void *)table[2][5]},
                                 sizeof(double) * (kPsCloudDoubles + kPfRedDoubles));
    if (rc) return rc;
    const int m = h.method == SSMQ_PS_MARGINAL ? (h.nuq > 0.0 ? 2 : 0) : 1;      // the lineage reads no density
    hipLaunchKernelGGL(table[m][h.D - 1], dim3((unsigned)h.B), dim3(kPfBlock), lds, s, a);
    return hip_fail(hipGetLastError(), m == 1 ? "k_particle_lineage" : "k_particle_smooth");
}

}  // namespace ssmq
