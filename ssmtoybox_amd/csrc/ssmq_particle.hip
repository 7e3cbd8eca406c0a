// Bootstrap particle filter, the whole time loop in one launch (include/ssmq.h ssmq_particle_filter_dev states the recursion).
//
// Mapping: one trajectory per workgroup of 256 threads (4 waves), particle i on thread i mod 256 (a thread walks i = tid, tid + 256,
// ...).  The cloud lives in LDS for the whole pass:
//     xa [D][N] | xb [D][N] | w [N] | red [96]                                 ((2 D + 1) N + 96 doubles, at most 104 KB + 768 B)
// xa holds the particles.  xb is free between two resamplings and carries, per step, row 0 = the unnormalised exp(log w - max) and then
// the normalised weights w~; resampling gathers xa[:, a(i)] into xb and the two swap.  w holds the normalised log-weights and, while a
// step resamples, the CDF (the log-weights are reset to -log N afterwards, so nothing is lost).  Nothing per particle goes to global
// memory unless the caller asks for the cloud.
//
// Order of the sums (all of them, the maximum included): a thread adds its own particles in ascending i; the 64 partials of a wave are
// combined by a butterfly (lane l adds the value of lane l ^ 32, then ^ 16, 8, 4, 2, 1 - both partners form the same sum, so every
// lane ends with the same bits); the four wave results r0 .. r3 are combined as (r0 + r1) + (r2 + r3).  The prefix sum of the CDF runs
// over chunks of 256 consecutive particles in ascending order: inside a wave an inclusive Hillis-Steele scan (distances 1, 2, 4, .. 32),
// then cdf[i] = ((carry + t0) + .. + t_{v-1}) + scan, t_v the total of wave v of the chunk, and carry <- (((carry + t0) + t1) + t2) + t3.
// Every one of these orders depends on N alone, so a trajectory's bits do not depend on B, the launch or the device.
//
// Random numbers (ssmq_rng.h): Philox4x32-10 keyed by the seed, counter = (global trajectory lo, hi, step, tag),
//     tag = purpose << 28 | particle << 4 | pair;   pair p gives z[2 p], z[2 p + 1] by Box-Muller
// purpose 8: initial particles (step 0), 9: process noise of step j, 10: the resampling uniform of step j (particle 0, pair 0).  The
// simulator's tags are purpose << 16 | .. with purpose <= 2, all below 1 << 28.
//
// Noise kind QK (compile time): 0 - Gaussian initial state and process noise, the kernel as it always was; 1 - either of the two may be
// a multivariate Student-t, v = mean + L z / sqrt(u), u ~ Gamma(nu / 2, scale 2 / nu) (sample_rv of ssmq_simulate.hip), z from the
// counters above and u by gamma_mt_tags (ssmq_rng.h), one u per particle and draw, its attempt t = 0 .. 15 in the low four bits (the
// pair field) of
//     purpose 11: the normal, 12: the uniform of attempt t for the initial particle (step 0)
//     purpose 13: the normal, 14: the uniform of attempt t for the process noise of step j
// so no counter is used twice: (step, purpose, particle, low four bits) names one draw, the purposes 8 .. 14 are disjoint, and 0 .. 7 and
// 15 stay free.  A side that is Gaussian (nu = 0 in the launch) draws no u and takes the factor 1 - decided per launch, the same in every
// thread.  A rejected attempt diverges inside a wave and nowhere else: the result is a function of the counters alone.
//
// Model dispatch is the run-time eval_integrand of ssmq_device.h, as in k_simulate; the kernel is instantiated over D and QK.
#include <cmath>
#include "ssmq_particle.h"
#include "ssmq_rng.h"

namespace ssmq {
namespace {

struct PfArgs {
    int32_t Y, dq, N, T, fid_dyn, fid_obs, student, pad;
    int64_t B, ld;
    uint64_t seed, traj_offset;
    double ess_threshold, lognorm, dof;
    double qm[kPfMaxQ], Lq[kPfMaxQ * kPfMaxQ], G[kPfMaxD * kPfMaxQ], rm[kPfMaxY], Lr[kPfMaxY * kPfMaxY];
    const double *y, *m0, *P0;
    double *fm, *fP, *ll, *ess;
    int32_t *status;
    double *part, *logw;
    int32_t *anc;
    FPar fd, fo;
    double nu0, nuq;                       // QK = 1: degrees of freedom of the initial state / the process noise, 0 = Gaussian
};

constexpr uint32_t kPfInit = 8u << 28, kPfNoise = 9u << 28, kPfResample = 10u << 28;
constexpr uint32_t kPfInitGammaN = 11u << 28, kPfInitGammaU = 12u << 28, kPfNoiseGammaN = 13u << 28, kPfNoiseGammaU = 14u << 28;

// the n <= M leading standard normals of (trajectory, step, purpose, particle); the rest zero
template <int M>
__device__ __forceinline__ void pf_normals(const PfArgs &a, uint64_t traj, uint32_t step, uint32_t purpose, uint32_t particle, int n,
                                           double (&z)[M]) {
#pragma unroll
    for (int p = 0; p < (M + 1) / 2; ++p) {
        double z0 = 0.0, z1 = 0.0;
#ifndef SSMQ_PF_NO_RNG
        if (2 * p < n) normal_pair(a.seed, traj, step, purpose | (particle << 4) | (uint32_t)p, &z0, &z1);
#else
        if (2 * p < n) { z0 = 0.25; z1 = -0.5; }     // timing variant: no Philox, no Box-Muller
#endif
        z[2 * p] = z0;
        if (2 * p + 1 < M) z[2 * p + 1] = (2 * p + 1 < n) ? z1 : 0.0;
    }
}

// 1 / sqrt(u), u ~ Gamma(nu / 2, scale 2 / nu), of (trajectory, step, particle): the factor on L z of a Student-t draw
__device__ __forceinline__ double pf_t_factor(const PfArgs &a, uint64_t traj, uint32_t step, uint32_t tag_normal, uint32_t tag_uniform,
                                              uint32_t particle, double nu) {
#ifndef SSMQ_PF_NO_RNG
    const double g = gamma_mt_tags(a.seed, traj, step, tag_normal | (particle << 4), tag_uniform | (particle << 4), 0.5 * nu) * (2.0 / nu);
    return 1.0 / sqrt(g);
#else
    return 1.0;
#endif
}

// pf_block_sum / pf_block_max (ssmq_particle.h): the sums and the maximum over the workgroup in the order stated at the top

template <int D, int QK>
__global__ __launch_bounds__(kPfBlock) void k_particle_filter(const PfArgs a) {
    extern __shared__ __align__(16) double lds[];
    const int N = a.N, Y = a.Y, T = a.T, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x, ld = a.ld;
    const uint64_t traj = a.traj_offset + (uint64_t)b;
    double *xa = lds, *xb = lds + (size_t)D * N, *w = lds + (size_t)2 * D * N, *red = w + N;
    const double qnan = __builtin_nan(""), dN = (double)N, log_unif = -log(dN);

    // initial particles x = m0 + chol(P0) z (every thread factors the D x D matrix itself: wave-uniform loads, D <= 6)
    {
        double L[D * D], m0[D];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            m0[c] = a.m0[c * ld + b];
#pragma unroll
            for (int r = c; r < D; ++r) {
                double s = a.P0[(int64_t)(r * D + c) * ld + b];
#pragma unroll
                for (int k = 0; k < c; ++k) s -= L[r * D + k] * L[c * D + k];
                L[r * D + c] = (r == c) ? sqrt(s) : s / L[c * D + c];
            }
        }
        for (int i = tid; i < N; i += kPfBlock) {
            double z[D];
            pf_normals<D>(a, traj, 0u, kPfInit, (uint32_t)i, D, z);
            double sc = 1.0;
            if constexpr (QK == 1) {
                if (a.nu0 > 0.0) sc = pf_t_factor(a, traj, 0u, kPfInitGammaN, kPfInitGammaU, (uint32_t)i, a.nu0);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k <= d; ++k) s += L[d * D + k] * z[k];
                if constexpr (QK == 1) s *= sc;
                xa[d * N + i] = m0[d] + s;
            }
            w[i] = log_unif;
        }
    }

    double total = 0.0;
    for (int j = 0; j < T; ++j) {
        const double t = (double)j;
        double yj[kPfMaxY];
#pragma unroll
        for (int e = 0; e < kPfMaxY; ++e) yj[e] = e < Y ? a.y[((int64_t)j * Y + e) * ld + b] : 0.0;

        // ---- propagate every particle and add the log-likelihood of y_j to its log-weight ----
        double vmax = -INFINITY;
        for (int i = tid; i < N; i += kPfBlock) {
            double xs[kMaxIntegrandIn], o[SSMQ_MAX_DIM], q[kPfMaxQ], z[kPfMaxQ];
#pragma unroll
            for (int k = 0; k < kMaxIntegrandIn; ++k) xs[k] = xa[(k < D ? k : 0) * N + i];
#pragma unroll
            for (int e = 0; e < SSMQ_MAX_DIM; ++e) o[e] = 0.0;
#ifndef SSMQ_PF_NO_MODEL
            eval_integrand(a.fid_dyn, xs, t, a.fd, o);
#else
#pragma unroll
            for (int d = 0; d < D; ++d) o[d] = 0.9 * xs[d];          // timing variant: no model evaluation
#endif
            pf_normals<kPfMaxQ>(a, traj, (uint32_t)j, kPfNoise, (uint32_t)i, a.dq, z);
            double sc = 1.0;
            if constexpr (QK == 1) {
                if (a.nuq > 0.0) sc = pf_t_factor(a, traj, (uint32_t)j, kPfNoiseGammaN, kPfNoiseGammaU, (uint32_t)i, a.nuq);
            }
#pragma unroll
            for (int r = 0; r < kPfMaxQ; ++r) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k <= r; ++k) s += a.Lq[r * kPfMaxQ + k] * z[k];
                if constexpr (QK == 1) s *= sc;
                q[r] = a.qm[r] + s;
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < kPfMaxQ; ++k) s += a.G[d * kPfMaxQ + k] * q[k];
                const double xn = o[d] + s;
                xa[d * N + i] = xn;
                if (a.part) __builtin_nontemporal_store(xn, &a.part[(((int64_t)j * D + d) * a.B + b) * N + i]);
            }
            // measurement model on the new particle, its inputs through the state index (as gather_inputs of ssmq_simulate.hip)
#pragma unroll
            for (int k = 0; k < kMaxIntegrandIn; ++k) {
                const int src = a.fo.n_idx > 0 ? (k < a.fo.n_idx ? a.fo.idx[k] : 0) : (k < D ? k : 0);
                xs[k] = xa[src * N + i];
            }
#pragma unroll
            for (int e = 0; e < SSMQ_MAX_DIM; ++e) o[e] = 0.0;
#ifndef SSMQ_PF_NO_MODEL
            eval_integrand(a.fid_obs, xs, t, a.fo, o);
#else
#pragma unroll
            for (int e = 0; e < kPfMaxY; ++e) o[e] = 0.5 * xs[e];
#endif
            // delta^2 = |Lr^-1 (y - h - r_mean)|^2 by forward substitution (rows beyond Y: zero residual, unit diagonal)
            double v[kPfMaxY], d2 = 0.0;
#pragma unroll
            for (int e = 0; e < kPfMaxY; ++e) {
                double s = e < Y ? yj[e] - o[e] - a.rm[e] : 0.0;
#pragma unroll
                for (int k = 0; k < e; ++k) s -= a.Lr[e * kPfMaxY + k] * v[k];
                v[e] = s / a.Lr[e * kPfMaxY + e];
                d2 += v[e] * v[e];
            }
            const double lp = a.student ? a.lognorm - 0.5 * (a.dof + (double)Y) * log1p(d2 / a.dof) : a.lognorm - 0.5 * d2;
            const double lw = w[i] + lp;
            w[i] = lw;
            vmax = pf_max(vmax, lw);
        }
        const double m = pf_block_max(vmax, red);
        if (!isfinite(m)) {
            // the trajectory fails at step j: NaN from here on (uniform over the workgroup: m is the same in every thread)
            for (int k = j * D + tid; k < T * D; k += kPfBlock) a.fm[(int64_t)k * ld + b] = qnan;
            for (int k = j * D * D + tid; k < T * D * D; k += kPfBlock) a.fP[(int64_t)k * ld + b] = qnan;
            for (int k = j + tid; k < T; k += kPfBlock) { a.ll[(int64_t)k * ld + b] = qnan; a.ess[(int64_t)k * ld + b] = qnan; }
            if (tid == 0) { a.ll[(int64_t)T * ld + b] = qnan; a.status[b] = 1 + j; }
            for (int k = j; k < T; ++k)
                for (int i = tid; i < N; i += kPfBlock) {
                    if (a.logw) a.logw[((int64_t)k * a.B + b) * N + i] = qnan;
                    if (a.anc) a.anc[((int64_t)k * a.B + b) * N + i] = -1;
                    if (a.part && k > j)
                        for (int d = 0; d < D; ++d) a.part[(((int64_t)k * D + d) * a.B + b) * N + i] = qnan;
                }
            return;
        }

        // ---- normalisation: S = sum exp(lw - m), ll_j = m + log S (the previous weights were normalised) ----
        double s1[1] = {0.0};
        for (int i = tid; i < N; i += kPfBlock) {
            const double e = exp(w[i] - m);
            xb[i] = e;
            s1[0] += e;
        }
        pf_block_sum<1>(s1, red);
        const double S = s1[0], lse = m + log(S);
        // ---- mean and sum of squared weights; xb row 0 <- w~ = e / S, w <- normalised log-weight ----
        double acc[D + 1];
#pragma unroll
        for (int d = 0; d <= D; ++d) acc[d] = 0.0;
        for (int i = tid; i < N; i += kPfBlock) {
            const double wt = xb[i] / S, lwn = w[i] - lse;
            xb[i] = wt;
            w[i] = lwn;
            if (a.logw) __builtin_nontemporal_store(lwn, &a.logw[((int64_t)j * a.B + b) * N + i]);
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += wt * xa[d * N + i];
            acc[D] += wt * wt;
        }
        pf_block_sum<D + 1>(acc, red);
        const double ess = 1.0 / acc[D];
        // ---- covariance, second pass around the mean (lower triangle, row-major packed) ----
        constexpr int NC = D * (D + 1) / 2;
        double cv[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) cv[k] = 0.0;
        for (int i = tid; i < N; i += kPfBlock) {
            const double wt = xb[i];
            double dx[D];
#pragma unroll
            for (int d = 0; d < D; ++d) dx[d] = xa[d * N + i] - acc[d];
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) cv[r * (r + 1) / 2 + c] += wt * (dx[r] * dx[c]);
        }
        pf_block_sum<NC>(cv, red);
        total += lse;
        if (tid == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) a.fm[((int64_t)j * D + d) * ld + b] = acc[d];
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) {
                    const double val = cv[r * (r + 1) / 2 + c];
                    a.fP[((int64_t)j * D * D + r * D + c) * ld + b] = val;
                    a.fP[((int64_t)j * D * D + c * D + r) * ld + b] = val;
                }
            a.ll[(int64_t)j * ld + b] = lse;
            a.ess[(int64_t)j * ld + b] = ess;
        }

        // ---- systematic resampling ----
        const bool resample = a.ess_threshold >= 1.0 ? true : (a.ess_threshold <= 0.0 ? false : ess < a.ess_threshold * dN);
        if (!resample) {
            if (a.anc)
                for (int i = tid; i < N; i += kPfBlock) a.anc[((int64_t)j * a.B + b) * N + i] = i;
            continue;
        }
        // CDF: inclusive prefix sum of w~ (xb row 0) into w, chunk by chunk (N is a multiple of 64: whole waves are in or out)
        double carry = 0.0;
        for (int base = 0; base < N; base += kPfBlock) {
            const int i = base + tid;
            double sc = i < N ? xb[i] : 0.0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double up = __shfl_up(sc, o);
                if (lane >= o) sc += up;
            }
            __syncthreads();
            if (lane == 63) red[wave] = sc;
            __syncthreads();
            double off = carry;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (v < wave) off += red[v];
                carry += red[v];
            }
            if (i < N) w[i] = off + sc;
        }
        __syncthreads();
        if (tid == 0) w[N - 1] = 1.0;
        __syncthreads();
        // ancestors: the smallest m with cdf[m] > p_i, by binary search; gather into xb (its row 0, w~, is not needed any more)
        const double u = uniform_one(a.seed, traj, (uint32_t)j, kPfResample);
        for (int i = tid; i < N; i += kPfBlock) {
            const double p = ((double)i + u) / dN;
            int lo = 0, hi = N - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (w[mid] > p) hi = mid; else lo = mid + 1;
            }
#pragma unroll
            for (int d = 0; d < D; ++d) xb[d * N + i] = xa[d * N + lo];
            if (a.anc) a.anc[((int64_t)j * a.B + b) * N + i] = lo;
        }
        __syncthreads();                   // every search and every gather is done
        for (int i = tid; i < N; i += kPfBlock) w[i] = log_unif;
        double *sw = xa; xa = xb; xb = sw;
    }
    if (tid == 0) { a.ll[(int64_t)T * ld + b] = total; a.status[b] = 0; }
}

typedef void (*pf_kernel)(const PfArgs);
template <int D, int QK> constexpr pf_kernel pf_kernel_of() { return k_particle_filter<D, QK>; }

}  // namespace

int launch_particle_filter(const PfLaunch &h, hipStream_t s) {
    PfArgs a;
    memset(&a, 0, sizeof(a));
    a.Y = h.Y; a.dq = h.dq; a.N = h.N; a.T = h.T; a.fid_dyn = h.f_dyn->id; a.fid_obs = h.f_obs->id; a.student = h.student;
    a.B = h.B; a.ld = h.ld; a.seed = h.seed; a.traj_offset = h.traj_offset; a.ess_threshold = h.ess_threshold; a.lognorm = h.lognorm;
    a.dof = h.dof; a.nu0 = h.nu0; a.nuq = h.nuq;
    memcpy(a.qm, h.qm, sizeof(a.qm)); memcpy(a.Lq, h.Lq, sizeof(a.Lq)); memcpy(a.G, h.G, sizeof(a.G));
    memcpy(a.rm, h.rm, sizeof(a.rm)); memcpy(a.Lr, h.Lr, sizeof(a.Lr));
    a.y = h.y; a.m0 = h.m0; a.P0 = h.P0; a.fm = h.fm; a.fP = h.fP; a.ll = h.ll; a.ess = h.ess; a.status = h.status;
    a.part = h.part; a.logw = h.logw; a.anc = h.anc;
    fill_fpar(h.f_dyn, &a.fd);
    fill_fpar(h.f_obs, &a.fo);
    static const pf_kernel table[2][kPfMaxD] = {
        {pf_kernel_of<1, 0>(), pf_kernel_of<2, 0>(), pf_kernel_of<3, 0>(), pf_kernel_of<4, 0>(), pf_kernel_of<5, 0>(), pf_kernel_of<6, 0>()},
        {pf_kernel_of<1, 1>(), pf_kernel_of<2, 1>(), pf_kernel_of<3, 1>(), pf_kernel_of<4, 1>(), pf_kernel_of<5, 1>(), pf_kernel_of<6, 1>()}};
    if (!pf_shape_ok(h.D, h.Y, h.dq, h.N) || h.B < 1 || h.B > 0x7fffffff || !pf_dof_ok(h.nu0) || !pf_dof_ok(h.nuq)) {
        set_error("particle filter: shape outside the kernel's range");
        return SSMQ_E_UNSUPPORTED;
    }
    const size_t lds = pf_lds_bytes(h.D, h.N);
    static thread_local unsigned attr_epoch = 0;
    int rc = set_max_dynamic_lds(attr_epoch, {(const void *)table[0][0], (const void *)table[0][1], (const void *)table[0][2],
                                              (const void *)table[0][3], (const void *)table[0][4], (const void *)table[0][5],
                                              (const void *)table[1][0], (const void *)table[1][1], (const void *)table[1][2],
                                              (const void *)table[1][3], (const void *)table[1][4], (const void *)table[1][5]},
                                 sizeof(double) * (kPfCloudDoubles + kPfRedDoubles));
    if (rc) return rc;
    hipLaunchKernelGGL(table[pf_noise_kind(h.nu0, h.nuq)][h.D - 1], dim3((unsigned)h.B), dim3(kPfBlock), lds, s, a);
    return hip_fail(hipGetLastError(), "k_particle_filter");
}

}  // namespace ssmq
