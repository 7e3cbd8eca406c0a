// Bootstrap particle filter (ssmq_particle.hip: k_particle_filter<D>; ssmq_api_particle.hip: ssmq_particle_filter_dev) and the particle
// smoothers over its cloud (ssmq_particle_smooth.hip: k_particle_smooth<D>, k_particle_lineage<D>; ssmq_particle_smoother_dev): what
// the entry points hand the launchers.  Host arrays are padded to the kernels' fixed strides so that the kernels index them statically.
#pragma once
#include <cmath>
#include "ssmq_host.h"

namespace ssmq {

constexpr int kPfBlock = 256;          // threads per workgroup = per trajectory
constexpr int kPfMaxD = 6, kPfMaxY = 4, kPfMaxQ = 6;
constexpr int kPfMinN = 64, kPfMaxN = 4096;
constexpr int kPfCloudDoubles = 13312; // (2 D + 1) N: two [D][N] particle buffers and the [N] weights / CDF - 104 KB
constexpr int kPfRedDoubles = 96;      // reduction scratch: 4 wave partials of up to D (D + 1) / 2 = 21 sums, 4 scan totals
constexpr int kPsCloudDoubles = 16384; // (2 D + 2) N over the filter's range: alpha, beta [D][N], two [N] rows - 128 KB

struct PfLaunch {
    const ssmq_integrand *f_dyn, *f_obs;
    int D, Y, dq, N, T, student;
    int64_t B, ld;
    uint64_t seed, traj_offset;
    double ess_threshold, lognorm, dof;                     // lognorm: the measurement density's log-normaliser
    double nu0, nuq;                                        // degrees of freedom of a Student-t initial state / process noise, 0 = Gaussian
    double qm[kPfMaxQ], Lq[kPfMaxQ * kPfMaxQ], G[kPfMaxD * kPfMaxQ], rm[kPfMaxY], Lr[kPfMaxY * kPfMaxY];   // zero-padded; Lr: unit diagonal
    const double *y, *m0, *P0;
    double *fm, *fP, *ll, *ess;
    int32_t *status;
    double *part, *logw;
    int32_t *anc;
};

// N a multiple of 64 in 64 .. 4096 is the caller's check; D, Y, dq and the LDS budget are checked here
inline bool pf_shape_ok(int D, int Y, int dq, int N) {
    return D >= 1 && D <= kPfMaxD && Y >= 1 && Y <= kPfMaxY && dq >= 1 && dq <= kPfMaxQ && N <= kPfMaxN && (2 * D + 1) * N <= kPfCloudDoubles;
}
// the degrees of freedom of a Student-t initial state or process noise: 0 (Gaussian) or at least 2, the range of the Gamma sampler
// (Marsaglia-Tsang, shape nu / 2 >= 1)
inline bool pf_dof_ok(double nu) { return nu == 0.0 || (nu >= 2.0 && nu < INFINITY); }
// the kernels' compile-time noise kind QK: 1 where either of the two is Student-t
inline int pf_noise_kind(double nu0, double nuq) { return (nu0 > 0.0 || nuq > 0.0) ? 1 : 0; }
inline size_t pf_lds_bytes(int D, int N) { return sizeof(double) * ((size_t)(2 * D + 1) * N + kPfRedDoubles); }
int launch_particle_filter(const PfLaunch &h, hipStream_t s);

// The smoothers over the filter's cloud (include/ssmq.h ssmq_particle_smoother_dev states both recursions).
struct PsLaunch {
    const ssmq_integrand *f_dyn;
    int D, N, T, method;                                    // method: SSMQ_PS_MARGINAL or SSMQ_PS_GENEALOGY
    double nuq;                                             // marginal: degrees of freedom of Student-t process noise, 0 = Gaussian
    int64_t B, ld;
    double Li[kPfMaxD * kPfMaxD], gq[kPfMaxD];              // marginal: inverse of chol(G Q G') (lower, zero-padded), G q_mean
    const double *part, *logw, *fm, *fP, *ess;
    const int32_t *anc, *status;
    double *sm, *sP, *ess_s, *logw_s;
    int32_t *lineage, *unique;
};

// marginal: alpha, beta [D][N], the filter's log-weights and the row that carries ls - lv; genealogy: the final weights [N] and two
// int32 rows [N] (the lineage and the marks of the distinct count) - both with the reduction scratch
inline size_t ps_lds_bytes(int method, int D, int N) {
    return sizeof(double) * ((size_t)(method == SSMQ_PS_MARGINAL ? 2 * D + 2 : 2) * N + kPfRedDoubles);
}
int launch_particle_smoother(const PsLaunch &h, hipStream_t s);

#ifdef __HIPCC__
// ---- workgroup reductions of the particle kernels, in the order stated at the top of ssmq_particle.hip ----
// sums of K values over the workgroup; every thread gets the results
template <int K>
__device__ __forceinline__ void pf_block_sum(double (&v)[K], double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < K; ++q) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[q] += __shfl_xor(v[q], o);
    }
    __syncthreads();                       // the readers of the previous reduction are done with red
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) red[q * 4 + wave] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = (red[q * 4] + red[q * 4 + 1]) + (red[q * 4 + 2] + red[q * 4 + 3]);
}

// maximum that keeps a NaN (so that one NaN log-weight fails the step)
__device__ __forceinline__ double pf_max(double x, double y) { return (y > x || y != y) ? y : x; }
__device__ __forceinline__ double pf_block_max(double v, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = pf_max(v, __shfl_xor(v, o));
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return pf_max(pf_max(red[0], red[1]), pf_max(red[2], red[3]));
}
#endif

}  // namespace ssmq
