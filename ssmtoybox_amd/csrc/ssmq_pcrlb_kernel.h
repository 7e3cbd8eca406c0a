// The sums of the posterior Cramer-Rao recursion (include/ssmq.h: ssmq_pcrlb_sums_dev) over B true trajectories, planes p_0 .. p_T
// [T+1][D][ld]: per step j and trajectory b
//     k_pcrlb_dyn   F = df/dx (p_j, j):      the lower triangle of F' Qi F (D (D + 1) / 2 sums) and all of F (D D sums)
//     k_pcrlb_obs   H = dh/dx (p_{j+1}, j):  the lower triangle of H' Ri H (D (D + 1) / 2 sums)
// One model per kernel, so a user model pairs freely with a built-in one.  A read-bound map (8 D (T + 1) B bytes) with a reduction.
//
// Mapping: workgroup (j, g) of 256 threads takes the trajectories 256 g .. 256 g + 255 of step j, one per lane.  The Jacobian comes
// from the front ends of ssmq_jacobian_kernel.h - jac_front_builtin<DT, ET> for the built-in models (ssmq_pcrlb.hip instantiates the
// shapes of the models that have a Jacobian), jac_front_user<F, D, E, DIN> for a user functor (ssmq_rtc.hip, at run time) - fed the
// state plane of the step as their "mean" and entry j of a table 0 .. T-1 as their time: the measurement kernel reads plane j + 1 at
// time j, as the filters do.  Qi / Ri travel in the argument block (wave-uniform: scalar registers).  The products are formed in
// registers, fully unrolled: W J first (E x K, K the columns of J that can be non-zero), then J' (W J); at most 57 sums per lane (D = 6).
//
// Reduction, in an order fixed by B alone: a butterfly inside each wave (l ^ 32, 16, .. 1 - every lane ends with the same bits), the four
// wave results through LDS as (w0 + w1) + (w2 + w3), one row of partial sums per workgroup written to the workspace [T][nwg][N] with
// plain vector stores - no atomics.  A second kernel, k_pcrlb_rows (ssmq_pcrlb.hip), adds the rows of a step in ascending order of g (a separate kernel
// and not the tail of the first: the last workgroup of a step would have to be found through a counter in memory, an atomic and a
// fence for T sums of a few hundred doubles).  Lanes b >= B hold exact zeros and never load their columns (padding may hold anything);
// 0 + s = s, so ld and the grid do not enter the bits.  A non-finite term is not masked: it makes the sums of its step non-finite.
// This header is also compiled by hiprtc: no host code.
#pragma once
#include "ssmq_jacobian_kernel.h"

namespace ssmq {

constexpr int kPcrlbBlock = 256;
constexpr int kPcrlbMaxD = 6, kPcrlbMaxY = 4;

struct PcrlbArgs {
    LinArgs lin;                  // D, E, din, fid, bcast, fp, B, ld of the model; mean and time are set per workgroup
    const double *x;              // planes [T+1][D][ld]
    const double *steps;          // [T]: 0 .. T-1
    double *ws;                   // [T][nwg][N] rows of partial sums
    double W[kPcrlbMaxD * kPcrlbMaxD];   // Qi [D][D] (transition) or Ri [E][E] (measurement), row-major
    int32_t T, nwg;
};

__host__ __device__ constexpr inline int pcrlb_tri(int D) { return D * (D + 1) / 2; }

// acc[0 .. D (D + 1) / 2) <- the lower triangle of J' W J, packed (SSMQ_PK); J: E x D at pitch D, columns >= K zero; W: E x E
template <int D, int E, int K>
__device__ __forceinline__ void pcrlb_quad(const double *J, const double *W, double *acc) {
    double WJ[E * K];
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double s = 0.0;
#pragma unroll
            for (int e2 = 0; e2 < E; ++e2) s += W[e * E + e2] * J[e2 * D + k];
            WJ[e * K + k] = s;
        }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) {
            double s = 0.0;
            if (i < K) {
#pragma unroll
                for (int e = 0; e < E; ++e) s += J[e * D + i] * WJ[e * K + k];
            }
            acc[SSMQ_PK(i, k)] = s;
        }
}

// The workgroup's sums of acc[0 .. N) in the order stated at the top, written to row[0 .. N)
template <int N>
__device__ __forceinline__ void pcrlb_reduce_store(double (&acc)[N], double *row) {
    __shared__ double red[4 * N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) red[wave * N + q] = acc[q];
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        const int q = threadIdx.x;
        row[q] = (red[q] + red[N + q]) + (red[2 * N + q] + red[3 * N + q]);
    }
}

// what a workgroup does before its lanes part: step j, group g, the lane's trajectory, the front end's argument block for the step
__device__ __forceinline__ void pcrlb_setup(const PcrlbArgs &a, int plane_shift, LinArgs &la, int &j, int &g, int64_t &b) {
    j = (int)(blockIdx.x / (unsigned)a.nwg);
    g = (int)(blockIdx.x % (unsigned)a.nwg);
    b = (int64_t)g * kPcrlbBlock + threadIdx.x;
    la = a.lin;
    la.mean = a.x + (int64_t)(j + plane_shift) * la.D * la.ld;
    la.time = a.steps + j;
    la.time_stride = 0;
}

template <int D, int K, class FRONT>
__device__ __forceinline__ void pcrlb_dyn_body(const PcrlbArgs &a, FRONT front) {
    constexpr int N = pcrlb_tri(D) + D * D;
    LinArgs la;
    int j, g;
    int64_t b;
    pcrlb_setup(a, 0, la, j, g, b);
    double acc[N];
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = 0.0;
    if (b < la.B) {
        double o[SSMQ_MAX_DIM], J[D * D];
        front(la, b, o, J);
        pcrlb_quad<D, D, K>(J, a.W, acc);
#pragma unroll
        for (int q = 0; q < D * D; ++q) acc[pcrlb_tri(D) + q] = J[q];
    }
    pcrlb_reduce_store<N>(acc, a.ws + ((int64_t)j * a.nwg + g) * N);
}

template <int D, int E, int K, class FRONT>
__device__ __forceinline__ void pcrlb_obs_body(const PcrlbArgs &a, FRONT front) {
    constexpr int N = pcrlb_tri(D);
    LinArgs la;
    int j, g;
    int64_t b;
    pcrlb_setup(a, 1, la, j, g, b);
    double acc[N];
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = 0.0;
    if (b < la.B) {
        double o[SSMQ_MAX_DIM], J[E * D];
        front(la, b, o, J);
        pcrlb_quad<D, E, K>(J, a.W, acc);
    }
    pcrlb_reduce_store<N>(acc, a.ws + ((int64_t)j * a.nwg + g) * N);
}

// built-in models: DT, ET > 0 the shape at compile time (a state index can put a measurement's entries anywhere: K = D)
template <int DT, int ET>
__global__ __launch_bounds__(kPcrlbBlock) void k_pcrlb_dyn(const PcrlbArgs a) {
    static_assert(DT > 0 && DT == ET && DT <= kPcrlbMaxD, "k_pcrlb_dyn: a D -> D model, D <= 6");
    pcrlb_dyn_body<DT, DT>(a, [](const LinArgs &la, int64_t b, double *o, double *J) { jac_front_builtin<DT, ET>(la, b, o, J); });
}
template <int DT, int ET>
__global__ __launch_bounds__(kPcrlbBlock) void k_pcrlb_obs(const PcrlbArgs a) {
    static_assert(DT > 0 && ET > 0 && DT <= kPcrlbMaxD && ET <= kPcrlbMaxY, "k_pcrlb_obs: D <= 6, Y <= 4");
    pcrlb_obs_body<DT, ET, DT>(a, [](const LinArgs &la, int64_t b, double *o, double *J) { jac_front_builtin<DT, ET>(la, b, o, J); });
}
// user functor Fn<F> (HAS_JAC): its Jacobian fills the DIN leading columns
template <int F, int D, int DIN>
__global__ __launch_bounds__(kPcrlbBlock) void k_pcrlb_dyn_fn(const PcrlbArgs a) {
    static_assert(D <= kPcrlbMaxD, "k_pcrlb_dyn_fn: D <= 6");
    pcrlb_dyn_body<D, DIN>(a, [](const LinArgs &la, int64_t b, double *o, double *J) { jac_front_user<F, D, D, DIN>(la, b, o, J); });
}
template <int F, int D, int E, int DIN>
__global__ __launch_bounds__(kPcrlbBlock) void k_pcrlb_obs_fn(const PcrlbArgs a) {
    static_assert(D <= kPcrlbMaxD && E <= kPcrlbMaxY, "k_pcrlb_obs_fn: D <= 6, Y <= 4");
    pcrlb_obs_body<D, E, DIN>(a, [](const LinArgs &la, int64_t b, double *o, double *J) { jac_front_user<F, D, E, DIN>(la, b, o, J); });
}

}  // namespace ssmq
