// Streaming Monte-Carlo moment transform: the kernel body (k_mc_moments<>), shared by the ahead-of-time instantiations of
// ssmq_mc_transform.hip and the run-time compiled ones of a user integrand (ssmq_rtc.hip embeds this header).
//
// Reference: ssmtoybox/mtran.py:62-94 (MonteCarloTransform.apply).  Nothing of size D n exists here: every unit sample is drawn
// where it is used.
//
// THE DRAW.  Sample j (0 <= j < n < 2^31) has the unit point z_j in R^D, two coordinates per Philox call:
//     (z_j[2 p], z_j[2 p + 1]) = normal_pair(seed, index = j, step = p, tag = kMcTag)        p = 0 .. ceil(D / 2) - 1   (ssmq_rng.h)
// i.e. Philox4x32-10 with counter (j, 0, p, kMcTag), key (seed lo, seed hi), two 53-bit uniforms u1 = ((o0 >> 5) 2^26 + (o1 >> 6)
// + 1/2) 2^-53, u2 likewise from (o2, o3), and Box-Muller r = sqrt(-2 log u1), z[2 p] = r cos(2 pi u2), z[2 p + 1] = r sin(2 pi u2).
// For odd D the second value of the last pair is dropped.  kMcTag = 0x4D435446 is used by nothing else in ssmq_rng.h's users.
// z_j is a function of (seed, j, p) alone - not of the batch item: every item of a batch sees the same unit samples, as the
// reference draws its unit points once and reuses them for every apply().
//
// THE SUMS.  One pass around the pivot c = f(m):  with df = f(m + L z) - c,
//     S1 = sum df,  S2 = sum df df' (lower triangle),  S3 = sum df z',  Sz = sum z          (NA = E + E (E + 1) / 2 + E D + D values)
// and ssmq_mc_transform.hip's k_mc_finish forms mean_f = c + S1 / n, cov_f = (S2 - S1 S1' / n) / (n - 1),
// cov_fx = ((S3 - S1 Sz' / n) / (n - 1)) L'.
//
// SMALL n.  What the one-pass form cancels is n (mean_f - c)^2 / ((n - 1) cov_f) of the digits of cov_f.  With many samples that
// is of order one, with a handful it is whatever the draw makes it (two samples that land close to each other on the same side
// of f(m)).  So for n <= kMcChunk - one chunk, where a pass is cheapest - ssmq_mc_transform.hip runs the pass twice: the second
// time around the pivot c = mean_f of the first (McMomArgs::pivot), which leaves S1 at rounding level and nothing to cancel.
// Still a function of (seed, n, the item's inputs) alone.
//
// THE ORDER.  The samples are cut into chunks of kMcChunk = 2048.  A workgroup of kMcBlock = 256 lanes takes one (item, chunk)
// tile: lane l adds the samples chunk kMcChunk + l + k kMcBlock, k = 0 .. 7, in that order; the 64 lanes of a wave are added by
// an xor butterfly (offsets 32, 16, ..., 1), the four waves in wave order; the tile's NA sums go to partial[item][chunk][.], and
// k_mc_finish adds the chunks in ascending order.  No floating-point atomics.  An item's bits are a function of (seed, n, its
// own inputs): tiles are independent of the grid, of B and of how many workgroups share an item.
#pragma once
#include "ssmq_device.h"
#include "ssmq_apply_small.h"
#include "ssmq_rng.h"

namespace ssmq {

constexpr uint32_t kMcTag = 0x4D435446u;
constexpr int kMcBlock = 256;
constexpr int kMcWaves = kMcBlock / 64;
constexpr int kMcChunk = 2048;
constexpr int kMcMaxDim = 6;                                       // D and E of the streaming route
__host__ __device__ constexpr int mc_tri(int d) { return d * (d + 1) / 2; }
__host__ __device__ constexpr int mc_na(int D, int E) { return E + mc_tri(E) + E * D + D; }
constexpr int kMcHead = 1 + kMcMaxDim + mc_tri(kMcMaxDim);         // per item: ok | c [E] | L packed [D (D + 1) / 2]

struct McMomArgs {
    const double *mean;      // [D][ld]
    const double *cov;       // [D*D][ld], lower triangle read
    const double *time;      // [B] or [1]
    double *partial;         // [items of this launch][chunks][NA]
    double *head;            // [items of this launch][kMcHead], written by the tile of chunk 0
    const double *pivot;     // null: the pivot is f(m); else planes [E][ld] of the pivot of every item (the second pass of small n)
    int64_t b0, ld, n, tiles;   // first item of this launch; tiles = items of this launch * chunks
    int32_t chunks, time_stride;
    uint64_t seed;
    FPar fp;
};

// the D unit coordinates of sample j
template <int D>
__device__ __forceinline__ void mc_unit_point(uint64_t seed, uint64_t j, double (&z)[D]) {
#pragma unroll
    for (int p = 0; p < (D + 1) / 2; ++p) {
        double z0, z1;
        normal_pair(seed, j, (uint32_t)p, kMcTag, &z0, &z1);
        pin_v(z0);      // the rounded product r cos / r sin is the draw: never fused into a sum that follows
        pin_v(z1);
        z[2 * p] = z0;
        if (2 * p + 1 < D) z[2 * p + 1] = z1;
    }
}

template <int F, int D, int E, int SEL>
__global__ __launch_bounds__(kMcBlock) void k_mc_moments(const McMomArgs a) {
    constexpr int TRI = mc_tri(D), NA = mc_na(D, E);
    constexpr int oS2 = E, oS3 = E + mc_tri(E), oSz = oS3 + E * D;
    using Fun = Fn<F>;
    constexpr int DIN = Fun::DIN;
    __shared__ double swave[kMcWaves * NA];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t item = tile / a.chunks, b = a.b0 + item;
        const int chunk = (int)(tile % a.chunks);
        double m[D], L[TRI];
#pragma unroll
        for (int d = 0; d < D; ++d) m[d] = a.mean[d * a.ld + b];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) L[SSMQ_PK(i, j)] = a.cov[(i * D + j) * a.ld + b];
        const bool ok = chol_packed<D>(L);
        Fun fn;
        fn.init(a.time[a.time_stride ? b : 0], a.fp);
        double c[E];
        {
            double xs[DIN];
            select_inputs<D, DIN, SEL>(m, xs);
            fn.template eval<E>(xs, c);
        }
        if (a.pivot) {
#pragma unroll
            for (int e = 0; e < E; ++e) c[e] = a.pivot[e * a.ld + b];
        }
        if (chunk == 0 && threadIdx.x == 0) {
            double *h = a.head + item * kMcHead;
            h[0] = ok ? 1.0 : 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) h[1 + e] = c[e];
#pragma unroll
            for (int i = 0; i < TRI; ++i) h[1 + kMcMaxDim + i] = L[i];
        }
        if (!ok) continue;                 // (the whole workgroup: the item's outputs are NaN, its partial rows are never read)
        double acc[NA];
#pragma unroll
        for (int v = 0; v < NA; ++v) acc[v] = 0.0;
        for (int k = 0; k < kMcChunk / kMcBlock; ++k) {
            const int64_t j = (int64_t)chunk * kMcChunk + (int64_t)k * kMcBlock + threadIdx.x;
            if (j >= a.n) break;
            double z[D], x[D], xs[DIN], o[E];
            mc_unit_point<D>(a.seed, (uint64_t)j, z);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                double s = m[d];
#pragma unroll
                for (int q = 0; q <= d; ++q) s += L[SSMQ_PK(d, q)] * z[q];
                x[d] = s;
            }
            select_inputs<D, DIN, SEL>(x, xs);
            fn.template eval<E>(xs, o);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double df = o[e] - c[e];
                o[e] = df;
                acc[e] += df;
            }
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int e2 = 0; e2 <= e; ++e2) acc[oS2 + SSMQ_PK(e, e2)] += o[e] * o[e2];
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int d = 0; d < D; ++d) acc[oS3 + e * D + d] += o[e] * z[d];
#pragma unroll
            for (int d = 0; d < D; ++d) acc[oSz + d] += z[d];
        }
#pragma unroll
        for (int v = 0; v < NA; ++v) {
            double s = acc[v];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0) swave[wave * NA + v] = s;
        }
        __syncthreads();
        if ((int)threadIdx.x < NA) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < kMcWaves; ++w) s += swave[w * NA + threadIdx.x];
            a.partial[tile * NA + threadIdx.x] = s;
        }
        __syncthreads();                   // swave is written again by the next tile
    }
}

#ifndef __HIPCC_RTC__
// grid of a launch over `tiles` tiles: enough workgroups to fill the device, never more than there are tiles (no result depends on it)
inline unsigned mc_grid(int64_t tiles) { return (unsigned)(tiles < 8192 ? tiles : 8192); }
#endif

}  // namespace ssmq
