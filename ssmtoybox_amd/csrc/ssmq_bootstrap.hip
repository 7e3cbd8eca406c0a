// Bootstrap variance of a sample mean, streamed on the device.
//
// Reference: ssmtoybox/utils.py:223-244 (bootstrap_var): S data sets of n entries drawn with replacement from the n entries of
// `data`, the mean of each, numpy.var of the S means.  The studies print +- 2 sqrt(bootstrap_var) next to every score
// (research/bsq/bsq_ungm.py:64-76, research/tpq/tpq_ungm.py:140-145).  The reference materialises the (S, n) matrix of draws; here
// every draw is generated where it is used, and nothing of size S n exists.
//
// THE DRAW.  Resample s (0 <= s < S) reads, at position i (0 <= i < n), entry j(s, i) of the included list:
//     (o0, o1, o2, o3) = Philox4x32-10(counter = (i >> 1, 0, s, kBootTag), key = (seed & 0xffffffff, seed >> 32))      (ssmq_rng.h)
//     word = o0 | o1 << 32   for even i,      word = o2 | o3 << 32   for odd i       (64 bits)
//     j    = (word * n) >> 64                                                         (the high half of the 128-bit product)
// with kBootTag = 0xB0075747.  One Philox call serves the positions 2 p and 2 p + 1.  j is a pure function of (seed, s, i, n): it
// does not depend on the number of rows, the launch geometry or the device, and it is uniform on 0 .. n-1 up to n / 2^64.
// The draws are shared by the R rows of a call, so row r of an R-row call is the single-row call on that row, bit for bit.
//
// THE SUMS.  The positions are cut into chunks of kBootChunk (a function of n alone).  A workgroup of kBootBlock lanes takes a
// (resample, chunk) tile: lane l adds, for k = 0, 1, ..., the entries at the positions 2 p and 2 p + 1, p = chunk kBootChunk / 2 +
// l + k kBootBlock, in that order; the 64 lanes of a wave are added by an xor butterfly (offsets 32, 16, ..., 1), the waves in wave
// order; the tile's R sums go to partial[s][chunk][r].  k_boot_means adds the chunks in chunk order and divides by n.  No
// floating-point atomics: the same (data, idx, S, seed) gives the same bits on every launch and every device.
//
// TWO ROUTES, one arithmetic: when the R n included values fit into the LDS of a CU next to the wave partials they are staged
// there once per workgroup (compacted: entry j of row r at [r n + j]) and a workgroup walks many tiles; otherwise they are
// gathered through L2 (data[r ld + idx[j]]).  SSMQ_BOOT_NO_LDS=1 forces the second route.
#include "ssmq_host.h"
#include "ssmq_rng.h"

namespace ssmq {
namespace {

constexpr uint32_t kBootTag = 0xB0075747u;
constexpr int kBootBlock = 512;                 // lanes of a workgroup
constexpr int kBootWaves = kBootBlock / 64;
constexpr int kBootChunk = 8192;                // positions of a tile: 8 Philox calls per lane
constexpr int kBootMaxRows = 19;                // D + 3 rows of the largest state
constexpr size_t kBootLdsMax = 160 * 1024 - 64;

struct BootArgs {
    const double *data;            // [R][ld]
    const int32_t *idx;            // [n] included entries, or null = 0 .. n-1
    double *partial;               // [S of this launch][chunks][R]
    int64_t ld, n, tiles;          // tiles = resamples of this launch * chunks
    int32_t R, chunks, s0;         // first resample of this launch
    uint64_t seed;
};

// RM: compile-time bound on R (accumulators in registers); WLDS: the included values are staged in LDS
template <int RM, bool WLDS>
__global__ __launch_bounds__(kBootBlock) void k_bootstrap_sums(BootArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    double *swave = sh;                                      // [kBootWaves][RM]
    double *sval = sh + kBootWaves * RM;                     // [R][n]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = a.R;
    const uint64_t n = (uint64_t)a.n;
    if (WLDS) {
        for (int64_t i = threadIdx.x; i < a.n; i += kBootBlock) {
            const int64_t e = a.idx ? (int64_t)a.idx[i] : i;
            for (int r = 0; r < R; ++r) sval[(int64_t)r * a.n + i] = a.data[(int64_t)r * a.ld + e];
        }
        __syncthreads();
    }
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint32_t s = (uint32_t)(a.s0 + tile / a.chunks);
        const int64_t chunk = tile % a.chunks;
        double acc[RM];
#pragma unroll
        for (int r = 0; r < RM; ++r) acc[r] = 0.0;
        const int64_t p_end = (a.n + 1) >> 1;                // Philox calls of a resample
        for (int k = 0; k < kBootChunk / 2 / kBootBlock; ++k) {
            const int64_t p = chunk * (kBootChunk / 2) + threadIdx.x + (int64_t)k * kBootBlock;
            if (p >= p_end) break;
            uint32_t c[4] = {(uint32_t)p, 0u, s, kBootTag};
            philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
            const uint64_t j0 = __umul64hi((uint64_t)c[0] | ((uint64_t)c[1] << 32), n);
            const uint64_t j1 = __umul64hi((uint64_t)c[2] | ((uint64_t)c[3] << 32), n);
            const bool two = 2 * p + 1 < a.n;
            if (WLDS) {
#pragma unroll
                for (int r = 0; r < RM; ++r)
                    if (r < R) {
                        acc[r] += sval[(int64_t)r * a.n + (int64_t)j0];
                        if (two) acc[r] += sval[(int64_t)r * a.n + (int64_t)j1];
                    }
            } else {
                const int64_t e0 = a.idx ? (int64_t)a.idx[j0] : (int64_t)j0;
                const int64_t e1 = a.idx ? (int64_t)a.idx[j1] : (int64_t)j1;      // j1 < n also where position 2 p + 1 does not exist
#pragma unroll
                for (int r = 0; r < RM; ++r)
                    if (r < R) {
                        acc[r] += a.data[(int64_t)r * a.ld + e0];
                        if (two) acc[r] += a.data[(int64_t)r * a.ld + e1];
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < RM; ++r)
            if (r < R) {
                double v = acc[r];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                if (lane == 0) swave[wave * RM + r] = v;
            }
        __syncthreads();
        if ((int)threadIdx.x < R) {
            double v = 0.0;
            for (int w = 0; w < kBootWaves; ++w) v += swave[w * RM + threadIdx.x];
            a.partial[tile * R + threadIdx.x] = v;
        }
        __syncthreads();                                     // swave is written again by the next tile
    }
}

// means[r][s0 + s] = (sum over chunks, in chunk order) / n
__global__ void k_boot_means(const double *partial, double *means, int chunks, int R, int S_launch, int s0, int S, double n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)S_launch * R) return;
    const int s = (int)(i / R), r = (int)(i % R);
    double v = 0.0;
    for (int c = 0; c < chunks; ++c) v += partial[((int64_t)s * chunks + c) * R + r];
    means[(int64_t)r * S + s0 + s] = v / n;
}

template <int RM>
int launch_boot_rm(const BootArgs &a, bool wlds, size_t lds, int64_t grid, hipStream_t s) {
    static thread_local unsigned attr_epoch = ~0u;
    int rc = set_max_dynamic_lds(attr_epoch, {(const void *)k_bootstrap_sums<RM, true>, (const void *)k_bootstrap_sums<RM, false>},
                                 kBootLdsMax);
    if (rc) return rc;
    if (wlds) hipLaunchKernelGGL((k_bootstrap_sums<RM, true>), dim3((unsigned)grid), dim3(kBootBlock), lds, s, a);
    else hipLaunchKernelGGL((k_bootstrap_sums<RM, false>), dim3((unsigned)grid), dim3(kBootBlock), lds, s, a);
    return hip_fail(hipGetLastError(), "k_bootstrap_sums");
}

int rows_bound(int R) { return R <= 1 ? 1 : R <= 4 ? 4 : R <= 8 ? 8 : kBootMaxRows; }

struct BootBuf {
    void *p = nullptr;
    ~BootBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return hip_fail(hipMalloc(&p, bytes ? bytes : 8), "hipMalloc"); }
};

// d_means [R][S] on the device <- the means of the S resamples of every row
int bootstrap_means(const double *d_data, int64_t ld, int R, const int32_t *d_idx, int64_t n, int S, uint64_t seed, double *d_means,
                    hipStream_t s) {
    const int RM = rows_bound(R);
    const int chunks = (int)((n + kBootChunk - 1) / kBootChunk);
    const size_t lds_waves = sizeof(double) * kBootWaves * RM, lds_vals = sizeof(double) * (size_t)R * (size_t)n;
    const bool wlds = lds_waves + lds_vals <= kBootLdsMax && !ssmq::sw("SSMQ_BOOT_NO_LDS");
    const size_t lds = wlds ? lds_waves + lds_vals : lds_waves;
    // the partials of at most 2^25 tiles' rows at a time (256 MiB): the resamples go in slabs, which changes no result
    const int64_t per_s = (int64_t)chunks * R;
    const int S_slab = (int)std::max<int64_t>(1, std::min<int64_t>(S, ((int64_t)1 << 25) / per_s));
    BootBuf partial;
    int rc = partial.alloc(sizeof(double) * (size_t)S_slab * per_s);
    if (rc) return rc;
    for (int s0 = 0; s0 < S; s0 += S_slab) {
        const int S_launch = std::min(S_slab, S - s0);
        BootArgs a{d_data, d_idx, (double *)partial.p, ld, n, (int64_t)S_launch * chunks, R, chunks, s0, seed};
        // the LDS route stages once per workgroup: as many workgroups as are resident (the LDS of a CU holds 160 KiB / lds of them);
        // the gather route has nothing to amortise.  The grid changes no result.
        const int64_t cap = wlds ? 256 * std::max<int64_t>(1, std::min<int64_t>(4, (int64_t)(kBootLdsMax / lds))) : 256 * 16;
        const int64_t grid = std::min<int64_t>(a.tiles, cap);
        switch (RM) {
            case 1: rc = launch_boot_rm<1>(a, wlds, lds, grid, s); break;
            case 4: rc = launch_boot_rm<4>(a, wlds, lds, grid, s); break;
            case 8: rc = launch_boot_rm<8>(a, wlds, lds, grid, s); break;
            default: rc = launch_boot_rm<kBootMaxRows>(a, wlds, lds, grid, s); break;
        }
        if (rc) break;
        const int64_t total = (int64_t)S_launch * R;
        hipLaunchKernelGGL(k_boot_means, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const double *)partial.p, d_means,
                           chunks, R, S_launch, s0, S, (double)n);
        if ((rc = hip_fail(hipGetLastError(), "k_boot_means"))) break;
    }
    hipError_t e = hipStreamSynchronize(s);      // `partial` is released on return
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

}  // namespace

bool bootstrap_range_ok(int64_t n, int S, int R) {
    return n >= 1 && n < ((int64_t)1 << 31) && S >= 1 && S <= (1 << 20) && R >= 1 && R <= kBootMaxRows;
}

}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_bootstrap_var_dev(const double *d_data, int64_t ld, int R, const int32_t *d_idx, int64_t n, int S, uint64_t seed,
                                      double *var, double *d_means) {
    if (!d_data || !var || !bootstrap_range_ok(n, S, R) || ld < n) {
        set_error("bootstrap_var: bad argument (1 <= n < 2^31, n <= ld, 1 <= S <= 2^20, 1 <= R <= 19)");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t s = stream();
    BootBuf own;
    if (!d_means) {
        if ((rc = own.alloc(sizeof(double) * (size_t)R * S))) return rc;
        d_means = (double *)own.p;
    }
    if ((rc = bootstrap_means(d_data, ld, R, d_idx, n, S, seed, d_means, s))) return rc;
    std::vector<double> m((size_t)R * S);
    SSMQ_HIP(hipMemcpyAsync(m.data(), d_means, sizeof(double) * m.size(), hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    // numpy.var (ddof 0) by the two-pass formula
    for (int r = 0; r < R; ++r) {
        const double *v = m.data() + (size_t)r * S;
        double mean = 0.0, ss = 0.0;
        for (int i = 0; i < S; ++i) mean += v[i];
        mean /= S;
        for (int i = 0; i < S; ++i) ss += (v[i] - mean) * (v[i] - mean);
        var[r] = ss / S;
    }
    return SSMQ_OK;
}

extern "C" int ssmq_bootstrap_var(const double *data, int64_t n, int S, uint64_t seed, double *var) {
    if (!data || !var || !bootstrap_range_ok(n, S, 1)) {
        set_error("bootstrap_var: bad argument (1 <= n < 2^31, 1 <= S <= 2^20)");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    BootBuf d;
    if ((rc = d.alloc(sizeof(double) * (size_t)n))) return rc;
    SSMQ_HIP(hipMemcpyAsync(d.p, data, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream()));
    SSMQ_HIP(hipStreamSynchronize(stream()));
    return ssmq_bootstrap_var_dev((const double *)d.p, n, 1, nullptr, n, S, seed, var, nullptr);
}
