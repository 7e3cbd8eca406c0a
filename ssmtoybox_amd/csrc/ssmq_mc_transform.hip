// Monte-Carlo moment transform of any sample count, streamed on the device: the ground truth of the reference's transform
// accuracy studies (MonteCarloTransform(dim, n=1e4): research/gpq/polar2cartesian.py:40, research/bsq/bsq_mtran.py:156,
// tests/test_mtran.py:38-52 up to n = 1e5).
//
// Reference: ssmtoybox/mtran.py:62-94 -
//     x_j = m + L z_j,  mean_f = sum f(x_j) / n,  cov_f = sum (f - mean_f)(f - mean_f)' / (n - 1),
//     cov_fx = sum (f - mean_f)(x_j - m)' / (n - 1).
//
// COUNTER LAYOUT, CHUNK SIZE, SUMMATION ORDER: stated in full in ssmq_mc_moments.h (the kernel body, which the run-time compiler
// embeds for user integrands).  In short: z_j[2 p], z_j[2 p + 1] = normal_pair(seed, j, p, 0x4D435446); chunks of kMcChunk = 2048
// samples, one workgroup of 256 lanes per (item, chunk) tile; k_mc_finish below adds an item's chunks in ascending order.
//
// THE PIVOT ALGEBRA (k_mc_finish).  With c = f(m), df_j = f(x_j) - c and the sums S1 = sum df, S2 = sum df df', S3 = sum df z',
// Sz = sum z of one pass:
//     mean_f = c + S1 / n
//     cov_f  = (S2 - S1 S1' / n) / (n - 1)                    (one value for both triangles)
//     cov_fx = ((S3 - S1 Sz' / n) / (n - 1)) L'               (x_j - m = L z_j)
// The pivot removes the offset of f, so S2 - S1 S1' / n cancels only what the spread of f around f(m) leaves.
// For n <= kMcChunk the pass runs twice, the second time around c = mean_f of the first (ssmq_mc_moments.h, SMALL n).
//
// RANGE.  1 <= D, E <= 6 (NA = E + E (E + 1) / 2 + E D + D accumulators per lane, 69 at D = E = 6), 2 <= n < 2^31, the built-in
// integrands in the (D, E, state-index) combinations of kMcTable, and user integrands without a state index.  Everything else:
// SSMQ_E_UNSUPPORTED before an output is touched.
//
// STATUS.  A covariance with a non-positive pivot: status 1 and NaN outputs for that item; the others are unaffected.
#include <algorithm>
#include "ssmq_host.h"
#include "ssmq_mc_moments.h"

namespace ssmq {
namespace {

struct McFinArgs {
    const double *partial, *head;
    double *mean_f, *cov_f, *cov_fx;   // [E][ld], [E*E][ld], [E*D][ld]
    int32_t *status;                   // [B]
    int64_t b0, ld;
    int32_t D, E, chunks;
    double n;
};

constexpr int kMcFinBlock = 128;

// one workgroup per item: lane v adds value v of the item's chunks in ascending order, then every lane forms outputs
__global__ __launch_bounds__(kMcFinBlock) void k_mc_finish(const McFinArgs a) {
    __shared__ double S[mc_na(kMcMaxDim, kMcMaxDim)];
    const int D = a.D, E = a.E, NA = mc_na(D, E);
    const int oS2 = E, oS3 = E + mc_tri(E), oSz = oS3 + E * D;
    const int64_t item = blockIdx.x, b = a.b0 + item;
    const double *h = a.head + item * kMcHead;
    const bool ok = h[0] != 0.0;
    const int tid = threadIdx.x;
    if (ok && tid < NA) {
        double s = 0.0;
        const double *p = a.partial + item * a.chunks * NA + tid;
        for (int c = 0; c < a.chunks; ++c) s += p[(int64_t)c * NA];
        S[tid] = s;
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    const double n = a.n, n1 = a.n - 1.0;
    const double *c = h + 1, *L = h + 1 + kMcMaxDim;
    for (int i = tid; i < E; i += kMcFinBlock) a.mean_f[i * a.ld + b] = ok ? c[i] + S[i] / n : nan;
    for (int i = tid; i < E * E; i += kMcFinBlock) {
        const int r = i / E, q = i % E, lo = r >= q ? r : q, hi = r >= q ? q : r;
        a.cov_f[i * a.ld + b] = ok ? (S[oS2 + SSMQ_PK(lo, hi)] - S[lo] * S[hi] / n) / n1 : nan;
    }
    for (int i = tid; i < E * D; i += kMcFinBlock) {
        const int e = i / D, d = i % D;
        double v = 0.0;
        for (int k = 0; k <= d; ++k) v += ((S[oS3 + e * D + k] - S[e] * S[oSz + k] / n) / n1) * L[SSMQ_PK(d, k)];
        a.cov_fx[i * a.ld + b] = ok ? v : nan;
    }
    if (tid == 0) a.status[b] = ok ? 0 : 1;
}

// z [D][count]: coordinate d of sample first + i at z[d * count + i]
__global__ void k_mc_unit_points(uint64_t seed, int D, int64_t first, int64_t count, double *z) {
    const int np = (D + 1) / 2;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * np) return;
    const int64_t i = t / np;
    const int p = (int)(t % np);
    double z0, z1;
    normal_pair(seed, (uint64_t)(first + i), (uint32_t)p, kMcTag, &z0, &z1);
    z[(int64_t)(2 * p) * count + i] = z0;
    if (2 * p + 1 < D) z[(int64_t)(2 * p + 1) * count + i] = z1;
}

typedef void (*mc_kernel_fn)(const McMomArgs);
struct McEntry {
    int fid, D, E, sel;
    mc_kernel_fn fn;
};
#define SSMQ_MC(F, D, E, SEL) {F, D, E, SEL, k_mc_moments<F, D, E, SEL>}
// (integrand, state dimension, outputs, state-index pattern: 0 the leading entries, 1 the entries 0, 2, ... - ssmq_apply_small.h)
const McEntry kMcTable[] = {
    SSMQ_MC(SSMQ_F_UNGM_DYN, 1, 1, 0),          SSMQ_MC(SSMQ_F_UNGM_MEAS, 1, 1, 0),
    SSMQ_MC(SSMQ_F_UNGMNA_DYN, 2, 1, 0),        SSMQ_MC(SSMQ_F_UNGMNA_MEAS, 2, 1, 0),
    SSMQ_MC(SSMQ_F_PENDULUM_DYN, 2, 2, 0),      SSMQ_MC(SSMQ_F_PENDULUM_MEAS, 2, 1, 0),
    SSMQ_MC(SSMQ_F_REENTRY1D_DYN, 3, 3, 0),     SSMQ_MC(SSMQ_F_RANGE_MEAS, 3, 1, 0),
    SSMQ_MC(SSMQ_F_REENTRY2D_DYN, 5, 5, 0),     SSMQ_MC(SSMQ_F_REENTRY2D_BIAS_DYN, 6, 6, 0),
    SSMQ_MC(SSMQ_F_RADAR2D_MEAS, 2, 2, 0),      SSMQ_MC(SSMQ_F_RADAR2D_MEAS, 5, 2, 0),
    SSMQ_MC(SSMQ_F_RADAR2D_MEAS, 6, 2, 0),      SSMQ_MC(SSMQ_F_RADAR2D_MEAS, 4, 2, 1),
    SSMQ_MC(SSMQ_F_RADAR2D_MEAS, 5, 2, 1),      SSMQ_MC(SSMQ_F_CT_DYN, 5, 5, 0),
    SSMQ_MC(SSMQ_F_BEARING_MEAS, 5, 4, 1),      SSMQ_MC(SSMQ_F_CV_DYN, 4, 4, 0),
};
#undef SSMQ_MC

struct McBuf {
    void *p = nullptr;
    ~McBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return hip_fail(hipMalloc(&p, bytes ? bytes : 8), "hipMalloc"); }
};

const char kMcRange[] = "mc_transform: the streaming Monte-Carlo transform covers 1 <= D <= 6, 1 <= E <= 6, 2 <= n < 2^31";

}  // namespace

bool mc_range_ok(int D, int E, int64_t n) {
    return D >= 1 && D <= kMcMaxDim && E >= 1 && E <= kMcMaxDim && n >= 2 && n < ((int64_t)1 << 31);
}

}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_mc_transform_dev(const ssmq_integrand *f, int D, int E, int64_t n, uint64_t seed, int64_t B, int64_t ld,
                                     const double *d_mean, const double *d_cov, const double *d_time, int time_stride,
                                     double *d_mean_f, double *d_cov_f, double *d_cov_fx, int32_t *d_status) {
    if (!f || !d_mean || !d_cov || !d_time || !d_mean_f || !d_cov_f || !d_cov_fx || !d_status || B < 0 || ld < B) {
        set_error("mc_transform: bad argument (null pointer, B < 0 or ld < B)");
        return SSMQ_E_ARG;
    }
    if (!mc_range_ok(D, E, n)) {
        set_error(kMcRange);
        return SSMQ_E_UNSUPPORTED;
    }
    FInfo fi;
    if (!integrand_info(f->id, &fi) || f->n_par < 0 || f->n_par > SSMQ_MAX_FPAR || f->n_idx < 0 || f->n_idx > SSMQ_MAX_FIDX) {
        set_error("mc_transform: unknown integrand id, or n_par / n_idx out of range");
        return SSMQ_E_ARG;
    }
    if (f->id == SSMQ_F_BEARING_MEAS) fi.dout = f->n_par / 2;
    if (fi.dout != E || (f->n_idx > 0 && f->n_idx < fi.din)) {
        set_error("mc_transform: the integrand's outputs do not match E, or its state index is shorter than its input");
        return SSMQ_E_ARG;
    }
    for (int k = 0; k < f->n_idx; ++k)
        if (f->idx[k] < 0 || f->idx[k] >= D) {
            set_error("mc_transform: state index out of range");
            return SSMQ_E_ARG;
        }
    const int sel = sel_pattern(f, fi.din);
    const bool user = is_user_integrand(f->id);
    mc_kernel_fn kern = nullptr;
    if (user) {
        if (f->n_idx != 0 || fi.din > D) {
            set_error("mc_transform: user integrands take the leading state entries (no state index, inputs <= D)");
            return SSMQ_E_UNSUPPORTED;
        }
    } else {
        for (const McEntry &e : kMcTable)
            if (e.fid == f->id && e.D == D && e.E == E && e.sel == sel) kern = e.fn;
        if (!kern) {
            set_error("mc_transform: no streaming kernel for integrand " + std::to_string(f->id) + " at D = " + std::to_string(D) +
                      ", E = " + std::to_string(E) + " with this state index (csrc/ssmq_mc_transform.hip: kMcTable)");
            return SSMQ_E_UNSUPPORTED;
        }
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    hipStream_t s = stream();
    const int NA = mc_na(D, E);
    const int chunks = (int)((n + kMcChunk - 1) / kMcChunk);
    // the partial sums of at most 2^25 values at a time (256 MiB), and at least one item: the items go in slabs, which changes no result
    const int64_t per_item = (int64_t)chunks * NA;
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)1 << 25) / per_item));
    McBuf partial, head;
    if ((rc = partial.alloc(sizeof(double) * (size_t)slab * per_item)) || (rc = head.alloc(sizeof(double) * (size_t)slab * kMcHead)))
        return rc;
    McMomArgs a{};
    a.mean = d_mean;
    a.cov = d_cov;
    a.time = d_time;
    a.partial = (double *)partial.p;
    a.head = (double *)head.p;
    a.ld = ld;
    a.n = n;
    a.chunks = chunks;
    a.time_stride = time_stride ? 1 : 0;
    a.seed = seed;
    fill_fpar(f, &a.fp);
    // one chunk: a second pass around the mean of the first (ssmq_mc_moments.h, SMALL n); the first pass's mean_f planes are its pivot
    const int passes = chunks == 1 ? 2 : 1;
    for (int64_t b0 = 0; b0 < B && !rc; b0 += slab)
    for (int pass = 0; pass < passes; ++pass) {
        const int64_t items = std::min(slab, B - b0);
        a.b0 = b0;
        a.tiles = items * chunks;
        a.pivot = pass ? d_mean_f : nullptr;
        if (user) {
            if ((rc = rtc_launch_mc(f, D, E, a, mc_grid(a.tiles), s))) break;
        } else {
            hipLaunchKernelGGL(kern, dim3(mc_grid(a.tiles)), dim3(kMcBlock), 0, s, a);
            if ((rc = hip_fail(hipGetLastError(), "k_mc_moments"))) break;
        }
        McFinArgs fa{a.partial, a.head, d_mean_f, d_cov_f, d_cov_fx, d_status, b0, ld, D, E, chunks, (double)n};
        hipLaunchKernelGGL(k_mc_finish, dim3((unsigned)items), dim3(kMcFinBlock), 0, s, fa);
        if ((rc = hip_fail(hipGetLastError(), "k_mc_finish"))) break;
    }
    hipError_t e = hipStreamSynchronize(s);      // `partial` and `head` are released on return
    if (rc) return rc;
    SSMQ_HIP(e);
    return SSMQ_OK;
}

extern "C" int ssmq_mc_unit_points(int D, uint64_t seed, int64_t first, int64_t count, double *z) {
    if (!z || D < 1 || D > kMcMaxDim || first < 0 || count < 0 || first + count > ((int64_t)1 << 31)) {
        set_error("mc_unit_points: bad argument (1 <= D <= 6, 0 <= first, first + count <= 2^31)");
        return SSMQ_E_ARG;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (count == 0) return SSMQ_OK;
    hipStream_t s = stream();
    McBuf d;
    if ((rc = d.alloc(sizeof(double) * (size_t)D * count))) return rc;
    const int64_t threads = count * ((D + 1) / 2);
    hipLaunchKernelGGL(k_mc_unit_points, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, seed, D, first, count, (double *)d.p);
    if ((rc = hip_fail(hipGetLastError(), "k_mc_unit_points"))) return rc;
    SSMQ_HIP(hipMemcpyAsync(z, d.p, sizeof(double) * (size_t)D * count, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    return SSMQ_OK;
}
