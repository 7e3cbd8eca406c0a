// Monte-Carlo expectations of the RBF kernel under a standard multivariate Student-t density: the reference's 'rbf-student'
// kernel (RBFStudent, bq/bqkern.py:457-536), whose weights the Student-t process quadrature filter (TPQSF) uses.
//
//   sample s:  z ~ N(0, I_D), u ~ Gamma(nu / 2, scale 2 / nu), x = z / sqrt(u)            (utils.py:349-382 multivariate_t)
//              k_i = exp(-1/2 sum_d ((x_d - xi_id) / ell_d)^2),  i < N                      (scaling=False: alpha = 1)
//   k_student_expect   [K1 | 1 | X]' K0 / S = [Q ; q ; R]   with K0, K1 (S x N) the kernel values at the two parameter rows
//                      (one matrix when the rows are equal) and X (S x D) the samples: q = E[k0], R = E[x k0'],
//                      Q[i][j] = E[k1_i k0_j] (bq/bqkern.py:521-523) in ONE pass over the same samples.  The reference draws
//                      three independent sample sets; every estimate here is still unbiased, and with one sample set Q - q q'
//                      is a sample covariance, hence positive semi-definite.
//   k_student_kxy      the reference's exp_xy_kxy estimator (bq/bqkern.py:529-536) as it is: 10 000 batches of 200 samples, per
//                      batch the sum of alpha^2 k(x_a, x_b) over all 200 x 200 pairs, the diagonal included, the total divided by
//                      num_samples - not the pair mean E k(x, y) but about 200 times it at the default 2e6 samples (SURVEY.md
//                      appendix B).  One workgroup per batch.
//
// k_student_expect, per workgroup of 4 waves: a chunk of 64 samples (32 when the two parameter rows differ) is drawn and its rows
// [K1 (16 NT) | 1, x_1 .. x_D, 0 .. (32) | K0 (16 NT, only when it differs)] are staged in LDS, NT = ceil(N / 16); then
// v_mfma_f64_16x16x4_f64 accumulates the 16 x 16 tiles of the product over the chunk's samples, 4 per instruction.  Wave w owns
// the row tiles w, w + 4, w + 8 and every column tile; with one parameter row only the tiles on or above the diagonal of Q are
// formed and the lower triangle is mirrored on output, so Q is symmetric bit for bit.  Operand maps (ssmq_gemm_mfma.hip): A lane l
// -> A[l & 15][l >> 4], B lane l -> B[l >> 4][l & 15], C/D register r of lane l -> row (l >> 4) + 4 r, column l & 15.  The row
// pitch is a multiple of 16 doubles plus 4, so the four 16-lane groups of an operand read fall on disjoint banks.
//
// Determinism: a draw is a function of (seed, sample index, purpose tag) alone (ssmq_rng.h).  The samples are cut into slots of
// kMcBlockSamples = 8192 consecutive samples (a compile-time constant; beyond 1024 slots, i.e. 8.4e6 samples, a slot is the
// smallest multiple of 8192 that keeps their number at 1024 - a function of num_samples alone, never of the device); a slot's sums
// are accumulated in sample order in the matrix cores' registers and written to scratch, and a second kernel adds the slots in
// index order.  No floating-point atomics: the result is the same bits from run to run and for every grid size.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "ssmq_host.h"
#include "ssmq_rng.h"

namespace ssmq {
namespace {

constexpr int kMcThreads = 256;
constexpr int kMcChunkMax = 64;            // samples staged per round (16 MFMA k-steps)
constexpr int kMcBlockSamples = 8192;      // samples behind one partial sum
constexpr int kMcMaxSlots = 1024;
constexpr int kMcMaxD = 16, kMcMaxN = 128;
constexpr int kMcExtra = 32;               // columns [1 | x | 0]: two row tiles
constexpr uint32_t kMcTagExpect = 0x10u, kMcTagKxy = 0x11u;   // purpose tags (the simulators use 0 .. 2)
constexpr int kKxyBatches = 10000, kKxyBatch = 200;           // hard-coded in the reference (bq/bqkern.py:530-531)

typedef double mc_d4 __attribute__((ext_vector_type(4)));

struct McArgs {
    int32_t D, N, sym, chunk, nslots, pad;
    int64_t S, slot_samples;
    uint64_t seed;
    double dof;
    const double *xi;            // [D][N]
    const double *par0, *par1;   // [1 + D] each (the same pointer when sym)
    double *part;                // [nslots][N + 1 + D][N]
};

// 1 / sqrt(u), u ~ Gamma(dof / 2, scale 2 / dof), for (seed, index, purpose).  gamma_mt needs a shape >= 1: below it,
// Gamma(a) = Gamma(a + 1) U^(1 / a) (Marsaglia & Tsang 2000, section 6).  u is kept away from 0 so that x stays finite.
__device__ __forceinline__ double student_scale(uint64_t seed, uint64_t idx, uint32_t purpose, double dof) {
    const double shape = 0.5 * dof;
    double g;
    if (shape >= 1.0) {
        g = gamma_mt(seed, idx, 0u, purpose << 16, shape);
    } else {
        g = gamma_mt(seed, idx, 0u, purpose << 16, shape + 1.0);
        g *= pow(uniform_one(seed, idx, 0u, (purpose << 16) | 0x1ffu), 1.0 / shape);
    }
    g = fmax(g * (2.0 / dof), 1e-300);
    return 1.0 / sqrt(g);
}

template <int NT>
__global__ __launch_bounds__(kMcThreads) void k_student_expect(const McArgs a) {
    constexpr int RPW = (NT + 2 + 3) / 4;    // row tiles per wave: NT of K1 and up to two of [1 | x]
    extern __shared__ double rows[];         // [chunk][pitch]
    __shared__ double s_xi[kMcMaxD * kMcMaxN];
    __shared__ double s_il0[kMcMaxD], s_il1[kMcMaxD], s_sc[kMcChunkMax];
    const int D = a.D, N = a.N, CH = a.chunk, tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int offE = 16 * NT, offB = a.sym ? 0 : 16 * NT + kMcExtra;
    const int pitch = offB + 16 * NT + (a.sym ? kMcExtra : 0) + 4;
    const int ET = (1 + D + 15) / 16;        // row tiles of [1 | x]
    const int M = N + 1 + D;

    for (int idx = tid; idx < D * N; idx += kMcThreads) s_xi[idx] = a.xi[idx];
    if (tid < D) {
        s_il0[tid] = 1.0 / a.par0[1 + tid];
        s_il1[tid] = 1.0 / a.par1[1 + tid];
    }
    __syncthreads();

    for (int slot = blockIdx.x; slot < a.nslots; slot += gridDim.x) {
        mc_d4 acc[RPW][NT];
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) acc[r][ct] = mc_d4{0.0, 0.0, 0.0, 0.0};
        const int64_t s_begin = (int64_t)slot * a.slot_samples;
        const int64_t s_end = s_begin + a.slot_samples < a.S ? s_begin + a.slot_samples : a.S;
        for (int64_t c0 = s_begin; c0 < s_end; c0 += CH) {
            // ---- draw: part 0 of the threads the mixing variables, the others the normal pairs -----------------------
            {
                const int s = tid % CH, part = tid / CH, nparts = kMcThreads / CH;
                const int64_t gs = c0 + s;
                const bool valid = gs < s_end;
                double *row = rows + s * pitch + offE;
                if (part == 0) {
                    s_sc[s] = valid ? student_scale(a.seed, (uint64_t)gs, kMcTagExpect, a.dof) : 0.0;
                    row[0] = valid ? 1.0 : 0.0;
                    for (int c = 1 + D; c < kMcExtra; ++c) row[c] = 0.0;
                } else {
                    for (int j = part - 1; 2 * j < D; j += nparts - 1) {
                        double z0 = 0.0, z1 = 0.0;
                        if (valid) normal_pair(a.seed, (uint64_t)gs, 0u, (kMcTagExpect << 16) | (uint32_t)j, &z0, &z1);
                        row[1 + 2 * j] = z0;
                        if (2 * j + 1 < D) row[2 + 2 * j] = z1;
                    }
                }
            }
            __syncthreads();
            for (int idx = tid; idx < CH * D; idx += kMcThreads) {
                const int s = idx / D, d = idx % D;
                rows[s * pitch + offE + 1 + d] *= s_sc[s];
            }
            __syncthreads();
            // ---- kernel values: lanes over the points, waves over the samples (x_d wave-uniform) -------------------------
            for (int i = lane; i < 16 * NT; i += 64) {
                for (int s = wave; s < CH; s += kMcThreads / 64) {
                    double *row = rows + s * pitch;
                    double k0 = 0.0, k1 = 0.0;
                    if (i < N && row[offE] != 0.0) {
                        double m0 = 0.0, m1 = 0.0;
                        for (int d = 0; d < D; ++d) {
                            const double df = row[offE + 1 + d] - s_xi[d * N + i];
                            const double t0 = df * s_il0[d], t1 = df * s_il1[d];
                            m0 += t0 * t0;
                            m1 += t1 * t1;
                        }
                        k0 = exp(-0.5 * m0);
                        k1 = a.sym ? k0 : exp(-0.5 * m1);
                    }
                    row[i] = k1;
                    if (!a.sym) row[offB + i] = k0;
                }
            }
            __syncthreads();
            // ---- [K1 | 1 | X]' K0 on the matrix cores, 4 samples per instruction ------------------------------------------
            for (int ks = 0; ks < CH / 4; ++ks) {
                const double *row = rows + (4 * ks + lg) * pitch;
                double bf[NT], af[RPW];
#pragma unroll
                for (int ct = 0; ct < NT; ++ct) bf[ct] = row[offB + 16 * ct + li];
#pragma unroll
                for (int r = 0; r < RPW; ++r) {
                    const int rt = wave + 4 * r;
                    af[r] = rt < NT + ET ? row[16 * rt + li] : 0.0;
                }
#pragma unroll
                for (int r = 0; r < RPW; ++r) {
                    const int rt = wave + 4 * r;
                    if (rt >= NT + ET) continue;
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct) {
                        if (a.sym && rt < NT && ct < rt) continue;          // below the diagonal of Q: mirrored on output
                        acc[r][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[r], bf[ct], acc[r][ct], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
        // ---- the slot's sums: rows [0, N) of Q, row N of q, rows N + 1 .. N + D of R ------------------------------------
        double *part = a.part + (int64_t)slot * M * N;
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int rt = wave + 4 * r;
            if (rt >= NT + ET) continue;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                if (a.sym && rt < NT && ct < rt) continue;
                const int j = 16 * ct + li;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int i = lg + 4 * g;
                    const int orow = rt < NT ? 16 * rt + i : N + 16 * (rt - NT) + i;
                    const bool ok = j < N && (rt < NT ? 16 * rt + i < N : 16 * (rt - NT) + i < 1 + D);
                    if (ok) part[(int64_t)orow * N + j] = acc[r][ct][g];
                }
            }
        }
    }
}

// slots added in index order, divided by S; the lower triangle of a symmetric Q mirrors the upper one
__global__ __launch_bounds__(256) void k_student_reduce(int D, int N, int sym, int nslots, double inv_s,
                                                        const double *__restrict__ part, double *__restrict__ q,
                                                        double *__restrict__ R, double *__restrict__ Q) {
    const int M = N + 1 + D;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * N) return;
    const int row = idx / N, col = idx % N;
    int src = idx;
    if (sym && row < N && row > col) src = col * N + row;
    double s = 0.0;
    for (int k = 0; k < nslots; ++k) s += part[(int64_t)k * M * N + src];
    s *= inv_s;
    if (row < N) {
        if (Q) Q[idx] = s;
    } else if (row == N) {
        if (q) q[col] = s;
    } else if (R) {
        R[(row - N - 1) * N + col] = s;
    }
}

struct KxyArgs {
    int32_t D, nbatch;
    uint64_t seed;
    double dof;
    const double *par;   // [1 + D]
    double *sums;        // [nbatch]
};

// sum of 256 per-thread values in a fixed order (tree over LDS)
__device__ __forceinline__ double mc_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void k_student_kxy(const KxyArgs a) {
    constexpr int P = kMcMaxD + 1;
    __shared__ double xs[kKxyBatch * P], red[256];
    const int D = a.D, tid = threadIdx.x;
    const double alpha = a.par[0];
    for (int b = blockIdx.x; b < a.nbatch; b += gridDim.x) {
        if (tid < kKxyBatch) {
            const uint64_t gs = (uint64_t)b * kKxyBatch + tid;
            const double sc = student_scale(a.seed, gs, kMcTagKxy, a.dof);
            for (int j = 0; 2 * j < D; ++j) {
                double z0, z1;
                normal_pair(a.seed, gs, 0u, (kMcTagKxy << 16) | (uint32_t)j, &z0, &z1);
                xs[tid * P + 2 * j] = z0 * sc / a.par[1 + 2 * j];
                if (2 * j + 1 < D) xs[tid * P + 2 * j + 1] = z1 * sc / a.par[2 + 2 * j];
            }
        }
        __syncthreads();
        double sum = 0.0;
        for (int idx = tid; idx < kKxyBatch * kKxyBatch; idx += 256) {
            const int i = idx / kKxyBatch, j = idx % kKxyBatch;
            double m = 0.0;
            for (int d = 0; d < D; ++d) {
                const double df = xs[i * P + d] - xs[j * P + d];
                m += df * df;
            }
            sum += exp(-0.5 * m);
        }
        const double tot = mc_block_sum(sum, red);
        if (tid == 0) a.sums[b] = (alpha * alpha) * tot;
    }
}

__global__ __launch_bounds__(256) void k_student_kxy_reduce(int nbatch, double inv_s, const double *__restrict__ sums,
                                                            double *__restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int b = threadIdx.x; b < nbatch; b += 256) s += sums[b];
    const double tot = mc_block_sum(s, red);
    if (threadIdx.x == 0) out[0] = tot * inv_s;
}

struct McBuf {
    void *p = nullptr;
    ~McBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return hip_fail(hipMalloc(&p, bytes ? bytes : 8), "hipMalloc"); }
    double *d() { return (double *)p; }
};

// test hook: SSMQ_STUDENT_MC_GRID = number of workgroups (the results do not depend on it)
int mc_grid(int natural) {
    const char *v = sw("SSMQ_STUDENT_MC_GRID");
    if (!v) return natural;
    const long g = strtol(v, nullptr, 10);
    return g >= 1 ? (int)std::min<long>(g, natural) : natural;
}

int mc_range(const char *what, int D, int N, double dof, int64_t S) {
    if (D < 1 || D > kMcMaxD || N < 1 || N > kMcMaxN || S < 1 || S >= ((int64_t)1 << 31) || !(dof > 0.0) || !(dof < 1e300)) {
        set_error(std::string(what) + ": supported are D <= 16, N <= 128, 1 <= num_samples < 2^31 and dof > 0");
        return SSMQ_E_UNSUPPORTED;
    }
    return SSMQ_OK;
}

template <int NT>
int launch_expect(const McArgs &a, int grid, size_t lds, hipStream_t s) {
    SSMQ_HIP(hipFuncSetAttribute((const void *)k_student_expect<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_student_expect<NT>, dim3(grid), dim3(kMcThreads), lds, s, a);
    return hip_fail(hipGetLastError(), "k_student_expect");
}

}  // namespace
}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_rbf_student_expect(int D, int N, const double *x, const double *par0, const double *par1, double dof,
                                       int64_t num_samples, uint64_t seed, double *q, double *R, double *Q) {
    int rc = mc_range("ssmq_rbf_student_expect", D, N, dof, num_samples);
    if (rc) return rc;
    if (!x || !par0) {
        set_error("ssmq_rbf_student_expect: null points or parameters");
        return SSMQ_E_ARG;
    }
    if ((rc = ensure_device())) return rc;
    hipStream_t s = stream();
    const bool sym = !par1 || memcmp(par0, par1, sizeof(double) * (1 + D)) == 0;
    const int NT = (N + 15) / 16, M = N + 1 + D;
    const int64_t nblk = (num_samples + kMcBlockSamples - 1) / kMcBlockSamples;
    const int64_t per = (nblk + kMcMaxSlots - 1) / kMcMaxSlots;
    McArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.N = N; a.sym = sym ? 1 : 0; a.chunk = sym ? kMcChunkMax : kMcChunkMax / 2;
    a.S = num_samples; a.slot_samples = per * kMcBlockSamples; a.nslots = (int)((nblk + per - 1) / per);
    a.seed = seed; a.dof = dof;
    const size_t n_in = (size_t)D * N + 2 * (size_t)(1 + D), n_out = (size_t)M * N;
    McBuf buf;
    if ((rc = buf.alloc(sizeof(double) * (n_in + n_out + (size_t)a.nslots * M * N)))) return rc;
    double *dxi = buf.d(), *dp0 = dxi + (size_t)D * N, *dp1 = dp0 + (1 + D), *dout = dp1 + (1 + D);
    a.part = dout + n_out;
    SSMQ_HIP(hipMemcpyAsync(dxi, x, sizeof(double) * D * N, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dp0, par0, sizeof(double) * (1 + D), hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dp1, sym ? par0 : par1, sizeof(double) * (1 + D), hipMemcpyHostToDevice, s));
    a.xi = dxi; a.par0 = dp0; a.par1 = sym ? dp0 : dp1;
    const int pitch = (sym ? 16 * NT + kMcExtra : 32 * NT + kMcExtra) + 4;
    const size_t lds = sizeof(double) * (size_t)pitch * a.chunk;
    const int grid = mc_grid(a.nslots);
    switch (NT) {
        case 1: rc = launch_expect<1>(a, grid, lds, s); break;
        case 2: rc = launch_expect<2>(a, grid, lds, s); break;
        case 3: rc = launch_expect<3>(a, grid, lds, s); break;
        case 4: rc = launch_expect<4>(a, grid, lds, s); break;
        case 5: rc = launch_expect<5>(a, grid, lds, s); break;
        case 6: rc = launch_expect<6>(a, grid, lds, s); break;
        case 7: rc = launch_expect<7>(a, grid, lds, s); break;
        default: rc = launch_expect<8>(a, grid, lds, s); break;
    }
    if (rc) return rc;
    double *dq = dout + (size_t)N * N, *dR = dq + N, *dQ = dout;
    hipLaunchKernelGGL(k_student_reduce, dim3((M * N + 255) / 256), dim3(256), 0, s, D, N, a.sym, a.nslots,
                       1.0 / (double)num_samples, a.part, dq, dR, dQ);
    if ((rc = hip_fail(hipGetLastError(), "k_student_reduce"))) return rc;
    if (q) SSMQ_HIP(hipMemcpyAsync(q, dq, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    if (R) SSMQ_HIP(hipMemcpyAsync(R, dR, sizeof(double) * D * N, hipMemcpyDeviceToHost, s));
    if (Q) SSMQ_HIP(hipMemcpyAsync(Q, dQ, sizeof(double) * N * N, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    return SSMQ_OK;
}

extern "C" int ssmq_rbf_student_kxy(int D, const double *par, double dof, int64_t num_samples, uint64_t seed, double *out,
                                    double *batch_sums) {
    int rc = mc_range("ssmq_rbf_student_kxy", D, 1, dof, num_samples);
    if (rc) return rc;
    if (!par || !out) {
        set_error("ssmq_rbf_student_kxy: null parameters or output");
        return SSMQ_E_ARG;
    }
    if ((rc = ensure_device())) return rc;
    hipStream_t s = stream();
    McBuf buf;
    if ((rc = buf.alloc(sizeof(double) * ((size_t)(1 + D) + 1 + kKxyBatches)))) return rc;
    double *dpar = buf.d(), *dout = dpar + (1 + D), *dsums = dout + 1;
    SSMQ_HIP(hipMemcpyAsync(dpar, par, sizeof(double) * (1 + D), hipMemcpyHostToDevice, s));
    KxyArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.nbatch = kKxyBatches; a.seed = seed; a.dof = dof; a.par = dpar; a.sums = dsums;
    hipLaunchKernelGGL(k_student_kxy, dim3(mc_grid(kKxyBatches)), dim3(256), 0, s, a);
    if ((rc = hip_fail(hipGetLastError(), "k_student_kxy"))) return rc;
    hipLaunchKernelGGL(k_student_kxy_reduce, dim3(1), dim3(256), 0, s, kKxyBatches, 1.0 / (double)num_samples, dsums, dout);
    if ((rc = hip_fail(hipGetLastError(), "k_student_kxy_reduce"))) return rc;
    SSMQ_HIP(hipMemcpyAsync(out, dout, sizeof(double), hipMemcpyDeviceToHost, s));
    if (batch_sums) SSMQ_HIP(hipMemcpyAsync(batch_sums, dsums, sizeof(double) * kKxyBatches, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    return SSMQ_OK;
}
