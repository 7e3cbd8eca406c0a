// Multi-output GP quadrature weights (include/ssmq.h: ssmq_weights_gp_mo; MultiOutputModel.bq_weights, bq/bqmod.py:1254-1315).
// Stage one is the per-row weights code as it stands (ssmq_weights_gp with P = E: K, Cholesky, iK, q, R, Q_ee, the diagonal
// blocks of Wc, the variances).  Stage two, here: one workgroup per pair i > j forms Q_ij from the two parameter rows with the
// arithmetic of k_rbf_kxkx (one statement of it: ssmq_rbf_kxkx.h), the two products iK_i Q_ij iK_j with the matrices in LDS, symmetrises and
// writes both blocks [i][j] and [j][i].
#include <cmath>
#include <vector>
#include "ssmq_host.h"
#include "ssmq_weights_host.h"
#include "ssmq_rbf_kxkx.h"

namespace ssmq {
namespace {

constexpr int kMoPairBlock = 256;

// Q [E][E][N][N], Wc [E][E][N][N] (device): the blocks of pair blockIdx.x (i > j, packed order i (i - 1) / 2 + j)
__global__ __launch_bounds__(kMoPairBlock) void k_weights_mo_pairs(int D, int N, int E, const double *__restrict__ x,
                                                                   const double *__restrict__ par, const double *__restrict__ iK,
                                                                   double *__restrict__ Q, double *__restrict__ Wc) {
    extern __shared__ __align__(16) double lds[];
    double *sQ = lds, *sT = lds + N * N;
    int i = 1, rest = blockIdx.x;
    while (rest >= i) { rest -= i; ++i; }
    const int j = rest;
    const double *par0 = par + i * (1 + D), *par1 = par + j * (1 + D);
    const double *iKi = iK + (size_t)i * N * N, *iKj = iK + (size_t)j * N * N;
    const int tid = threadIdx.x;
    // Q_ij = exp_x_kxkx(par_i, par_j), scaling=False: the entry arithmetic of k_rbf_kxkx (ssmq_rbf_kxkx.h)
    const RbfKxkxPre pre = rbf_kxkx_pre(D, par0, par1, 0);
    for (int idx = tid; idx < N * N; idx += kMoPairBlock) {
        const double q = rbf_kxkx_entry(D, N, x, par0, par1, pre, idx / N, idx % N);
        sQ[idx] = q;
        if (Q) {
            Q[((size_t)i * E + j) * N * N + idx] = q;       // both blocks hold Q_ij untransposed, as the reference stores them
            Q[((size_t)j * E + i) * N * N + idx] = q;
        }
    }
    __syncthreads();
    if (!Wc) return;
    for (int idx = tid; idx < N * N; idx += kMoPairBlock) {     // T = iK_i Q_ij
        const int r = idx / N, s = idx % N;
        double acc = 0.0;
        for (int k = 0; k < N; ++k) acc += iKi[r * N + k] * sQ[k * N + s];
        sT[idx] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < N * N; idx += kMoPairBlock) {     // W = T iK_j, over Q_ij
        const int r = idx / N, s = idx % N;
        double acc = 0.0;
        for (int k = 0; k < N; ++k) acc += sT[r * N + k] * iKj[k * N + s];
        sQ[idx] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < N * N; idx += kMoPairBlock) {
        const int r = idx / N, s = idx % N;
        const double w = 0.5 * (sQ[r * N + s] + sQ[s * N + r]);  // (a + b = b + a: the block equals its transpose bit for bit)
        Wc[((size_t)i * E + j) * N * N + idx] = w;
        Wc[((size_t)j * E + i) * N * N + idx] = w;
    }
}

}  // namespace
}  // namespace ssmq

extern "C" int ssmq_weights_gp_mo(int D, int N, int E, const double *xi, const double *par, double jitter, double *wm, double *Wcc,
                                  double *iK, double *q, double *R, double *Wc, double *Q, double *model_var, double *integral_var,
                                  int32_t *status) {
    using namespace ssmq;
    if (D < 1 || N < 1 || E < 1 || !xi || !par) {
        set_error("weights_gp_mo: bad argument");
        return SSMQ_E_ARG;
    }
    if (D > SSMQ_MAX_DIM || E > SSMQ_MO_MAX_OUT || N > SSMQ_MO_MAX_PTS) {
        set_error("weights_gp_mo: the multi-output weights support D <= 16, E <= 8, N <= 64");
        return SSMQ_E_UNSUPPORTED;
    }
    // stage one: row e of `par` exactly as the single-output weights take it
    const size_t nn = (size_t)N * N;
    std::vector<double> iK1(E * nn), Q1(E * nn), Wc1(E * nn);
    std::vector<int32_t> st(E, 0);
    int rc = ssmq_weights_gp(D, N, xi, par, E, jitter, wm, Wc ? Wc1.data() : nullptr, Wcc, iK1.data(), q, Q ? Q1.data() : nullptr, R,
                             model_var, integral_var, st.data());
    if (status) std::copy(st.begin(), st.end(), status);
    if (rc) return rc;
    if (iK) std::copy(iK1.begin(), iK1.end(), iK);
    for (int e = 0; e < E; ++e) {
        if (Wc) std::copy(Wc1.begin() + e * nn, Wc1.begin() + (e + 1) * nn, Wc + ((size_t)e * E + e) * nn);
        if (Q) std::copy(Q1.begin() + e * nn, Q1.begin() + (e + 1) * nn, Q + ((size_t)e * E + e) * nn);
    }
    if (E == 1 || (!Wc && !Q)) return SSMQ_OK;
    // stage two: the cross pairs
    hipStream_t s = stream();
    DBuf dx, dp, dk, dq, dw;
    if ((rc = dx.alloc(sizeof(double) * D * N)) || (rc = dp.alloc(sizeof(double) * E * (1 + D))) || (rc = dk.alloc(sizeof(double) * E * nn)) ||
        (rc = dq.alloc(sizeof(double) * (Q ? (size_t)E * E * nn : 1))) || (rc = dw.alloc(sizeof(double) * (Wc ? (size_t)E * E * nn : 1))))
        return rc;
    SSMQ_HIP(hipMemcpyAsync(dx.p, xi, sizeof(double) * D * N, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dp.p, par, sizeof(double) * E * (1 + D), hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dk.p, iK1.data(), sizeof(double) * E * nn, hipMemcpyHostToDevice, s));
    const size_t lds = sizeof(double) * 2 * nn;      // 64 KB at N = 64
    static thread_local unsigned attr_epoch = ~0u;
    if ((rc = set_max_dynamic_lds(attr_epoch, {(const void *)k_weights_mo_pairs}, sizeof(double) * 2 * SSMQ_MO_MAX_PTS * SSMQ_MO_MAX_PTS)))
        return rc;
    hipLaunchKernelGGL(k_weights_mo_pairs, dim3(E * (E - 1) / 2), dim3(kMoPairBlock), lds, s, D, N, E, dx.d(), dp.d(), dk.d(),
                       Q ? dq.d() : nullptr, Wc ? dw.d() : nullptr);
    if ((rc = hip_fail(hipGetLastError(), "k_weights_mo_pairs"))) return rc;
    // the kernel wrote the blocks i != j; the diagonal ones are stage one's
    std::vector<double> hq(Q ? (size_t)E * E * nn : 0), hw(Wc ? (size_t)E * E * nn : 0);
    if (Q) SSMQ_HIP(hipMemcpyAsync(hq.data(), dq.p, sizeof(double) * E * E * nn, hipMemcpyDeviceToHost, s));
    if (Wc) SSMQ_HIP(hipMemcpyAsync(hw.data(), dw.p, sizeof(double) * E * E * nn, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < E; ++i)
        for (int j = 0; j < E; ++j) {
            if (i == j) continue;
            const size_t o = ((size_t)i * E + j) * nn;
            if (Q) std::copy(hq.begin() + o, hq.begin() + o + nn, Q + o);
            if (Wc) std::copy(hw.begin() + o, hw.begin() + o + nn, Wc + o);
        }
    return SSMQ_OK;
}
