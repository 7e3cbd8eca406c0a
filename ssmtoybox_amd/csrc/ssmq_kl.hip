// KL and symmetrised KL divergence of batches of Gaussian pairs: the score of the reference's moment-transform accuracy studies
// (symmetrized_kl_divergence(mean_mc, cov_mc, mean, cov): research/gpq/polar2cartesian.py:92-93, research/bsq/bsq_mtran.py:179).
//
// Reference: ssmtoybox/utils.py:151-182 (kl_divergence) - as written there, with log(det P0 / det P1):
//     KL(0, 1) = 0.5 (tr(P1^-1 P0) + (m0 - m1)' P1^-1 (m0 - m1) + log(det P0 / det P1) - E)
// and :185-220 (symmetrized_kl_divergence) = 0.5 (KL(0, 1) + KL(1, 0)).
//
// One pair per lane, through the two Cholesky factors, taken in double-double arithmetic (the reference goes through det and inv):
//     tr(P1^-1 P0) = |L1^-1 L0|_F^2,   (m0 - m1)' P1^-1 (m0 - m1) = |L1^-1 (m0 - m1)|^2,   log(det P0 / det P1) = 2 sum (log L0_ii - log L1_ii)
// A pair with a factor that fails (a non-positive pivot) gets status 1 and NaN.  E <= 6, the range of the streaming Monte-Carlo
// transform whose output it scores.
#include "ssmq_host.h"

namespace ssmq {
namespace {

constexpr int kKlBlock = 64;
constexpr int kKlMaxDim = 6;

struct KlArgs {
    const double *m0, *P0, *m1, *P1;   // planes [E][ld], [E*E][ld]; with bcast0 m0 [E], P0 [E*E]
    double *kl;                        // [B]
    int32_t *status;                   // [B]
    int64_t B, ld;
    int32_t bcast0, symmetrized;
};

// Double-double arithmetic (an unevaluated sum h + l, |l| <= ulp(h) / 2; Dekker 1971, Knuth's two-sum, the product's error by
// one FMA).  The factorisations and substitutions below run in it: in plain fp64 the backward error eps |P| of a Cholesky factor
// becomes cond(P) eps in tr(P1^-1 P0) - 2e-10 of the value at condition 1e6, ten times what the reference's LU loses on the
// same pairs - while here the factor is exact to ~1e-32 |P| and the result carries the rounding of its last additions only.
// Nothing else in the library needs it; one pair per lane, so the cost (about 20 x the flops of E^3 / 3) is not on any hot path.
// The error-free transformations need every sum and product rounded exactly once, as written: contraction is off from here to the
// end of the file (the gfx950 back end fuses a product into a sum even where the product has other users - a two_sum fed the
// rounded product -p of a two_prod then adds the exact product instead, and its error term is no longer the sum's error: measured,
// the errors of the condition-1e6 pairs were those of plain fp64).  The fma() calls below are explicit.
#pragma clang fp contract(off)
struct dd {
    double h, l;
};
__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd quick_two_sum(double a, double b) {   // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_add(dd x, dd y) {
    dd s = two_sum(x.h, y.h);
    s.l += x.l + y.l;
    return quick_two_sum(s.h, s.l);
}
__device__ __forceinline__ dd dd_neg(dd x) { return {-x.h, -x.l}; }
__device__ __forceinline__ dd dd_mul(dd x, dd y) {
    dd p = two_prod(x.h, y.h);
    p.l += x.h * y.l + x.l * y.h;
    return quick_two_sum(p.h, p.l);
}
__device__ __forceinline__ dd dd_div(dd x, dd y) {
    const double q1 = x.h / y.h;
    dd r = dd_add(x, dd_neg(dd_mul(y, dd{q1, 0.0})));
    const double q2 = r.h / y.h;
    r = dd_add(r, dd_neg(dd_mul(y, dd{q2, 0.0})));
    const double q3 = r.h / y.h;
    const dd q = quick_two_sum(q1, q2);
    return dd_add(q, dd{q3, 0.0});
}
__device__ __forceinline__ dd dd_sqrt(dd x) {                      // x.h > 0
    const double s = sqrt(x.h);
    const dd r = dd_add(x, dd_neg(two_prod(s, s)));
    return quick_two_sum(s, r.h / (2.0 * s));
}

// Lower Cholesky factor of a packed symmetric matrix, left-looking as chol_packed<> (ssmq_device.h), in double-double; false at
// the first non-positive (or NaN) pivot - the factor is then without meaning and the caller writes NaN
template <int E>
__device__ __forceinline__ bool kl_chol(dd (&L)[E * (E + 1) / 2]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        dd ajj = L[SSMQ_PK(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) ajj = dd_add(ajj, dd_neg(dd_mul(L[SSMQ_PK(j, k)], L[SSMQ_PK(j, k)])));
        ok = ok && (ajj.h > 0.0);
        ajj = dd_sqrt(ajj);
        L[SSMQ_PK(j, j)] = ajj;
#pragma unroll
        for (int i = j + 1; i < E; ++i) {
            dd s = L[SSMQ_PK(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s = dd_add(s, dd_neg(dd_mul(L[SSMQ_PK(i, k)], L[SSMQ_PK(j, k)])));
            L[SSMQ_PK(i, j)] = dd_div(s, ajj);
        }
    }
    return ok;
}

// |La^-1 Lb|_F^2 + |La^-1 dm|^2: forward substitution, column by column (La^-1 Lb is lower triangular)
template <int E>
__device__ __forceinline__ dd kl_whitened(const dd (&La)[E * (E + 1) / 2], const dd (&Lb)[E * (E + 1) / 2], const dd (&dm)[E]) {
    dd acc = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < E; ++j) {
        dd w[E];
#pragma unroll
        for (int i = j; i < E; ++i) {
            dd s = Lb[SSMQ_PK(i, j)];
#pragma unroll
            for (int k = j; k < i; ++k) s = dd_add(s, dd_neg(dd_mul(La[SSMQ_PK(i, k)], w[k])));
            w[i] = dd_div(s, La[SSMQ_PK(i, i)]);
            acc = dd_add(acc, dd_mul(w[i], w[i]));
        }
    }
    dd v[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        dd s = dm[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = dd_add(s, dd_neg(dd_mul(La[SSMQ_PK(i, k)], v[k])));
        v[i] = dd_div(s, La[SSMQ_PK(i, i)]);
        acc = dd_add(acc, dd_mul(v[i], v[i]));
    }
    return acc;
}

template <int E>
__global__ __launch_bounds__(kKlBlock) void k_kl_divergence(const KlArgs a) {
    constexpr int TRI = E * (E + 1) / 2;
    const int64_t b = (int64_t)blockIdx.x * kKlBlock + threadIdx.x;
    if (b >= a.B) return;
    dd L0[TRI], L1[TRI], dm[E];
    const int64_t s0 = a.bcast0 ? 1 : a.ld, o0 = a.bcast0 ? 0 : b;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        dm[i] = two_sum(a.m0[i * s0 + o0], -a.m1[i * a.ld + b]);
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            L0[SSMQ_PK(i, j)] = {a.P0[(i * E + j) * s0 + o0], 0.0};
            L1[SSMQ_PK(i, j)] = {a.P1[(i * E + j) * a.ld + b], 0.0};
        }
    }
    const bool ok0 = kl_chol<E>(L0), ok1 = kl_chol<E>(L1);
    dd ld01 = {0.0, 0.0};              // sum (log L0_ii - log L1_ii), log(h + l) = log h + l / h
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const dd d0 = L0[SSMQ_PK(i, i)], d1 = L1[SSMQ_PK(i, i)];
        ld01 = dd_add(ld01, two_sum(log(d0.h) + d0.l / d0.h, -(log(d1.h) + d1.l / d1.h)));
    }
    const dd two_ld = {2.0 * ld01.h, 2.0 * ld01.l}, minus_e = {-(double)E, 0.0};
    const dd w01 = dd_add(kl_whitened<E>(L1, L0, dm), minus_e);
    dd kl = dd_add(w01, two_ld);       // 2 KL(0, 1)
    double out = 0.5 * (kl.h + kl.l);
    if (a.symmetrized) {               // 0.5 (KL(0, 1) + KL(1, 0)): the log-determinant terms cancel; the quadratic term is even in dm
        const dd w10 = dd_add(kl_whitened<E>(L0, L1, dm), minus_e);
        kl = dd_add(w01, w10);
        out = 0.25 * (kl.h + kl.l);
    }
    const bool ok = ok0 && ok1;
    a.kl[b] = ok ? out : __builtin_nan("");
    a.status[b] = ok ? 0 : 1;
}

}  // namespace
}  // namespace ssmq

using namespace ssmq;

extern "C" int ssmq_kl_divergence_dev(int E, int64_t B, int64_t ld, const double *d_m0, const double *d_P0, int bcast0,
                                      const double *d_m1, const double *d_P1, int symmetrized, double *d_kl, int32_t *d_status) {
    if (!d_m0 || !d_P0 || !d_m1 || !d_P1 || !d_kl || !d_status || B < 0 || ld < B) {
        set_error("kl_divergence: bad argument (null pointer, B < 0 or ld < B)");
        return SSMQ_E_ARG;
    }
    if (E < 1 || E > kKlMaxDim) {
        set_error("kl_divergence: 1 <= E <= 6 on the device");
        return SSMQ_E_UNSUPPORTED;
    }
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    const KlArgs a{d_m0, d_P0, d_m1, d_P1, d_kl, d_status, B, ld, bcast0 ? 1 : 0, symmetrized ? 1 : 0};
    const dim3 grid((unsigned)((B + kKlBlock - 1) / kKlBlock)), block(kKlBlock);
    hipStream_t s = stream();
    switch (E) {
        case 1: hipLaunchKernelGGL(k_kl_divergence<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_kl_divergence<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_kl_divergence<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_kl_divergence<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_kl_divergence<5>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(k_kl_divergence<6>, grid, block, 0, s, a); break;
    }
    return hip_fail(hipGetLastError(), "k_kl_divergence");
}
