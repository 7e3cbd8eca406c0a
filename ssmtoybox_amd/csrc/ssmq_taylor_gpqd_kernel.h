// The Taylor-GPQD transform's argument block and triangular helpers (both routes) and its kernel for a user model (ssmq_rtc.hip
// instantiates it at run time).  The built-in models keep k_taylor_gpqd<DT, ET> of ssmq_taylor_gpqd.hip, where the formulas are
// written out; a user model's shape is known when its kernel is compiled, so every shape of the run-time route gets a
// register-resident body.
#pragma once
#include "ssmq_device.h"

namespace ssmq {

struct TaylorGpqdArgs {
    int32_t D, E, din, fid, time_stride, bcast;      // bcast: no state index and din == 1 < D
    const double *mean, *cov, *time, *cov_add;       // planes [D][ld], [D*D][ld]; time [B] or [1]; cov_add [E*E] or null
    double *mean_f, *cov_f, *cov_fx;                 // planes [E][ld], [E*E][ld], [E*D][ld]
    double *model_var, *integ_var;                   // [B] each, or null
    int32_t *status;
    int64_t B, ld;
    double cov_scale, ccov_scale, alpha;
    double ell[SSMQ_MAX_DIM];
    FPar fp;
};

// lower Cholesky factor of the n x n matrix A (row-major, pitch n; the lower triangle is read and overwritten), ri = 1 / diagonal;
// returns the product of the diagonal of the factor (= sqrt(det A)), ok = every pivot positive
__device__ __forceinline__ double chol_lower(double *A, double *ri, int n, bool &ok) {
    double prod = 1.0;
#pragma unroll
    for (int j = 0; j < n; ++j) {
        double ajj = A[j * n + j];
#pragma unroll
        for (int k = 0; k < j; ++k) ajj -= A[j * n + k] * A[j * n + k];
        ok = ok && (ajj > 0.0);
        double s, r;
        sqrt_rsqrt(ajj, s, r);
        A[j * n + j] = s;
        ri[j] = r;
        prod *= s;
#pragma unroll
        for (int i = j + 1; i < n; ++i) {
            double v = A[i * n + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= A[i * n + k] * A[j * n + k];
            A[i * n + j] = v * r;
        }
    }
    return prod;
}
// x <- (L L')^-1 x
__device__ __forceinline__ void chol_solve_vec(const double *L, const double *ri, double *x, int n) {
#pragma unroll
    for (int i = 0; i < n; ++i) {
        double v = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i * n + k] * x[k];
        x[i] = v * ri[i];
    }
#pragma unroll
    for (int i = n - 1; i >= 0; --i) {
        double v = x[i];
#pragma unroll
        for (int k = i + 1; k < n; ++k) v -= L[k * n + i] * x[k];
        x[i] = v * ri[i];
    }
}

// The transform for the user functor Fn<F> (HAS_JAC): one trajectory per lane, the planes, the time argument, the cov_add /
// cov_scale / ccov_scale hooks, the variance planes and status 1 with NaN outputs on a non-positive pivot, all as k_taylor_gpqd.
// Every dimension is a template argument: all loops unroll, every array index is static.  The model's dout x DIN Jacobian lands
// in the DIN leading columns of the E x D matrix (pitch D); the zero columns behind them are left out of the products.  The
// per-item algebra is k_taylor_gpqd's, sum by sum; what differs is what is kept: column c of X = (Lam / 2 + P)^-1 P is folded
// into J Wc as soon as it is solved for (Wc = Lam / 2 X is never held as a matrix), and the symmetric P is held through its
// lower triangle - what keeps the D = E = 6 body in registers.
template <int F, int D, int E, int DIN>
__global__ __launch_bounds__(256) void k_taylor_gpqd_fn(const TaylorGpqdArgs a) {
    static_assert(Fn<F>::HAS_JAC, "k_taylor_gpqd_fn: the integrand has no Jacobian");
    static_assert(DIN >= 1 && DIN <= D, "k_taylor_gpqd_fn: the integrand reads the leading DIN <= D state entries");
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    const int64_t ld = a.ld;
    double x[D], o[E], J[E * D], C[E * D], W[E * D];
    double P[D * D], L[D * D], lam[D], ri[D], col[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = a.mean[d * ld + b];
    // the lower triangle of P; P[i * D + j] with j > i is never read below (SSMQ_PL swaps the indices)
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) P[i * D + j] = a.cov[(int64_t)(i * D + j) * ld + b];
#define SSMQ_PL(i, j) P[(i) >= (j) ? (i) * D + (j) : (j) * D + (i)]
    const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
    Fn<F> fn;
    fn.init(t, a.fp);
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = 0.0;
    fn.template eval<E>(x, o);
#pragma unroll
    for (int i = 0; i < E * D; ++i) J[i] = 0.0;
    fn.jac(x, J, D);
    bool ok = true;
    double ell_prod = 1.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        lam[d] = a.ell[d] * a.ell[d];
        ell_prod *= a.ell[d];
    }
    // C = J P (E x D)
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < DIN; ++k) s += J[e * D + k] * SSMQ_PL(k, d);
            C[e * D + d] = s;
        }
    // Lam + P = L L':  wm = sqrt(det Lam / det(Lam + P)),  cov_fx = C (Lam + P)^-1 Lam  (row e: one solve with the symmetric matrix)
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i * D + j] = P[i * D + j] + (i == j ? lam[i] : 0.0);
    const double wm = div_nr(ell_prod, chol_lower(L, ri, D, ok));
#pragma unroll
    for (int e = 0; e < E; ++e) {
#pragma unroll
        for (int d = 0; d < D; ++d) col[d] = C[e * D + d];
        chol_solve_vec(L, ri, col, D);
#pragma unroll
        for (int d = 0; d < D; ++d) a.cov_fx[(int64_t)(e * D + d) * ld + b] = col[d] * lam[d] * a.ccov_scale;      // (NaN below if a pivot fails)
    }
    // Lam / 2 + P = L L':  wc = sqrt(det(Lam / 2) / det(Lam / 2 + P)),  X = (Lam / 2 + P)^-1 P column by column,  Wc = Lam / 2 X,
    // W = J Wc (E x D) column by column
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i * D + j] = P[i * D + j] + (i == j ? 0.5 * lam[i] : 0.0);
    double half_prod = ell_prod;
#pragma unroll
    for (int d = 0; d < D; ++d) half_prod *= 0.70710678118654752440;
    const double wc = div_nr(half_prod, chol_lower(L, ri, D, ok));
    double tr = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
#pragma unroll
        for (int d = 0; d < D; ++d) col[d] = SSMQ_PL(d, c);
        chol_solve_vec(L, ri, col, D);
        tr += 0.5 * col[c];                          // tr(Wc Lam^-1) = tr(X) / 2
#pragma unroll
        for (int d = 0; d < D; ++d) col[d] = 0.5 * lam[d] * col[d];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < DIN; ++k) s += J[e * D + k] * col[k];
            W[e * D + c] = s;
        }
    }
#undef SSMQ_PL
    const double a2 = a.alpha * a.alpha;
    const double model_var = a2 - a2 * wc * (1.0 + tr), integ_var = a2 * wc - wm * wm;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int e = 0; e < E; ++e) a.mean_f[e * ld + b] = ok ? wm * o[e] : nan;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            double s = o[e] * o[e2];
#pragma unroll
            for (int d = 0; d < DIN; ++d) s += W[e * D + d] * J[e2 * D + d];
            s = wc * s - (wm * o[e]) * (wm * o[e2]) + model_var;
            s *= a.cov_scale;
            if (a.cov_add) s += a.cov_add[e * E + e2];
            a.cov_f[(int64_t)(e * E + e2) * ld + b] = ok ? s : nan;
        }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < E * D; ++i) a.cov_fx[(int64_t)i * ld + b] = nan;
    }
    if (a.model_var) a.model_var[b] = ok ? model_var : nan;
    if (a.integ_var) a.integ_var[b] = ok ? integ_var : nan;
    a.status[b] = ok ? 0 : 1;
}

}  // namespace ssmq
