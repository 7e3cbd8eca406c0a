// The two transforms that run on a model's Jacobian, one trajectory per lane, element planes in and out (element e of trajectory b
// at ptr[e ld + b]): 8 (D + D^2) bytes read and 8 (E + E^2 + E D) written per trajectory - HBM-bound maps.
//
// Linearisation (mtran.py:49-59: LinearizationTransform - the transform of ExtendedKalman, ssinf.py:347-357):
//   mean_f = f(mean),  J = f(mean, dx=True),  cov_fx = J cov,  cov_f = cov_fx J'.
//
// Taylor-GPQD (mtran.py:668-701: TaylorGPQDTransform - the transform of ExtendedKalmanGPQD, ssinf.py:1302-1319): the linearisation
// read as single-point Gaussian-process quadrature with derivative observations and an RBF kernel (scale alpha, length-scales ell,
// Lam = diag(ell^2)).  With f = f(mean), J = f(mean, dx=True), P = cov:
//   wm = det(Lam^-1 P + I)^-1/2,  wc = det(2 Lam^-1 P + I)^-1/2,  Wc = Lam/2 (Lam/2 + P)^-1 P,
//   model_var = alpha^2 - alpha^2 wc (1 + tr(Wc Lam^-1)),  integ_var = alpha^2 wc - wm^2,
//   mean_f = wm f,  cov_f = wc (f f' + J Wc J') - mean_f mean_f' + model_var (the scalar on EVERY entry, mtran.py:699),
//   cov_fx = J P (Lam + P)^-1 Lam   - (E, D), the convention of include/ssmq.h; the reference returns the transpose.
// On top of the linearisation's arithmetic: the Cholesky factors of Lam + P and Lam / 2 + P, whose pivots give both determinants
// (det(Lam^-1 P + I) = det(Lam + P) / det Lam), E triangular solve pairs for the cross-covariance and D for Wc - O(D^3) operations
// on registers.  Wc and the damping are formed as Lam (..)^-1 P, never as P - P (..)^-1 P or Lam - Lam (..)^-1 Lam: with long
// length-scales those differences cancel.  The symmetric P is read once, through its lower triangle.
// A pivot that is not positive (P not positive semi-definite) gives status 1 and NaN outputs.
//
// The model front ends make f(mean) and the E x D Jacobian (pitch D, zero where the model has no entry): jac_front_builtin for the
// models of ssmq_device.h, reached through the run-time switches eval_integrand / jac_integrand, used by k_linearize and
// k_taylor_gpqd; jac_front_user for a functor Fn<F> that ssmq_rtc.hip compiles at run time.  The linearisation kernels are: bounds
// check, front end, linearize_item - the algebra once for both.  The Taylor-GPQD kernels k_taylor_gpqd / k_taylor_gpqd_fn keep
// their item algebra in their own __global__ functions: moved into a shared inlined function, the same text compiles to 254 / 256
// registers at the 6-D user shapes where it takes 210 / 220 here, and loses a wave per SIMD.  The two copies hold
// the same sums in the same order and differ in what they keep, as said at the second.  This header is also compiled by hiprtc:
// no host code.
#pragma once
#include "ssmq_device.h"

namespace ssmq {

struct LinArgs {
    int32_t D, E, din, fid, time_stride, bcast;      // bcast: no state index and din == 1 < D
    const double *mean, *cov, *time, *cov_add;       // planes [D][ld], [D*D][ld]; time [B] or [1]; cov_add [E*E] or null
    double *mean_f, *cov_f, *cov_fx;                 // planes [E][ld], [E*E][ld], [E*D][ld]
    int32_t *status;
    int64_t B, ld;
    double cov_scale, ccov_scale;
    FPar fp;
};
struct TaylorGpqdArgs : LinArgs {
    double *model_var, *integ_var;                   // [B] each, or null
    double alpha;
    double ell[SSMQ_MAX_DIM];
};

// Built-in model: DT, ET > 0 are the transform's dimensions at compile time (everything in registers), 0 means run-time sizes and
// private arrays of the maximal size (scratch memory - the fallback).  o[SSMQ_MAX_DIM], J[EM * DM].  The inputs are gathered
// through the state index where there is one; the model's Jacobian is placed into the columns of the full state as
// MeasurementModel.meas_eval does (ssmod.py:985-1009): through the state index, or - without one - by `out[:, None] = jac`, which
// for a one-column Jacobian and a wider state BROADCASTS it into every column (Pendulum2DMeasurement on the 2-D state: both
// columns cos(x0)) - kept.
template <int DT, int ET>
__device__ __forceinline__ void jac_front_builtin(const LinArgs &a, const int64_t b, double *o, double *J) {
    constexpr int DM = DT > 0 ? DT : SSMQ_MAX_DIM, EM = ET > 0 ? ET : SSMQ_MAX_DIM;
    const int D = DT > 0 ? DT : a.D, E = ET > 0 ? ET : a.E, din = a.din;
    double x[DM], xs[kMaxIntegrandIn], Js[EM * DM];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = a.mean[d * a.ld + b];
#pragma unroll
    for (int k = 0; k < kMaxIntegrandIn; ++k) {
        const int src = a.fp.n_idx > 0 ? (k < a.fp.n_idx ? a.fp.idx[k] : 0) : (k < D ? k : 0);
        if (DT > 0) {                    // static register indices: a select chain over the DT candidates
            double v = x[0];
#pragma unroll
            for (int q = 1; q < DM; ++q) v = (src == q) ? x[q] : v;
            xs[k] = k < DM ? v : 0.0;
        } else {
            xs[k] = x[src];
        }
    }
    const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
    for (int e = 0; e < SSMQ_MAX_DIM; ++e) o[e] = 0.0;
    eval_integrand(a.fid, xs, t, a.fp, o);
    // the model's Jacobian with the compile-time pitch DM, then placed - every index static at the compile-time shapes (a pitch of
    // din, known only at run time, would put Js into scratch memory; at the run-time sizes it is there anyway, and the pitch din
    // keeps the zeroing and the placement short)
    const int pj = DT > 0 ? DM : din;
#pragma unroll
    for (int i = 0; i < E * pj; ++i) Js[i] = 0.0;
    jac_integrand<EM, DM, DT == 0>(a.fid, xs, t, a.fp, Js, pj, E);
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double v = 0.0;
            if (a.fp.n_idx > 0) {
#pragma unroll
                for (int k = 0; k < pj; ++k) v = (k < din && a.fp.idx[k] == d) ? Js[e * pj + k] : v;
            } else if (a.bcast) {
                v = Js[e * pj];
            } else {
                v = d < din ? Js[e * pj + d] : 0.0;
            }
            J[e * D + d] = v;
        }
}

// User functor Fn<F> (HAS_JAC): every dimension is a template argument, so all loops unroll and every array index is static.  The
// model reads the DIN leading state entries and its E x DIN Jacobian lands in the DIN leading columns.  o[E], J[E * D].
template <int F, int D, int E, int DIN>
__device__ __forceinline__ void jac_front_user(const LinArgs &a, const int64_t b, double *o, double *J) {
    static_assert(Fn<F>::HAS_JAC, "the integrand has no Jacobian");
    static_assert(DIN >= 1 && DIN <= D, "the integrand reads the leading DIN <= D state entries");
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = a.mean[d * a.ld + b];
    const double t = a.time ? a.time[a.time_stride ? b : 0] : 0.0;
    Fn<F> fn;
    fn.init(t, a.fp);
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = 0.0;
    fn.template eval<E>(x, o);
#pragma unroll
    for (int i = 0; i < E * D; ++i) J[i] = 0.0;
    fn.jac(x, J, D);
}

// The linearisation's item body: cov_fx = J cov, cov_f = cov_fx J' with the cov_add / cov_scale / ccov_scale hooks, from f(mean) in
// o and J; all remaining reads, arithmetic and stores.  DT, ET as above; KT: only the KT leading columns of J can be non-zero (DIN
// for a user model, D for a built-in one, whose state index can put an entry anywhere) - the terms of the columns behind them are
// left out of both products, they would add 0 * cov.
template <int DT, int ET, int KT>
__device__ __forceinline__ void linearize_item(const LinArgs &a, const int64_t b, const double *o, const double *J) {
    constexpr int DM = DT > 0 ? DT : SSMQ_MAX_DIM, EM = ET > 0 ? ET : SSMQ_MAX_DIM;
    const int D = DT > 0 ? DT : a.D, E = ET > 0 ? ET : a.E, K = DT > 0 ? KT : D;
    const int64_t ld = a.ld;
    double C[EM * DM];
    // Every sum stays in a register, which matters at the run-time sizes, where C lives in scratch memory.  The load of cov[k][d]
    // is written once per e: that each entry is READ once at the compile-time shapes is left to the compiler, which merges the
    // equal loads (no store lies between them).
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) s += J[e * D + k] * a.cov[(int64_t)(k * D + d) * ld + b];
            C[e * D + d] = s;
        }
#pragma unroll
    for (int e = 0; e < E; ++e) a.mean_f[e * ld + b] = o[e];
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            double s = 0.0;
#pragma unroll
            for (int d = 0; d < K; ++d) s += C[e * D + d] * J[e2 * D + d];
            s *= a.cov_scale;
            if (a.cov_add) s += a.cov_add[e * E + e2];
            a.cov_f[(int64_t)(e * E + e2) * ld + b] = s;
        }
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) a.cov_fx[(int64_t)(e * D + d) * ld + b] = C[e * D + d] * a.ccov_scale;
    a.status[b] = 0;
}

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

// The linearisation kernels: <DT, ET> for the built-in models (ssmq_linear.hip instantiates the shapes of the models that have a
// Jacobian, and <0, 0>), <F, D, E, DIN> for a user model (ssmq_rtc.hip instantiates it at run time: every shape gets a
// register-resident body).
template <int DT, int ET>
__global__ __launch_bounds__(256) void k_linearize(const LinArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    double o[SSMQ_MAX_DIM], J[(DT > 0 ? DT : SSMQ_MAX_DIM) * (ET > 0 ? ET : SSMQ_MAX_DIM)];
    jac_front_builtin<DT, ET>(a, b, o, J);
    linearize_item<DT, ET, DT>(a, b, o, J);
}
template <int F, int D, int E, int DIN>
__global__ __launch_bounds__(256) void k_linearize_fn(const LinArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    double o[E], J[E * D];
    jac_front_user<F, D, E, DIN>(a, b, o, J);
    linearize_item<D, E, DIN>(a, b, o, J);
}

// Taylor-GPQD for the built-in models, the formulas of the head of this file written out: full P and X = (Lam / 2 + P)^-1 P
template <int DT, int ET>
__global__ __launch_bounds__(256) void k_taylor_gpqd(const TaylorGpqdArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    constexpr int DM = DT > 0 ? DT : SSMQ_MAX_DIM, EM = ET > 0 ? ET : SSMQ_MAX_DIM;
    const int D = DT > 0 ? DT : a.D, E = ET > 0 ? ET : a.E;
    const int64_t ld = a.ld;
    double o[SSMQ_MAX_DIM], J[EM * DM], C[EM * DM];
    double P[DM * DM], L[DM * DM], X[DM * DM], lam[DM], ri[DM], col[DM];
    // the lower triangle of P, mirrored
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double v = a.cov[(int64_t)(i * D + j) * ld + b];
            P[i * D + j] = v;
            P[j * D + i] = v;
        }
    jac_front_builtin<DT, ET>(a, b, o, J);
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
            for (int k = 0; k < D; ++k) s += J[e * D + k] * P[k * D + d];
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
    // Lam / 2 + P = L L':  wc = sqrt(det(Lam / 2) / det(Lam / 2 + P)),  X = (Lam / 2 + P)^-1 P column by column,  Wc = Lam / 2 X
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
        for (int d = 0; d < D; ++d) col[d] = P[d * D + c];
        chol_solve_vec(L, ri, col, D);
        tr += 0.5 * col[c];                          // tr(Wc Lam^-1) = tr(X) / 2
#pragma unroll
        for (int d = 0; d < D; ++d) X[d * D + c] = 0.5 * lam[d] * col[d];
    }
    const double a2 = a.alpha * a.alpha;
    const double model_var = a2 - a2 * wc * (1.0 + tr), integ_var = a2 * wc - wm * wm;
    const double nan = __builtin_nan("");
    // C <- J Wc (E x D)
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += J[e * D + k] * X[k * D + d];
            C[e * D + d] = s;
        }
#pragma unroll
    for (int e = 0; e < E; ++e) a.mean_f[e * ld + b] = ok ? wm * o[e] : nan;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            double s = o[e] * o[e2];
#pragma unroll
            for (int d = 0; d < D; ++d) s += C[e * D + d] * J[e2 * D + d];
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
