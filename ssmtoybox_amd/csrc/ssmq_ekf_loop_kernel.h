// The extended Kalman filter's whole forward pass as one kernel (ssinf.py:347-357: ExtendedKalman, both transforms a
// linearisation, additive noise): one trajectory per lane, steps 0 .. T-1 in one launch, the filtered mean and covariance in
// registers from step to step.  Per step and trajectory the launch loop (k_linearize | k_linearize | k_kalman_update) moves
// 8 (2 D + 5 D^2 + 3 Y + 2 Y^2 + 2 Y D) bytes and three status words through HBM; this kernel reads the 8 Y bytes of y[k] and
// writes the 8 (D + D^2) of fm[k], fP[k] - with KEEP also the 8 (D + 2 D^2) of the predictive moments the smoother reads.
//
// One step, in the launch loop's order:
//   dyn front end at (m, t_k)      -> f(m), J                      (jac_front_builtin / jac_front_user, called as they are)
//   C_xx = J P,  P- = C_xx J' + GQG,  m- = f(m)                    (the sums of linearize_item, operands from registers)
//   obs front end at (m-, t_k)     -> h(m-), H
//   P_yx = H P-,  S = P_yx H' + R,  y- = h(m-)                     (linearize_item again)
//   gain, m = m- + gain (y - y-),  P = P- - (gain S) gain'         (the update of kalman_update_item<D, Y>, Y = 1 shortcut included)
// Neither covariance is symmetrised: the launch loop carries the full D x D matrix from kernel to kernel, so do the registers here.
// The sums and their order are those of linearize_item (ssmq_jacobian_kernel.h); the update is the per-lane linear algebra of
// ssmq_device.h: gain_from_cov<>, which kalman_update_item (ssmq_update.h) calls too, and sandwich<>, whose sums
// kalman_update_item writes out around its loads and stores.  The two routes agree to rounding, not to the bit (the compiler
// contracts and schedules the two kernels separately).
//
// The model front end is a template parameter (EkfFrontBuiltin, EkfFrontUser): it gets the state as a register array behind the
// planes' interface - a LinArgs whose mean plane is that array (ld = 1, item 0) and whose time argument is the step's - so the
// front ends of the linearisation kernels run unchanged; at the compile-time shapes every index is static and nothing of it reaches
// memory.  GQG, R and the time tables are the pass's constants (ssmq_host.h: PassConsts), read through the constant address space;
// a model with a time table gets the step's entry by value (FPar::tval), the entry the launch loop's kernels load themselves.
// status[b]: 0, or 1 + the first step whose innovation matrix is not positive definite; from that step on the trajectory's outputs
// are NaN (the NaN state propagates).  Lanes b >= B touch nothing.  This header is also compiled by hiprtc: no host code.
#pragma once
#include "ssmq_jacobian_kernel.h"

namespace ssmq {

struct EkfLoopArgs {
    LinArgs dyn, obs;                        // D, E, din, fid, bcast and fp of the two models (fp.ttab: the pass's table or null); no planes
    const double *y, *m0, *P0;               // [T][Y][ld], [D][ld], [D*D][ld]
    double *fm, *fP;                         // [T][D][ld], [T][D*D][ld]
    double *pm, *pP, *pC;                    // KEEP: predictive mean, covariance and C_xx of every step, [T][D][ld], [T][D*D][ld] twice
    int32_t *status;                         // [B]
    const double *gqg, *rr;                  // [D*D], [Y*Y]
    int64_t B, ld;
    int32_t T;
};

// f(x), J of a model at the state held in registers: x[D] -> o[SSMQ_MAX_DIM], J[E * D] (pitch D).  KT: only the KT leading columns
// of J can be non-zero (linearize_item).
__device__ __forceinline__ LinArgs ekf_front_args(const LinArgs &model, const double *x, const double *t, const int k) {
    LinArgs l = model;
    l.mean = x; l.ld = 1;
    l.time = t; l.time_stride = 0;
    if (model.fp.ttab) {
        l.fp.tval = ((cdouble_p)model.fp.ttab)[k];
        l.fp.use_tval = 1;
    }
    return l;
}
template <int D, int E>
struct EkfFrontBuiltin {
    static constexpr int KT = D;
    static __device__ __forceinline__ void run(const LinArgs &model, const double *x, const int k, double *o, double *J) {
        const double t = (double)k;
        const LinArgs l = ekf_front_args(model, x, &t, k);
        jac_front_builtin<D, E>(l, 0, o, J);
    }
};
template <int F, int D, int E, int DIN>
struct EkfFrontUser {
    static constexpr int KT = DIN;
    static __device__ __forceinline__ void run(const LinArgs &model, const double *x, const int k, double *o, double *J) {
        const double t = (double)k;
        const LinArgs l = ekf_front_args(model, x, &t, k);
        jac_front_user<F, D, E, DIN>(l, 0, o, J);
    }
};

// cov_fx = J cov (E x D), cov_f = cov_fx J' + add (E x E): the two products of linearize_item at cov_scale = ccov_scale = 1
template <int D, int E, int KT>
__device__ __forceinline__ void ekf_linearize_reg(const double *J, const double *cov, const cdouble_p add, double *C, double *cov_f) {
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < KT; ++k) s += J[e * D + k] * cov[k * D + d];
            C[e * D + d] = s;
        }
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int e2 = 0; e2 < E; ++e2) {
            double s = 0.0;
#pragma unroll
            for (int d = 0; d < KT; ++d) s += C[e * D + d] * J[e2 * D + d];
            s += add[e * E + e2];
            cov_f[e * E + e2] = s;
        }
}

// The measurement update of kalman_update_item<D, Y> (Gaussian) on register operands: m_pr, P_pr (D x D), Py (Y x Y),
// Pyx (Y x D), dy = y - y_mean in, m, P out (before the status is applied); returns whether Py is positive definite.
template <int D, int Y>
__device__ __forceinline__ bool ekf_update_reg(const double *m_pr, const double *P_pr, const double *Py, const double *Pyx, const double *dy,
                                               double *m, double *P) {
    double S[Y * (Y + 1) / 2];
#pragma unroll
    for (int i = 0; i < Y; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) S[SSMQ_PK(i, j)] = Py[i * Y + j];
    double G[D][Y];
    const bool ok = gain_from_cov<D, Y>(S, [&](int i, int d) { return Pyx[i * D + d]; }, G);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < Y; ++i) s += G[d][i] * dy[i];
        m[d] = m_pr[d] + s;
    }
    // P = P_pr - (gain P_y) gain'
    sandwich<D, Y>(G, [&](int i, int j) { return Py[i * Y + j]; },
                   [&](int d, int d2, double s) { P[d * D + d2] = P_pr[d * D + d2] - s; });
    return ok;
}

// One trajectory, all steps.  FD / FO: the front ends of the transition and the measurement model.
template <int D, int Y, bool KEEP, class FD, class FO>
__device__ __forceinline__ void ekf_loop_item(const EkfLoopArgs &a, const int64_t b) {
    const int64_t ld = a.ld;
    const cdouble_p gqg = (cdouble_p)a.gqg, rr = (cdouble_p)a.rr;
    const double nan = __builtin_nan("");
    double m[D], P[D * D], yk[Y];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = a.m0[d * ld + b];
#pragma unroll
    for (int i = 0; i < D * D; ++i) P[i] = a.P0[i * ld + b];
#pragma unroll
    for (int i = 0; i < Y; ++i) yk[i] = a.y[i * ld + b];
    int32_t agg = 0;
    for (int k = 0; k < a.T; ++k) {
        // the next step's measurement is asked for before this step's arithmetic (the last step asks for its own again)
        const int kn = k + 1 < a.T ? k + 1 : k;
        double yn[Y];
#pragma unroll
        for (int i = 0; i < Y; ++i) yn[i] = a.y[((int64_t)kn * Y + i) * ld + b];
        // time update
        double o[SSMQ_MAX_DIM], J[D * D], C[D * D], mp[D], Pp[D * D];
        FD::run(a.dyn, m, k, o, J);
        ekf_linearize_reg<D, D, FD::KT>(J, P, gqg, C, Pp);
#pragma unroll
        for (int d = 0; d < D; ++d) mp[d] = o[d];
        if (KEEP) {
#pragma unroll
            for (int d = 0; d < D; ++d) a.pm[((int64_t)k * D + d) * ld + b] = mp[d];
#pragma unroll
            for (int i = 0; i < D * D; ++i) a.pP[((int64_t)k * D * D + i) * ld + b] = Pp[i];
#pragma unroll
            for (int i = 0; i < D * D; ++i) a.pC[((int64_t)k * D * D + i) * ld + b] = C[i];
        }
        // measurement moments
        double oy[SSMQ_MAX_DIM], H[Y * D], Pyx[Y * D], Py[Y * Y], dy[Y];
        FO::run(a.obs, mp, k, oy, H);
        ekf_linearize_reg<D, Y, FO::KT>(H, Pp, rr, Pyx, Py);
#pragma unroll
        for (int i = 0; i < Y; ++i) dy[i] = yk[i] - oy[i];
        // update
        const bool ok = ekf_update_reg<D, Y>(mp, Pp, Py, Pyx, dy, m, P);
        if (agg == 0 && !ok) agg = k + 1;
        const bool good = agg == 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            m[d] = good ? m[d] : nan;
            a.fm[((int64_t)k * D + d) * ld + b] = m[d];
        }
#pragma unroll
        for (int i = 0; i < D * D; ++i) {
            P[i] = good ? P[i] : nan;
            a.fP[((int64_t)k * D * D + i) * ld + b] = P[i];
        }
#pragma unroll
        for (int i = 0; i < Y; ++i) yk[i] = yn[i];
    }
    a.status[b] = agg;
}

// Built-in models: the (D, Y) pairs their Jacobians can form are instantiated in ssmq_filter_ekf.hip.  One wave per workgroup:
// the kernel is a chain of dependent arithmetic per lane, and small batches spread over as many compute units as they have waves.
constexpr int kEkfBlock = 64;
template <int D, int Y, bool KEEP>
__global__ __launch_bounds__(kEkfBlock) void k_ekf_loop(const EkfLoopArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kEkfBlock + threadIdx.x;
    if (b >= a.B) return;
    ekf_loop_item<D, Y, KEEP, EkfFrontBuiltin<D, D>, EkfFrontBuiltin<D, Y>>(a, b);
}

}  // namespace ssmq
