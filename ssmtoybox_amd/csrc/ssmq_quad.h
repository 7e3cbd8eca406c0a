// One trajectory on the four lanes of a quad (16 trajectories per wave): what the quad time-loop kernels share.
//   ssmq_filter_quad.hip       heavy sigma-point shapes: points dealt to the lanes, partial sums all-reduced (other summation order)
//   ssmq_filter_ungm_quad.hip  scalar BQ shapes: only the dynamics integrand is dealt, its values are broadcast and every lane
//                              carries on with the replicated sums of the one-lane kernel (same operations, same order, same bits)
#pragma once
#include "ssmq_apply_small.h"

namespace ssmq {

constexpr int kQuadTraj = 16;     // trajectories per wave

// v of another lane of the quad: CTRL = the DPP quad_perm control, lane i reads lane (CTRL >> 2 i) & 3.  Two 32-bit moves per
// double (`v_mov_b32_dpp quad_perm`, the only DPP form that moves fp64 data between the lanes of a quad).
template <int CTRL>
__device__ __forceinline__ double quad_perm(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// lane q's v in all four lanes: quad_perm:[q,q,q,q]
__device__ __forceinline__ double quad_bcast(int q, double v) {
    switch (q) {
        case 0: return quad_perm<0x00>(v);
        case 1: return quad_perm<0x55>(v);
        case 2: return quad_perm<0xAA>(v);
        default: return quad_perm<0xFF>(v);
    }
}

// The N points of a scalar transform (D = 1, moment_transform_core<>'s Points) dealt to the lanes of a quad that carries one
// replicated trajectory: lane q evaluates the integrand at the points 4 s + q alone, every f(x_n) is broadcast to the quad, and each
// lane forms the transform's sums from the same N values in the same order as a lane that evaluated them all.
template <int N>
struct QuadScalarPoints {
    static constexpr bool kDealt = true;
    static constexpr bool kCentre = false;
    static constexpr int S = (N + 3) / 4;
    double xi[S];       // this lane's unit points; where 4 s + q >= N the first point (evaluated like the others, never read)
    // once, before a time loop.  xi_all: the transform's N unit points (const_layout: xi), q: the lane's place in its quad
    __device__ __forceinline__ void init(cdouble_p xi_all, int q) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            double v = xi_all[0];
#pragma unroll
            for (int j = 1; j < 4; ++j)
                if (4 * s + j < N) v = (q == j) ? xi_all[4 * s + j] : v;
            if (s > 0) v = (q == 0) ? xi_all[4 * s] : v;
            xi[s] = v;
            pin_v(xi[s]);
        }
    }
    template <class Fun>
    __device__ __forceinline__ void values(const Fun &fn, const double (&m)[1], const double (&L)[1], double (&fx)[1][N]) const {
        static_assert(Fun::DIN == 1, "QuadScalarPoints: scalar integrands");
        double fq[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            // an explicit fma: the instruction the one-lane kernel's m + L xi contracts to, whatever the contraction setting
            const double x[1] = {fma(xi[s], L[0], m[0])};
            double o[1];
            fn.template eval<1>(x, o);
            fq[s] = o[0];
        }
#pragma unroll
        for (int n = 0; n < N; ++n) fx[0][n] = quad_bcast(n & 3, fq[n >> 2]);
    }
};

}  // namespace ssmq
