// RBFGauss.exp_x_kxkx for two parameter rows (bq/bqkern.py:366-415), entry by entry: the one statement of its arithmetic,
// shared by k_rbf_kxkx (ssmq_kernel_methods.hip) and k_weights_mo_pairs (ssmq_weights_mo.hip).
//   Q[i][j] = det(R)^-1/2 exp(xi_i + xi'_j + maha(Lam0^-1 x_i, -Lam1^-1 x_j; R^-1) / 2), R = Lam0^-1 + Lam1^-1 + I,
//   xi = 2 log(alpha0) - |Lam0^-1/2 x_i|^2 / 2, xi' likewise with row 1 (all matrices diagonal)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace ssmq {

// what does not depend on the entry: c = det(R)^-1/2 and the two log-scale terms (scaling = use alpha)
struct RbfKxkxPre {
    double c, la0, la1;
};
__device__ inline RbfKxkxPre rbf_kxkx_pre(int D, const double *par0, const double *par1, int scaling) {
    RbfKxkxPre p;
    p.la0 = scaling ? 2.0 * log(par0[0]) : 2.0 * log(1.0);
    p.la1 = scaling ? 2.0 * log(par1[0]) : 2.0 * log(1.0);
    double det = 1.0;
    for (int d = 0; d < D; ++d) {
        const double s0 = 1.0 / par0[1 + d], s1 = 1.0 / par1[1 + d];
        det *= (s0 * s0 + s1 * s1) + 1.0;
    }
    p.c = 1.0 / sqrt(det);
    return p;
}
// entry (i, j) for the points x [D][N]
__device__ inline double rbf_kxkx_entry(int D, int N, const double *x, const double *par0, const double *par1, const RbfKxkxPre &p,
                                        int i, int j) {
    double n0 = 0.0, n1 = 0.0, m2i = 0.0, m2j = 0.0, mij = 0.0;
    for (int d = 0; d < D; ++d) {
        const double s0 = 1.0 / par0[1 + d], s1 = 1.0 / par1[1 + d];
        const double il0 = s0 * s0, il1 = s1 * s1;
        const double z0 = s0 * x[d * N + i], z1 = s1 * x[d * N + j];
        n0 += z0 * z0;
        n1 += z1 * z1;
        const double v = 1.0 / ((il0 + il1) + 1.0);
        const double yi = il0 * x[d * N + i], yj = -(il1 * x[d * N + j]);
        m2i += (yi * v) * yi;
        m2j += (yj * v) * yj;
        mij += (yi * v) * yj;
    }
    const double mh = (m2i + m2j) - 2.0 * mij;
    return p.c * exp(((p.la0 - 0.5 * n0) + (p.la1 - 0.5 * n1)) + 0.5 * mh);
}

}  // namespace ssmq
