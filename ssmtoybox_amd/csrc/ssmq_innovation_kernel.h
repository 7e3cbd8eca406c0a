// Innovation scores of a filter pass: normalised innovation squared (NIS) e' S^-1 e and the measurement log-likelihood
// log p(y_k | y_1..k-1) of every step of every trajectory, from the FILTERED moments the pass left in HBM.
//
// Step k's predictive measurement moments depend only on (fm[k-1], fP[k-1]) - on (m0, P0) for k = 0 - so the T B items are
// independent: k_innovation<> (ssmq_score_step.h, beside the step it calls) replays both transforms of the step and scores the
// innovation - predict_and_score<>, the first half of the step of the likelihood-scoring kernels - one item per lane, no recursion.
// This header holds its arguments and innovation_score<>, which the step builds on.  The dispatch table, the scoring half on its
// own (k_innovation_score: the launch-loop route) and the per-trajectory totals: ssmq_innovation.hip.
#pragma once
#include "ssmq_filter_fused_kernel.h"

namespace ssmq {

struct InnovArgs {
    const double *y;            // [T][Y][ld]
    const double *m0, *P0;      // [D][ld], [D*D][ld]
    const double *fm, *fP;      // [T][D][ld], [T][D*D][ld]: the filtered moments (lower triangle of fP read)
    double *ymean, *S;          // [T][Y][ld], [T][Y*Y][ld], or null: not stored
    double *nis, *ll;           // [T][ld]
    const double *c_dyn, *c_obs, *gqg, *rr;
    int64_t B, ld;
    int32_t T, emv_dyn, emv_obs, nblk;   // nblk: blocks of 64 trajectories per step
    double nu_dyn, nu_obs;
    FPar fd, fo;
};

// e = y - y_mean; S: in = packed lower triangle of the innovation covariance, out = its Cholesky factor (the operation order of
// chol_packed<>).  nis = |L^-1 e|^2, ll = -(Y log 2 pi + log det S + nis) / 2.  Returns false at a non-positive (or NaN) pivot.
// YT > 0: Y fixed at compile time, everything in registers; YT = 0: Y = y_rt <= SSMQ_MAX_DIM at run time.
// The factor and the forward substitution are chol_packed<> and tri_solve_fwd<> (ssmq_device.h) written out, with log det and nis
// accumulated on the way: as helper calls the kernels came out with other register counts and the run-time-size one 5 % longer.
template <int YT>
__device__ __forceinline__ bool innovation_score(int y_rt, const double *e, double *S, double &nis, double &ll) {
    const int Y = YT ? YT : y_rt;
    constexpr int UN = YT ? YT : 1;   // fixed Y: unrolled in full; run-time Y: loops
    double v[YT ? YT : SSMQ_MAX_DIM];
    bool ok = true;
    double lg = 0.0, q = 0.0;
#pragma unroll UN
    for (int j = 0; j < Y; ++j) {
        double ajj = S[SSMQ_PK(j, j)];
#pragma unroll UN
        for (int k = 0; k < j; ++k) ajj -= S[SSMQ_PK(j, k)] * S[SSMQ_PK(j, k)];
        ok = ok && (ajj > 0.0);
        double r;
        sqrt_rsqrt(ajj, ajj, r);
        S[SSMQ_PK(j, j)] = ajj;
        lg += log(ajj);
#pragma unroll UN
        for (int i = j + 1; i < Y; ++i) {
            double s = S[SSMQ_PK(i, j)];
#pragma unroll UN
            for (int k = 0; k < j; ++k) s -= S[SSMQ_PK(i, k)] * S[SSMQ_PK(j, k)];
            S[SSMQ_PK(i, j)] = s * r;
        }
    }
#pragma unroll UN
    for (int i = 0; i < Y; ++i) {
        double s = e[i];
#pragma unroll UN
        for (int k = 0; k < i; ++k) s -= S[SSMQ_PK(i, k)] * v[k];
        v[i] = div_nr(s, S[SSMQ_PK(i, i)]);
        q += v[i] * v[i];
    }
    nis = q;
    ll = -0.5 * ((double)Y * 1.8378770664093453 /* log(2 pi) */ + 2.0 * lg + q);
    return ok;
}

}  // namespace ssmq
