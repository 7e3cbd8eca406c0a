// Iterated posterior linearisation smoother (IPLS; Garcia-Fernandez, Svensson, Sarkka, IEEE TAC 2017) of the additive-noise Gaussian
// filters.  x_{-1} ~ N(m0, P0); step k = 0 .. T-1: x_k = f(x_{k-1}, k) + G q, y_k = h(x_k, k) + r.  One iteration takes linearisation
// moments (ml_j, Pl_j), j = -1 .. T-1 (plane j + 1 of lin_m / lin_P, lower triangle read), and is ONE launch of k_ipls_pass<>:
//   forward, k = 0 .. T-1, (m, P) = this iteration's filtered moments of step k - 1 ((m0, P0) for k = 0):
//     z, S_z, C_f = tf_dyn(ml_{k-1}, Pl_{k-1}, k)     F = C_f Pl_{k-1}^-1     Lambda = S_z - F Pl_{k-1} F'
//     m- = z + F (m - ml_{k-1})      P- = F P F' + Lambda + G Q G'      C_k = P F'   (cov(x_{k-1}, x_k))
//     y^, S_y, C_h = tf_obs(ml_k, Pl_k, k)            the affine update of iplf_update<> with prior (m-, P-) and iterate (ml_k, Pl_k)
//   backward, k = T-1 .. 0, from (ms_{T-1}, Ps_{T-1}) = (m_{T-1}, P_{T-1}):
//     G_k = C_k (P-_k)^-1     ms_{k-1} = m_{k-1} + G_k (ms_k - m-_k)     Ps_{k-1} = P_{k-1} + G_k (Ps_k - P-_k) G_k'
// With L = chol(Pl) and V = C L^-T: F = V L^-1 and F Pl F' = V V' (the algebra of iplf_update<>), so only Pl (by the transform), S and
// P-_k are factored, Lambda and Omega never.  Without linearisation moments (lin_m null: the first iteration) every transform is
// taken at the running moments, where the step is the plain filter step: m- = z, P- = S_z + G Q G', C_k = C_f', S = S_y + R,
// K = C_h' S^-1.  The forward sweep leaves m-_k, P-_k, C_k (workspace) and the filtered moments (fm, fP) in HBM planes and the
// backward sweep of the SAME lane reads them back: a lane reads only what it wrote itself, in program order, through pointers the
// compiler has to assume alias - ordinary single-thread memory semantics, no fence and no second kernel needed (plain stores for
// those planes, streaming stores for the smoothed ones nobody reads in this launch).  Host-free: the run-time compiler
// instantiates k_ipls_pass<> for user models.
#pragma once
#include "ssmq_iterated_kernel.h"

namespace ssmq {

struct IplsArgs {
    const double *y;              // [T][Y][ld]
    const double *m0, *P0;        // [D][ld], [D*D][ld] (lower triangle read)
    const double *lin_m, *lin_P;  // [T+1][D][ld], [T+1][D*D][ld] (lower triangle read; plane 0 = the initial state) or both null
    double *fm, *fP;              // [T][D][ld], [T][D*D][ld]: this iteration's filtered moments
    double *pm, *pP, *pC;         // workspace [T][D][ld], [T][D(D+1)/2][ld], [T][D*D][ld]: m-_k, P-_k (packed lower), C_k
    double *sm0, *sP0, *sm, *sP;  // [D][ld], [D*D][ld], [T][D][ld], [T][D*D][ld]: this iteration's smoothed moments
    double *delta;                // [ld] or null: max_{k,d} |ms_k[d] - ref_k[d]| / sqrt(Ps_k[d][d]), ref = lin_m (the filtered means without)
    int32_t *status;              // [B] in / out: nonzero = failed in an earlier iteration (the lane only writes NaN); 0 or 1 + failing step
    const double *c_dyn, *c_obs, *gqg, *rr;
    int64_t B, ld;
    int32_t T, emv_dyn, emv_obs;
    double nu_dyn, nu_obs;
    FPar fd, fo;
};

// One forward step.  In: (m, Pl) the filtered moments of step k - 1 (Pl packed lower); lin: linearise at (lm0, lL0) for the dynamics
// and (lm1, lL1) for the measurement (packed lower covariances, factored in place), else at the running moments.  Out: the prior
// (mp, Pp packed lower), Ck [D][D] row-major = cov(x_{k-1}, x_k), the filtered moments (mn, Pn packed lower).  False when a
// factorisation fails or the filtered mean is not finite (a NaN measurement fails the step it belongs to, not the next one).
template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO>
__device__ __forceinline__ bool ipls_step(bool lin, const double (&m)[D], const double (&Pl)[D * (D + 1) / 2], double (&lm0)[D],
                                          double (&lL0)[D * (D + 1) / 2], double (&lm1)[D], double (&lL1)[D * (D + 1) / 2], double t,
                                          const FPar &fd, const FPar &fo, const CoreParams &cpd, const CoreParams &cpo,
                                          const double (&yk)[Y], double (&mp)[D], double (&Pp)[D * (D + 1) / 2], double (&Ck)[D * D],
                                          double (&mn)[D], double (&Pn)[D * (D + 1) / 2]) {
    constexpr int DP = D * (D + 1) / 2;
    bool ok;
    if (lin) {
        {
            RegSink<D, D> pr;      // z, S_z + G Q G', C_f [e][d] = cov(f_e, x_d); the core leaves chol(Pl_{k-1}) in lL0
            ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, true, 0, RegSink<D, D>>(lm0, lL0, t, fd, cpd, pr);
            double V[D * D], F[D * D], FP[D * D];
            // V = C_f L^-T (forward substitution per row), F = V L^-1 (backward substitution): the sums of tri_solve_fwd<> /
            // tri_solve_bwd<> (ssmq_device.h), written out - see the list there; below also gain_from_cov<> and sandwich<>
#pragma unroll
            for (int e = 0; e < D; ++e) {
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    double s = pr.cx[e][i];
#pragma unroll
                    for (int q = 0; q < i; ++q) s -= lL0[SSMQ_PK(i, q)] * V[e * D + q];
                    V[e * D + i] = div_nr(s, lL0[SSMQ_PK(i, i)]);
                }
#pragma unroll
                for (int i = D - 1; i >= 0; --i) {
                    double s = V[e * D + i];
#pragma unroll
                    for (int q = i + 1; q < D; ++q) s -= lL0[SSMQ_PK(q, i)] * F[e * D + q];
                    F[e * D + i] = div_nr(s, lL0[SSMQ_PK(i, i)]);
                }
            }
            // m- = z + F (m - ml);  FP = F P, C_k = P F' = (F P)'
#pragma unroll
            for (int e = 0; e < D; ++e) {
                double s = pr.mf[e];
#pragma unroll
                for (int d = 0; d < D; ++d) s += F[e * D + d] * (m[d] - lm0[d]);
                mp[e] = s;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    double u = 0.0;
#pragma unroll
                    for (int q = 0; q < D; ++q) u += F[e * D + q] * Pl[q >= d ? SSMQ_PK(q, d) : SSMQ_PK(d, q)];
                    FP[e * D + d] = u;
                    Ck[d * D + e] = u;
                }
            }
            // P- = (S_z + G Q G') + (F P F' - V V'): the bracket is F (P - Pl) F'
#pragma unroll
            for (int e = 0; e < D; ++e)
#pragma unroll
                for (int e2 = 0; e2 <= e; ++e2) {
                    double fpf = 0.0, vv = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        fpf += FP[e * D + d] * F[e2 * D + d];
                        vv += V[e * D + d] * V[e2 * D + d];
                    }
                    Pp[SSMQ_PK(e, e2)] = pr.cv[SSMQ_PK(e, e2)] + (fpf - vv);
                }
        }
        RegSink<D, Y> ob;      // y^, S_y + R, C_h at the linearisation moments of step k; chol(Pl_k) stays in lL1
        ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, 0, RegSink<D, Y>>(lm1, lL1, t, fo, cpo, ob) && ok;
        ok = iplf_update<D, Y>(D, Y, mp, Pp, lm1, lL1, ob.mf, ob.cv, &ob.cx[0][0], yk, mn, Pn) && ok;
    } else {
        {
            double L[DP];
#pragma unroll
            for (int i = 0; i < DP; ++i) L[i] = Pl[i];
            RegSink<D, D> pr;
            ok = moment_transform_core<D, D, ND, FD, FORM, TP, 0, true, 0, RegSink<D, D>>(m, L, t, fd, cpd, pr);
#pragma unroll
            for (int e = 0; e < D; ++e) {
                mp[e] = pr.mf[e];
#pragma unroll
                for (int d = 0; d < D; ++d) Ck[d * D + e] = pr.cx[e][d];
            }
#pragma unroll
            for (int i = 0; i < DP; ++i) Pp[i] = pr.cv[i];
        }
        double L2[DP];
#pragma unroll
        for (int i = 0; i < DP; ++i) L2[i] = Pp[i];
        RegSink<D, Y> ob;
        ok = moment_transform_core<D, Y, NO, FO, FORM, TP, SELO, true, 0, RegSink<D, Y>>(mp, L2, t, fo, cpo, ob) && ok;
        // the plain update: K = C_h' S^-1, m = m- + K (y - y^), P = P- - (K S) K'
        double S[Y * (Y + 1) / 2], K[D * Y];
#pragma unroll
        for (int i = 0; i < Y * (Y + 1) / 2; ++i) S[i] = ob.cv[i];
        if (Y == 1) {   // scalar measurement: one division, as the fused time loop
            ok = (S[0] > 0.0) && ok;
#pragma unroll
            for (int d = 0; d < D; ++d) K[d] = div_nr(ob.cx[0][d], S[0]);
        } else {
            ok = chol_packed<Y>(Y, S) && ok;
#pragma unroll
            for (int d = 0; d < D; ++d) {
#pragma unroll
                for (int i = 0; i < Y; ++i) {
                    double s = ob.cx[i][d];
#pragma unroll
                    for (int q = 0; q < i; ++q) s -= S[SSMQ_PK(i, q)] * K[d * Y + q];
                    K[d * Y + i] = div_nr(s, S[SSMQ_PK(i, i)]);
                }
#pragma unroll
                for (int i = Y - 1; i >= 0; --i) {
                    double s = K[d * Y + i];
#pragma unroll
                    for (int q = i + 1; q < Y; ++q) s -= S[SSMQ_PK(q, i)] * K[d * Y + q];
                    K[d * Y + i] = div_nr(s, S[SSMQ_PK(i, i)]);
                }
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double s = 0.0, w[Y];
#pragma unroll
            for (int i = 0; i < Y; ++i) s += K[d * Y + i] * (yk[i] - ob.mf[i]);
            mn[d] = mp[d] + s;
#pragma unroll
            for (int j = 0; j < Y; ++j) {
                double u = 0.0;
#pragma unroll
                for (int i = 0; i < Y; ++i) u += K[d * Y + i] * ob.cv[i >= j ? SSMQ_PK(i, j) : SSMQ_PK(j, i)];
                w[j] = u;
            }
#pragma unroll
            for (int d2 = 0; d2 <= d; ++d2) {
                double u = 0.0;
#pragma unroll
                for (int j = 0; j < Y; ++j) u += w[j] * K[d2 * Y + j];
                Pn[SSMQ_PK(d, d2)] = Pp[SSMQ_PK(d, d2)] - u;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) ok = ok && (mn[d] - mn[d] == 0.0);
    return ok;
}

// One backward step.  mf, Pf: the filtered moments of step k - 1; mp, Pp: the prior of step k (Pp is factored in place); Ck [D][D];
// ms, Ps: the smoothed moments of step k.  Out: mo, Po, the smoothed moments of step k - 1.  Covariances packed lower.  False when
// P-_k is not positive definite.
template <int D>
__device__ __forceinline__ bool ipls_back(const double (&mf)[D], const double (&Pf)[D * (D + 1) / 2], const double (&mp)[D],
                                          double (&Pp)[D * (D + 1) / 2], const double (&Ck)[D * D], const double (&ms)[D],
                                          const double (&Ps)[D * (D + 1) / 2], double (&mo)[D], double (&Po)[D * (D + 1) / 2]) {
    constexpr int DP = D * (D + 1) / 2;
    double dP[DP], G[D * D];
#pragma unroll
    for (int i = 0; i < DP; ++i) dP[i] = Ps[i] - Pp[i];
    const bool ok = chol_packed<D>(D, Pp);
    // G = C_k (P-)^-1: per row the sums of cho_solve_row<> (ssmq_device.h), written out: see the list there
#pragma unroll
    for (int d = 0; d < D; ++d) {
        double v[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double s = Ck[d * D + i];
#pragma unroll
            for (int q = 0; q < i; ++q) s -= Pp[SSMQ_PK(i, q)] * v[q];
            v[i] = div_nr(s, Pp[SSMQ_PK(i, i)]);
        }
#pragma unroll
        for (int i = D - 1; i >= 0; --i) {
            double s = v[i];
#pragma unroll
            for (int q = i + 1; q < D; ++q) s -= Pp[SSMQ_PK(q, i)] * G[d * D + q];
            G[d * D + i] = div_nr(s, Pp[SSMQ_PK(i, i)]);
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        double s = 0.0, w[D];
#pragma unroll
        for (int e = 0; e < D; ++e) s += G[d * D + e] * (ms[e] - mp[e]);
        mo[d] = mf[d] + s;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double u = 0.0;
#pragma unroll
            for (int e = 0; e < D; ++e) u += G[d * D + e] * dP[e >= j ? SSMQ_PK(e, j) : SSMQ_PK(j, e)];
            w[j] = u;
        }
#pragma unroll
        for (int d2 = 0; d2 <= d; ++d2) {
            double u = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) u += w[j] * G[d2 * D + j];
            Po[SSMQ_PK(d, d2)] = Pf[SSMQ_PK(d, d2)] + u;
        }
    }
    return ok;
}

// One iteration: the forward sweep, then the backward sweep, one trajectory per lane, grid of ceil(B / 64) blocks.  Launch bounds:
// those of k_iplf_loop<> of the same shape.  A lane that fails - or failed in an earlier iteration - writes NaN to every output.
template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO>
__global__ SSMQ_PASS_LAUNCH_BOUNDS(D, FORM) void k_ipls_pass(const IplsArgs a) {
    const uint32_t b = blockIdx.x * kSmallBlock + threadIdx.x;
    if ((int64_t)b >= a.B) return;
    const int64_t ld = a.ld;
    constexpr int DP = D * (D + 1) / 2;
    const bool lin = a.lin_m != nullptr;
    const CoreParams cpd{(cdouble_p)a.c_dyn, (cdouble_p)a.gqg, a.emv_dyn, a.nu_dyn, 1.0, 1.0};
    const CoreParams cpo{(cdouble_p)a.c_obs, (cdouble_p)a.rr, a.emv_obs, a.nu_obs, 1.0, 1.0};
    FPar fd = a.fd, fo = a.fo;
    int32_t agg = a.status[b];
    const bool skip = agg != 0;      // failed in an earlier iteration: the status stays, the outputs of this one are NaN
    double m[D], Pl[DP];
    if (!skip) {
#pragma unroll
        for (int d = 0; d < D; ++d) m[d] = a.m0[d * ld + b];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) Pl[SSMQ_PK(i, j)] = a.P0[(i * D + j) * ld + b];
        // ---- forward ---------------------------------------------------------------------------------------------------------
#pragma unroll 1
        for (int k = 0; k < a.T; ++k) {
            const double t = (double)k;   // both transforms of step k use time index k, in every iteration
            if constexpr (HasTimeTable<FD>::value) { fd.tval = ((cdouble_p)a.fd.ttab)[k]; fd.use_tval = 1; }   // host: non-null
            if constexpr (HasTimeTable<FO>::value) { fo.tval = ((cdouble_p)a.fo.ttab)[k]; fo.use_tval = 1; }
            double yk[Y], lm0[D], lL0[DP], lm1[D], lL1[DP];
#pragma unroll
            for (int i = 0; i < Y; ++i) yk[i] = a.y[((int64_t)k * Y + i) * ld + b];
            if (lin) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    lm0[d] = a.lin_m[((int64_t)k * D + d) * ld + b];
                    lm1[d] = a.lin_m[((int64_t)(k + 1) * D + d) * ld + b];
#pragma unroll
                    for (int j = 0; j <= d; ++j) {
                        lL0[SSMQ_PK(d, j)] = a.lin_P[((int64_t)k * D * D + d * D + j) * ld + b];
                        lL1[SSMQ_PK(d, j)] = a.lin_P[((int64_t)(k + 1) * D * D + d * D + j) * ld + b];
                    }
                }
            }
            double mp[D], Pp[DP], Ck[D * D], mn[D], Pn[DP];
            const bool ok = ipls_step<D, Y, ND, NO, FD, FO, FORM, TP, SELO>(lin, m, Pl, lm0, lL0, lm1, lL1, t, fd, fo, cpd, cpo, yk, mp, Pp,
                                                                            Ck, mn, Pn);
            if (!ok) {
                agg = k + 1;
                break;
            }
            // (plain stores: the backward sweep of this lane reads these planes back)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                m[d] = mn[d];
                a.fm[((int64_t)k * D + d) * ld + b] = mn[d];
                a.pm[((int64_t)k * D + d) * ld + b] = mp[d];
            }
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    const double p = Pn[SSMQ_PK(i, j)];   // both triangles from the one value
                    Pl[SSMQ_PK(i, j)] = p;
                    a.fP[((int64_t)k * D * D + i * D + j) * ld + b] = p;
                    if (j != i) a.fP[((int64_t)k * D * D + j * D + i) * ld + b] = p;
                    a.pP[((int64_t)k * DP + SSMQ_PK(i, j)) * ld + b] = Pp[SSMQ_PK(i, j)];
                }
#pragma unroll
            for (int i = 0; i < D * D; ++i) a.pC[((int64_t)k * D * D + i) * ld + b] = Ck[i];
        }
    }
    // ---- backward: (m, Pl) = the filtered moments of step T - 1 = the smoothed ones, the same bits ----------------------------------
    double worst = 0.0;
    if (agg == 0) {
#pragma unroll 1
        for (int k = a.T - 1; k >= -1; --k) {
            // (m, Pl) = (ms_k, Ps_k): out, and into delta
            double *om = k >= 0 ? a.sm + (int64_t)k * D * ld : a.sm0, *oP = k >= 0 ? a.sP + (int64_t)k * D * D * ld : a.sP0;
            const double *rf = lin ? a.lin_m + (int64_t)(k + 1) * D * ld : (k >= 0 ? a.fm + (int64_t)k * D * ld : a.m0);
            double ref[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                ref[d] = rf[d * ld + b];
                SSMQ_STORE(om[d * ld + b], m[d]);
            }
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    SSMQ_STORE(oP[(i * D + j) * ld + b], Pl[SSMQ_PK(i, j)]);
                    if (j != i) SSMQ_STORE(oP[(j * D + i) * ld + b], Pl[SSMQ_PK(i, j)]);
                }
            const double dl = iplf_delta<D>(D, m, ref, Pl);
            worst = (dl <= worst) ? worst : dl;
            if (k < 0) break;
            double mf[D], Pf[DP], mp[D], Pp[DP], Ck[D * D], mo[D], Po[DP];
            const double *fmk = k > 0 ? a.fm + (int64_t)(k - 1) * D * ld : a.m0, *fPk = k > 0 ? a.fP + (int64_t)(k - 1) * D * D * ld : a.P0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                mf[d] = fmk[d * ld + b];
                mp[d] = a.pm[((int64_t)k * D + d) * ld + b];
#pragma unroll
                for (int j = 0; j <= d; ++j) {
                    Pf[SSMQ_PK(d, j)] = fPk[(d * D + j) * ld + b];
                    Pp[SSMQ_PK(d, j)] = a.pP[((int64_t)k * DP + SSMQ_PK(d, j)) * ld + b];
                }
            }
#pragma unroll
            for (int i = 0; i < D * D; ++i) Ck[i] = a.pC[((int64_t)k * D * D + i) * ld + b];
            if (!ipls_back<D>(mf, Pf, mp, Pp, Ck, m, Pl, mo, Po)) {
                agg = k + 1;
                break;
            }
#pragma unroll
            for (int d = 0; d < D; ++d) m[d] = mo[d];
#pragma unroll
            for (int i = 0; i < DP; ++i) Pl[i] = Po[i];
        }
    }
    if (agg == 0) {
        if (a.delta) SSMQ_STORE(a.delta[b], worst);
        if (!skip) a.status[b] = 0;
        return;
    }
    // ---- a failed trajectory: every output of this iteration is NaN -------------------------------------------------------------------
    const double nan = __builtin_nan("");
#pragma unroll 1
    for (int64_t i = 0; i < (int64_t)a.T * D; ++i) {
        a.fm[i * ld + b] = nan;
        a.sm[i * ld + b] = nan;
    }
#pragma unroll 1
    for (int64_t i = 0; i < (int64_t)a.T * D * D; ++i) {
        a.fP[i * ld + b] = nan;
        a.sP[i * ld + b] = nan;
    }
#pragma unroll 1
    for (int i = 0; i < D; ++i) a.sm0[i * ld + b] = nan;
#pragma unroll 1
    for (int i = 0; i < D * D; ++i) a.sP0[i * ld + b] = nan;
    if (a.delta) a.delta[b] = nan;
    a.status[b] = agg;
}

}  // namespace ssmq
