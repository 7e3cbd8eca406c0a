// Interacting multiple-model (IMM) filter over noise modes (Blom & Bar-Shalom 1988): k_imm_loop<> runs M mode-matched filters of ONE
// pair of models and weights - mode j is the filter with the row gqg[j], rr[j], x0[j] of k_noise_sweep<> (ssmq_noise_sweep_kernel.h) -
// on B measurement sequences in ONE launch, couples them every step through the Markov mixing probabilities and weights them by the
// per-step measurement likelihood.  Per trajectory and step k, every sum over modes ascending in the mode index:
//     c_j = sum_i Pi[i][j] mu_i;   w_ij = Pi[i][j] mu_i / c_j   (c_j == 0: w_ij = delta_ij - a mode nobody can reach keeps its moments)
//     m0_j = sum_i w_ij m_i;       P0_j = sum_i w_ij (P_i + (m_i - m0_j)(m_i - m0_j)')
//     mode j's filter step from (m0_j, P0_j): predict_and_score<> -> ll_j, then kalman_update_lower<> (ssmq_score_step.h: the step of
//                                             the row kernels, the one k_noise_sweep<> runs)
//     a_j = log c_j + ll_j (-inf: c_j == 0);  amax = max_j a_j;  loglik[k] = amax + log sum_j exp(a_j - amax);  mu_j = exp(a_j - loglik[k])
//     fm[k] = sum_j mu_j m_j;      fP[k] = sum_j mu_j (P_j + (m_j - fm)(m_j - fm)')   (both triangles from the one value)
//
// Mapping: one workgroup = 64 trajectories x M waves; wave j is mode j, lane l is trajectory blockIdx.x * 64 + l.  What belongs to
// the mode is wave-uniform and read by scalar loads through the constant address space, as in k_noise_sweep<>: gqg + j * gqg_stride,
// rr + j * rr_stride, x0 + j * x0_stride (a stride of 0: shared), column j of Pi.
//
// LDS (dynamic): lds[M][NW][64] doubles, NW = D + D (D + 1) / 2 + 1 - slot j is written by wave j alone: m_j [D] | packed lower
// triangle of P_j | one word, a_j and then mu_j; a lane reads and writes column `lane` only (consecutive lanes 8 bytes apart:
// conflict-free ds_read_b64).  The modes meet once per step: every wave publishes its updated moments and a_j; after the barrier
// every wave reads all a_i and forms loglik[k] (the same bits in every wave); after a second barrier wave j replaces a_j by
// mu_j = exp(a_j - loglik[k]) - ONE exponential per wave - and after a third every wave reads all M slots: it forms the combined
// moments of step k (the same bits in every wave; the output planes are dealt to the waves round robin) and, from the same slots,
// the mixed moments of ITS mode for step k + 1; a fourth barrier ends the reads.  The mixing of step 0 reads the published initial
// moments with mu0_j in the word.
//
// BARRIERS - a workgroup whose waves disagree on a barrier hangs the device, so every wave of a workgroup executes exactly the same
// barriers, 2 + 4 T of them, whatever its data:
//   * the step loop runs T times for every lane: no break, no early return - not for b >= B, not for a failed trajectory;
//   * lanes with b >= B compute on the clamped index B - 1 and have every global store predicated off;
//   * a failed trajectory is carried by a poison flag that travels through LDS: a wave whose mixed moments or scores of step k are not
//     finite numbers publishes a_j = NaN; every wave reads all a_i, so all of them set status = 1 + k at the same step, and from
//     there on the flag turns every store of the trajectory into NaN while the arithmetic goes on on whatever the registers hold
//     (no index and no branch around a barrier depends on it).
// Nothing a trajectory computes depends on the lanes around it.
#pragma once
#include "ssmq_score_step.h"

namespace ssmq {

constexpr int kImmMaxModes = 8;

struct ImmArgs {
    const double *y;                   // [T][Y][ld]
    const double *c_dyn, *c_obs;       // const_layout(D, D, ND, FORM), const_layout(D, Y, NO, FORM): one block each, shared by all modes
    const double *gqg, *rr, *x0;       // mode j at + j * stride: [D*D], [Y*Y], m0 [D] | P0 [D*D]
    int64_t gqg_stride, rr_stride, x0_stride;   // in doubles; 0: shared by all modes
    const double *pi, *mu0;            // [M][M] row-stochastic, [M]
    double *fm, *fP;                   // [T][D][ld], [T][D*D][ld]
    double *mode_prob;                 // [T][M][ld]
    double *ll_steps, *ll_total;       // [T][ld], [ld]
    int32_t *status;                   // [ld]
    int64_t B, ld;
    int32_t T, M;
    int32_t emv_dyn, emv_obs;
    double nu_dyn, nu_obs;             // t-process form: the handles' tp_nu
    FPar fd, fo;                       // fd.ttab / fo.ttab: the time tables [T] of the integrands that have one
};

__host__ __device__ constexpr inline int imm_slot_words(int D) { return D + D * (D + 1) / 2 + 1; }
__host__ __device__ constexpr inline size_t imm_lds_bytes(int D, int M) { return sizeof(double) * (size_t)M * imm_slot_words(D) * kSmallBlock; }

__device__ __forceinline__ bool imm_finite(double v) { return fabs(v) < __builtin_inf(); }

// The mixed moments of mode j from the M published slots (the word of slot i holds mu_i).  Returns whether c_j and every mixed moment
// is a finite number; *cj = c_j.  No barrier inside.
template <int D>
__device__ __forceinline__ bool imm_mix(const double *lds, int M, int lane, int j, cdouble_p pi, double (&m0)[D], double (&P0)[D * (D + 1) / 2],
                                        double *cj) {
    constexpr int PK = D * (D + 1) / 2, NW = imm_slot_words(D);
    auto mu = [&](int i) { return lds[((size_t)i * NW + D + PK) * kSmallBlock + lane]; };
    double c = 0.0;
#pragma unroll 1
    for (int i = 0; i < M; ++i) c += pi[i * M + j] * mu(i);
    const bool reach = c != 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) m0[d] = 0.0;
#pragma unroll
    for (int q = 0; q < PK; ++q) P0[q] = 0.0;
#pragma unroll 1
    for (int i = 0; i < M; ++i) {
        const double w = reach ? div_nr(pi[i * M + j] * mu(i), c) : (i == j ? 1.0 : 0.0);
        const double *s = lds + (size_t)i * NW * kSmallBlock + lane;
#pragma unroll
        for (int d = 0; d < D; ++d) m0[d] += w * s[d * kSmallBlock];
    }
#pragma unroll 1
    for (int i = 0; i < M; ++i) {
        const double w = reach ? div_nr(pi[i * M + j] * mu(i), c) : (i == j ? 1.0 : 0.0);
        const double *s = lds + (size_t)i * NW * kSmallBlock + lane;
        double e[D];
#pragma unroll
        for (int d = 0; d < D; ++d) e[d] = s[d * kSmallBlock] - m0[d];
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) P0[SSMQ_PK(r, q)] += w * (s[(D + SSMQ_PK(r, q)) * kSmallBlock] + e[r] * e[q]);
    }
    bool ok = imm_finite(c);
#pragma unroll
    for (int d = 0; d < D; ++d) ok = ok && imm_finite(m0[d]);
#pragma unroll
    for (int q = 0; q < PK; ++q) ok = ok && imm_finite(P0[q]);
    *cj = c;
    return ok;
}

// Launch bounds: a workgroup is up to kImmMaxModes waves (two per SIMD).
template <int D, int Y, int ND, int NO, int FD, int FO, int SELO, int FORM, int TP>
__global__ __launch_bounds__(kSmallBlock * kImmMaxModes) void k_imm_loop(const ImmArgs a) {
    static_assert(FORM == SSMQ_FORM_BQ || (FORM == SSMQ_FORM_SIGMA && !TP), "k_imm_loop: BQ form, or the sigma-point form without t-process");
    // EVERY WAVE OF THE WORKGROUP EXECUTES EVERY __syncthreads() BELOW, 2 + 4 T OF THEM: no return and no break anywhere in this
    // kernel, out-of-range lanes run on a clamped index with their stores predicated off, failed trajectories run on (see the top
    // of this file).
    extern __shared__ __align__(16) double lds[];
    constexpr int PK = D * (D + 1) / 2, NW = imm_slot_words(D);
    const int lane = threadIdx.x & (kSmallBlock - 1);
    const int j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: the wave's mode (host: blockDim.x = 64 M)
    const int M = a.M;
    const int64_t braw = (int64_t)blockIdx.x * kSmallBlock + lane;
    const bool live = braw < a.B;                                            // stores of the other lanes are predicated off
    const int64_t b = live ? braw : a.B - 1;                                 // (host: B >= 1)
    const int64_t ld = a.ld;
    const double nan = __builtin_nan("");
    const CoreParams cpd{(cdouble_p)a.c_dyn, (cdouble_p)(a.gqg + (int64_t)j * a.gqg_stride), a.emv_dyn, a.nu_dyn, 1.0, 1.0};
    const CoreParams cpo{(cdouble_p)a.c_obs, (cdouble_p)(a.rr + (int64_t)j * a.rr_stride), a.emv_obs, a.nu_obs, 1.0, 1.0};
    const cdouble_p x0 = (cdouble_p)(a.x0 + (int64_t)j * a.x0_stride);
    const cdouble_p pi = (cdouble_p)a.pi, mu0 = (cdouble_p)a.mu0;
    double *const own = lds + (size_t)j * NW * kSmallBlock + lane;           // slot j, this lane's column
    double m[D], Pl[PK];
    load_x0<D>(x0, m, Pl);
    // ---- the initial moments meet: mixing of step 0 with mu = mu0 ------------------------------------------------------------------
#pragma unroll
    for (int d = 0; d < D; ++d) own[d * kSmallBlock] = m[d];
#pragma unroll
    for (int q = 0; q < PK; ++q) own[(D + q) * kSmallBlock] = Pl[q];
    own[(D + PK) * kSmallBlock] = mu0[j];
    __syncthreads();                                                         // barrier 1 of 2 + 4 T
    double cj;
    bool mix_ok = imm_mix<D>(lds, M, lane, j, pi, m, Pl, &cj);
    __syncthreads();                                                         // barrier 2: every slot has been read
    FPar fd = a.fd, fo = a.fo;
    int32_t st = 0;
    double total = 0.0;
#pragma unroll 1
    for (int k = 0; k < a.T; ++k) {
        double yk[Y];
        step_inputs<Y, FD, FO>(a.y, k, ld, b, yk, fd, fo);
        const double t = (double)k;   // both transforms of step k + 1 use time index k (ssinf.py:104, 276-288)
        // ---- mode j's step from the mixed moments: the two halves of ssmq_score_step.h (no break, no return, no barrier in them) ------
        RegSinkNoCross<D, D> pr;
        RegSink<D, Y> ob;
        double S[Y * (Y + 1) / 2], nis, ll;
        bool ok = predict_and_score<D, Y, ND, NO, FD, FO, FORM, TP, SELO, 0>(m, Pl, t, fd, fo, cpd, cpo, yk, pr, ob, S, nis, ll) && mix_ok;
        ok = ok && imm_finite(nis) && imm_finite(ll);
        kalman_update_lower<D, Y, 0>(pr, ob, yk, 1.0, m, Pl);   // the lower triangle: what the mixing reads
        // ---- the modes meet: updated moments and a_j (NaN: the poison flag) ---------------------------------------------------------
        const double aj = !ok ? nan : (cj != 0.0 ? log(cj) + ll : -__builtin_inf());
#pragma unroll
        for (int d = 0; d < D; ++d) own[d * kSmallBlock] = m[d];
#pragma unroll
        for (int q = 0; q < PK; ++q) own[(D + q) * kSmallBlock] = Pl[q];
        own[(D + PK) * kSmallBlock] = aj;
        __syncthreads();                                                     // barrier 3 + 4 k: every slot of step k is written
        const double *const col = lds + lane;
        double amax = -__builtin_inf();
        bool all_ok = true;
#pragma unroll 1
        for (int i = 0; i < M; ++i) {
            const double ai = col[((size_t)i * NW + D + PK) * kSmallBlock];
            all_ok = all_ok && (ai == ai);
            amax = ai > amax ? ai : amax;
        }
        double se = 0.0;
#pragma unroll 1
        for (int i = 0; i < M; ++i) se += exp(col[((size_t)i * NW + D + PK) * kSmallBlock] - amax);
        const double lk = amax + log(se);
        __syncthreads();                                                     // barrier 4 + 4 k: every a_i has been read
        own[(D + PK) * kSmallBlock] = exp(aj - lk);
        __syncthreads();                                                     // barrier 5 + 4 k: every word holds mu_i
        auto mu = [&](int i) { return col[((size_t)i * NW + D + PK) * kSmallBlock]; };
        double cm[D], cP[PK];
#pragma unroll
        for (int d = 0; d < D; ++d) cm[d] = 0.0;
#pragma unroll
        for (int q = 0; q < PK; ++q) cP[q] = 0.0;
#pragma unroll 1
        for (int i = 0; i < M; ++i) {
            const double w = mu(i);
            const double *s = col + (size_t)i * NW * kSmallBlock;
#pragma unroll
            for (int d = 0; d < D; ++d) cm[d] += w * s[d * kSmallBlock];
        }
#pragma unroll 1
        for (int i = 0; i < M; ++i) {
            const double w = mu(i);
            const double *s = col + (size_t)i * NW * kSmallBlock;
            double dm[D];
#pragma unroll
            for (int d = 0; d < D; ++d) dm[d] = s[d * kSmallBlock] - cm[d];
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int q = 0; q <= r; ++q) cP[SSMQ_PK(r, q)] += w * (s[(D + SSMQ_PK(r, q)) * kSmallBlock] + dm[r] * dm[q]);
        }
        bool good = all_ok && imm_finite(lk);
#pragma unroll
        for (int d = 0; d < D; ++d) good = good && imm_finite(cm[d]);
#pragma unroll
        for (int q = 0; q < PK; ++q) good = good && imm_finite(cP[q]);
        if (st == 0 && !good) st = k + 1;                                    // the same word in every wave: all of them read the same slots
        const bool dead = st != 0;
        total += lk;
        // ---- the outputs of step k: the planes dealt to the waves round robin -------------------------------------------------------
        int plane = 0;
        auto mine = [&]() { return live && (plane++ % M) == j; };
        if (mine()) SSMQ_STORE(a.ll_steps[(int64_t)k * ld + b], dead ? nan : lk);
#pragma unroll 1
        for (int i = 0; i < M; ++i) {
            const double v = mu(i);
            if (mine()) SSMQ_STORE(a.mode_prob[((int64_t)k * M + i) * ld + b], dead ? nan : v);
        }
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (mine()) SSMQ_STORE(a.fm[((int64_t)k * D + d) * ld + b], dead ? nan : cm[d]);
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) {
                const double v = dead ? nan : cP[SSMQ_PK(r, q)];             // both triangles from the one value
                if (mine()) SSMQ_STORE(a.fP[((int64_t)k * D * D + r * D + q) * ld + b], v);
                if (q != r && mine()) SSMQ_STORE(a.fP[((int64_t)k * D * D + q * D + r) * ld + b], v);
            }
        // ---- the mixed moments of step k + 1, from the same slots ---------------------------------------------------------------------
        mix_ok = imm_mix<D>(lds, M, lane, j, pi, m, Pl, &cj);
        __syncthreads();                                                     // barrier 6 + 4 k: every slot has been read
    }
    if (live && j == 0) {
        a.ll_total[b] = st != 0 ? nan : total;
        a.status[b] = st;
    }
}

}  // namespace ssmq
