// The per-trajectory state machine of the batched marginalised GP-quadrature filter (ssmq_gp_marginal_filter_batch), written once
// for its three routes: the host rounds (ssmq_marginal.hip), the device rounds and the one-launch kernel
// (ssmq_marginal_device.hip).  A trajectory walks ssinf.py:66-118 / 1083-1273 by itself: Laplace step by BFGS (ssmq_bfgs.h), Laplace
// posterior and its sigma points, mixture over the parameter points, next time step.  A route decides where the points a
// trajectory waits for are evaluated and where their results lie (the Res accessors); everything between is here.
// exp / log / isfinite are the device library's on the device and glibc's on the host, as in ssmq_bfgs.h: the two differ in last
// bits (tests/test_gpu_parity.py::test_marginal_filter_device_rounds_match_host_rounds) and no common approximation stands in.
#pragma once
#include "ssmq_host.h"
#include "ssmq_bfgs.h"
#include <cstring>

// Unnamed namespace, as the code had in its one unit: MgArgs is part of the kernels' signatures and so of their names.
namespace {

using namespace ssmq_bfgs;

// why a trajectory left the batch (failed[b] = step + 65536 reason; include/ssmq.h)
enum { WHY_PRIOR_NOT_PD = 1, WHY_LAPLACE_NOT_FINITE = 2, WHY_LAPLACE_NOT_PD = 3, WHY_MIXTURE_ITEM = 4, WHY_MIXTURE_NOT_FINITE = 5 };
SSMQ_BFGS_HD inline int32_t why(int k, int reason) { return k < 65536 ? k + 65536 * reason : k; }

template <int PM>
struct TrajD {
    int k, mode;                     // time step being worked on (1 .. T); 0: optimising, 1: waiting for the mixture points, 2: done / failed
    RunT<PM> run;
    double xm[SSMQ_MAX_DIM], xP[SSMQ_MAX_DIM * SSMQ_MAX_DIM];          // filtered state moments
    double pm[PM], pc[PM * PM], Lp[PM * PM], logdet2;                  // parameter prior of this step, its factor
    double pts[PM * 2 * PM];         // [NP][P] marginalisation points of this step
};

// One call's shapes, inputs and outputs as the state machine reads them, and - device routes only, null / unused in the host
// rounds - what the kernels share beyond that.  The pointers are device pointers in the device routes, host pointers in the host rounds.
struct MgArgs {
    void *traj;
    int64_t B;
    int32_t T, P, Pd, Po, NP, D, Din, Y, dq;
    const double *y;                 // [B][T][Y]
    const double *x0_mean, *x0_cov, *prior_mean, *prior_cov, *q_mean, *q_cov, *upts, *uwts;
    double fd_step, param_jitter;
    int32_t *first;                  // [B] item offset of every trajectory in this round
    signed char *modes;              // [B] TrajD::mode of every trajectory, compact (what the scan reads)
    int32_t *count;                  // [0] items of this round, [1] unfinished trajectories, [2] rounds that had items, [3] scans done
    volatile int32_t *hflag;         // pinned host memory the device writes after every scan: [0] unfinished trajectories, [1] scans done
    unsigned long long *totals;      // [0] items, [1] BFGS iterations
    ssmq::ThetaDev th;
    double *fm, *fP;                 // [B][T][D], [B][T][D D], NaN where nothing was produced
    int32_t *failed;                 // [B]
};

// the shapes and scalars of a call; the pointers are the route's to set
inline MgArgs mg_args(const ssmq::MarginalCall &c) {
    MgArgs a;
    memset(&a, 0, sizeof(a));
    a.B = c.B; a.T = c.T; a.NP = c.NP; a.Din = c.h_dyn->D; a.D = c.h_dyn->E; a.Y = c.h_obs->E; a.dq = a.Din - a.D;
    a.Pd = a.Din + 1; a.Po = c.h_obs->D + 1; a.P = a.Pd + a.Po;
    a.fd_step = c.fd_step; a.param_jitter = c.param_jitter;
    return a;
}

// points a trajectory in `mode` waits for: the objective at xt and at its P forward-difference neighbours, or the NP mixture points
SSMQ_BFGS_HD inline int mg_items(int mode, int P, int NP) { return mode == 0 ? P + 1 : (mode == 1 ? NP : 0); }

// log N(theta | pm, C) = -(v'v + 2 sum log diag L + P log 2 pi) / 2, v = L^-1 (theta - pm), C = L L'   (ssinf.py:1200-1218)
template <int PM>
SSMQ_BFGS_HD inline __attribute__((always_inline)) double mg_log_prior(const double *pm, const double *Lp, double logdet2, int P,
                                                                      const double *theta) {
    double v[PM], q = 0.0;
    for (int i = 0; i < P; ++i) {
        double s = theta[i] - pm[i];
        for (int k = 0; k < i; ++k) s -= Lp[i * P + k] * v[k];
        v[i] = s / Lp[i * P + i];
        q += v[i] * v[i];
    }
    return -0.5 * (q + logdet2 + P * log(2.0 * M_PI));
}

// the Laplace step of time step t.k starts from the prior (t.pm, t.pc)
template <int PM>
SSMQ_BFGS_HD inline void mg_begin_step(TrajD<PM> &t, const MgArgs &a, int64_t b) {
    if (!chol_lower(t.pc, a.P, t.Lp, &t.logdet2)) {     // numpy.linalg.cholesky would raise in _param_log_prior
        t.mode = 2;
        a.failed[b] = why(t.k, WHY_PRIOR_NOT_PD);
        return;
    }
    bfgs_start(t.run, a.P, t.pm);
    t.mode = 0;
}

// a trajectory before its first step: x0, the parameter prior, not failed   (PX, DX: P and D at compile time, or 0 = a.P, a.D)
template <int PX = 0, int DX = 0, int PM>
SSMQ_BFGS_HD inline void mg_init(TrajD<PM> &t, const MgArgs &a, int64_t b) {
    const int P = PX ? PX : a.P, D = DX ? DX : a.D;
    t.k = 1;
    for (int i = 0; i < D; ++i) t.xm[i] = a.x0_mean[i];
    for (int i = 0; i < D * D; ++i) t.xP[i] = a.x0_cov[i];
    for (int i = 0; i < P; ++i) t.pm[i] = a.prior_mean[i];
    for (int i = 0; i < P * P; ++i) t.pc[i] = a.prior_cov[i];
    a.failed[b] = 0;
    mg_begin_step(t, a, b);
}

// coordinate i of the j-th point the trajectory waits for: xt + fd_step e_(j - 1) while it optimises, else the j-th mixture point
// (PX: the parameter count at compile time, or 0 = a.P)
template <int PX = 0, int PM>
SSMQ_BFGS_HD inline __attribute__((always_inline)) double mg_point(const TrajD<PM> &t, const MgArgs &a, int j, int i) {
    const int P = PX ? PX : a.P;
    return t.mode == 0 ? t.run.xt[i] + ((j == i + 1) ? a.fd_step : 0.0) : t.pts[(size_t)j * P + i];
}

// m [Din] = [mean; q_mean], c [Din][pitch] = blockdiag(cov, Q) for dynamics that take their noise as an argument (ssinf.py:1174-1176)
template <int PM>
SSMQ_BFGS_HD inline void mg_moments(const TrajD<PM> &t, const MgArgs &a, double *m, double *c, int pitch) {
    const int D = a.D, Din = a.Din, dq = a.dq;
    for (int i = 0; i < Din * pitch; ++i) c[i] = 0.0;
    for (int i = 0; i < D; ++i) {
        m[i] = t.xm[i];
        for (int k = 0; k < D; ++k) c[i * pitch + k] = t.xP[i * D + k];
    }
    for (int i = 0; i < dq; ++i) {
        m[D + i] = a.q_mean[i];
        for (int k = 0; k < dq; ++k) c[(D + i) * pitch + D + k] = a.q_cov[i * dq + k];
    }
}

// The trajectory takes the results of the points it waited for (res: ll(j), st(j), m(i, j), P(i, j) of its j-th point) and moves
// on: an optimiser step; with the run finished the Laplace posterior and its sigma points; or the mixture and the next time step.
// Returns the BFGS iteration count of a run that finished in this call, 0 otherwise.
// PX: the parameter count at compile time (= PM), or 0 = a.P at run time.  With PX every loop of the optimiser has a constant trip
// count: unrolled, its small arrays in registers - at run-time bounds they are indexed private memory and the device kernel took
// 40 us per round for 1 024 trajectories (a wave walks the union of its lanes' branches, a few thousand dependent instructions).
template <int PM, int PX, class Res, bool IN_PLACE = false>
SSMQ_BFGS_HD inline __attribute__((always_inline)) int mg_advance_one(TrajD<PM> &t, const MgArgs &a, int64_t b, const Res &res) {
    const int P = PX ? PX : a.P, D = a.D, NP = a.NP, T = a.T;
    const double inf = __builtin_huge_val();
    if (t.mode == 0) {
        // On the device the optimiser works on a LOCAL copy of its state (private memory: lane-interleaved and cached) and writes
        // it back once: on the 3 KB-strided structs themselves every one of its few hundred dependent accesses was a cache miss
        // of its own (38 us per round for 1 024 trajectories).
        // (IN_PLACE: the state is in LDS - k_mg_persistent - or in host memory, and the optimiser works on it where it is)
        RunT<PM> run_copy;
        if constexpr (!IN_PLACE) run_copy = t.run;
        RunT<PM> &run = IN_PLACE ? t.run : run_copy;
        double vals[PM + 1];
        for (int j = 0; j <= P; ++j) {
            // log N(theta | prior) at the row as it was evaluated
            double th[PM];
            for (int i = 0; i < P; ++i) th[i] = run.xt[i] + ((j == i + 1) ? a.fd_step : 0.0);
            const double val = -res.ll(j) - mg_log_prior<PM>(t.pm, t.Lp, t.logdet2, P, th);
            vals[j] = __builtin_isfinite(val) ? val : inf;
        }
        bfgs_advance(run, P, a.fd_step, vals);
        if constexpr (!IN_PLACE) t.run = run;
        if (run.phase != PH_DONE) return 0;
        // Laplace posterior (ssinf.py:1272-1273) and its sigma points (:1103-1106)
        double pcn[PM * PM], L[PM * PM];
        bool fin = true;
        for (int i = 0; i < P; ++i) {
            t.pm[i] = run.x[i];
            fin = fin && __builtin_isfinite(t.pm[i]);
            for (int k = 0; k < P; ++k) {
                pcn[i * P + k] = run.H[i * P + k] + (i == k ? a.param_jitter : 0.0);
                fin = fin && __builtin_isfinite(pcn[i * P + k]);
            }
        }
        if (!fin || !chol_lower(pcn, P, L, nullptr)) {
            t.mode = 2;
            a.failed[b] = why(t.k, fin ? WHY_LAPLACE_NOT_PD : WHY_LAPLACE_NOT_FINITE);
            return run.k;
        }
        for (int i = 0; i < P * P; ++i) t.pc[i] = pcn[i];
        for (int j = 0; j < NP; ++j)
            for (int i = 0; i < P; ++i) {
                double s = t.pm[i];
                for (int k = 0; k <= i; ++k) s += L[i * P + k] * a.upts[(size_t)k * NP + j];
                t.pts[(size_t)j * P + i] = s;
            }
        t.mode = 1;
        return run.k;
    }
    // mixture over the parameter points (ssinf.py:1108-1115): plain weighted sums of the conditional moments
    bool ok = true;
    for (int j = 0; j < NP; ++j) ok = ok && res.st(j) == 0;
    const bool items_ok = ok;
    double xm[SSMQ_MAX_DIM], xP[SSMQ_MAX_DIM * SSMQ_MAX_DIM];
    for (int i = 0; i < D; ++i) xm[i] = 0.0;
    for (int i = 0; i < D * D; ++i) xP[i] = 0.0;
    for (int j = 0; j < NP; ++j) {
        const double w = a.uwts[j];
        for (int i = 0; i < D; ++i) xm[i] += res.m(i, j) * w;
        for (int i = 0; i < D * D; ++i) xP[i] += res.P(i, j) * w;
    }
    for (int i = 0; i < D; ++i) ok = ok && __builtin_isfinite(xm[i]);
    for (int i = 0; i < D * D; ++i) ok = ok && __builtin_isfinite(xP[i]);
    if (!ok) {                               // where forward_pass raises LinAlgError for this trajectory
        t.mode = 2;
        a.failed[b] = why(t.k, items_ok ? WHY_MIXTURE_NOT_FINITE : WHY_MIXTURE_ITEM);
        return 0;
    }
    for (int i = 0; i < D; ++i) {
        t.xm[i] = xm[i];
        a.fm[((size_t)b * T + (t.k - 1)) * D + i] = xm[i];
    }
    for (int i = 0; i < D * D; ++i) {
        t.xP[i] = xP[i];
        a.fP[((size_t)b * T + (t.k - 1)) * D * D + i] = xP[i];
    }
    if (t.k == T) {
        t.mode = 2;
    } else {
        ++t.k;
        mg_begin_step(t, a, b);
    }
    return 0;
}

}  // namespace
