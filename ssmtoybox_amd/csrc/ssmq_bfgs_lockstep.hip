// Batched Laplace step of the marginalised GP-quadrature filter: B independent BFGS runs in lock step.  Host code only: the
// drivers of the optimiser in ssmq_bfgs.h on a host objective (pinned against SciPy on the CPU, tests/test_bfgs_lockstep.py) and
// on the theta-conditioned filter step.
//
// Reference: MarginalInference._param_posterior_moments (ssinf.py:1243-1273) runs scipy.optimize.minimize(method='BFGS')
// on the negative log posterior of the kernel parameters, ONE trajectory at a time, once per time step; its callers loop
// over Monte-Carlo trajectories in Python (research/tpq/tpq_base.py:175-192).  The objective of trajectory b at theta is
//   - log N(y_b | moments of the theta-conditioned filter step)  -  log N(theta | prior mean_b, prior cov_b)
// (ssinf.py:1153-1241) and costs one theta step on the device (ssmq_gp_theta_step); a forward-difference gradient costs
// param_dim more.  Here every trajectory keeps its own optimiser state and each ROUND sends the points all unfinished
// trajectories are waiting for - (param_dim + 1) per trajectory - to the device in ONE ssmq_gp_theta_step call.
//
// The optimiser is a restatement of what SciPy 1.15.3 (the pinned version of this image; not part of the reference tree) runs
// for method='BFGS' with jac=True and default options: _minimize_bfgs (gtol 1e-5 on the max-norm, maxiter 200 n, initial
// inverse Hessian I, "old_old_fval = f0 + |g0| / 2"), line_search_wolfe1 -> scalar_search_wolfe1 (c1 1e-4, c2 0.9, amin 1e-100,
// amax 1e100, xtol 1e-14, at most 100 trial steps) -> MINPACK-2's DCSRCH / DCSTEP (More' & Thuente; SciPy's _dcsrch.py), written
// as a per-trajectory state machine because the function values arrive a round later.  Where SciPy falls back to its second
// line search (line_search_wolfe2: DCSRCH ended in an ERROR or WARNING task, or refused to start) the state machine goes on
// with scalar_search_wolfe2 / _zoom as well (PH_LINE2 below); the status SSMQ_BFGS_FALLBACK of round 3's first version
// ("the caller finishes this trajectory with SciPy") is no longer produced.
// Two deliberate differences from the reference's serial path, both where its objective RAISES: an objective point whose
// kernel matrix / covariance is not positive definite (or whose value is not finite) counts as +inf here and the search goes
// on - numpy.linalg.LinAlgError propagates out of scipy.optimize.minimize in the reference and ends that trajectory's
// forward_pass (ssinf.py:1088-1122); the batch instead reports it through `failed` only if the Laplace covariance or a
// marginalisation point then fails.  And NaN is tested before maxiter (SciPy: warnflag 1 before 3).
#include "ssmq_marginal_traj.h"
#include <cmath>
#include <cstring>
#include <vector>

using namespace ssmq;

namespace {

using Run = RunT<kMaxPar>;

// values of the objective at n rows of parameters: rows [n][P], `traj[i]` = the trajectory row i belongs to; vals [n]
struct Evaluator {
    virtual int eval(int64_t n, const int64_t *traj, const double *rows, double *vals) = 0;
    virtual ~Evaluator() {}
};

// One trajectory's optimiser takes the objective values at its pending point r.xt (vals[0]) and at the forward-difference
// points (vals[1 + i]: r.xt + fd_step e_i) and either finishes (r.phase = PH_DONE, r.status) or leaves the next point in r.xt.
// B BFGS runs in lock step.  theta [B][P] start points in / minimisers out; skip[b] != 0: trajectory b is not run (status kept).
int bfgs_lockstep(int64_t B, int P, double fd_step, Evaluator &ev, double *theta, double *hess_inv, int32_t *status, int32_t *iters,
                  int64_t *rounds_out) {
    std::vector<Run> run((size_t)B);
    for (int64_t b = 0; b < B; ++b) {
        Run &r = run[b];
        bfgs_start(r, P, theta + (size_t)b * P);
        if (status[b] != 0) {
            r.phase = PH_DONE;
            r.status = status[b];
        }
    }
    std::vector<int64_t> want, traj;
    std::vector<double> rows, vals;
    int64_t rounds = 0;
    const int per = P + 1;
    for (;;) {
        want.clear();
        for (int64_t b = 0; b < B; ++b)
            if (run[b].phase != PH_DONE) want.push_back(b);
        if (want.empty()) break;
        const int64_t nw = (int64_t)want.size(), items = nw * per;
        rows.resize((size_t)items * P); vals.resize((size_t)items); traj.resize((size_t)items);
        // objective and forward-difference gradient at xt: rows [xt; xt + h e_i]
        for (int64_t w = 0; w < nw; ++w) {
            const Run &r = run[want[w]];
            for (int j = 0; j < per; ++j) {
                traj[(size_t)(w * per + j)] = want[w];
                for (int i = 0; i < P; ++i) rows[(size_t)(w * per + j) * P + i] = r.xt[i] + ((j == i + 1) ? fd_step : 0.0);
            }
        }
        const int rc = ev.eval(items, traj.data(), rows.data(), vals.data());
        if (rc < 0) return rc;
        ++rounds;
        for (int64_t w = 0; w < nw; ++w) bfgs_advance(run[want[w]], P, fd_step, &vals[(size_t)(w * per)]);
    }
    for (int64_t b = 0; b < B; ++b) {
        const Run &r = run[b];
        for (int i = 0; i < P; ++i) theta[(size_t)b * P + i] = r.x[i];
        std::memcpy(hess_inv + (size_t)b * P * P, r.H, sizeof(double) * P * P);
        status[b] = r.status;
        if (iters) iters[b] = r.k;
    }
    if (rounds_out) *rounds_out = rounds;
    return SSMQ_OK;
}

// objective of the marginalised filter: -log N(y_b | theta-conditioned step) - log N(theta | prior_b)   (ssinf.py:1153-1241)
struct MarginalObjective : Evaluator {
    ssmq_transform *h_dyn, *h_obs;
    const ssmq_integrand *f_dyn, *f_obs;
    int Din, D, Y, Pd, Po, P;
    double jitter, time;
    const double *mean, *cov, *y, *GQG, *R, *prior_mean;
    std::vector<double> Lp, logdet2;                 // per trajectory: Cholesky factor of the prior covariance, 2 sum log diag
    std::vector<double> pd, po, mm, cc, yy, ll, om, oc;
    std::vector<int32_t> st;
    double log_prior(int64_t b, const double *th) const {
        return mg_log_prior<kMaxPar>(prior_mean + (size_t)b * P, &Lp[(size_t)b * P * P], logdet2[(size_t)b], P, th);
    }
    int eval(int64_t items, const int64_t *traj, const double *rows, double *vals) override {
        pd.resize((size_t)items * Pd); po.resize((size_t)items * Po);
        mm.resize((size_t)items * Din); cc.resize((size_t)items * Din * Din); yy.resize((size_t)items * Y);
        ll.resize((size_t)items); om.resize((size_t)items * D); oc.resize((size_t)items * D * D); st.assign((size_t)items, 0);
        for (int64_t it = 0; it < items; ++it) {
            const int64_t b = traj[it];
            for (int i = 0; i < P; ++i) {
                const double e = std::exp(rows[(size_t)it * P + i]);        // the kernel parameters are exp(theta)
                if (i < Pd) pd[(size_t)it * Pd + i] = e;
                else po[(size_t)it * Po + (i - Pd)] = e;
            }
            std::memcpy(&mm[(size_t)it * Din], mean + (size_t)b * Din, sizeof(double) * Din);
            std::memcpy(&cc[(size_t)it * Din * Din], cov + (size_t)b * Din * Din, sizeof(double) * Din * Din);
            std::memcpy(&yy[(size_t)it * Y], y + (size_t)b * Y, sizeof(double) * Y);
        }
        const int rc = ssmq_gp_theta_step(h_dyn, f_dyn, h_obs, f_obs, items, pd.data(), po.data(), jitter, mm.data(), cc.data(), 0,
                                          yy.data(), 0, time, GQG, R, om.data(), oc.data(), ll.data(), st.data());
        if (rc < 0) return rc;          // argument / device error; rc > 0 only reports items that are not positive definite
        for (int64_t it = 0; it < items; ++it) vals[it] = -ll[(size_t)it] - log_prior(traj[it], rows + (size_t)it * P);
        return 0;
    }
};

// a host function as the objective: the optimiser's restatement is pinned against scipy.optimize.minimize on the CPU with it
struct CallbackObjective : Evaluator {
    ssmq_objective_fn fn;
    void *ctx;
    int P;
    int eval(int64_t items, const int64_t *traj, const double *rows, double *vals) override { return fn(ctx, items, P, traj, rows, vals); }
};

}  // namespace

extern "C" int ssmq_bfgs_lockstep_host(ssmq_objective_fn fn, void *ctx, int64_t B, int P, double fd_step, double *theta,
                                       double *hess_inv, int32_t *status, int32_t *iters, int64_t *rounds) {
    if (!fn || B < 0 || P < 1 || P > kMaxPar || (B > 0 && (!theta || !hess_inv || !status))) {
        set_error("bfgs_lockstep_host: bad argument");
        return SSMQ_E_ARG;
    }
    for (int64_t b = 0; b < B; ++b) status[b] = 0;
    CallbackObjective ev;
    ev.fn = fn; ev.ctx = ctx; ev.P = P;
    return bfgs_lockstep(B, P, fd_step, ev, theta, hess_inv, status, iters, rounds);
}

// The analytic-gradient mode of the same state machine on a host objective: B runs in lock step, each round one call of fn
// for the pending points of the unfinished runs (value and gradient together, as minimize(..., jac=True) takes them).
extern "C" int ssmq_bfgs_jac_lockstep_host(ssmq_objective_grad_fn fn, void *ctx, int64_t B, int P, double gtol, int maxiter,
                                           double *theta, double *fun, double *jac, double *hess_inv, int32_t *status,
                                           int32_t *nit, int32_t *nfev) {
    if (!fn || B < 0 || P < 1 || P > kMaxPar || (B > 0 && (!theta || !fun || !jac || !hess_inv || !status))) {
        set_error("bfgs_jac_lockstep_host: bad argument");
        return SSMQ_E_ARG;
    }
    if (maxiter < 0) maxiter = 200 * P;
    std::vector<Run> run((size_t)B);
    std::vector<int32_t> evals((size_t)B, 0);
    for (int64_t b = 0; b < B; ++b) bfgs_start(run[b], P, theta + (size_t)b * P);
    std::vector<int64_t> want;
    std::vector<double> rows, vals, grads;
    for (;;) {
        want.clear();
        for (int64_t b = 0; b < B; ++b)
            if (run[b].phase != PH_DONE) want.push_back(b);
        if (want.empty()) break;
        const int64_t nw = (int64_t)want.size();
        rows.resize((size_t)nw * P); vals.resize((size_t)nw); grads.resize((size_t)nw * P);
        for (int64_t w = 0; w < nw; ++w)
            for (int i = 0; i < P; ++i) rows[(size_t)w * P + i] = run[want[w]].xt[i];
        const int rc = fn(ctx, nw, P, want.data(), rows.data(), vals.data(), grads.data());
        if (rc < 0) return rc;
        for (int64_t w = 0; w < nw; ++w) {
            ++evals[want[w]];
            bfgs_advance_jac(run[want[w]], P, vals[w], &grads[(size_t)w * P], gtol, maxiter);
        }
    }
    for (int64_t b = 0; b < B; ++b) {
        const Run &r = run[b];
        for (int i = 0; i < P; ++i) {
            theta[(size_t)b * P + i] = r.x[i];
            jac[(size_t)b * P + i] = r.g[i];
        }
        std::memcpy(hess_inv + (size_t)b * P * P, r.H, sizeof(double) * P * P);
        fun[b] = r.old_fval;
        status[b] = r.status;
        if (nit) nit[b] = r.k;
        if (nfev) nfev[b] = evals[b];
    }
    return SSMQ_OK;
}

extern "C" int ssmq_gp_marginal_laplace_batch(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                              const ssmq_integrand *f_obs, int64_t B, double jitter, const double *mean,
                                              const double *cov, const double *y, double time, const double *GQG, const double *R,
                                              const double *prior_mean, const double *prior_cov, double fd_step, double *theta,
                                              double *hess_inv, int32_t *status, int32_t *iters, int64_t *rounds_out) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("ssmq_gp_marginal_laplace_batch");
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo("ssmq_gp_marginal_laplace_batch");
    if (is_trunc(h_dyn) || is_trunc(h_obs)) return refuse_trunc("ssmq_gp_marginal_laplace_batch");
    if (is_gpqd(h_dyn) || is_gpqd(h_obs)) return refuse_gpqd("ssmq_gp_marginal_laplace_batch");
    if (is_taylor_gpqd(h_dyn) || is_taylor_gpqd(h_obs)) return refuse_taylor_gpqd("ssmq_gp_marginal_laplace_batch");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || B < 0 || (B > 0 && (!mean || !cov || !y || !prior_mean || !prior_cov || !theta ||
                                                                     !hess_inv || !status))) {
        set_error("marginal_laplace_batch: null argument");
        return SSMQ_E_ARG;
    }
    MarginalObjective ev;
    ev.h_dyn = h_dyn; ev.h_obs = h_obs; ev.f_dyn = f_dyn; ev.f_obs = f_obs;
    ev.Din = h_dyn->D; ev.D = h_dyn->E; ev.Y = h_obs->E; ev.Pd = ev.Din + 1; ev.Po = h_obs->D + 1; ev.P = ev.Pd + ev.Po;
    ev.jitter = jitter; ev.time = time; ev.mean = mean; ev.cov = cov; ev.y = y; ev.GQG = GQG; ev.R = R; ev.prior_mean = prior_mean;
    const int P = ev.P;
    if (P > kMaxPar) {
        set_error("marginal_laplace_batch: too many kernel parameters");
        return SSMQ_E_UNSUPPORTED;
    }
    if (rounds_out) *rounds_out = 0;
    if (B == 0) return SSMQ_OK;
    ev.Lp.resize((size_t)B * P * P);
    ev.logdet2.assign((size_t)B, 0.0);
    for (int64_t b = 0; b < B; ++b)      // numpy.linalg.cholesky would raise in _param_log_prior
        status[b] = chol_lower(prior_cov + (size_t)b * P * P, P, &ev.Lp[(size_t)b * P * P], &ev.logdet2[(size_t)b]) ? 0 : SSMQ_BFGS_PRIOR_NOT_PD;
    return bfgs_lockstep(B, P, fd_step, ev, theta, hess_inv, status, iters, rounds_out);
}
