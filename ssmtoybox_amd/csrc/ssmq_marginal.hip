// ssmq_gp_marginal_filter_batch: the marginalised GP-quadrature filter for B trajectories - the entry point and its host rounds.
// The per-trajectory state machine is ssmq_marginal_traj.h; the routes that run it on the device are ssmq_marginal_device.hip; the
// lock-step Laplace step of ONE time step (ssmq_gp_marginal_laplace_batch) and the SciPy provenance of the optimiser are
// ssmq_bfgs_lockstep.hip.
#include "ssmq_marginal_traj.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstring>
#include <limits>
#include <vector>

using namespace ssmq;

// ---------------------------------------------------------------------------------------------------------------------------
// The whole marginalised filter for B trajectories, every trajectory at its own pace.
//
// ssmq_gp_marginal_laplace_batch keeps the trajectories in lock step PER TIME STEP: a step costs as many device rounds as its
// slowest trajectory needs (a few run 50 BFGS iterations on a noisy objective), and the others wait.  Trajectories are
// independent across time steps as well (research/tpq/tpq_base.py:175-192 loops over them), so here each one walks
// ssinf.py:66-118 / 1083-1273 by itself - Laplace step (BFGS), marginalisation over the parameter sigma points, next time
// step - and a round sends whatever every unfinished trajectory is waiting for, with its own time index
// (ssmq_gp_theta_step_times): (param_dim + 1) objective points or NP marginalisation points.  The number of rounds is the
// LONGEST trajectory's total, not the sum over the steps of the slowest one's.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// The host side of a round (parameter rows in, optimiser steps out) is independent per trajectory: with a thousand trajectories
// in flight it was 40 % of the call (17 + 23 of 101 ms at B = 1 024), so rounds with many active trajectories are cut into
// chunks for a few worker threads that live for the duration of the call.  Small rounds (the long tail of a few slow
// trajectories) run inline: waking the workers costs more than they would save.
class Workers {
public:
    explicit Workers(int n) {
        for (int i = 0; i < n; ++i) th_.emplace_back([this, i] { loop(i); });
    }
    ~Workers() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
            ++gen_;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    // fn(begin, end) over [0, n) in chunks, the calling thread included; returns when all of it is done
    void run(size_t n, const std::function<void(size_t, size_t)> &fn) {
        const size_t parts = th_.size() + 1;
        if (th_.empty() || n < 256) {
            fn(0, n);
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            fn_ = &fn;
            n_ = n;
            chunk_ = (n + parts - 1) / parts;
            pending_ = (int)th_.size();
            ++gen_;
        }
        cv_.notify_all();
        fn(0, std::min(n, chunk_));
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return pending_ == 0; });
    }

private:
    void loop(int i) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(size_t, size_t)> *fn;
            size_t b, e;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                fn = fn_;
                b = std::min(n_, chunk_ * (size_t)(i + 1));
                e = std::min(n_, chunk_ * (size_t)(i + 2));
            }
            if (b < e) (*fn)(b, e);
            {
                std::lock_guard<std::mutex> g(m_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t, size_t)> *fn_ = nullptr;
    size_t n_ = 0, chunk_ = 0;
    int pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

using Traj = TrajD<kMaxPar>;

// where a trajectory's item results of this round are: the host arrays of ssmq_gp_theta_step_times, from item f0 on
struct HostResults {
    const double *ll_, *om_, *oc_;
    const int32_t *st_;
    int64_t f0;
    int D;
    double ll(int j) const { return ll_[f0 + j]; }
    int32_t st(int j) const { return st_[f0 + j]; }
    double m(int i, int j) const { return om_[(size_t)(f0 + j) * D + i]; }
    double P(int i, int j) const { return oc_[(size_t)(f0 + j) * D * D + i]; }
};

// The host rounds (SSMQ_MARGINAL_HOST_ROUNDS=1, and every shape without a device route): the state machines on the host, per round
// ONE theta step of whatever every unfinished trajectory waits for.
int marginal_filter_host_rounds(const MarginalCall &c) {
    MgArgs a = mg_args(c);
    const int64_t B = a.B;
    const int T = a.T, P = a.P, Pd = a.Pd, Po = a.Po, Din = a.Din, D = a.D, Y = a.Y;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<Traj> tr((size_t)B);
    a.traj = tr.data();
    a.y = c.y; a.x0_mean = c.x0_mean; a.x0_cov = c.x0_cov; a.prior_mean = c.prior_mean; a.prior_cov = c.prior_cov;
    a.q_mean = c.q_mean; a.q_cov = c.q_cov; a.upts = c.upts; a.uwts = c.uwts;
    a.fm = c.fm; a.fP = c.fP; a.failed = c.failed;
    for (int64_t i = 0; i < (int64_t)B * T * D; ++i) c.fm[i] = nan;
    for (int64_t i = 0; i < (int64_t)B * T * D * D; ++i) c.fP[i] = nan;
    for (int64_t b = 0; b < B; ++b) mg_init(tr[b], a, b);
    std::vector<int64_t> who, first;
    std::vector<double> pd, po, mm, cc, yy, tt, ll, om, oc;
    std::vector<int32_t> st;
    int64_t rounds = 0, iters = 0, total_items = 0;
    // worker threads: SSMQ_MARGINAL_THREADS (0 = none), else up to 8 and never more than the trajectories could use
    int n_workers = 7;
    if (const char *e = ssmq::sw("SSMQ_MARGINAL_THREADS")) n_workers = std::max(0, atoi(e) - 1);
    n_workers = (int)std::min<int64_t>(std::min<unsigned>((unsigned)n_workers, std::max(1u, std::thread::hardware_concurrency()) - 1), B / 256);
    Workers pool(n_workers);
    const bool timing = ssmq::sw("SSMQ_MARGINAL_TIMING") != nullptr;      // host-side budget of the rounds, printed at the end
    double t_pack = 0.0, t_call = 0.0, t_adv = 0.0;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    for (;;) {
        const double t0 = timing ? now() : 0.0;
        who.clear(); first.clear();
        int64_t items = 0;
        for (int64_t b = 0; b < B; ++b)
            if (tr[b].mode != 2) {
                who.push_back(b);
                first.push_back(items);
                items += mg_items(tr[b].mode, P, a.NP);
            }
        if (who.empty()) break;
        pd.resize((size_t)items * Pd); po.resize((size_t)items * Po);
        mm.resize((size_t)items * Din); cc.resize((size_t)items * Din * Din); yy.resize((size_t)items * Y); tt.resize((size_t)items);
        ll.resize((size_t)items); om.resize((size_t)items * D); oc.resize((size_t)items * D * D); st.assign((size_t)items, 0);
        pool.run(who.size(), [&](size_t w0, size_t w1) {
        for (size_t w = w0; w < w1; ++w) {
            const int64_t b = who[w];
            const Traj &t = tr[b];
            const int n = mg_items(t.mode, P, a.NP);
            for (int j = 0; j < n; ++j) {
                const int64_t it = first[w] + j;
                for (int i = 0; i < P; ++i) {
                    const double e = std::exp(mg_point(t, a, j, i));   // the kernel parameters are exp(theta)
                    if (i < Pd) pd[(size_t)it * Pd + i] = e;
                    else po[(size_t)it * Po + (i - Pd)] = e;
                }
                mg_moments(t, a, &mm[(size_t)it * Din], &cc[(size_t)it * Din * Din], Din);
                std::memcpy(&yy[(size_t)it * Y], c.y + ((size_t)b * T + (t.k - 1)) * Y, sizeof(double) * Y);
                tt[(size_t)it] = (double)t.k;
            }
        }
        });
        const double t1 = timing ? now() : 0.0;
        const int rc = ssmq_gp_theta_step_times(c.h_dyn, c.f_dyn, c.h_obs, c.f_obs, items, pd.data(), po.data(), c.jitter, mm.data(), cc.data(),
                                                0, yy.data(), 0, tt.data(), c.GQG, c.R, om.data(), oc.data(), ll.data(), st.data());
        if (rc < 0) return rc;
        const double t2 = timing ? now() : 0.0;
        ++rounds;
        total_items += items;
        std::atomic<int64_t> iters_round{0};
        pool.run(who.size(), [&](size_t w0, size_t w1) {
        int64_t iters_mine = 0;
        for (size_t w = w0; w < w1; ++w)
            iters_mine += mg_advance_one<kMaxPar, 0, HostResults, true>(tr[who[w]], a, who[w],
                                                                         HostResults{ll.data(), om.data(), oc.data(), st.data(), first[w], D});
        iters_round += iters_mine;
        });
        iters += iters_round.load();
        if (timing) {
            const double t3 = now();
            t_pack += t1 - t0; t_call += t2 - t1; t_adv += t3 - t2;
        }
    }
    if (timing)
        fprintf(stderr, "marginal_filter_batch: %lld rounds, %lld items: pack %.2f ms, theta step %.2f ms, optimiser / mixtures %.2f ms\n",
                (long long)rounds, (long long)total_items, 1e3 * t_pack, 1e3 * t_call, 1e3 * t_adv);
    for (int64_t b = 0; b < B; ++b) {
        if (c.theta_last) std::memcpy(c.theta_last + (size_t)b * P, tr[b].pm, sizeof(double) * P);
        if (c.pcov_last) std::memcpy(c.pcov_last + (size_t)b * P * P, tr[b].pc, sizeof(double) * P * P);
    }
    if (c.stats) {
        c.stats[0] = rounds; c.stats[1] = iters; c.stats[2] = total_items;
    }
    return SSMQ_OK;
}

}  // namespace

extern "C" int ssmq_gp_marginal_filter_batch(ssmq_transform *h_dyn, const ssmq_integrand *f_dyn, ssmq_transform *h_obs,
                                             const ssmq_integrand *f_obs, int64_t B, int T, double jitter, const double *y,
                                             const double *x0_mean, const double *x0_cov, const double *q_mean,
                                             const double *q_cov, const double *GQG, const double *R, const double *prior_mean,
                                             const double *prior_cov, const double *upts, const double *uwts, int NP,
                                             double fd_step, double param_jitter, double *fm, double *fP, int32_t *failed,
                                             double *theta_last, double *pcov_last, int64_t *stats) {
    if (is_user_integrand(f_dyn) || is_user_integrand(f_obs)) return refuse_user_integrand("ssmq_gp_marginal_filter_batch");
    if (is_mo(h_dyn) || is_mo(h_obs)) return refuse_mo("ssmq_gp_marginal_filter_batch");
    if (is_trunc(h_dyn) || is_trunc(h_obs)) return refuse_trunc("ssmq_gp_marginal_filter_batch");
    if (is_gpqd(h_dyn) || is_gpqd(h_obs)) return refuse_gpqd("ssmq_gp_marginal_filter_batch");
    if (is_taylor_gpqd(h_dyn) || is_taylor_gpqd(h_obs)) return refuse_taylor_gpqd("ssmq_gp_marginal_filter_batch");
    SSMQ_HANDLE_LOCK(h_dyn, h_obs);
    if (!h_dyn || !h_obs || !f_dyn || !f_obs || B < 0 || T < 0 || (B > 0 && T > 0 && (!y || !x0_mean || !x0_cov || !prior_mean ||
        !prior_cov || !upts || !uwts || !fm || !fP || !failed))) {
        set_error("marginal_filter_batch: null argument");
        return SSMQ_E_ARG;
    }
    const MarginalCall c{h_dyn, f_dyn, h_obs, f_obs, B, T, jitter, y, x0_mean, x0_cov, q_mean, q_cov, GQG, R, prior_mean, prior_cov,
                         upts, uwts, NP, fd_step, param_jitter, fm, fP, failed, theta_last, pcov_last, stats};
    const MgArgs shape = mg_args(c);
    if (shape.P > kMaxPar || NP < 1 || NP > 2 * kMaxPar || shape.dq < 0 || (shape.dq > 0 && (!q_mean || !q_cov))) {
        set_error("marginal_filter_batch: bad shape (parameters, parameter points, or noise moments of augmented dynamics missing)");
        return SSMQ_E_ARG;
    }
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (B == 0 || T == 0) return SSMQ_OK;
    // the state machines on the device where the theta step has its two-launch route and the parameter count an instantiation
    // (SSMQ_MARGINAL_HOST_ROUNDS=1: the host rounds, round 4's route, kept as the second implementation of the same filter)
    if (!ssmq::sw("SSMQ_MARGINAL_HOST_ROUNDS") && shape.P <= 16 && NP <= 32 && theta_dev_supported(h_dyn, f_dyn, h_obs, f_obs)) {
        const int rc = marginal_filter_batch_device(c);
        if (rc != SSMQ_E_UNSUPPORTED) return rc;
    }
    return marginal_filter_host_rounds(c);
}
