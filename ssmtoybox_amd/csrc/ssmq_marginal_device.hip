// The batched marginalised GP-quadrature filter (ssmq_gp_marginal_filter_batch, ssmq_marginal.hip) with the per-trajectory state
// machines of ssmq_marginal_traj.h ON THE DEVICE: as rounds of a few launches, or - small systems - the whole filter in one launch.
//
// ---- device-resident rounds ------------------------------------------------------------------------------------------------------
// One thread per trajectory packs the points it is
// waiting for straight into the theta step's device arena (k_mg_scan: item offsets by a block-wide scan; k_mg_fill), the theta
// step runs on them with the item count read from device memory (theta_dev_enqueue: k_theta_weights, k_theta_chain), and the same
// thread takes the values and advances its optimiser / mixture / time step (k_mg_advance: mg_advance_one, the code the host
// rounds run).  The host only queues rounds - four or five launches each, no copy, no synchronisation - a few ahead of the
// progress the device reports through two integers in pinned host memory (unfinished trajectories - also the bound of the next
// launches' grids - and scans done).
// Round 4's host rounds cost ~85 us each (55 us of which copies, synchronisation and host turn-around: DESIGN.md 3.13) and
// the number of rounds is set by the ONE longest trajectory.
#include "ssmq_marginal_traj.h"
#include "ssmq_theta_item.h"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

using namespace ssmq;

namespace {

constexpr int kRoundsAhead = 12;       // rounds queued ahead of the device's progress

// what the host steers by, written to pinned host memory after every scan (ONE thread): the number of unfinished trajectories, then -
// behind a system-scope fence - the number of scans done.  The host never waits for a round: it keeps a few rounds queued ahead
// of the scan count it sees and stops queueing when a scan has found nothing unfinished.
__device__ __forceinline__ void mg_publish(const MgArgs &a, int unfinished) {
    const int seq = a.count[3] + 1;
    a.count[3] = seq;
    if (a.hflag) {
        a.hflag[0] = unfinished;
        __threadfence_system();
        a.hflag[1] = seq;
    }
}

template <int PM>
__global__ void k_mg_init(const MgArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    TrajD<PM> &t = ((TrajD<PM> *)a.traj)[b];
    mg_init(t, a, b);
    a.modes[b] = (signed char)t.mode;
}

// item offsets of this round (one workgroup; trajectories in order, so the item order is the host rounds'): every thread takes
// four consecutive trajectories (their modes from the compact mirror a.modes), wave prefix sums by shuffles, the four wave totals
// through LDS
template <int PM>
__global__ __launch_bounds__(256) void k_mg_scan(const MgArgs a) {
    __shared__ int32_t wtot[4], wact[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0, act = 0;
    for (int64_t base = 0; base < a.B; base += 1024) {
        int n[4], mine = 0, alive = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = base + 4 * (int64_t)threadIdx.x + q;
            const int mode = b < a.B ? (int)a.modes[b] : 2;
            n[q] = mg_items(mode, a.P, a.NP);
            mine += n[q];
            alive += mode != 2;
        }
        int incl = mine, asum = alive;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
            asum += __shfl_xor(asum, off, 64);
        }
        if (lane == 63) wtot[wave] = incl;
        if (lane == 0) wact[wave] = asum;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        int run = before + incl - mine;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = base + 4 * (int64_t)threadIdx.x + q;
            if (b < a.B) a.first[b] = run;
            run += n[q];
        }
        carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        act += wact[0] + wact[1] + wact[2] + wact[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.count[0] = carry;
        a.count[1] = act;
        if (carry > 0) {
            a.count[2] += 1;
            a.totals[0] += (unsigned long long)carry;
        }
        mg_publish(a, act);
    }
}

// the points trajectory b waits for, as items of the theta step (what the host rounds pack into rows / pd / po / mm / cc / yy / tt);
// one thread per (trajectory, item slot): `per` = max(P + 1, NP) slots per trajectory
// SCAN: the item offsets are formed HERE, by every workgroup for its own trajectories (256 / per of them) from the compact mode
// mirror - a sweep over B bytes per workgroup instead of a kernel of its own (k_mg_scan: 4.4 us + a launch gap per round); used
// while that sweep is short (B <= 8 192).  Workgroup 0 also leaves the round's item and trajectory counts.
template <int PM, bool SCAN>
__global__ __launch_bounds__(256) void k_mg_fill(const MgArgs a, int per) {
    int64_t b;
    int j;
    int32_t first_b = 0;
    if constexpr (SCAN) {
        __shared__ int32_t red[3][4], nloc[64];
        const int tpb = 256 / per;                                  // trajectories of this workgroup (per <= 32: >= 8)
        const int lb = threadIdx.x / per;
        j = threadIdx.x - lb * per;
        const int64_t b_first = (int64_t)blockIdx.x * tpb;
        b = b_first + lb;
        int pre = 0, tot = 0, act = 0;
        for (int64_t i = threadIdx.x; i < a.B; i += 256) {
            const int mode = (int)a.modes[i];
            const int n = mg_items(mode, a.P, a.NP);
            tot += n;
            act += mode != 2;
            if (i < b_first) pre += n;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            pre += __shfl_xor(pre, off, 64);
            tot += __shfl_xor(tot, off, 64);
            act += __shfl_xor(act, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = pre; red[1][threadIdx.x >> 6] = tot; red[2][threadIdx.x >> 6] = act;
        }
        if (threadIdx.x < 64) {
            const int64_t bb = b_first + threadIdx.x;
            const int mode = (threadIdx.x < tpb && bb < a.B) ? (int)a.modes[bb] : 2;
            nloc[threadIdx.x] = mg_items(mode, a.P, a.NP);
        }
        __syncthreads();
        first_b = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        for (int l = 0; l < lb && l < tpb; ++l) first_b += nloc[l];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const int total = red[1][0] + red[1][1] + red[1][2] + red[1][3];
            a.count[0] = total;
            a.count[1] = red[2][0] + red[2][1] + red[2][2] + red[2][3];
            if (total > 0) {
                a.count[2] += 1;
                a.totals[0] += (unsigned long long)total;
            }
            mg_publish(a, a.count[1]);
        }
        if (lb >= tpb || b >= a.B) return;
        if (j == 0) a.first[b] = first_b;
    } else {
        const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        b = tid / per;
        j = (int)(tid - b * per);
        if (b >= a.B) return;
        first_b = a.first[b];
    }
    const TrajD<PM> &t = ((const TrajD<PM> *)a.traj)[b];
    if (t.mode == 2) return;
    const int P = a.P, Pd = a.Pd, Po = a.Po, Din = a.Din, Y = a.Y;
    if (j >= mg_items(t.mode, P, a.NP)) return;
    const int64_t ld = a.th.ld;
    const int64_t it = (int64_t)first_b + j;
    for (int i = 0; i < P; ++i) {
        const double e = exp(mg_point(t, a, j, i));        // the kernel parameters are exp(theta)
        if (i < Pd) a.th.pard[(size_t)it * Pd + i] = e;
        else a.th.paro[(size_t)it * Po + (i - Pd)] = e;
    }
    mg_moments(t, a, a.th.mean + (size_t)it * Din, a.th.cov + (size_t)it * Din * Din, Din);
    for (int k = 0; k < Y; ++k) a.th.ysoa[(size_t)k * ld + it] = a.y[((size_t)b * a.T + (t.k - 1)) * Y + k];
    a.th.tt[it] = (double)t.k;
}

// where a trajectory's item results of this round are: the theta step's device arena (rounds route) ...
struct ArenaResults {
    const ThetaDev &th;
    int64_t f0;
    __device__ __forceinline__ double ll(int j) const { return th.ll[f0 + j]; }
    __device__ __forceinline__ int32_t st(int j) const { return th.st_all[f0 + j]; }
    __device__ __forceinline__ double m(int i, int j) const { return th.m_fi[(size_t)i * th.ld + f0 + j]; }
    __device__ __forceinline__ double P(int i, int j) const { return th.P_fi[(size_t)i * th.ld + f0 + j]; }
};

// kAdvPerWave trajectories per wave (every (64 / kAdvPerWave)-th lane): a wave walks the union of its lanes' branches, fewer
// lanes = fewer of them
#ifndef SSMQ_MG_ADV_PER_WAVE
#define SSMQ_MG_ADV_PER_WAVE 8
#endif
constexpr int kAdvPerWave = SSMQ_MG_ADV_PER_WAVE;
template <int PM, int PX>
__global__ __launch_bounds__(64) void k_mg_advance(const MgArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kAdvPerWave + threadIdx.x / (64 / kAdvPerWave);
    if (threadIdx.x % (64 / kAdvPerWave) != 0 || b >= a.B) return;
    if (a.modes[b] == 2) return;
    const int iters = mg_advance_one<PM, PX>(((TrajD<PM> *)a.traj)[b], a, b, ArenaResults{a.th, (int64_t)a.first[b]});
    if (iters) atomicAdd(&a.totals[1], (unsigned long long)iters);
    a.modes[b] = (signed char)((const TrajD<PM> *)a.traj)[b].mode;
}

template <int PM>
__global__ void k_mg_finish(const MgArgs a, double *theta_last, double *pcov_last) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const TrajD<PM> &t = ((const TrajD<PM> *)a.traj)[b];
    for (int i = 0; i < a.P; ++i) theta_last[(size_t)b * a.P + i] = t.pm[i];
    for (int i = 0; i < a.P * a.P; ++i) pcov_last[(size_t)b * a.P * a.P + i] = t.pc[i];
}

// ---- the whole filter in ONE launch (small systems) --------------------------------------------------------------------------------
// Trajectories never interact, and with the theta step of an item a per-lane device function (ssmq_theta_item.h) nothing in a
// round needs another kernel: a group of PER = max(P + 1, NP) lanes owns a trajectory, every lane of the group evaluates ONE of
// the points the trajectory waits for, the group's first lane takes the values and advances the trajectory's state machine, and
// the wave (64 / PER trajectories) loops until all of its trajectories are through their T steps or have failed.  No scan, no
// packing, no kernel boundary and no host between two evaluations; the exit condition is per wave and every path of the state
// machine is bounded (BFGS: 200 P iterations of at most 100 + 10 + 10 line-search evaluations).  Item inputs and results cross
// lanes through a few hundred bytes of LDS per trajectory.  Same arithmetic as the rounds route - same device functions, same
// exp / log - so the two agree bit for bit (tests/test_gpu_parity.py::test_marginal_filter_one_launch_matches_device_rounds).
struct MgItem {
    int32_t fid_dyn, fid_obs, emv_dyn, emv_obs;
    FPar fpd, fpo;
    double jitter;
};

template <int TPW, int PER, int D>
struct LdsResults {
    const double (*ll_)[PER];
    const double (*m_)[PER][D];
    const double (*P_)[PER][D * D];
    const int32_t (*st_)[PER];
    int g;
    __device__ __forceinline__ double ll(int j) const { return ll_[g][j]; }
    __device__ __forceinline__ int32_t st(int j) const { return st_[g][j]; }
    __device__ __forceinline__ double m(int i, int j) const { return m_[g][j][i]; }
    __device__ __forceinline__ double P(int i, int j) const { return P_[g][j][i]; }
};

template <int PX, int DIN, int D, int Y, int ND, int NO>
__global__ __launch_bounds__(64) void k_mg_persistent(const MgArgs a, const MgItem it) {
    constexpr int PER = 2 * PX, TPW = 64 / PER, PM = PX, Pd = DIN + 1, dq = DIN - D;
    __shared__ int32_t s_n[TPW];
    __shared__ double o_ll[TPW][PER], o_m[TPW][PER][D], o_P[TPW][PER][D * D];
    __shared__ int32_t o_st[TPW][PER];
    const int lane = threadIdx.x, g = lane / PER, j = lane - g * PER;
    const int64_t b = (int64_t)blockIdx.x * TPW + g;
    const bool in_group = g < TPW;
    const bool member = in_group && b < a.B;
    const bool leader = member && j == 0;
    // The trajectories' states live in LDS for the length of the kernel (3 KB each): the optimiser reads and writes its state
    // every round - on the arena's 3 KB-strided structs each of those accesses is an L2 round trip on the wave's critical path -
    // and the lanes of the group read the point they are to evaluate straight from it.
    static_assert(sizeof(TrajD<PM>) % sizeof(double) == 0, "TrajD: a whole number of doubles");
    __shared__ double s_traj[TPW][sizeof(TrajD<PM>) / sizeof(double)];      // (raw: the struct has member initialisers)
    TrajD<PM> *tp = reinterpret_cast<TrajD<PM> *>(s_traj[in_group ? g : 0]);
    if (leader) {
        mg_init<PX, D>(*tp, a, b);
    }
    if (in_group && j == 0) s_n[g] = leader ? mg_items(tp->mode, PX, a.NP) : 0;
    __syncthreads();
    int32_t rounds = 0;
    unsigned long long items = 0;
    for (;;) {
        int any = 0;
#pragma unroll
        for (int gg = 0; gg < TPW; ++gg) any += s_n[gg];
        if (any == 0) break;                                   // (the same for every lane of the wave)
        ++rounds;
        items += (unsigned long long)any;
        // ---- one point per lane: the theta-conditioned filter step ------------------------------------------------------------------
        if (member && j < s_n[g]) {
            const TrajD<PM> &t = *tp;
            double par_d[Pd], par_o[D + 1], m[DIN], cv[DIN][DIN], yv[Y], m_fi[D], P_fi[D][D], ll;
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const double e = exp(mg_point<PX>(t, a, j, i));    // the kernel parameters are exp(theta)
                if (i < Pd) par_d[i] = e;
                else par_o[i - Pd] = e;
            }
            // [mean; q_mean], blockdiag(cov, Q) as mg_moments forms them, unrolled at the compile-time shapes: m and cv stay in registers
#pragma unroll
            for (int i = 0; i < DIN; ++i)
#pragma unroll
                for (int k = 0; k < DIN; ++k) cv[i][k] = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                m[i] = t.xm[i];
#pragma unroll
                for (int k = 0; k < D; ++k) cv[i][k] = t.xP[i * D + k];
            }
#pragma unroll
            for (int i = 0; i < dq; ++i) {
                m[D + i] = a.q_mean[i];
#pragma unroll
                for (int k = 0; k < dq; ++k) cv[D + i][D + k] = a.q_cov[i * dq + k];
            }
#pragma unroll
            for (int i = 0; i < Y; ++i) yv[i] = a.y[((size_t)b * a.T + (t.k - 1)) * Y + i];
            const int32_t st = theta_item::theta_item_core<DIN, D, Y, ND, NO>(it.fid_dyn, it.fid_obs, it.fpd, it.fpo, it.emv_dyn, it.emv_obs,
                                                                            a.th.xid, a.th.xio, par_d, par_o, m, cv, yv, (double)t.k, a.th.gq,
                                                                            a.th.rr, it.jitter, m_fi, P_fi, ll);
            o_ll[g][j] = ll;
            o_st[g][j] = st;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                o_m[g][j][d] = m_fi[d];
#pragma unroll
                for (int d2 = 0; d2 < D; ++d2) o_P[g][j][d * D + d2] = P_fi[d][d2];
            }
        }
        __syncthreads();
        // ---- the group's first lane advances: optimiser step, or Laplace posterior and its sigma points, or the mixture and the next
        // time step - and says what the trajectory waits for next
        if (leader && s_n[g] > 0) {
            const int iters = mg_advance_one<PM, PX, LdsResults<TPW, PER, D>, true>(*tp, a, b, LdsResults<TPW, PER, D>{o_ll, o_m, o_P, o_st, g});
            if (iters) atomicAdd(&a.totals[1], (unsigned long long)iters);
            s_n[g] = mg_items(tp->mode, PX, a.NP);
        }
        __syncthreads();
    }
    if (leader) {                                              // what k_mg_finish reads: the last step's parameter posterior
        TrajD<PM> &o = ((TrajD<PM> *)a.traj)[b];
        for (int i = 0; i < PX; ++i) o.pm[i] = tp->pm[i];
        for (int i = 0; i < PX * PX; ++i) o.pc[i] = tp->pc[i];
    }
    if (lane == 0) {
        atomicMax(&a.count[2], rounds);
        atomicAdd(&a.totals[0], items);
    }
}

typedef void (*mg_persistent_kernel)(const MgArgs, const MgItem);
struct MgPersistentEntry {
    int P, Din, D, Y, Nd, No;
    mg_persistent_kernel k;
};
#define SSMQ_MGP(PX, DIN, D, Y, ND, NO) {PX, DIN, D, Y, ND, NO, &k_mg_persistent<PX, DIN, D, Y, ND, NO>}
// the shapes of k_theta_item (ssmq_theta_item.hip): P = Din + D + 2 log-parameters
const MgPersistentEntry kMgPersistent[] = {
    SSMQ_MGP(4, 1, 1, 1, 2, 2), SSMQ_MGP(4, 1, 1, 1, 3, 3), SSMQ_MGP(5, 2, 1, 1, 4, 2), SSMQ_MGP(5, 2, 1, 1, 5, 3), SSMQ_MGP(6, 2, 2, 1, 4, 4),
    SSMQ_MGP(6, 2, 2, 1, 5, 5),
};

// Returns SSMQ_OK having produced everything, SSMQ_E_UNSUPPORTED if this shape has no device-resident route (the caller then runs
// the host rounds), or an error.
template <int PM, int PX>
int mg_device(const MarginalCall &c) {
    MgArgs a = mg_args(c);
    const int64_t B = a.B;
    const int T = a.T, P = a.P, NP = a.NP, Din = a.Din, D = a.D, Y = a.Y, dq = a.dq;
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t s = stream();
    const int per = std::max(P + 1, NP);
    const int64_t cap = B * per;
    if (cap > 0x7fffffff / 2) return SSMQ_E_UNSUPPORTED;
    // one arena: theta step | trajectory states | offsets and counters | inputs | outputs
    auto al = [](size_t n) { return (n + 255) / 256 * 256; };
    const size_t th_bytes = theta_dev_bytes(c.h_dyn, c.h_obs, cap);
    const size_t n_fm = (size_t)B * T * D, n_fP = (size_t)B * T * D * D;
    const size_t statics = (size_t)D + (size_t)D * D + P + (size_t)P * P + dq + (size_t)dq * dq + (size_t)P * NP + NP;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al(bytes); return o; };
    const size_t o_th = take(th_bytes), o_tr = take(sizeof(TrajD<PM>) * (size_t)B), o_first = take(sizeof(int32_t) * (size_t)B), o_modes = take((size_t)B),
                 o_count = take(sizeof(int32_t) * 4), o_tot = take(sizeof(unsigned long long) * 8), o_y = take(sizeof(double) * (size_t)B * T * Y),
                 o_st = take(sizeof(double) * statics), o_fm = take(sizeof(double) * n_fm), o_fP = take(sizeof(double) * n_fP),
                 o_failed = take(sizeof(int32_t) * (size_t)B), o_tl = take(sizeof(double) * (size_t)B * P),
                 o_pl = take(sizeof(double) * (size_t)B * P * P);
    char *dev = nullptr;
    SSMQ_HIP(hipMalloc((void **)&dev, off));
    struct Free { char *p; ~Free() { if (p) hipFree(p); } } guard{dev};
    theta_dev_carve(a.th, c.h_dyn, c.h_obs, cap, dev + o_th);
    a.traj = dev + o_tr;
    a.first = (int32_t *)(dev + o_first); a.modes = (signed char *)(dev + o_modes); a.count = (int32_t *)(dev + o_count); a.totals = (unsigned long long *)(dev + o_tot);
    a.y = (const double *)(dev + o_y);
    a.fm = (double *)(dev + o_fm); a.fP = (double *)(dev + o_fP); a.failed = (int32_t *)(dev + o_failed);
    // what the trajectories share: one host block, one copy
    std::vector<double> hs(statics);
    {
        double *h = hs.data(), *d = (double *)(dev + o_st);
        auto put = [&](const double *src, size_t n, const double **dst) {
            if (n) std::memcpy(h, src, sizeof(double) * n);
            *dst = d;
            h += n; d += n;
        };
        put(c.x0_mean, D, &a.x0_mean); put(c.x0_cov, (size_t)D * D, &a.x0_cov); put(c.prior_mean, P, &a.prior_mean);
        put(c.prior_cov, (size_t)P * P, &a.prior_cov); put(c.q_mean, dq, &a.q_mean); put(c.q_cov, (size_t)dq * dq, &a.q_cov);
        put(c.upts, (size_t)P * NP, &a.upts); put(c.uwts, NP, &a.uwts);
    }
    SSMQ_HIP(hipMemcpyAsync(dev + o_st, hs.data(), sizeof(double) * statics, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemcpyAsync(dev + o_y, c.y, sizeof(double) * (size_t)B * T * Y, hipMemcpyHostToDevice, s));
    SSMQ_HIP(hipMemsetAsync(dev + o_count, 0, sizeof(int32_t) * 4, s));
    SSMQ_HIP(hipMemsetAsync(dev + o_tot, 0, sizeof(unsigned long long) * 8, s));
    SSMQ_HIP(hipMemsetAsync(dev + o_fm, 0xff, sizeof(double) * (n_fm + 0), s));      // all-ones bit pattern: a NaN
    SSMQ_HIP(hipMemsetAsync(dev + o_fP, 0xff, sizeof(double) * n_fP, s));
    if ((rc = theta_dev_upload_static(a.th, c.h_dyn, c.h_obs, c.GQG, c.R, s))) return rc;
    const unsigned tb = 64, tg = (unsigned)((B + tb - 1) / tb);
    Ctx &cx = ctx();                                // 64 bytes of pinned, device-visible host memory, kept with the thread's context
    if (!cx.pinned_flags) SSMQ_HIP(hipHostMalloc(&cx.pinned_flags, 64, hipHostMallocPortable | hipHostMallocMapped));
    volatile int32_t *hf = (volatile int32_t *)cx.pinned_flags;
    hf[0] = (int32_t)std::min<int64_t>(B, 0x7fffffff);
    hf[1] = 0;
    a.hflag = hf;
    // the whole filter in one launch where the item step is a per-lane device function (k_mg_persistent); SSMQ_MARGINAL_ROUNDS=1
    // keeps the rounds below (the route of every other shape)
    int32_t hc[4] = {0, 0, 0, 0};
    const MgPersistentEntry *pe = nullptr;
    if (!ssmq::sw("SSMQ_MARGINAL_ROUNDS") && !ssmq::sw("SSMQ_NO_THETA_ITEM") && NP == 2 * P && PX == P)
        for (const MgPersistentEntry &e : kMgPersistent)
            if (e.P == P && e.Din == Din && e.D == D && e.Y == Y && e.Nd == c.h_dyn->N && e.No == c.h_obs->N) pe = &e;
    if (pe) {
        MgItem it;
        memset(&it, 0, sizeof(it));
        it.fid_dyn = c.f_dyn->id; it.fid_obs = c.f_obs->id; it.emv_dyn = c.h_dyn->emv_mode; it.emv_obs = c.h_obs->emv_mode; it.jitter = c.jitter;
        fill_fpar(c.f_dyn, &it.fpd);
        fill_fpar(c.f_obs, &it.fpo);
        const int tpw = 64 / (2 * P);
        hipLaunchKernelGGL(pe->k, dim3((unsigned)((B + tpw - 1) / tpw)), dim3(64), 0, s, a, it);
        if ((rc = hip_fail(hipGetLastError(), "k_mg_persistent"))) return rc;
    } else {
    hipLaunchKernelGGL(k_mg_init<PM>, dim3(tg), dim3(tb), 0, s, a);
    const bool fused_scan = B <= 8192 && per <= 32 && !ssmq::sw("SSMQ_MARGINAL_SCAN_KERNEL");
    const int64_t tpb_fill = 256 / per;
    // Rounds are queued kRoundsAhead ahead of the scan count the device reports through pinned host memory; nothing in this loop
    // waits for the device (round 5's first version synchronised every eighth round: a bubble of a copy and a launch each time).
    // The number of unfinished trajectories only falls, so the latest value seen bounds the grids of every round queued after it.
    int64_t launched = 0;
    int32_t last_seen = -1;
    auto last_progress = std::chrono::steady_clock::now();
    for (;;) {
        const int32_t seen = hf[1];
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const int32_t unfinished = hf[0];
        if (seen > 0 && unfinished == 0) break;               // a scan found every trajectory done: what is queued finds nothing to do
        if (launched - seen >= kRoundsAhead) {
            // every wait in this library has an end: a device that reports no scan for a minute is asked for its error
            if (seen != last_seen) {
                last_seen = seen;
                last_progress = std::chrono::steady_clock::now();
            } else if (std::chrono::steady_clock::now() - last_progress > std::chrono::seconds(60)) {
                SSMQ_HIP(hipStreamSynchronize(s));
                if (hf[1] == seen) {
                    set_error("marginal_filter_batch: the device rounds made no progress");
                    return SSMQ_E_HIP;
                }
            }
            std::this_thread::yield();
            continue;
        }
        const int64_t bound = std::max<int64_t>(1, unfinished) * per;
        if (fused_scan) {
            hipLaunchKernelGGL((k_mg_fill<PM, true>), dim3((unsigned)((B + tpb_fill - 1) / tpb_fill)), dim3(256), 0, s, a, per);
        } else {
            hipLaunchKernelGGL(k_mg_scan<PM>, dim3(1), dim3(256), 0, s, a);
            hipLaunchKernelGGL((k_mg_fill<PM, false>), dim3((unsigned)((B * per + 255) / 256)), dim3(256), 0, s, a, per);
        }
        if ((rc = theta_dev_enqueue(a.th, c.h_dyn, c.f_dyn, c.h_obs, c.f_obs, c.jitter, bound, a.count, s))) return rc;
        hipLaunchKernelGGL((k_mg_advance<PM, PX>), dim3((unsigned)((B + kAdvPerWave - 1) / kAdvPerWave)), dim3(64), 0, s, a);
        if ((rc = hip_fail(hipGetLastError(), "marginal filter: device rounds"))) return rc;
        ++launched;
    }
    }   // rounds route
    hipLaunchKernelGGL(k_mg_finish<PM>, dim3(tg), dim3(tb), 0, s, a, (double *)(dev + o_tl), (double *)(dev + o_pl));
    SSMQ_HIP(hipMemcpyAsync(c.fm, a.fm, sizeof(double) * n_fm, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipMemcpyAsync(c.fP, a.fP, sizeof(double) * n_fP, hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipMemcpyAsync(c.failed, a.failed, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, s));
    if (c.theta_last) SSMQ_HIP(hipMemcpyAsync(c.theta_last, dev + o_tl, sizeof(double) * (size_t)B * P, hipMemcpyDeviceToHost, s));
    if (c.pcov_last) SSMQ_HIP(hipMemcpyAsync(c.pcov_last, dev + o_pl, sizeof(double) * (size_t)B * P * P, hipMemcpyDeviceToHost, s));
    unsigned long long tot[8] = {0, 0};
    SSMQ_HIP(hipMemcpyAsync(hc, a.count, sizeof(hc), hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipMemcpyAsync(tot, a.totals, sizeof(tot), hipMemcpyDeviceToHost, s));
    SSMQ_HIP(hipStreamSynchronize(s));
    if (c.stats) {
        c.stats[0] = hc[2]; c.stats[1] = (int64_t)tot[1]; c.stats[2] = (int64_t)tot[0];
    }
    return SSMQ_OK;
}

}  // namespace

// (P = D + Din + 2: 4 scalar state, 5 scalar state with its noise as an argument, 6 / 8 two / three states)
int ssmq::marginal_filter_batch_device(const MarginalCall &c) {
    const int P = mg_args(c).P;
    return P == 4 ? mg_device<4, 4>(c) : P == 5 ? mg_device<5, 5>(c) : P == 6 ? mg_device<6, 6>(c) : P == 8 ? mg_device<8, 8>(c) : mg_device<16, 0>(c);
}
