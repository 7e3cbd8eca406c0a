// Innovation scores of a filter pass (ssmq_filter_innovations_dev): the dispatch table of k_innovation<> (ssmq_score_step.h) -
// every shape the fused time loop is instantiated for, one recursion-free launch over all T B items -, the scoring half on its
// own for the launch-loop route (k_innovation_score: reads the y_mean / P_y planes one step's transforms left) and the totals of
// every trajectory (k_innovation_total: ascending k, one lane per trajectory - a trajectory's bits do not depend on the batch).
#include <cstring>
#include "ssmq_score_step.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

template <int D, int Y, int ND, int NO, int FD, int FO, int FORM, int TP, int SELO, int OPT>
static hipError_t launch_innov(const InnovArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_innovation<D, Y, ND, NO, FD, FO, FORM, TP, SELO, OPT>), dim3((unsigned)a.T * (unsigned)a.nblk), dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*innov_fn)(const InnovArgs &, hipStream_t);
struct InnovEntry {
    FilterShape shape;
    innov_fn fn;
    const char *name;
};
#define SSMQ_INNOV_ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                                       \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT},                                                                    \
     &launch_innov<D, Y, N, N, FD, FO, FORM, TP, SELO, OPT>,                                                       \
     "k_innovation<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO "," #FORM ",TP=" #TP ",SELO=" #SELO ",OPT=" #OPT ">"}

// every shape of ssmq_filter_shapes.h, the fast paths as the fused time loop has them
static const InnovEntry kInnov[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, SSMQ_INNOV_ONE),
    SSMQ_SHAPES_MID(SSMQ_SHAPE, SSMQ_INNOV_ONE),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE_FAST, SSMQ_INNOV_ONE),
    SSMQ_SHAPES_HEAVY_SR(SSMQ_SHAPE, SSMQ_INNOV_ONE),
};

// 1-D grid of T ceil(B / 64) blocks
static bool innov_grid_ok(const FilterPass &p) { return ((p.B + kSmallBlock - 1) / kSmallBlock) * (int64_t)p.T < (int64_t)1 << 31; }

InnovArgs innov_args(const FilterPass &p, const InnovOut &o) {
    InnovArgs a;
    memset(&a, 0, sizeof(a));
    a.y = p.y; a.m0 = p.m0; a.P0 = p.P0; a.fm = p.fm; a.fP = p.fP;
    a.ymean = o.ymean; a.S = o.S; a.nis = o.nis; a.ll = o.ll;
    a.c_dyn = p.hd->d_small; a.c_obs = p.ho->d_small; a.gqg = p.gqg; a.rr = p.rr; a.B = p.B; a.ld = p.ld; a.T = p.T;
    a.emv_dyn = p.hd->emv_mode; a.emv_obs = p.ho->emv_mode; a.nu_dyn = p.hd->tp_nu; a.nu_obs = p.ho->tp_nu;
    a.nblk = (int32_t)((p.B + kSmallBlock - 1) / kSmallBlock);
    fill_fpar(p.fd, &a.fd);
    fill_fpar(p.fo, &a.fo);
    a.fd.ttab = p.ttab_dyn;
    a.fo.ttab = p.ttab_obs;
    return a;
}

// 1: launched (dry run: a kernel exists, its name set), 0: no one-launch kernel for this pair, < 0: error
int try_launch_innovation(const FilterPass &p, const InnovOut &o) {
    if (!p.dry_run && !innov_grid_ok(p)) {
        set_error("filter_innovations: T * ceil(B / 64) must stay below 2^31");
        return SSMQ_E_ARG;
    }
    if (is_user_integrand(p.fd) || is_user_integrand(p.fo)) return rtc_launch_innovation(p, o);
    if (!same_family(p)) return 0;
    for (const int opt : opt_preference(p.hd, p.ho))
    for (const InnovEntry &e : kInnov) {
        if (opt < 0) break;      // (no such variant for these handles: next opt)
        if (!(e.shape == shape_of(p, opt))) continue;
        if (has_time_table(p.fd->id) && !p.ttab_dyn && !p.dry_run) return 0;   // the kernels read the table
        if (p.name) *p.name = e.name;
        if (p.dry_run) return 1;
        const int rc = hip_fail(e.fn(innov_args(p, o), p.s), e.name);
        return rc ? rc : 1;
    }
    return 0;
}

// ---- the scoring half alone: one step, the planes the step's transforms wrote -------------------------------------------------
struct ScoreArgs {
    const double *y, *y_mean, *P_y;      // [Y][ld], [Y][ld], [Y*Y][ld] (lower triangle read)
    const double *m_in;                  // [D][ld]: the mean the step started from (NaN: the filter failed earlier)
    const int32_t *st_a, *st_b;          // [B]: nonzero = that transform's Cholesky failed
    double *ymean, *S;                   // [Y][ld], [Y*Y][ld] of this step, or null
    double *nis, *ll;                    // [ld] of this step
    int64_t B, ld;
    int32_t D, Y;
};

constexpr int kScoreBlock = 256;
constexpr int kScoreRegMaxY = 8;         // Y up to here: unrolled, in registers; above: run-time loops

template <int YT>
__global__ __launch_bounds__(kScoreBlock) void k_innovation_score(const ScoreArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
    if (b >= a.B) return;
    const int64_t ld = a.ld;
    const int Y = YT ? YT : a.Y;
    constexpr int YM = YT ? YT : SSMQ_MAX_DIM, UN = YT ? YT : 1;
    double e[YM], ym[YM], Sv[YM * (YM + 1) / 2], S[YM * (YM + 1) / 2], nis, ll;
    bool ok = a.st_a[b] == 0 && a.st_b[b] == 0;
    for (int d = 0; d < a.D; ++d) {
        const double v = a.m_in[d * ld + b];
        ok = ok && (v == v);
    }
#pragma unroll UN
    for (int i = 0; i < Y; ++i) {
        ym[i] = a.y_mean[i * ld + b];
        e[i] = a.y[i * ld + b] - ym[i];
#pragma unroll UN
        for (int j = 0; j <= i; ++j) S[SSMQ_PK(i, j)] = Sv[SSMQ_PK(i, j)] = a.P_y[((int64_t)i * Y + j) * ld + b];
    }
    ok = innovation_score<YT>(Y, e, S, nis, ll) && ok;
    const double nan = __builtin_nan("");
    a.nis[b] = ok ? nis : nan;
    a.ll[b] = ok ? ll : nan;
    if (a.ymean) {
#pragma unroll UN
        for (int i = 0; i < Y; ++i) a.ymean[i * ld + b] = ok ? ym[i] : nan;
    }
    if (a.S) {
#pragma unroll UN
        for (int i = 0; i < Y; ++i)
#pragma unroll UN
            for (int j = 0; j <= i; ++j) {
                const double v = ok ? Sv[SSMQ_PK(i, j)] : nan;   // both triangles from the one value
                a.S[((int64_t)i * Y + j) * ld + b] = v;
                if (j != i) a.S[((int64_t)j * Y + i) * ld + b] = v;
            }
    }
}

int launch_innovation_score(int D, int Y, int64_t B, int64_t ld, const double *y, const double *y_mean, const double *P_y,
                            const double *m_in, const int32_t *st_a, const int32_t *st_b, double *ymean, double *S, double *nis,
                            double *ll, hipStream_t s) {
    if (Y < 1 || Y > SSMQ_MAX_DIM || D < 1) {
        set_error("innovation_score: 1 <= Y <= " + std::to_string(SSMQ_MAX_DIM));
        return SSMQ_E_UNSUPPORTED;
    }
    const ScoreArgs a{y, y_mean, P_y, m_in, st_a, st_b, ymean, S, nis, ll, B, ld, D, Y};
    const dim3 grid((unsigned)((B + kScoreBlock - 1) / kScoreBlock)), block(kScoreBlock);
    switch (Y <= kScoreRegMaxY ? Y : 0) {
#define SSMQ_SCORE_CASE(YT) case YT: hipLaunchKernelGGL(k_innovation_score<YT>, grid, block, 0, s, a); break;
        SSMQ_SCORE_CASE(1) SSMQ_SCORE_CASE(2) SSMQ_SCORE_CASE(3) SSMQ_SCORE_CASE(4)
        SSMQ_SCORE_CASE(5) SSMQ_SCORE_CASE(6) SSMQ_SCORE_CASE(7) SSMQ_SCORE_CASE(8)
#undef SSMQ_SCORE_CASE
        default: hipLaunchKernelGGL(k_innovation_score<0>, grid, block, 0, s, a); break;
    }
    return hip_fail(hipGetLastError(), "k_innovation_score");
}

// ---- totals of every trajectory: ll_total = sum_k ll[k], nis_mean = sum_k nis[k] / T, both in ascending k; status = 1 + the first
// step whose scores are NaN (0: none) - found by this scan, the totals NaN from there on --------------------------------------
__global__ __launch_bounds__(kScoreBlock) void k_innovation_total(const double *nis, const double *ll, double *total, int32_t *status,
                                                                  int64_t B, int64_t ld, int T) {
    const int64_t b = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
    if (b >= B) return;
    double sl = 0.0, sn = 0.0;
    int32_t st = 0;
    for (int k = 0; k < T; ++k) {
        const double n = nis[(int64_t)k * ld + b], l = ll[(int64_t)k * ld + b];
        if (st == 0 && !(n == n && l == l)) st = k + 1;
        sl += l;
        sn += n;
    }
    total[b] = sl;
    total[ld + b] = sn / (double)T;
    status[b] = st;
}

int launch_innovation_total(int64_t B, int64_t ld, int T, const double *nis, const double *ll, double *total, int32_t *status,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_innovation_total, dim3((unsigned)((B + kScoreBlock - 1) / kScoreBlock)), dim3(kScoreBlock), 0, s, nis, ll, total,
                       status, B, ld, T);
    return hip_fail(hipGetLastError(), "k_innovation_total");
}

}  // namespace ssmq
