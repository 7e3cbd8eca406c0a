// The scalar UNGM filter pass (BQ form, Gaussian recursion: GPQ-Kalman and the other BQ filters of SSMQ_SHAPES_UNGM; the headline,
// BASELINE configs[1]) with ONE TRAJECTORY ON THE FOUR LANES OF A QUAD, for batches whose waves each sit alone on a SIMD.  Such a
// wave is bound by the instructions it issues per step, and the one piece of a step that does the same work once per sigma point
// is the dynamics integrand x / 2 + 25 x / (1 + x^2) + 8 cos(1.2 k): ten instructions and a reciprocal per point.  Here lane q of a
// quad evaluates it at point q alone and the N values are broadcast to the quad (`v_mov_b32_dpp quad_perm:[n,n,n,n]`, two per
// double); from there every lane runs the sums, the measurement transform and the update of the one-lane kernel on a replicated
// state - QuadScalarPoints (ssmq_quad.h).  No partial sums, no all-reduce: every value comes from the same operations in the same
// order as in k_filter_fused<1, 1, N, N, ..., OPT = 0, STU = 0>, so the results are the same bits (tests/test_ungm_quad_gpu.py,
// tests/test_ungm_quad_scaffold_gpu.py).  All four lanes issue the step's two stores - same address, same bits: a store block
// predicated on the lane would end each step in a branch.  16 trajectories per wave: four times the waves of the one-lane kernel,
// taken while they still have a SIMD each (try_launch_quad).
//
// The kernel has its OWN TIME LOOP (UngmQuadPass below), not fused_pass<>: on a wave that pays one issue slot per instruction the
// step bookkeeping of the generic loop - a 64-bit plane offset multiplied out of the clamped step index, three 64-bit vector
// addresses rebuilt per step, the copy of the prefetched measurement - was a fifth of what the arithmetic costs.  D = Y = 1: y[k],
// fm[k] and fP[k] are planes of one pitch, so ONE 32-bit lane byte offset `vo` (8 b, + 8 ld per step) addresses all three against
// uniform bases (`global_load / global_store v, s[base:base+1]`; the measurement one plane ahead through the base y + 8 ld), and the
// time table is read at a scalar byte offset (+ 8 per step).  The last step is peeled - it requests nothing ahead, so no index is
// clamped - and the steps before it run two per trip with the measurement alternating between two registers.  The loop keeps no
// failure count: the status word is made behind it, from the last covariance and - on a failed trajectory - from the covariances
// the pass stored (first_nan_step).
#include "ssmq_filter_fused_kernel.h"

namespace ssmq {
namespace {

typedef const __attribute__((address_space(4))) char *cbyte_p;

// The first step k whose stored fP[k] is NaN, for a trajectory whose LAST one is (the cold tail of a failed trajectory; o: its
// byte offset in step 0's plane).  The planes are read back behind the wave's own stores (vmcnt(0)) - a wave's 16 trajectories
// are one 128-byte line of a plane, which no other wave writes or holds - with the pass's 32-bit offsets, by loads that go past
// the vector L1 (agent scope), kChunk requested back to back before the first is looked at.
__device__ __forceinline__ int32_t first_nan_step(const char *fP, uint32_t o, const uint32_t pitch, const int T) {
    constexpr int kChunk = 8;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int32_t last = T - 1;
    const uint32_t o_last = o + (uint32_t)last * pitch;
    int32_t first = last;
    for (int32_t k0 = 0; k0 < last && first == last; k0 += kChunk) {
        double v[kChunk];
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {     // (behind the last step: the last step's, a NaN that changes nothing)
            v[j] = __hip_atomic_load((const double *)(fP + (k0 + j < last ? o : o_last)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            o += pitch;
        }
#pragma unroll
        for (int j = kChunk - 1; j >= 0; --j) first = (v[j] != v[j] && k0 + j < first) ? k0 + j : first;
    }
    return first;
}

// The transform constants a step reads, REQUESTED ONCE at the top of the kernel and held in scalar registers for the whole pass:
// the dynamics' wm, Wc, emv and G Q G' (its points are dealt - QuadScalarPoints - and it forms no cross-covariance), the
// measurement's xi, wm, Wcc, Wc, emv and R.  moment_transform_core<> reads them as c[cl...] off the same uniform pointers; a
// constant-address-space load of an address already loaded HERE, above every branch of the kernel, is this value, so the loop
// and both peeled steps run on these registers and request nothing but their time-table entry.  Left to itself the compiler
// hoisted the loads into the loop's pre-header only - behind the waits for the initial state, a scalar-cache round trip of its
// own in front of the first step - and, the pre-header not being on the path of a pass of one or two steps, loaded everything
// again in each peeled step, with its waits inside the step's dependent chain.  hold() is where the values have to BE in
// registers: once behind the requests, once behind the loop (which keeps them live across it).
// N = 5 (37 + 46 constants) does not fit the scalar file and moves constants through lanes as it is: kHeld is false there and the
// kernel is what it was.
template <int N>
struct UngmQuadConsts {
    static constexpr bool kHeld = N <= 3;
    SBuf<N> wm_d, xi_o, wm_o, wcc_o;
    SBuf<N * N> wc_d, wc_o;
    SBuf<1> emv_d, add_d, emv_o, add_o;
    __device__ __forceinline__ void request(const CoreParams &cpd, const CoreParams &cpo) {
        constexpr ConstLayout cl = const_layout(1, 1, N, SSMQ_FORM_BQ);
        sload(wm_d, cpd.c + cl.wm);
        sload(wc_d, cpd.c + cl.Wc);
        sload(emv_d, cpd.c + cl.emv);
        sload(add_d, cpd.cadd);
        sload(xi_o, cpo.c + cl.xi);
        sload(wm_o, cpo.c + cl.wm);
        sload(wcc_o, cpo.c + cl.Wcc);
        sload(wc_o, cpo.c + cl.Wc);
        sload(emv_o, cpo.c + cl.emv);
        sload(add_o, cpo.cadd);
    }
    __device__ __forceinline__ void hold() const {
        spin(wm_d);
        spin(wc_d);
        spin(emv_d);
        spin(add_d);
        spin(xi_o);
        spin(wm_o);
        spin(wcc_o);
        spin(wc_o);
        spin(emv_o);
        spin(add_o);
    }
};

// The pass of one quad's trajectory.  step<AHEAD>() is the step of fused_pass<1, 1, N, N, UNGM_DYN, UNGM_MEAS, FORM_BQ, TP = 0,
// SELO = 0, OPT = 0, STU = 0> - the same calls and the same update lines on the same operands in the same order - around the
// addressing described above.  CENTRE: the measurement transform's first unit point is +0.0 (the host looked) and its point 0 is
// evaluated at the predictive mean itself (PointsPerLaneCentre, ssmq_apply_small.h) - the dynamics' points are dealt and gain nothing.
template <int N, bool CENTRE>
struct UngmQuadPass {
    CoreParams cpd, cpo;
    FPar fd, fo;
    QuadScalarPoints<N> qpts;
    const char *ynx;      // uniform: the measurement plane AFTER the one `vo` points into
    char *fm, *fP;        // uniform
    cbyte_p tt;           // uniform: the dynamics' time table
    uint32_t pitch;       // 8 ld
    uint32_t vo;          // lane: byte offset of this trajectory in the current step's planes
    uint32_t to;          // uniform: byte offset of the NEXT step's time-table entry
    double m[1], Pl[1];
    double tdn;           // the time-table entry of the step about to run

    // One step on the measurement ycur.  AHEAD: requests the next step's measurement into ynext and its time-table entry, and has
    // the measurement ARRIVE before the step's stores are issued (the one vmcnt wait of a step: behind the stores it would wait
    // for their acknowledgement as well).
    template <bool AHEAD>
    __device__ __forceinline__ void step(int k, const double ycur, double &ynext) {
        const double t = (double)k;   // (unused: the integrands take their time constant from tval)
        fd.tval = tdn;
        // the next step's offset, formed HERE and not behind the stores: the top of a step is one dependent chain (v_rsq, the
        // Newton steps, the integrand), and the hazard-aware scheduler puts this one independent add into the wait state behind
        // v_rsq_f64 that is an s_nop otherwise.  (N = 5: the second live offset costs more moves of constants than the slot.)
        constexpr bool kEarly = N <= 3;
        uint32_t vn = 0;
        if constexpr (kEarly) vn = vo + pitch;
        if constexpr (AHEAD) {
            ynext = *(const double *)(ynx + vo);
        }
        // ---- time update: predictive state moments, + G Q G' ----------------------------------------------------------------
        RegSinkNoCross<1, 1> pr;
        bool ok = moment_transform_core<1, 1, N, SSMQ_F_UNGM_DYN, SSMQ_FORM_BQ, 0, 0, false, 0>(m, Pl, t, fd, cpd, pr, qpts);
        if constexpr (AHEAD) {
            // the next entry of the time table is requested BEHIND the integrand that consumed this step's: scalar loads return
            // out of order, so the wait in front of that use is for all of them, a request just made included.  (One 128-bit
            // request per loop trip for both of its entries - half a load, a wait and an add less per step - was built and
            // measured 1.2 % SLOWER: profiles/r22_ungm_quad_centre.txt.)
            __builtin_amdgcn_sched_barrier(0);
            tdn = *(cdouble_p)(tt + to);
            to += 8;
        }
        // ---- predictive measurement moments, + R ------------------------------------------------------------------------------
        double L2[1] = {pr.cv[0]};
        RegSink<1, 1> ob;
        ok = moment_transform_core<1, 1, N, SSMQ_F_UNGM_MEAS, SSMQ_FORM_BQ, 0, 0, true, 0, RegSink<1, 1>>(pr.mf, L2, t, fo, cpo, ob,
                                                                                                          PointsPerLaneT<CENTRE>()) && ok;
        // ---- measurement update: the scalar lines of fused_pass (see there for the NaN that carries a failure) ----------------
        double S = ob.cv[0];
        int hi = __double2hiint(S);
        hi = (S > 0.0) ? hi : 0x7ff80000;
        S = __hiloint2double(hi, __double2loint(S));
        const double G = div_nr(ob.cx[0][0], S);
        double s = 0.0;
        s += G * (ycur - ob.mf[0]);
        m[0] = pr.mf[0] + s;
        double w = 0.0;
        w += G * ob.cv[0];
        double s2 = 0.0;
        s2 += w * G;
        double p = pr.cv[0] - s2;
        // (tied to the step's results: on its own the pin - and with it the wait - moves up to the request)
        if constexpr (AHEAD) asm volatile("" : "+v"(ynext), "+v"(m[0]), "+v"(p));
        SSMQ_STORE(*(double *)(fm + vo), m[0]);
        SSMQ_STORE(*(double *)(fP + vo), p);
        Pl[0] = p;
        vo = kEarly ? vn : vo + pitch;
    }
};

template <int N, bool CENTRE>
__global__ __launch_bounds__(kSmallBlock, 2) void k_filter_ungm_quad(const FusedArgs a) {
    const uint32_t b = blockIdx.x * kQuadTraj + (threadIdx.x >> 2);
    const int T = a.T;
    // every argument field the kernel reads, requested in ONE batch in front of the early-out (whose operands arrive with the
    // rest): one round trip to the argument segment where there were three dependent ones - B and T; the pointers behind the
    // branch; ld, the time table and the outputs behind the first loads
    if constexpr (UngmQuadConsts<N>::kHeld)
        asm volatile("" ::"s"(a.y), "s"(a.m0), "s"(a.P0), "s"(a.fm), "s"(a.fP), "s"(a.status), "s"(a.c_dyn), "s"(a.c_obs), "s"(a.gqg),
                     "s"(a.rr), "s"((uint32_t)a.B), "s"((uint32_t)a.ld), "s"(T), "s"(a.fd.ttab));
    // (host, try_launch_ungm_quad: T >= 1 and 8 ld T < 2^31, so B <= ld fits 32 bits with room to spare)
    if (b >= (uint32_t)a.B || T < 1) return;
    UngmQuadPass<N, CENTRE> u;
    u.cpd = CoreParams{(cdouble_p)a.c_dyn, (cdouble_p)a.gqg, a.emv_dyn, a.nu_dyn, 1.0, 1.0};
    u.cpo = CoreParams{(cdouble_p)a.c_obs, (cdouble_p)a.rr, a.emv_obs, a.nu_obs, 1.0, 1.0};
    u.fd = a.fd;
    u.fo = a.fo;
    u.fd.use_tval = 1;
    u.pitch = 8u * (uint32_t)a.ld;
    u.vo = 8u * b;
    u.to = 8;
    u.ynx = (const char *)a.y + u.pitch;
    u.fm = (char *)a.fm;
    u.fP = (char *)a.fP;
    u.tt = (cbyte_p)a.fd.ttab;                    // host: non-null
    u.m[0] = *(const double *)((const char *)a.m0 + u.vo);
    u.Pl[0] = *(const double *)((const char *)a.P0 + u.vo);
    double ya = *(const double *)((const char *)a.y + u.vo), yb;
    u.tdn = *(cdouble_p)u.tt;
    // ... and, in the same flight as the initial state, the first time-table entry and the lane's points, every constant of a step
    // (requested in FRONT of qpts.init, whose pin is a wait: behind it they would be a round trip of their own)
    UngmQuadConsts<N> cst;
    if constexpr (cst.kHeld) cst.request(u.cpd, u.cpo);
    u.qpts.init(u.cpd.c + const_layout(1, 1, N, SSMQ_FORM_BQ).xi, (int)(threadIdx.x & 3));
    if constexpr (cst.kHeld) {
        cst.hold();
        asm volatile("" ::"s"(u.tdn));
    }
    // everything requested so far has ARRIVED before the loop is entered (fused_pass: a load pending at the loop header leaves a
    // vmcnt(n > 0) in the body that waits for the previous step's stores)
    pin_v(u.m[0]);
    pin_v(u.Pl[0]);
    pin_v(ya);
    // T - 1 steps that request their successor's inputs - two per trip, the measurement alternating between ya and yb (no copy),
    // and an odd one after them - then the last step, which requests nothing.  The time-table offset counts the trips: from 8 by
    // 16 to 8 + 16 ((T - 1) / 2), which is 8 T for odd T and 8 (T - 1) for even T
    int k = 0;
#pragma unroll 1
    for (const uint32_t to_end = 8u * (uint32_t)((T - 1) | 1); u.to != to_end; k += 2) {
        u.template step<true>(k, ya, yb);
        u.template step<true>(k + 1, yb, ya);
    }
    if constexpr (cst.kHeld) cst.hold();
    if (!(T & 1)) {
        u.template step<true>(k++, ya, yb);
        ya = yb;
    }
    u.template step<false>(k, ya, yb);
    // status: 0, or 1 + the first step whose covariance is NaN.  Nothing in the loop counts: a NaN in p STAYS - Pl NaN -> v_rsq
    // NaN -> every point, sum and S of the next step NaN, and the poison select keeps a NaN S - so the last p tells whether the
    // trajectory failed, and where is read back from what it stored.
    int32_t status = 0;
    if (!(u.Pl[0] == u.Pl[0])) status = 1 + first_nan_step((const char *)a.fP, 8u * b, u.pitch, T);
    *(int32_t *)((char *)a.status + 4u * b) = status;
}

// k: the kernel for any points; k_centre: the one for a measurement transform whose first unit point is +0.0, or null.  N = 2, the
// 'sr' points, has no centre.  N = 5 keeps its body: without the centre's fma it is the same 579 instructions a trip - 3.5 VALU per
// step fewer, but 2 SALU moves of constants and 1.5 s_nop (4 wait states) more.  One name for both: they are the same pass.
typedef void (*ungm_quad_kernel)(const FusedArgs);
struct UngmQuadEntry {
    int N;
    ungm_quad_kernel k, k_centre;
    const char *name;
};
#define SSMQ_UQ_C(N) &k_filter_ungm_quad<N, true>
#define SSMQ_UQ(N, C) {N, &k_filter_ungm_quad<N, false>, C, "k_filter_ungm_quad<N=" #N ",SSMQ_FORM_BQ,TP=0>"}
const UngmQuadEntry kUngmQuad[] = {SSMQ_UQ(2, nullptr), SSMQ_UQ(3, SSMQ_UQ_C(3)), SSMQ_UQ(5, nullptr)};

// the bits of +0.0, not a comparison: -0.0 == 0.0 too, and a handle with that point keeps the body that multiplies by it
bool is_plus_zero(double v) {
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u == 0;
}

}  // namespace

// try_launch_quad's entry for the scalar UNGM shapes (its switches and its bound on the batch have been applied; the pass is
// Gaussian and same_family): 1 launched on `waves` blocks (dry_run: would be), 0 not this shape family, < 0 error.
int try_launch_ungm_quad(const FilterPass &p, int64_t waves) {
    const ssmq_transform *hd = p.hd, *ho = p.ho;
    if (p.fd->id != SSMQ_F_UNGM_DYN || p.fo->id != SSMQ_F_UNGM_MEAS || hd->D != 1 || hd->E != 1 || ho->D != 1 || ho->E != 1) return 0;
    if (hd->form != SSMQ_FORM_BQ || hd->tp_nu > 0.0 || ho->N != hd->N || p.sel_obs != 0) return 0;
    if (!p.ttab_dyn && !p.dry_run) return 0;          // the kernels read the time table
    // the kernels' byte offsets into y, fm and fP are 32-bit: passes of 8 ld T >= 2^31 bytes a plane set keep k_filter_fused (a name
    // query that gives no pitch and no step count - ld = T = 0 - is about the batch alone)
    if (p.ld >= ((int64_t)1 << 28) || 8 * p.ld * p.T >= ((int64_t)1 << 31)) return 0;
    if (p.T < 1 && !p.dry_run) return 0;
    for (const UngmQuadEntry &e : kUngmQuad) {
        if (e.N != hd->N) continue;
        if (p.name) *p.name = e.name;
        if (p.dry_run) return 1;
        FusedArgs a = fused_args(p);
        a.lpw = kQuadTraj;
        // the handle's own points, as uploaded (D = 1: xi[0] is the first): a centre of exactly +0.0 takes the body without its fma
        const bool centre = e.k_centre && !ho->xi.empty() && is_plus_zero(ho->xi[0]);
        hipLaunchKernelGGL(centre ? e.k_centre : e.k, dim3((unsigned)waves), dim3(kSmallBlock), 0, p.s, a);
        const int rc = hip_fail(hipGetLastError(), e.name);
        return rc ? rc : 1;
    }
    return 0;
}

}  // namespace ssmq
