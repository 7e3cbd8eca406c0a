// Posterior Cramer-Rao sums for the built-in models: the instantiations of k_pcrlb_dyn<D, D> / k_pcrlb_obs<D, Y>
// (ssmq_pcrlb_kernel.h, where mapping and summation order are described) for the models that have a Jacobian (ssmq_device.h:
// jac_integrand) - transitions of D = 1 (UNGM), 2 (pendulum), 4 (constant velocity), 5 (coordinated turn), measurements with one
// output (UNGM, pendulum) on any state of D <= 6, reached through a state index or the reference's one-column broadcast, radar on
// D = 4, 5 and four bearings on D = 5 - and the launcher of both kernels of a pair; a user model's kernel is compiled for it at
// run time (ssmq_rtc.hip: rtc_launch_pcrlb).
#include "ssmq_pcrlb.h"
#include "ssmq_pcrlb_kernel.h"

namespace ssmq {

bool pcrlb_builtin_dyn_shape(int D) { return D == 1 || D == 2 || D == 4 || D == 5; }
bool pcrlb_builtin_obs_shape(int D, int Y) {
    return (D >= 1 && D <= kPcrlbMaxD && Y == 1) || ((D == 4 || D == 5) && Y == 2) || (D == 5 && Y == 4);
}

namespace {

// sums[j][off + q] = the rows (j, 0), (j, 1), .. of the workspace added in ascending order; one workgroup of 64 threads per step
// (N <= 57 sums)
struct PcrlbRowsArgs {
    const double *ws;             // [T][nwg][N]
    double *sums;                 // [T][S]
    int32_t nwg, N, S, off;
};
__global__ __launch_bounds__(64) void k_pcrlb_rows(const PcrlbRowsArgs a) {
    const int j = blockIdx.x, q = threadIdx.x;
    if (q >= a.N) return;
    const double *r = a.ws + (int64_t)j * a.nwg * a.N + q;
    double s = r[0];
    for (int g = 1; g < a.nwg; ++g) s += r[(int64_t)g * a.N];
    a.sums[(int64_t)j * a.S + a.off + q] = s;
}

template <int D>
void launch_dyn(const PcrlbArgs &a, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL((k_pcrlb_dyn<D, D>), dim3(grid), dim3(kPcrlbBlock), 0, s, a);
}
template <int D, int Y = 1>
void launch_obs(const PcrlbArgs &a, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL((k_pcrlb_obs<D, Y>), dim3(grid), dim3(kPcrlbBlock), 0, s, a);
}

// the argument block of one model's kernel; E: its outputs, W: Qi / Ri [E][E]
PcrlbArgs make_args(const PcrlbLaunch &h, const ssmq_integrand *f, int E, int din, const double *W) {
    PcrlbArgs a;
    memset(&a, 0, sizeof(a));
    a.lin.D = h.D; a.lin.E = E; a.lin.din = din; a.lin.fid = f->id;
    a.lin.bcast = (!is_user_integrand(f) && f->n_idx == 0 && din == 1 && h.D > 1) ? 1 : 0;
    a.lin.B = h.B; a.lin.ld = h.ld;
    fill_fpar(f, &a.lin.fp);
    a.x = h.x; a.steps = h.ws; a.ws = h.ws + ((size_t)h.T + 7) / 8 * 8;
    for (int i = 0; i < E * E; ++i) a.W[i] = W[i];
    a.T = h.T; a.nwg = (int32_t)pcrlb_groups(h.B);
    return a;
}

int launch_rows(const PcrlbArgs &a, int N, int S, int off, double *sums, hipStream_t s) {
    PcrlbRowsArgs r{a.ws, sums, a.nwg, N, S, off};
    hipLaunchKernelGGL(k_pcrlb_rows, dim3((unsigned)a.T), dim3(64), 0, s, r);
    return hip_fail(hipGetLastError(), "k_pcrlb_rows");
}

}  // namespace

int launch_pcrlb(const PcrlbLaunch &h, hipStream_t s, const char **name_dyn, const char **name_obs, bool dry_run) {
    const int D = h.D, Y = h.Y, tri = D * (D + 1) / 2, S = pcrlb_sums_width(D);
    const unsigned grid = (unsigned)((int64_t)h.T * pcrlb_groups(h.B));
    int rc;
    // the transition: F' Qi F and F
    PcrlbArgs a = make_args(h, h.f_dyn, D, h.din_dyn, h.Qi);
    if (is_user_integrand(h.f_dyn)) {
        if ((rc = rtc_launch_pcrlb(true, h.f_dyn, a, grid, s, name_dyn, dry_run))) return rc;
    } else {
        if (name_dyn) *name_dyn = "k_pcrlb_dyn";
        if (!dry_run) {
            if (D == 1) launch_dyn<1>(a, grid, s);
            else if (D == 2) launch_dyn<2>(a, grid, s);
            else if (D == 4) launch_dyn<4>(a, grid, s);
            else if (D == 5) launch_dyn<5>(a, grid, s);
            else {
                set_error("k_pcrlb_dyn: no instantiation for this built-in shape");
                return SSMQ_E_UNSUPPORTED;
            }
            if ((rc = hip_fail(hipGetLastError(), "k_pcrlb_dyn"))) return rc;
        }
    }
    if (!dry_run && (rc = launch_rows(a, tri + D * D, S, 0, h.sums, s))) return rc;
    // the measurement: H' Ri H (the rows of the workspace are free again: same stream)
    a = make_args(h, h.f_obs, Y, h.din_obs, h.Ri);
    if (is_user_integrand(h.f_obs)) {
        if ((rc = rtc_launch_pcrlb(false, h.f_obs, a, grid, s, name_obs, dry_run))) return rc;
    } else {
        if (name_obs) *name_obs = "k_pcrlb_obs";
        if (!dry_run) {
            if (!pcrlb_builtin_obs_shape(D, Y)) {
                set_error("k_pcrlb_obs: no instantiation for this built-in shape");
                return SSMQ_E_UNSUPPORTED;
            }
            if (Y == 2 && D == 4) launch_obs<4, 2>(a, grid, s);
            else if (Y == 2) launch_obs<5, 2>(a, grid, s);
            else if (Y == 4) launch_obs<5, 4>(a, grid, s);
            else switch (D) {
                case 1: launch_obs<1>(a, grid, s); break;
                case 2: launch_obs<2>(a, grid, s); break;
                case 3: launch_obs<3>(a, grid, s); break;
                case 4: launch_obs<4>(a, grid, s); break;
                case 5: launch_obs<5>(a, grid, s); break;
                default: launch_obs<6>(a, grid, s); break;
            }
            if ((rc = hip_fail(hipGetLastError(), "k_pcrlb_obs"))) return rc;
        }
    }
    if (!dry_run && (rc = launch_rows(a, tri, S, tri + D * D, h.sums, s))) return rc;
    return SSMQ_OK;
}

}  // namespace ssmq
