// Posterior Cramer-Rao sums (ssmq_pcrlb.hip: k_pcrlb_dyn<>, k_pcrlb_obs<>, k_pcrlb_rows; ssmq_rtc.hip: the _fn kernels of a user
// model; ssmq_api_pcrlb.hip: ssmq_pcrlb_sums_dev, ssmq_pcrlb_finalize): what the entry point hands the launchers.
#pragma once
#include "ssmq_host.h"

namespace ssmq {

constexpr int kPcrlbHostMaxD = 6, kPcrlbHostMaxY = 4;      // (= kPcrlbMaxD, kPcrlbMaxY of ssmq_pcrlb_kernel.h)

inline int pcrlb_sums_width(int D) { return D * (D + 1) + D * D; }
inline int64_t pcrlb_groups(int64_t B) { return (B + 255) / 256; }
// doubles of the workspace: the time table [T] (rounded up to 8), then the rows [T][nwg][D (D + 1) / 2 + D D] both kernels share
inline size_t pcrlb_ws_doubles(int D, int T, int64_t B) {
    return ((size_t)T + 7) / 8 * 8 + (size_t)T * (size_t)pcrlb_groups(B) * (size_t)(D * (D + 1) / 2 + D * D);
}

struct PcrlbLaunch {
    const ssmq_integrand *f_dyn, *f_obs;
    int D, Y, T, din_dyn, din_obs;
    int64_t B, ld;
    double Qi[kPcrlbHostMaxD * kPcrlbHostMaxD], Ri[kPcrlbHostMaxY * kPcrlbHostMaxY];      // [D][D], [Y][Y] row-major
    const double *x;       // device planes [T+1][D][ld]
    double *ws;            // device, pcrlb_ws_doubles(): its first T entries hold 0 .. T-1 already
    double *sums;          // device [T][pcrlb_sums_width(D)]
};
// both kernels and k_pcrlb_rows after each on stream s; names (each may be null) receive the kernels' names; dry_run: the names alone
// (nothing compiled, nothing launched, the buffers not read).  SSMQ_OK or < 0.
int launch_pcrlb(const PcrlbLaunch &h, hipStream_t s, const char **name_dyn, const char **name_obs, bool dry_run);
// whether ssmq_pcrlb.hip instantiates the built-in shape
bool pcrlb_builtin_dyn_shape(int D);
bool pcrlb_builtin_obs_shape(int D, int Y);
// smallest and largest eigenvalue of a symmetric n x n matrix, n <= 6 (ssmq_api_particle.hip)
void ps_eig_range(const double *A, int n, double *lo, double *hi);
// the _fn kernel of a user integrand (ssmq_rtc.hip); a: the argument block of the AOT launcher
struct PcrlbArgs;
int rtc_launch_pcrlb(bool dyn, const ssmq_integrand *f, const PcrlbArgs &a, unsigned grid, hipStream_t s, const char **name, bool dry_run);

}  // namespace ssmq
