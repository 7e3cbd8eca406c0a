// Bootstrap particle filter (ssmq_particle.hip: k_particle_filter<D>; ssmq_api_particle.hip: ssmq_particle_filter_dev): what the
// entry point hands the launcher.  Host arrays are padded to the kernel's fixed strides so that the kernel indexes them statically.
#pragma once
#include "ssmq_host.h"

namespace ssmq {

constexpr int kPfBlock = 256;          // threads per workgroup = per trajectory
constexpr int kPfMaxD = 6, kPfMaxY = 4, kPfMaxQ = 6;
constexpr int kPfMinN = 64, kPfMaxN = 4096;
constexpr int kPfCloudDoubles = 13312; // (2 D + 1) N: two [D][N] particle buffers and the [N] weights / CDF - 104 KB
constexpr int kPfRedDoubles = 96;      // reduction scratch: 4 wave partials of up to D (D + 1) / 2 = 21 sums, 4 scan totals

struct PfLaunch {
    const ssmq_integrand *f_dyn, *f_obs;
    int D, Y, dq, N, T, student;
    int64_t B, ld;
    uint64_t seed, traj_offset;
    double ess_threshold, lognorm, dof;                     // lognorm: the measurement density's log-normaliser
    double qm[kPfMaxQ], Lq[kPfMaxQ * kPfMaxQ], G[kPfMaxD * kPfMaxQ], rm[kPfMaxY], Lr[kPfMaxY * kPfMaxY];   // zero-padded; Lr: unit diagonal
    const double *y, *m0, *P0;
    double *fm, *fP, *ll, *ess;
    int32_t *status;
    double *part, *logw;
    int32_t *anc;
};

// N a multiple of 64 in 64 .. 4096 is the caller's check; D, Y, dq and the LDS budget are checked here
inline bool pf_shape_ok(int D, int Y, int dq, int N) {
    return D >= 1 && D <= kPfMaxD && Y >= 1 && Y <= kPfMaxY && dq >= 1 && dq <= kPfMaxQ && N <= kPfMaxN && (2 * D + 1) * N <= kPfCloudDoubles;
}
inline size_t pf_lds_bytes(int D, int N) { return sizeof(double) * ((size_t)(2 * D + 1) * N + kPfRedDoubles); }
int launch_particle_filter(const PfLaunch &h, hipStream_t s);

}  // namespace ssmq
