// Counter-based random numbers shared by the device simulator (ssmq_simulate.hip) and the Monte-Carlo kernel expectations
// (ssmq_student_mc.hip): Philox4x32-10 (Salmon et al., SC'11; no state), keyed by the seed, counter = (index lo, index hi, step,
// tag).  Every draw is a pure function of (seed, index, step, tag), so results do not depend on the launch geometry.
#pragma once
#include "ssmq_device.h"

namespace ssmq {

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// two independent standard normals for (trajectory, step, purpose, pair)
__device__ __forceinline__ void normal_pair(uint64_t seed, uint64_t traj, uint32_t step, uint32_t tag, double *z0,
                                            double *z1) {
    uint32_t c[4] = {(uint32_t)traj, (uint32_t)(traj >> 32), step, tag};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    // 53-bit uniforms in (0, 1): 27 + 26 bits, offset by half a step
    const double u1 = ((double)(((uint64_t)(c[0] >> 5) << 26) | (uint64_t)(c[1] >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(((uint64_t)(c[2] >> 5) << 26) | (uint64_t)(c[3] >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    *z0 = r * cs;
    *z1 = r * sn;
}

// one 53-bit uniform in (0, 1) for (trajectory, step, tag)
__device__ __forceinline__ double uniform_one(uint64_t seed, uint64_t traj, uint32_t step, uint32_t tag) {
    uint32_t c[4] = {(uint32_t)traj, (uint32_t)(traj >> 32), step, tag};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ((double)(((uint64_t)(c[0] >> 5) << 26) | (uint64_t)(c[1] >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
}

// Gamma(shape, 1), shape >= 1 (Marsaglia & Tsang 2000): attempt t draws its normal from tag base + 0x100 + t and its
// uniform from tag base + 0x180 + t - counter-based, so the result is a pure function of (seed, trajectory, step, purpose).
// 16 attempts fail together with probability < 1e-20; the last candidate is then taken.
__device__ __forceinline__ double gamma_mt(uint64_t seed, uint64_t traj, uint32_t step, uint32_t base, double shape) {
    const double d = shape - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double v = 1.0;
    for (uint32_t t = 0; t < 16; ++t) {
        double x, unused;
        normal_pair(seed, traj, step, base | (0x100u + t), &x, &unused);
        const double u = uniform_one(seed, traj, step, base | (0x180u + t));
        const double w = 1.0 + c * x;
        v = w * w * w;
        if (v > 0.0 && log(u) < 0.5 * x * x + d - d * v + d * log(v)) break;
        v = fabs(v) > 0.0 ? fabs(v) : 1.0;
    }
    return d * v;
}

// The same sampler for callers whose tags keep other bits than gamma_mt's 0x100 / 0x180 (the particle kernels: tag = purpose << 28 |
// particle << 4 | pair, where 0x100 is particle 16): the two tag bases are given, their low four bits zero, and attempt t = 0 .. 15
// draws its normal from tag_normal | t and its uniform from tag_uniform | t.  Same arithmetic, same acceptance test, same fallback.
__device__ __forceinline__ double gamma_mt_tags(uint64_t seed, uint64_t traj, uint32_t step, uint32_t tag_normal, uint32_t tag_uniform,
                                                double shape) {
    const double d = shape - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double v = 1.0;
    for (uint32_t t = 0; t < 16; ++t) {
        double x, unused;
        normal_pair(seed, traj, step, tag_normal | t, &x, &unused);
        const double u = uniform_one(seed, traj, step, tag_uniform | t);
        const double w = 1.0 + c * x;
        v = w * w * w;
        if (v > 0.0 && log(u) < 0.5 * x * x + d - d * v + d * log(v)) break;
        v = fabs(v) > 0.0 ? fabs(v) : 1.0;
    }
    return d * v;
}

}  // namespace ssmq
