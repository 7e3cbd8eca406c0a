"""Timing record of the streaming Monte-Carlo transform (profiles/README.md, "mc transform"): reentry 5 -> 5,
n = 1e4 at B = 1e3 and n = 1e6 at B = 1, and beside them the sigma-point route of k_apply_big at n = 4096 on the same inputs.
Device-resident buffers, median wall time of 7 calls after 2 warm-up calls (each call ends with its results complete).

Run:  python tools/micro/mc_transform_time.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssmod  # noqa: E402


def run(tf, f, B, rng):
    D = 5
    mean = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932]) + 1e-3 * rng.standard_normal((B, D))
    a = rng.standard_normal((B, D, D)) * 1e-2
    cov = np.einsum('bij,bkj->bik', a, a) + 1e-6 * np.eye(D)
    d_m, d_c = _lib.SoA.from_host(mean), _lib.SoA.from_host(cov)
    d_t = _lib.DeviceBuffer(8)
    d_t.upload(np.zeros(1))
    d_mf, d_cf, d_cfx, d_st = _lib.SoA(D, B), _lib.SoA(D * D, B), _lib.SoA(D * D, B), _lib.DeviceBuffer(4 * d_m.ld)
    ts = []
    for it in range(9):
        _lib.sync()
        t0 = time.perf_counter()
        tf.apply_batch_dev(f, d_m, d_c, d_t, d_mf, d_cf, d_cfx, d_st)
        _lib.sync()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts[2:]))


def main():
    amd.set_device(0)
    rng = np.random.default_rng(0)
    f = ssmod.ReentryVehicle2DTransition(ssmod.GaussRV(5), ssmod.GaussRV(3)).dyn_eval
    rows = []
    for n, B in ((10 ** 4, 1000), (10 ** 6, 1), (4096, 1000), (4096, 1)):
        tf = amd.MonteCarloTransform(5, n, seed=1)
        rows.append(('k_mc_moments', n, B, run(tf, f, B, rng)))
    for B in (1000, 1):
        tf = amd.MonteCarloTransform(5, 4096)
        rows.append((tf.kernel_name(f), 4096, B, run(tf, f, B, rng)))
    for name, n, B, ms in rows:
        print('{:<16} n = {:>8} B = {:>5}: {:9.3f} ms  ({:.2f} ns per sample)'.format(name, n, B, ms, 1e6 * ms / (n * B)))


if __name__ == '__main__':
    main()
