#!/usr/bin/env python3
"""The likelihood sweep (one launch of k_filter_sweep over P rows x B sequences) against the route it replaces (P x: construct the
filter, forward_pass_dev, innovations_dev) on the same device-resident UNGM measurements: P = 32, B = 1e4, T = 100 by default
(`sweep_time.py [P] [B] [T]`).  Warm-up first, then medians over blocks of repeated calls, every call ended by a device sync (both
routes are host-synchronous as their users see them); a run of its own, nothing else on the device.
Reported: (a) the sweep call with its two theta-batched weights calls, those weights calls alone, and the difference; (b) the P
constructions, and the P fused passes + innovation launches, separately."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402

P, B, T = (int(v) for v in (sys.argv[1:4] + ['32', '10000', '100'][len(sys.argv) - 1:]))
WARM, BLOCKS, REPS = 3, 5, 4


def median_ms(fn):
    for _ in range(WARM):
        fn()
    blocks = []
    for _ in range(BLOCKS):
        _lib.sync()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        _lib.sync()
        blocks.append(1e3 * (time.perf_counter() - t0) / REPS)
    return float(np.median(blocks)), float(min(blocks)), float(max(blocks))


amd.set_device(0)
dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
grid = ssinf.par_grid([1.0], np.geomspace(0.3, 100.0, P))
alg = ssinf.GaussianProcessKalman(dyn, obs, grid[:1], grid[:1], 'rbf', 'ut')
d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=0)
print('device {}; P = {}, B = {}, T = {}, ld = {}; {}'.format(amd.device_name(), P, B, T, ld, alg.likelihood_sweep_kernel_name(P)))


def sweep():
    for buf in alg.likelihood_sweep_dev(d_y, B, ld, T, grid, grid)[:4]:
        if buf is not None:
            buf.free()


def weights():
    alg.tf_dyn.model.bq_weights_batch(grid)
    alg.tf_obs.model.bq_weights_batch(grid)


def construct():
    return [ssinf.GaussianProcessKalman(dyn, obs, grid[p:p + 1], grid[p:p + 1], 'rbf', 'ut') for p in range(P)]


filters = construct()


def passes():
    for f in filters:
        d_fm, d_fP, d_st = f.forward_pass_dev(d_y, B, ld, T)
        bufs = f.innovations_dev(d_y, d_fm, d_fP, B, ld, T)
        for buf in (d_fm, d_fP, d_st) + tuple(bufs):
            buf.free()


res = {name: median_ms(fn) for name, fn in (('sweep call (weights included)', sweep), ('two theta-batched weights calls', weights),
                                            ('{} constructions'.format(P), construct), ('{} x (forward_pass_dev + innovations_dev)'.format(P), passes))}
for name, (med, lo, hi) in res.items():
    print('{:48s} median {:9.3f} ms   (blocks {:.3f} .. {:.3f})'.format(name, med, lo, hi))
a, w = res['sweep call (weights included)'][0], res['two theta-batched weights calls'][0]
c, q = res['{} constructions'.format(P)][0], res['{} x (forward_pass_dev + innovations_dev)'.format(P)][0]
print('sweep without its weights calls {:.3f} ms; parent route {:.3f} ms in all: x {:.2f} (launches alone x {:.2f})'.format(a - w, c + q, (c + q) / a, q / max(a - w, 1e-9)))
for buf in (d_x, d_y):
    buf.free()
