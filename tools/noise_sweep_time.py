#!/usr/bin/env python3
"""The noise sweep (one launch of k_noise_sweep over P rows x B sequences) against the route it replaces (P x: forward_pass_dev +
innovations_dev of a filter built with the row's process noise) on the same device-resident measurements:
`noise_sweep_time.py [ungm|ct] [P] [B] [T]`, UnscentedKalman on UNGM (P = 16, B = 1e4, T = 100) or on coordinated turn + four
bearings (P = 16, B = 1e4, T = 20).  Warm-up first, then the two routes alternate block by block, every block a few calls ended by a
device sync (both routes are host-synchronous as their users see them); medians over the blocks.  A run of its own, nothing else on
the device.  The two routes are also compared: largest |difference| of loglik_total relative to max(1, |value|)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else 'ungm'
P, B, T = (int(v) for v in (sys.argv[2:5] + ['16', '10000', '100' if which == 'ungm' else '20'][len(sys.argv[2:5]):]))
WARM, BLOCKS, REPS = 2, 7, {'sweep': 20, 'passes': 3}


def models(q_cov=None):
    if which == 'ungm':
        return (sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]) if q_cov is None else q_cov)),
                sm.UNGMMeasurement(sm.GaussRV(1), 1))
    m0 = np.array([130.0, 35.0, -20.0, 20.0, -4 * np.pi / 180])
    sensors = np.vstack((1000 * np.eye(2), -1000 * np.eye(2))).astype(float)
    return (sm.CoordinatedTurnTransition(sm.GaussRV(5, m0, np.diag([5.0, 5.0, 5.0, 5.0, 1e-4])),
                                         sm.GaussRV(5, cov=np.diag([0.1, 0.1, 0.1, 0.1, 1e-6]) if q_cov is None else q_cov)),
            sm.BearingMeasurement(sm.GaussRV(4, cov=1e-4 * np.eye(4)), 5, state_index=[0, 2], sensor_pos=sensors))


amd.set_device(0)
dyn, obs = models()
alg = ssinf.UnscentedKalman(dyn, obs)
q_rows = ssinf.noise_grid(alg.q_cov, np.geomspace(0.1, 10.0, P))
filters = [ssinf.UnscentedKalman(*models(q)) for q in q_rows]
d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=0)
print('device {}; {}: P = {}, B = {}, T = {}, ld = {}; sweep {}; two-call path {} | {}'.format(
    amd.device_name(), which, P, B, T, ld, alg.noise_sweep_kernel_name(P), filters[0].kernel_name(B), filters[0].innovations_kernel_name(B)))


def sweep(keep=False):
    bufs = alg.noise_sweep_dev(d_y, B, ld, T, q_cov=q_rows)
    tot = bufs[0].download((P, ld))[:, :B] if keep else None
    for buf in bufs:
        if buf is not None:
            buf.free()
    return tot


def passes(keep=False):
    tot = []
    for f in filters:
        d_fm, d_fP, d_st = f.forward_pass_dev(d_y, B, ld, T)
        bufs = f.innovations_dev(d_y, d_fm, d_fP, B, ld, T)
        if keep:
            tot.append(bufs[2].download((2, ld))[0, :B])
        for buf in (d_fm, d_fP, d_st) + tuple(bufs):
            buf.free()
    return np.stack(tot) if keep else None


a, b = sweep(True), passes(True)
print('largest |sweep - two-call| of loglik_total / max(1, |value|): {:.3g}; rows bit-equal: {} of {}'.format(
    float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)))), sum(bool(np.array_equal(a[p], b[p], equal_nan=True)) for p in range(P)), P))
for _ in range(WARM):
    sweep()
    passes()
blocks = {'sweep': [], 'passes': []}
for _ in range(BLOCKS):
    for name, fn in (('sweep', sweep), ('passes', passes)):
        _lib.sync()
        t0 = time.perf_counter()
        for _ in range(REPS[name]):
            fn()
        _lib.sync()
        blocks[name].append(1e3 * (time.perf_counter() - t0) / REPS[name])
med = {k: float(np.median(v)) for k, v in blocks.items()}
for name, label in (('sweep', 'noise_sweep_dev, one call'), ('passes', '{} x (forward_pass_dev + innovations_dev)'.format(P))):
    print('{:48s} median {:9.3f} ms   (blocks {:.3f} .. {:.3f})'.format(label, med[name], min(blocks[name]), max(blocks[name])))
print('two-call path / sweep: x {:.2f}'.format(med['passes'] / med['sweep']))
for buf in (d_x, d_y):
    buf.free()
