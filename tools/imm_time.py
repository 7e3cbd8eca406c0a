#!/usr/bin/env python3
"""The IMM pass over M noise modes (one launch of k_imm_loop) next to two references on the same device-resident measurements:
`noise_sweep_dev` with P = M rows - the same filter arithmetic without coupling and without moment stores - and M x
`forward_pass_dev` - what a host-coupled IMM would at least cost.  `imm_time.py [ungm|ct] [M] [B] [T]`: UnscentedKalman on UNGM
(M = 4, B = 1e4, T = 100) or on coordinated turn + four bearings (M = 2, B = 1e4, T = 20).  Warm-up first, then the three routes
alternate block by block, every block a few calls ended by a device sync (all three are host-synchronous as their users see them);
medians over the blocks.  A run of its own, nothing else on the device."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else 'ungm'
M, B, T = (int(v) for v in (sys.argv[2:5] + ['4' if which == 'ungm' else '2', '10000', '100' if which == 'ungm' else '20'][len(sys.argv[2:5]):]))
WARM, BLOCKS, REPS = 2, 7, {'imm': 10, 'sweep': 10, 'passes': 5}


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
q_rows = ssinf.noise_grid(alg.q_cov, np.geomspace(0.3, 3.0, M))
pi = ssinf.mode_transition(M, 0.95)
filters = [ssinf.UnscentedKalman(*models(q)) for q in q_rows]
d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=0)
print('device {}; {}: M = {}, B = {}, T = {}, ld = {}; imm {}; sweep {}; forward pass {}'.format(
    amd.device_name(), which, M, B, T, ld, alg.imm_kernel_name(M), alg.noise_sweep_kernel_name(M), filters[0].kernel_name(B)))


def free(bufs):
    for buf in bufs:
        if buf is not None:
            buf.free()


def imm():
    free(alg.imm_pass_dev(d_y, B, ld, T, pi, q_cov=q_rows))


def sweep():
    free(alg.noise_sweep_dev(d_y, B, ld, T, q_cov=q_rows))


def passes():
    for f in filters:
        free(f.forward_pass_dev(d_y, B, ld, T))


bufs = alg.imm_pass_dev(d_y, B, ld, T, pi, q_cov=q_rows)
st = bufs[5].download((ld,), dtype=np.int32)[:B]
print('imm: {} of {} trajectories failed; mean final mode probabilities {}'.format(
    int(np.count_nonzero(st)), B, np.nanmean(bufs[2].download((T, M, ld))[-1, :, :B], axis=1)))
free(bufs)
routes = (('imm', imm), ('sweep', sweep), ('passes', passes))
for _ in range(WARM):
    for _, fn in routes:
        fn()
blocks = {name: [] for name, _ in routes}
for _ in range(BLOCKS):
    for name, fn in routes:
        _lib.sync()
        t0 = time.perf_counter()
        for _ in range(REPS[name]):
            fn()
        _lib.sync()
        blocks[name].append(1e3 * (time.perf_counter() - t0) / REPS[name])
med = {k: float(np.median(v)) for k, v in blocks.items()}
for name, label in (('imm', 'imm_pass_dev, one call'), ('sweep', 'noise_sweep_dev with P = {}, one call'.format(M)),
                    ('passes', '{} x forward_pass_dev'.format(M))):
    print('{:48s} median {:9.3f} ms   (blocks {:.3f} .. {:.3f})'.format(label, med[name], min(blocks[name]), max(blocks[name])))
print('imm / noise sweep: x {:.2f};  imm / M forward passes: x {:.2f}'.format(med['imm'] / med['sweep'], med['imm'] / med['passes']))
free((d_x, d_y))
