#!/usr/bin/env python3
"""Wall clock of the five-state scoring kernels that the other timing tools do not reach - the BQ, t-process and sigma-point
instantiations of k_noise_sweep, k_imm_loop and k_filter_sweep on the reentry vehicle (D = 5, Y = 2) and on coordinated turn + four
bearings (D = 5, Y = 4), unscented (N = 11) and spherical-radial (N = 10) points - for comparing two builds of libssmq.so
(SSMQ_LIBRARY selects the library): `score_step_time.py [B] [T]`, B = 10 000 sequences, T = 20 steps, P = 8 noise rows / kernel
parameter rows, M = 2 modes.  Per case two warm-up calls, then 7 blocks of 10 host-synchronous calls on device-resident
measurements, each block ended by a device sync; median and spread of the blocks."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402

B, T = (int(v) for v in (sys.argv[1:3] + ['10000', '20'][len(sys.argv) - 1:]))
P, M, BLOCKS, REPS = 8, 2, 7, 10


def models(which):
    if which == 'reentry':
        m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
        return (sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1.0])),
                                              sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6]))),
                sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-3 ** 2])), 5, radar_loc=np.array([6374.0, 0.0])))
    m0 = np.array([130.0, 35.0, -20.0, 20.0, -4 * np.pi / 180])
    sensors = np.vstack((1000 * np.eye(2), -1000 * np.eye(2))).astype(float)
    return (sm.CoordinatedTurnTransition(sm.GaussRV(5, m0, np.diag([5.0, 5.0, 5.0, 5.0, 1e-4])), sm.GaussRV(5, cov=np.diag([0.1, 0.1, 0.1, 0.1, 1e-6]))),
            sm.BearingMeasurement(sm.GaussRV(4, cov=1e-4 * np.eye(4)), 5, state_index=[0, 2], sensor_pos=sensors))


def make(which, kind, pts):
    dyn, obs = models(which)
    par = np.array([[1.0] + [3.0] * 5])
    if kind == 'sigma':
        return (ssinf.UnscentedKalman if pts == 'ut' else ssinf.CubatureKalman)(dyn, obs)
    if kind == 'gp':
        return ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', pts)
    return ssinf.StudentProcessKalman(dyn, obs, par, par, 'rbf', pts, nu=4.0)


def free(bufs):
    for buf in bufs:
        if buf is not None and hasattr(buf, 'free'):
            buf.free()


def timed(fn):
    for _ in range(2):
        fn()
    blocks = []
    for _ in range(BLOCKS):
        _lib.sync()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        _lib.sync()
        blocks.append(1e3 * (time.perf_counter() - t0) / REPS)
    return float(np.median(blocks)), min(blocks), max(blocks)


amd.set_device(0)
print('device {}; B = {}, T = {}, P = {}, M = {}'.format(amd.device_name(), B, T, P, M))
data = {}
for which in ('reentry', 'ct'):
    dyn, obs = models(which)
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=0)
    d_x.free()
    data[which] = d_y
CASES = [('noise', 'reentry', 'tp', 'sr'), ('noise', 'reentry', 'tp', 'ut'), ('noise', 'ct', 'gp', 'sr'), ('noise', 'ct', 'gp', 'ut'),
         ('noise', 'ct', 'tp', 'sr'), ('noise', 'ct', 'tp', 'ut'), ('imm', 'reentry', 'sigma', 'sr'), ('imm', 'reentry', 'sigma', 'ut'),
         ('imm', 'ct', 'tp', 'sr'), ('imm', 'ct', 'sigma', 'sr'), ('imm', 'ct', 'sigma', 'ut'), ('sweep', 'ct', 'gp', 'sr'), ('sweep', 'ct', 'gp', 'ut')]
for entry, which, kind, pts in CASES:
    alg, d_y = make(which, kind, pts), data[which]
    if entry == 'noise':
        rows = ssinf.noise_grid(alg.q_cov, np.geomspace(0.3, 3.0, P))
        name, fn = alg.noise_sweep_kernel_name(P), lambda: free(alg.noise_sweep_dev(d_y, B, ld, T, q_cov=rows))
    elif entry == 'imm':
        rows, pi = ssinf.noise_grid(alg.q_cov, np.geomspace(0.3, 3.0, M)), ssinf.mode_transition(M, 0.95)
        name, fn = alg.imm_kernel_name(M), lambda: free(alg.imm_pass_dev(d_y, B, ld, T, pi, q_cov=rows))
    else:
        grid = np.hstack((np.ones((P, 1)), np.geomspace(2.0, 10.0, P)[:, None] * np.ones((1, 5))))
        name, fn = alg.likelihood_sweep_kernel_name(P), lambda: free(alg.likelihood_sweep_dev(d_y, B, ld, T, grid, grid)[:4])
    med, lo, hi = timed(fn)
    print('{:5s} {:7s} {:5s} {}  median {:8.3f} ms  (blocks {:.3f} .. {:.3f})  {}'.format(entry, which, kind, pts, med, lo, hi, name), flush=True)
for d_y in data.values():
    d_y.free()
