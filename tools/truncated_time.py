#!/usr/bin/env python3
"""Two measurements of the truncated sigma-point path (csrc/ssmq_apply_trunc.hip), on one device:

1. k_apply_trunc (TruncatedUnscentedTransform(5, 2)) next to k_apply_small's plain unscented transform (UnscentedTransform(5)) on
   the radar measurement model (D = 5, E = 2) at B = 1e5, device-resident planes: time per launch and the fraction of the
   algorithmic HBM traffic 8 B (D + D^2 + 1 + E + E^2 + E D) bytes at 8 TB/s.  hipEvent timing around blocks of launches after a
   warm-up; the launches rotate through enough buffer sets that a set's planes have left the last-level cache before they are
   used again; the two kernels alternate block by block and the median over the rounds is reported.
2. TruncatedUnscentedKalman.forward_pass_dev (launch loop of 3 T launches) next to UnscentedKalman.forward_pass_dev (one fused
   kernel) on reentry-2D + radar, 1e4 trajectories x 50 steps, the same measurements: host clock around the call, which ends in a
   device synchronise; alternating, median.

    python tools/truncated_time.py [B] [rounds]     ->  JSON lines (also the last lines of the output)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402

amd.set_device(0)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
PER_BLOCK = 12
CACHE_BYTES = 1 << 30          # rotate through at least this much: four times the last-level cache
HBM_BYTES_PER_S = 8e12

M0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
D, E = 5, 2
obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-6])), 5)
f = obs.meas_eval
tfs = {'k_apply_small (UnscentedTransform(5))': amd.UnscentedTransform(D), 'k_apply_trunc (TruncatedUnscentedTransform(5, 2))': amd.TruncatedUnscentedTransform(D, 2)}
for k, tf in tfs.items():
    print(k, '->', tf.kernel_name(f), flush=True)
nbytes = 8.0 * B * (D + D * D + 1 + E + E * E + E * D)
n_sets = max(2, int(np.ceil(CACHE_BYTES / nbytes)))
rng = np.random.default_rng(1)
scale = np.array([1e-2, 1e-2, 1e-3, 1e-3, 0.5])
means = M0 + scale * rng.standard_normal((B, D))
a = rng.standard_normal((B, D, D)) / np.sqrt(D)
covs = (np.einsum('bij,bkj->bik', a, a) + 0.05 * np.eye(D)) * scale[:, None] * scale[None, :]
sets = []
for s in range(n_sets):
    mean, cov = _lib.SoA.from_host(means), _lib.SoA.from_host(covs)
    sets.append((mean, cov, _lib.SoA(E, B), _lib.SoA(E * E, B), _lib.SoA(E * D, B), _lib.DeviceBuffer(4 * mean.ld)))
tbuf = _lib.DeviceBuffer(8)
tbuf.upload(np.zeros(1))


def block(tf, n, start):
    for i in range(n):
        mean, cov, mf, cf, cfx, st = sets[(start + i) % n_sets]
        tf.apply_batch_dev(f, mean, cov, tbuf, mf, cf, cfx, st, 0)


for tf in tfs.values():          # warm-up: code objects, clocks
    block(tf, 2 * n_sets, 0)
_lib.sync()
times = {k: [] for k in tfs}
for r in range(ROUNDS):
    for k, tf in tfs.items():
        e0, e1 = _lib.Event(), _lib.Event()
        e0.record()
        block(tf, PER_BLOCK, r)
        e1.record()
        _lib.sync()
        times[k].append(e0.elapsed_ms(e1) / PER_BLOCK)
med = {k: float(np.median(v)) for k, v in times.items()}
kp, kt = list(tfs)
for k in tfs:
    print('%s: B = %d, %d buffer sets, %.1f us per launch (min %.1f, max %.1f), %.3f of the HBM floor (%d algorithmic bytes per item at 8 TB/s)' % (
        k, B, n_sets, 1e3 * med[k], 1e3 * min(times[k]), 1e3 * max(times[k]), nbytes / HBM_BYTES_PER_S / (med[k] * 1e-3), int(nbytes / B)), flush=True)
res1 = {'what': 'apply', 'D': D, 'D_eff': 2, 'E': E, 'B': B, 'buffer_sets': n_sets, 'us_plain': 1e3 * med[kp], 'us_trunc': 1e3 * med[kt],
        'ratio': med[kt] / med[kp], 'hbm_fraction_plain': nbytes / HBM_BYTES_PER_S / (med[kp] * 1e-3),
        'hbm_fraction_trunc': nbytes / HBM_BYTES_PER_S / (med[kt] * 1e-3)}
for s in sets:
    for b in s:
        (b.buf if hasattr(b, 'buf') else b).free()

# ---- the filters ---------------------------------------------------------------------------------------------------------
NB, T = 10000, 50
dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, M0, np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1])), sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6])))
x = dyn.simulate_discrete(T, 64)
y = obs.simulate_measurements(x)
ld = (NB + 63) // 64 * 64
yb = np.ascontiguousarray(np.tile(y.transpose(1, 0, 2), (1, 1, ld // 64)))
d_y = _lib.DeviceBuffer(yb.nbytes)
d_y.upload(yb)
algs = {'UnscentedKalman': ssinf.UnscentedKalman(dyn, obs), 'TruncatedUnscentedKalman': ssinf.TruncatedUnscentedKalman(dyn, obs)}
ftimes = {k: [] for k in algs}
for r in range(2 + ROUNDS):
    for k, alg in algs.items():
        t0 = time.perf_counter()
        bufs = alg.forward_pass_dev(d_y, NB, ld, T)
        dt = time.perf_counter() - t0
        if r == 0:
            st = bufs[2].download((ld,), dtype=np.int32)[:NB]
            print('%s: %s; %d of %d trajectories flagged' % (k, alg.kernel_name(NB), int(np.count_nonzero(st)), NB), flush=True)
        for b in bufs:
            b.free()
        if r >= 2:
            ftimes[k].append(dt)
fmed = {k: float(np.median(v)) for k, v in ftimes.items()}
for k in algs:
    print('%s.forward_pass_dev: %d x %d, %.2f ms (min %.2f, max %.2f)' % (k, NB, T, 1e3 * fmed[k], 1e3 * min(ftimes[k]), 1e3 * max(ftimes[k])), flush=True)
res2 = {'what': 'filter', 'B': NB, 'T': T, 'ms_ukf_fused': 1e3 * fmed['UnscentedKalman'], 'ms_truncated_loop': 1e3 * fmed['TruncatedUnscentedKalman'],
        'ratio': fmed['TruncatedUnscentedKalman'] / fmed['UnscentedKalman']}
print(json.dumps(res1), flush=True)
print(json.dumps(res2), flush=True)
