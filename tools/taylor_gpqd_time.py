#!/usr/bin/env python3
"""k_taylor_gpqd (TaylorGPQDTransform, csrc/ssmq_jacobian_kernel.h) against k_linearize (LinearizationTransform) on device-resident
planes: time per launch, the HBM rate on the algorithmic bytes 8 (D + D^2 + E + E^2 + E D) per trajectory and the ratio of the
two, for the pendulum dynamics (D = E = 2) and the constant-velocity model (D = E = 4) at B = 1e6.

hipEvent timing around blocks of launches after a warm-up; the launches rotate through enough buffer sets that a set's planes
have left the 256 MB last-level cache before they are used again; the two kernels alternate block by block and the median
over the rounds is reported, so that clock drift hits both alike.

    python tools/taylor_gpqd_time.py [B] [rounds]     ->  one JSON line per shape (also the last lines of the output)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssmod as sm  # noqa: E402

amd.set_device(0)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
PER_BLOCK = 12
CACHE_BYTES = 1 << 30          # rotate through at least this much: four times the last-level cache

results = []
for name, mod in (('pendulum 2-D', sm.Pendulum2DTransition(sm.GaussRV(2), sm.GaussRV(2), dt=0.01)),
                  ('constant velocity 4-D', sm.ConstantVelocity(sm.GaussRV(4), sm.GaussRV(2), dt=0.5))):
    D, E = mod.dim_in, mod.dim_state
    f = mod.dyn_eval
    tfs = {'k_linearize': amd.LinearizationTransform(D),
           'k_taylor_gpqd': amd.TaylorGPQDTransform(D, np.array([[1.5] + [2.0 + 0.5 * d for d in range(D)]]))}
    nbytes = 8.0 * B * (D + D * D + E + E * E + E * D)
    n_sets = max(2, int(np.ceil(CACHE_BYTES / nbytes)))
    rng = np.random.default_rng(1)
    means = rng.standard_normal((B, D))
    a = rng.standard_normal((B, D, D)) / np.sqrt(D)
    covs = np.einsum('bij,bkj->bik', a, a) + 0.2 * np.eye(D)
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
    for k in tfs:
        print('%s %s: B = %d, %d buffer sets, %.1f us per launch (min %.1f, max %.1f), %.0f GB/s on %d algorithmic bytes per trajectory' % (
            name, k, B, n_sets, 1e3 * med[k], 1e3 * min(times[k]), 1e3 * max(times[k]), nbytes / (med[k] * 1e-3) / 1e9, int(nbytes / B)),
            flush=True)
    results.append({'shape': name, 'D': D, 'E': E, 'B': B, 'buffer_sets': n_sets, 'us_linearize': 1e3 * med['k_linearize'],
                    'us_taylor_gpqd': 1e3 * med['k_taylor_gpqd'], 'ratio': med['k_taylor_gpqd'] / med['k_linearize'],
                    'gbps_taylor_gpqd': nbytes / (med['k_taylor_gpqd'] * 1e-3) / 1e9})
    for s in sets:
        for b in s:
            (b.buf if hasattr(b, 'buf') else b).free()
for r in results:
    print(json.dumps(r), flush=True)
