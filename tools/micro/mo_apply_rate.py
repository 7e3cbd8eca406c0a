"""Times ssmq_apply_batch_dev for a multi-output GP handle (k_apply_mo) and for the single-output GP handle on the same inputs,
in one process: warm-up, then >= 100 launches timed one by one with events over rotated buffer sets, the median reported.

    python tools/micro/mo_apply_rate.py [--shape 6|5] [--batch 100000] [--launches 120]

Prints one JSON line per transform: time, algorithmic bytes per trajectory, share of 8 TB/s, and the ratio to the single-output
kernel of the same run.  Run each GPU step under its own time limit (timeout -k 10 300 python tools/micro/mo_apply_rate.py ...)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssmod as sm  # noqa: E402

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, default=6, choices=(5, 6))
    ap.add_argument('--batch', type=int, default=100000)
    ap.add_argument('--launches', type=int, default=120)
    ap.add_argument('--sets', type=int, default=4)
    a = ap.parse_args()
    D = E = a.shape
    model = sm.ReentryVehicle2DBiasTransition() if D == 6 else sm.ReentryVehicle2DTransition()
    f = model.dyn_eval
    rng = np.random.default_rng(0)
    par = np.column_stack((rng.uniform(0.5, 2.0, E), rng.uniform(1.0, 3.5, (E, D))))
    tfs = {'single-output': amd.GaussianProcessTransform(D, E, par[:1]),
           'multi-output': amd.MultiOutputGaussianProcessTransform(D, E, par)}
    B = a.batch
    m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932, 0.3][:D])
    s0 = np.array([1e-2, 1e-2, 1e-2, 1e-2, 0.3, 0.3][:D])
    sets = []
    for _ in range(a.sets):       # rotated so that no launch finds its inputs in cache from the one before
        mean = m0 + s0 * rng.standard_normal((B, D))
        A = 0.3 * s0[None, :, None] * rng.standard_normal((B, D, D))
        cov = A @ A.transpose(0, 2, 1) + 1e-3 * np.diag(s0 ** 2)
        sets.append((_lib.SoA.from_host(mean), _lib.SoA.from_host(cov), _lib.SoA(E, B), _lib.SoA(E * E, B), _lib.SoA(E * D, B),
                     _lib.DeviceBuffer(4 * ((B + 63) // 64 * 64))))
    time = _lib.DeviceBuffer(8)
    time.upload(np.zeros(1))
    nbytes = 8 * (D + D * D + E + E * E + E * D)
    base = None
    for name, tf in tfs.items():
        for k in range(10):
            mean, cov, mf, cf, cfx, st = sets[k % a.sets]
            tf.apply_batch_dev(f, mean, cov, time, mf, cf, cfx, st)
        _lib.sync()
        ms = []
        for k in range(a.launches):
            mean, cov, mf, cf, cfx, st = sets[k % a.sets]
            e0, e1 = _lib.Event(), _lib.Event()
            e0.record()
            tf.apply_batch_dev(f, mean, cov, time, mf, cf, cfx, st)
            e1.record()
            ms.append(e0.elapsed_ms(e1))
        t = float(np.median(ms)) * 1e-3
        base = t if base is None else base
        print(json.dumps({'transform': name, 'kernel': tf.kernel_name(f), 'D': D, 'E': E, 'N': 2 * D + 1, 'B': B,
                          'launches': a.launches, 'median_us': round(t * 1e6, 2), 'min_us': round(min(ms) * 1e3, 2),
                          'bytes_per_trajectory': nbytes, 'share_of_8TBps': round(B * nbytes / t / PEAK, 4),
                          'ratio_to_single_output': round(t / base, 3)}))


if __name__ == '__main__':
    main()
