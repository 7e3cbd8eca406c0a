"""
ML-II fits per second: Model.optimize_batch on the device (one launch, one workgroup per fit) at B = 1, 1e3 and 1e4, for
  ut6    UT points at D = 6 (N = 13), E = 6 outputs;
  sc100  100 scattered points at D = 1, E = 1;
each fit with data of its own and a start of its own.  Wall time of the whole call (upload, launch, download), best of
three, after one warm-up call.
  python tools/ml2_time.py [OUT.json]                    device timings
  python tools/ml2_time.py --reference REF_ROOT [OUT]    the reference's model.optimize on the host (one SciPy call per fit),
                                                         for the same cases; REF_ROOT is a checkout of the reference
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cases(B, rng):
    out = {}
    # UT at D = 6: the reference's unit sigma points (kappa = 0 here, N = 2 D + 1 = 13)
    D = 6
    x = np.hstack([np.zeros((D, 1)), np.sqrt(D) * np.eye(D), -np.sqrt(D) * np.eye(D)])
    y = np.sin((x + 1.5) ** -1).T[None] + 0.05 * rng.standard_normal((B, x.shape[1], 6))
    out['ut6'] = (x, y, np.log([1.0] + [3.0] * D) + 0.1 * rng.standard_normal((B, D + 1)))
    x1 = np.sort(np.random.default_rng(1).uniform(-4, 4, (1, 100)), axis=1)
    y1 = np.sin(x1).T[None] + 0.05 * rng.standard_normal((B, 100, 1))
    out['sc100'] = (x1, y1, np.log([1.0, 0.5]) + 0.1 * rng.standard_normal((B, 2)))
    return out


def device(path):
    import ssmtoybox_amd as amd
    from ssmtoybox_amd.bq.bqmod import GaussianProcessModel
    amd.set_device(0)
    res = {'device': amd.device_name()}
    for B in (1, 1000, 10000):
        for name, (x, y, x0) in cases(B, np.random.default_rng(B)).items():
            m = GaussianProcessModel(x.shape[0], np.ones((1, x.shape[0] + 1)), 'rbf', 'ut')
            m.optimize_batch(x0, y, x)                          # warm-up (module load, allocations)
            best = np.inf
            for _ in range(3):
                t0 = time.perf_counter()
                r = m.optimize_batch(x0, y, x)
                best = min(best, time.perf_counter() - t0)
            res['{}_B{}'.format(name, B)] = {'seconds': best, 'fits_per_s': B / best, 'mean_nit': float(r['nit'].mean()),
                                             'mean_nfev': float(r['nfev'].mean()), 'max_nfev': int(r['nfev'].max()),
                                             'success': float(r['success'].mean())}
            print(name, B, json.dumps(res['{}_B{}'.format(name, B)]), flush=True)
    if path:
        with open(path, 'w') as f:
            json.dump(res, f, indent=1)


def reference(ref_root, path):
    import warnings
    sys.path.insert(0, ref_root)
    from tests.golden import make_golden  # noqa: F401  (import shims for the reference)
    from ssmtoybox.bq.bqmod import GaussianProcessModel
    res = {}
    B = 20
    for name, (x, y, x0) in cases(B, np.random.default_rng(B)).items():
        m = GaussianProcessModel(x.shape[0], np.ones((1, x.shape[0] + 1)), 'rbf', 'ut')
        t0 = time.perf_counter()
        nit, ok = [], 0
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for b in range(B):
                try:
                    r = m.optimize(x0[b], y[b], x)
                    nit.append(r.nit)
                    ok += 1
                except np.linalg.LinAlgError:
                    pass
        dt = time.perf_counter() - t0
        res['{}_reference'.format(name)] = {'fits': B, 'seconds': dt, 'fits_per_s': B / dt, 'mean_nit': float(np.mean(nit)),
                                            'completed': ok}
        print(name, json.dumps(res['{}_reference'.format(name)]), flush=True)
    if path:
        with open(path, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--reference':
        reference(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        device(sys.argv[1] if len(sys.argv) > 1 else None)
