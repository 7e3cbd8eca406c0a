"""
Times of Model.predict_batch (ssmq_gp_predict_batch: k_predict_fit + k_predict_test) on three shapes, and of the only route
there was before it - a Python loop of kernel.eval_inv_dot + kernel.eval per fit with NumPy einsum on the host.

  (a) B = 10 000 fits, D = E = 6, N = 13, M = 64       the optimize_batch -> predict_batch shape
  (b) B = 1, D = 1, N = 100, M = 100 000                a plotting grid
  (c) B = 256, D = 16, N = 128, M = 4 096               the top of the range (packed factorisation)

HIP events on the calling thread's stream around the whole call (uploads, both kernels, downloads: the entry point takes
host arrays); warm-up calls first, then the median and the spread of the timed calls.  The loop route is timed on LOOP_FITS
fits and scaled to B (it is linear in B: every fit is three synchronous library calls); it uses the library's existing entry
points only, so it is the same on the commit before predict existed.

Run:  python tools/predict_time.py [--out profiles/r09_predict_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib  # noqa: E402
from ssmtoybox_amd.bq.bqmod import GaussianProcessModel  # noqa: E402

CASES = (('a', 10000, 6, 6, 13, 64), ('b', 1, 1, 1, 100, 100000), ('c', 256, 16, 2, 128, 4096))
LOOP_FITS = 8


def timed(fn, warmup=3, reps=9):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = _lib.Event(), _lib.Event()
        e0.record()
        fn()
        e1.record()
        _lib.sync()
        ms.append(e0.elapsed_ms(e1))
    return np.median(ms), np.min(ms), np.max(ms)


def loop_route(m, xt, y, x, par, fits):
    t0 = time.perf_counter()
    for b in range(fits):
        iK = m.kernel.eval_inv_dot(par[b], x)
        kx = np.vstack([m.kernel.eval(par[b], xt[:, c:c + 4096], x) for c in range(0, xt.shape[1], 4096)])   # eval: <= 4096 points
        mean = kx.dot(iK).dot(y[b])
        var = par[b, 0] ** 2 - np.einsum('im,mn,ni->i', kx, iK, kx.T)
    return (time.perf_counter() - t0) * 1e3 / fits, mean, var


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    amd.set_device(0)
    rng = np.random.default_rng(9)
    lines = ['predict_batch on {}: HIP events around the whole call, median [min .. max] of 9 after 3 warm-up calls'.format(
        amd.device_name())]
    for name, B, D, E, N, M in CASES:
        m = GaussianProcessModel(D, np.ones((1, D + 1)), 'rbf', 'ut')
        x = rng.standard_normal((D, N)) if name != 'b' else np.sort(rng.uniform(-4, 4, (1, N)), axis=1)
        xt = 1.5 * rng.standard_normal((D, M))
        y = rng.standard_normal((B, N, E))
        ell = {'a': 2.0, 'b': 0.3, 'c': 3.0}[name]
        par = np.hstack((0.8 + 0.4 * rng.random((B, 1)), ell * (0.9 + 0.2 * rng.random((B, D)))))
        med, lo, hi = timed(lambda: m.predict_batch(xt, y, x, par=par))
        per_loop, mean, var = loop_route(m, xt, y, x, par, min(B, LOOP_FITS))
        r = m.predict_batch(xt, y[:1], x, par=par[:1])
        b = min(B, LOOP_FITS) - 1
        rb = m.predict_batch(xt, y[b:b + 1], x, par=par[b:b + 1])
        agree = max(np.abs(rb['mean'][0] - mean).max(), np.abs(rb['var'][0] - var).max())
        assert r['status'][0] == 0
        lines.append('({}) B {:6d} D {:2d} E {:2d} N {:3d} M {:6d}: {:9.3f} ms [{:.3f} .. {:.3f}]   loop route {:.3f} ms / fit on {} '
                     'fit(s) -> {:.1f} ms for B (scaled)   ratio {:.1f}   max |difference| {:.1e}'.format(
                         name, B, D, E, N, M, med, lo, hi, per_loop, min(B, LOOP_FITS), per_loop * B, per_loop * B / med, agree))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
