"""
Time of one 'rbf-student' weights construction (GaussianProcessModel.bq_weights with an RBFStudent kernel: ssmq_rbf_student_expect
+ ssmq_rbf_student_kxy + ssmq_weights_gp_given) at the default 2e6 samples, on two shapes:

  (a) D = 5, fully-symmetric degree-5 points N = 51, ell = 3
  (b) D = 1, fully-symmetric degree-3 points N = 3, ell = 1

HIP events on the calling thread's stream around the whole call (uploads, every kernel, downloads: the entry points take host
arrays) and around its three parts; warm-up calls first, then the median and the spread of the timed calls.  The executed flop
of the matrix-core kernel are those of the 16 x 16 tiles it forms (tiles below the diagonal of Q are skipped): 2 * 256 * tiles
* num_samples rounded up to whole chunks of 64; its own time comes from a kernel trace (rocprofv3 --kernel-trace --stats), this
script gives the enclosing entry point's.

Run:  python tools/student_mc_time.py [--out profiles/r10_student_mc_time.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib  # noqa: E402
from ssmtoybox_amd.bq.bqmod import GaussianProcessModel  # noqa: E402

CASES = (('a', 5, 3.0, 5), ('b', 1, 1.0, 3))


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


def tiles(D, N):
    nt, et = (N + 15) // 16, (1 + D + 15) // 16
    return nt * (nt + 1) // 2 + et * nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert amd.device_count() >= 1
    amd.set_device(0)
    lines = ['device: {}'.format(amd.device_name())]
    for tag, D, ell, deg in CASES:
        par = np.array([[1.0] + [ell] * D])
        m = GaussianProcessModel(D, par, 'rbf-student', 'fs', {'degree': deg})
        k, x = m.kernel, m.points
        N, S = x.shape[1], k.num_samples
        whole = timed(lambda: m.bq_weights(par))
        expect = timed(lambda: k.expectations(par, x))
        kxy = timed(lambda: k.exp_xy_kxy(par))
        flop = 2.0 * 256 * tiles(D, N) * ((S + 63) // 64 * 64)
        lines.append('({}) D = {} N = {} S = {:.0e}: bq_weights {:.3f} ms (min {:.3f}, max {:.3f}); expectations {:.3f} ms '
                     '(min {:.3f}, max {:.3f}); exp_xy_kxy {:.3f} ms (min {:.3f}, max {:.3f}); executed matrix-core flop of '
                     'k_student_expect {:.3e}'.format(tag, D, N, S, *whole, *expect, *kxy, flop))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
