#!/usr/bin/env python3
"""Fixed part and per-step part of the headline pass (GPQ-Kalman on UNGM, B = 1e4, N = 3: one launch of k_filter_ungm_quad<3>):
HIP-event timed blocks of back-to-back passes at T = 2, 10, 26, 50, 100, 200 and the least-squares line time = a + b T through the
block medians - `a` is what a pass costs outside its time loop (launch, front and tail of the kernel), `b` a step.  The sweep is
repeated REPS times, each with its own fit, so the spread of a and b is on the page.  SSMQ_LIBRARY selects a library variant,
SSMQ_FUSED_QUAD=0/1 the kernel; `python tools/ungm_quad_tsweep.py once T` runs the T-step pass alone (for a kernel trace)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd                      # noqa: E402
from ssmtoybox_amd import _lib                   # noqa: E402
from bench import FilterBench                    # noqa: E402

B = int(os.environ.get('B', 10000))
STEPS = (2, 10, 26, 50, 100, 200)
REPS = int(os.environ.get('REPS', 5))
N = int(os.environ.get('N', 200))               # passes per timed block
lib = os.path.basename(os.environ.get('SSMQ_LIBRARY', 'libssmq.so'))


def block_us(wl, n):
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(n):
        wl.step()
    e1.record()
    _lib.sync()
    return e0.elapsed_ms(e1) * 1e3 / n


if len(sys.argv) > 2 and sys.argv[1] == 'once':
    T = int(sys.argv[2])
    wl = FilterBench(amd, B, T, 1, 'ungm', 'gpqkf')
    for _ in range(20):
        wl.step()
    _lib.sync()
    ts = [block_us(wl, N) for _ in range(5)]
    print('%s T=%d %s  event-to-event us/pass: median %.3f  blocks %s' % (lib, T, wl.kernel[-36:], float(np.median(ts)), ' '.join('%.3f' % t for t in ts)))
    sys.exit(0)

wls = {T: FilterBench(amd, B, T, 1, 'ungm', 'gpqkf') for T in STEPS}
for wl in wls.values():
    for _ in range(20):
        wl.step()
_lib.sync()
fits = []
for rep in range(REPS):
    med = []
    for T in STEPS:
        for _ in range(20):
            wls[T].step()
        med.append(float(np.median([block_us(wls[T], N) for _ in range(5)])))
    b, a = np.polyfit(np.array(STEPS, dtype=float), np.array(med), 1)
    res = np.array(med) - (a + b * np.array(STEPS))
    fits.append((a, b))
    print('%-22s rep %d  us/pass at T=%s: %s   a = %.3f us  b = %.4f us/step  residuals %s' % (
        lib, rep, '/'.join(map(str, STEPS)), ' '.join('%.3f' % m for m in med), a, b, ' '.join('%+.3f' % r for r in res)))
fa, fb = np.array(fits).T
print('%-22s %s  a: median %.3f min %.3f max %.3f us   b: median %.4f min %.4f max %.4f us/step' % (
    lib, wls[100].kernel[-36:], np.median(fa), fa.min(), fa.max(), np.median(fb), fb.min(), fb.max()))
