#!/usr/bin/env python3
"""Two timings of the scoring recursion k_filter_score<> on device-resident UNGM measurements (`student_sweep_time.py [P] [B] [T]`,
default P = 32, B = 1e4, T = 100); a run of its own, nothing else on the device, every call ended by a device sync.
(1) The StudentProcessKalmanSweep likelihood sweep (one launch over P rows x B sequences, its two theta-batched weights calls included)
    against the two-call route for the same rows (P x forward_pass_dev + innovations_dev on filters constructed beforehand, and the P
    constructions), in the order A B B A: medians of blocks of repeated calls, both A blocks and both B blocks reported.
(2) `student_scores_dev` of a FullySymmetricStudent and of a StudentProcessStudent against `forward_pass_dev` (the fused Studentian
    pass, which stores every filtered moment) on the same data, A B B A as well; the ratio scores / forward is reported.
Wall-clock times of host-synchronous calls; kernel time alone is not profiled here."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402

P, B, T = (int(v) for v in (sys.argv[1:4] + ['32', '10000', '100'][len(sys.argv) - 1:]))
WARM, BLOCKS, REPS = 2, 3, 3


def median_ms(fn, warm=WARM):
    for _ in range(warm):
        fn()
    blocks = []
    for _ in range(BLOCKS):
        _lib.sync()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        _lib.sync()
        blocks.append(1e3 * (time.perf_counter() - t0) / REPS)
    return float(np.median(blocks))


def abba(a, b):
    """Medians in the order A B B A (the first A and B warmed up): (a1, b1, b2, a2)."""
    a1, b1 = median_ms(a), median_ms(b)
    b2, a2 = median_ms(b, 0), median_ms(a, 0)
    return a1, b1, b2, a2


def free(bufs):
    for buf in bufs:
        if buf is not None and hasattr(buf, 'free'):
            buf.free()


amd.set_device(0)
g = lambda cov=None: sm.GaussRV(1, cov=cov)      # noqa: E731
t4 = lambda scale=None: sm.StudentRV(1, scale=scale, dof=4.0)      # noqa: E731
dyn, obs = sm.UNGMTransition(g(), g(np.array([[10.0]]))), sm.UNGMMeasurement(g(), 1)
sdyn, sobs = sm.UNGMTransition(t4(), t4(np.array([[10.0]]))), sm.UNGMMeasurement(t4(), 1)
grid = ssinf.par_grid([1.0], np.geomspace(0.3, 100.0, P))
nu = np.where(np.arange(P) % 2 == 0, 3.0, 4.0)
alg = ssinf.StudentProcessKalmanSweep(dyn, obs, grid[:1], grid[:1], 'rbf', 'ut')
d_x, d_y, ld = sm.simulate_dev(sdyn, sobs, T, B, seed=0)
print('device {}; P = {}, B = {}, T = {}, ld = {}'.format(amd.device_name(), P, B, T, ld))
print('(1) sweep: {}'.format(alg.likelihood_sweep_kernel_name(P)))


def construct():
    out = []
    for p in range(P):
        f = ssinf.StudentProcessKalman(dyn, obs, grid[p:p + 1], grid[p:p + 1], 'rbf', 'ut')
        f.tf_dyn.model.nu = f.tf_obs.model.nu = float(nu[p])
        out.append(f)
    return out


filters = construct()
print('    two-call route: {} | {}'.format(filters[0].kernel_name(B), filters[0].innovations_kernel_name(B)))


def sweep():
    free(alg.likelihood_sweep_dev(d_y, B, ld, T, grid, grid, nu=nu)[:4])


def passes():
    for f in filters:
        d_fm, d_fP, d_st = f.forward_pass_dev(d_y, B, ld, T)
        free((d_fm, d_fP, d_st) + tuple(f.innovations_dev(d_y, d_fm, d_fP, B, ld, T)))


a1, b1, b2, a2 = abba(sweep, passes)
c = median_ms(construct, 1)
print('    sweep call (weights included)            A {:9.3f} ms ... A {:9.3f} ms'.format(a1, a2))
print('    {} x (forward_pass_dev + innovations_dev)  B {:9.3f} ms,  B {:9.3f} ms;  the {} constructions {:9.3f} ms'.format(P, b1, b2, P, c))
print('    two-call launches / sweep: x {:.2f};  with the constructions: x {:.2f}'.format((b1 + b2) / (a1 + a2), (b1 + b2 + 2 * c) / (a1 + a2)))

for name, f in (('FullySymmetricStudent', ssinf.FullySymmetricStudent(sdyn, sobs, degree=3)),
                ('StudentProcessStudent', ssinf.StudentProcessStudent(sdyn, sobs, np.array([[1.0, 3.0]]), np.array([[1.0, 3.0]])))):
    print('(2) {}: {} against {}'.format(name, f.student_scores_kernel_name(), f.kernel_name(B)))
    a1, b1, b2, a2 = abba(lambda: free(f.student_scores_dev(d_y, B, ld, T)), lambda: free(f.forward_pass_dev(d_y, B, ld, T)))
    print('    student_scores_dev A {:8.3f} ms ... A {:8.3f} ms;  forward_pass_dev B {:8.3f} ms, B {:8.3f} ms;  scores / forward = {:.2f}'.format(
        a1, a2, b1, b2, (a1 + a2) / (b1 + b2)))
free((d_x, d_y))
