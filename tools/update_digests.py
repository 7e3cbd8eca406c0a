#!/usr/bin/env python3
"""One SHA-256 per output array (raw bytes, status included) of the three measurement-update variants of the Gaussian filters -
iterated posterior linearisation, outlier-robust, masked / gated - on the cases of their tests, for comparing two builds of
libssmq.so bit by bit (SSMQ_LIBRARY selects the library).  Each line also carries the kernel name the library reports.

  iterated   tests/test_iterated_gpu.py: every ONE_LAUNCH and LOOP case with J = 1 and J = 3; the launch-loop flag on the one-launch
             cases; a trajectory that starts from P0 = -I; cv_bearing4 of tests/test_masked_gpu.py (D = 4, Y = 4: k_iplf_update<0, 0>)
  robust     tests/test_robust_gpu.py: every ONE_LAUNCH and LOOP case with J = 1 and J = 4; the launch-loop flag; P0 = -I and a NaN
             measurement; cv_bearing4 (k_robust_update<0, 0>)
  masked     tests/test_masked_gpu.py: every ONE_LAUNCH and LOOP case (cv_bearing4: D = 4, Y = 4, the run-time shape <0, 0>) with the
             'pattern' and the 'random' mask plane; NaN as missing (no plane); the launch-loop flag; the gate cases of
             tests/_masked_oracle.py; P0 = -I and a NaN in an observed component
  t0         T = 0 through the three raw C entry points (the Python layer refuses it): the status plane alone is written

user_pend is the user pendulum pair, compiled at run time from the embedded source.  A one-off comparison tool, not an interface: it
imports the test modules for their case builders and reaches for the raw C entry points to get at T = 0; when those move it has to
move with them.

    python tools/update_digests.py > listing.txt"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib  # noqa: E402
from ssmtoybox_amd.mtran import resolve_integrand  # noqa: E402
from tests import _masked_oracle as mko  # noqa: E402
from tests import test_iterated_gpu as tit, test_robust_gpu as trb, test_masked_gpu as tmk  # noqa: E402
from tests.test_innovation_gpu import simulate  # noqa: E402

amd.set_device(0)
B = tit.B


def digests(case, kernel, out):
    for name in sorted(out):
        a = np.ascontiguousarray(out[name])
        print('%-44s %-10s %s  %s' % (case, name, hashlib.sha256(a.tobytes()).hexdigest(), kernel), flush=True)


def bad_p0(alg):
    D = alg.x0_cov.shape[0]
    P0 = np.broadcast_to(alg.x0_cov, (B, D, D)).copy()
    P0[37] = -np.eye(D)
    return P0


def bearing4():
    """The D = 4, Y = 4 pair no per-item kernel is instantiated for in registers, with measurements of its own."""
    alg = tmk.make_case('cv_bearing4')
    return alg, simulate(alg, B, tit.T, 3)


def iterated():
    def run(alg, y, J, **kw):
        fm, fP, delta = alg.iterated_pass_batch(y, J, raise_on_failure=False, return_delta=True, **kw)
        return dict(fm=fm, fP=fP, delta=delta, status=alg.status.copy())
    for name in tit.ONE_LAUNCH + tit.LOOP:
        alg, _, y = tit.case_data(name)
        for J in (1, 3):
            digests('iterated %s J=%d' % (name, J), alg.iterated_kernel_name(J), run(alg, y, J))
        if name in tit.ONE_LAUNCH and name != 'user_pend':
            for J in (1, 3):
                digests('iterated %s J=%d loop' % (name, J), alg.iterated_kernel_name(J, launch_loop=True), run(alg, y, J, launch_loop=True))
    for name in ('pend_gpqkf', 'cv_radar', 'pend_ghkf'):
        alg, _, y = tit.case_data(name)
        digests('iterated %s J=3 P0=-I' % name, alg.iterated_kernel_name(3), run(alg, y, 3, x0_cov=bad_p0(alg)))
    alg, y = bearing4()
    for J in (1, 3):
        digests('iterated cv_bearing4 J=%d' % J, alg.iterated_kernel_name(J), run(alg, y, J))


def robust():
    def run(alg, y, J, **kw):
        fm, fP, lam, delta = alg.robust_pass_batch(y, dof=trb.DOF, iterations=J, raise_on_failure=False, return_weights=True, **kw)
        return dict(fm=fm, fP=fP, lam=lam, delta=delta, status=alg.status.copy())
    for name in trb.ONE_LAUNCH + trb.LOOP:
        alg, _, y, _ = trb.case_data(name)
        for J in (1, 4):
            digests('robust %s J=%d' % (name, J), alg.robust_kernel_name(J), run(alg, y, J))
        if name in trb.ONE_LAUNCH and name != 'user_pend':
            for J in (1, 4):
                digests('robust %s J=%d loop' % (name, J), alg.robust_kernel_name(J, launch_loop=True), run(alg, y, J, launch_loop=True))
    for name in ('pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf'):
        alg, _, y, _ = trb.case_data(name)
        yn = y.copy()
        yn[0, 2, 11] = np.nan
        for J in (1, 4):
            digests('robust %s J=%d P0=-I, NaN y' % (name, J), alg.robust_kernel_name(J), run(alg, yn, J, x0_cov=bad_p0(alg)))
    alg, y = bearing4()
    for J in (1, 4):
        digests('robust cv_bearing4 J=%d' % J, alg.robust_kernel_name(J), run(alg, y, J))


def masked():
    def run(alg, y, mask, **kw):
        out = alg.masked_pass_batch(y, mask=mask, raise_on_failure=False, return_scores=True, **kw)
        return dict(fm=out['fm'], fP=out['fP'], used=out['used'], nis=out['nis'], ll=out['loglik'], status=alg.status.copy())
    for name in tmk.ONE_LAUNCH + tmk.LOOP:
        for kind in ('pattern', 'random'):
            alg, _, y, mask = tmk.case_data(name, kind)
            digests('masked %s %s' % (name, kind), alg.masked_kernel_name(), run(alg, y, mask))
            if name in tmk.ONE_LAUNCH and name != 'user_pend':
                digests('masked %s %s loop' % (name, kind), alg.masked_kernel_name(launch_loop=True), run(alg, y, mask, launch_loop=True))
        # NaN as missing: no plane, the cleared components hold NaN
        alg, _, y, mask = tmk.case_data(name, 'pattern')
        Y = y.shape[0]
        clear = ((mask[None, :, :] >> np.arange(Y)[:, None, None]) & 1) == 0
        digests('masked %s NaN=missing' % name, alg.masked_kernel_name(), run(alg, np.where(clear, np.nan, y), None))
        digests('masked %s pattern gate=inf' % name, alg.masked_kernel_name(), run(alg, y, mask, gate=np.inf))
    for name in mko.GATE_CASES:
        alg, y, mask, gate = mko.gate_case(name)
        digests('masked gate %s' % name, alg.masked_kernel_name(), run(alg, y, mask, gate=gate[1:]))
        digests('masked gate %s loop' % name, alg.masked_kernel_name(launch_loop=True), run(alg, y, mask, gate=gate[1:], launch_loop=True))
    for name in ('pend_gpqkf', 'cv_radar', 'ct_bearing', 'pend_ghkf'):
        alg, _, y, mask = tmk.case_data(name, 'pattern')
        yn = y.copy()
        yn[0, 2, int(np.flatnonzero(mask[2] & 1)[3])] = np.nan
        digests('masked %s P0=-I, NaN y' % name, alg.masked_kernel_name(), run(alg, yn, mask, x0_cov=bad_p0(alg)))


def t0():
    """T = 0 through the raw C entry points on the UNGM pair: SSMQ_OK, the status plane zeroed, nothing else touched."""
    lib = _lib.load()
    alg, _, _ = tit.case_data('ungm_ukf')
    ld, sent = 128, -7.0259e+211
    f_dyn, e_dyn = resolve_integrand(alg.mod_dyn.dyn_eval)
    f_obs, e_obs = resolve_integrand(alg.mod_obs.meas_eval)
    head = (ctypes.c_void_p(alg.tf_dyn._handle_for(e_dyn)), ctypes.byref(f_dyn), ctypes.c_void_p(alg.tf_obs._handle_for(e_obs)),
            ctypes.byref(f_obs), B, ld, 0)
    gqg, pg = _lib.as_c(alg.G.dot(alg.q_cov).dot(alg.G.T))      # (the arrays stay alive next to their pointers)
    rr, pr = _lib.as_c(alg.r_cov)
    plane = np.full((1, ld), sent)
    bufs = [_lib.DeviceBuffer(plane.nbytes) for _ in range(9)]      # y, m0, P0 and up to six outputs
    vp = [ctypes.c_void_p(b.ptr) for b in bufs]
    calls = (('iterated', lambda: lib.ssmq_filter_iterated_dev(*head, 2, 0, vp[0], vp[1], vp[2], pg, pr, vp[3], vp[4], vp[5], vp[8])),
             ('robust', lambda: lib.ssmq_filter_robust_dev(*head, 2, 0, vp[0], vp[1], vp[2], pg, pr, ctypes.c_double(4.0), vp[3], vp[4], vp[5],
                                                           vp[6], vp[8])),
             ('masked', lambda: lib.ssmq_filter_masked_dev(*head, 0, vp[0], None, vp[1], vp[2], pg, pr, None, vp[3], vp[4], vp[5], vp[6], vp[7],
                                                           vp[8])))
    for what, call in calls:
        for b in bufs:
            b.upload(plane)
        rc = call()
        _lib.sync()
        digests('t0 %s rc=%d' % (what, rc), '-', {'out%d' % i: bufs[i].download(plane.shape) for i in range(3, 9)})
    for b in bufs:
        b.free()


if __name__ == '__main__':
    iterated()
    robust()
    masked()
    t0()
