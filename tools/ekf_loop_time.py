#!/usr/bin/env python3
"""ExtendedKalman's forward pass on device-resident planes: the one-kernel pass (k_ekf_loop, csrc/ssmq_ekf_loop_kernel.h) against
the captured launch loop it replaces (SSMQ_NO_EKF_LOOP=1: k_linearize | k_linearize | k_kalman_update per step, 3 T launches) - and,
with --parent-lib, against the launch loop of another build of the library (the commit before the kernel), called through the C
ABI in the same process.  UNGM at B = 1e4, T = 100 (the configs[1] shape), where the fused GaussianProcessKalman pass - strictly
more arithmetic per step - is timed in the same run, and the pendulum at B = 1e5, T = 50.

ssmq_filter_forward_dev on planes that stay on the device; hipEvent timing around blocks of passes after a warm-up (code objects,
the captured graph, clocks); the routes alternate block by block and the median over the rounds is reported with the smallest and
the largest block, so that clock drift hits all routes alike and the run-to-run spread can be read next to the difference.

    python tools/ekf_loop_time.py [--parent-lib PATH] [--rounds N]     ->  one JSON line per shape (also the last lines of the output)"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402
from ssmtoybox_amd.mtran import resolve_integrand  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--parent-lib', default=None)
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--per-block', type=int, default=5)
opt = ap.parse_args()

amd.set_device(0)
lib = _lib.load()
parent = None
if opt.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(opt.parent_lib))
    for name, (res, args) in _lib._PROTOTYPES.items():
        if hasattr(parent, name):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = res, args
    assert parent.ssmq_version() == lib.ssmq_version()
    _lib.check(parent.ssmq_set_device(0), 'parent ssmq_set_device')


class Events:
    """A pair of hipEvents on the stream of library `l`."""

    def __init__(self, l):
        self.l, self.e = l, [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.e:
            _lib.check(l.ssmq_event_create(ctypes.byref(e)), 'ssmq_event_create')

    def record(self, i):
        _lib.check(self.l.ssmq_event_record(self.e[i]), 'ssmq_event_record')

    def ms(self):
        _lib.check(self.l.ssmq_sync(), 'ssmq_sync')
        out = ctypes.c_float(0)
        _lib.check(self.l.ssmq_event_elapsed_ms(self.e[0], self.e[1], ctypes.byref(out)), 'ssmq_event_elapsed_ms')
        return out.value


def ungm_models():
    return (sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), sm.UNGMMeasurement(sm.GaussRV(1), 1))


def pendulum_models():
    dt = 0.01
    q2 = sm.GaussRV(2, cov=0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]]))
    return (sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0]), cov=0.01 * np.eye(2)), q2, dt=dt),
            sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2))


results = []
for shape, models, B, T in (('UNGM', ungm_models, 10000, 100), ('pendulum', pendulum_models, 100000, 50)):
    dyn, obs = models()
    D, Y = dyn.dim_state, obs.dim_out
    ld = (B + 63) // 64 * 64
    y = obs.simulate_measurements(dyn.simulate_discrete(T, B, seed=1), seed=2)
    d_y = _lib.DeviceBuffer(8 * T * Y * ld)
    _lib.upload_study(y, Y, ld, d_y)
    ekf = ssinf.ExtendedKalman(dyn, obs)
    m0, P0 = np.zeros((D, ld)), np.zeros((D * D, ld))
    m0[:] = np.asarray(ekf.x0_mean, dtype=float).reshape(D, 1)
    P0[:] = np.asarray(ekf.x0_cov, dtype=float).reshape(D * D, 1)
    d_m0, d_P0 = _lib.DeviceBuffer(m0.nbytes), _lib.DeviceBuffer(P0.nbytes)
    d_m0.upload(m0)
    d_P0.upload(P0)
    gqg, pg = _lib.as_c(ekf.G.dot(ekf.q_cov).dot(ekf.G.T))
    rr, pr = _lib.as_c(ekf.r_cov)
    f_dyn, e_dyn = resolve_integrand(dyn.dyn_eval)
    f_obs, e_obs = resolve_integrand(obs.meas_eval)

    def route(l, h_dyn, h_obs, env):
        """One route: its own output planes (a captured loop is keyed by them), the library it runs in, the switch it runs under."""
        bufs = (_lib.DeviceBuffer(8 * T * D * ld), _lib.DeviceBuffer(8 * T * D * D * ld), _lib.DeviceBuffer(4 * ld))

        def run(n):
            if env:
                os.environ[env] = '1'
            for _ in range(n):
                _lib.check(l.ssmq_filter_forward_dev(ctypes.c_void_p(h_dyn), ctypes.byref(f_dyn), ctypes.c_void_p(h_obs), ctypes.byref(f_obs), B, ld, T,
                                                     ctypes.c_void_p(d_y.ptr), ctypes.c_void_p(d_m0.ptr), ctypes.c_void_p(d_P0.ptr), pg, pr,
                                                     ctypes.c_void_p(bufs[0].ptr), ctypes.c_void_p(bufs[1].ptr), ctypes.c_void_p(bufs[2].ptr)),
                           'ssmq_filter_forward_dev')
            if env:
                del os.environ[env]
        return {'run': run, 'ev': Events(l), 'bufs': bufs, 'ms': []}

    h_dyn, h_obs = ekf.tf_dyn._handle_for(e_dyn), ekf.tf_obs._handle_for(e_obs)
    routes = {'k_ekf_loop': route(lib, h_dyn, h_obs, None), 'launch_loop': route(lib, h_dyn, h_obs, 'SSMQ_NO_EKF_LOOP')}
    assert 'k_ekf_loop' in ekf.kernel_name(B), ekf.kernel_name(B)
    if parent is not None:
        parent.ssmq_transform_create_linear.restype = ctypes.c_void_p
        routes['parent_launch_loop'] = route(parent, parent.ssmq_transform_create_linear(D, D), parent.ssmq_transform_create_linear(D, Y), None)
    if shape == 'UNGM':
        par = np.array([[1.0, 3.0]])
        gpq = ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut')
        assert 'k_filter_' in gpq.kernel_name(B), gpq.kernel_name(B)      # (k_filter_fused, since 3.41 k_filter_ungm_quad)
        routes['gpq_kalman_fused'] = route(lib, gpq.tf_dyn._handle_for(e_dyn), gpq.tf_obs._handle_for(e_obs), None)
    for r in routes.values():          # warm-up: code objects, the captured loop, clocks
        r['run'](3)
    _lib.sync()
    if parent is not None:
        parent.ssmq_sync()
    for _ in range(opt.rounds):
        for r in routes.values():
            r['ev'].record(0)
            r['run'](opt.per_block)
            r['ev'].record(1)
            r['ms'].append(r['ev'].ms() / opt.per_block)
    # the routes filtered the same data: the one-kernel pass against the loops, norm-wise
    ref = [routes['k_ekf_loop']['bufs'][i].download((T * n * ld,)) for i, n in ((0, D), (1, D * D))]
    step_bytes = 8 * (Y + D + D * D)
    out = {'shape': shape, 'D': D, 'Y': Y, 'B': B, 'T': T, 'rounds': opt.rounds, 'passes_per_block': opt.per_block,
           'bytes_per_trajectory_step_fused': step_bytes}
    for k, r in routes.items():
        med, lo, hi = float(np.median(r['ms'])), min(r['ms']), max(r['ms'])
        out['us_' + k] = 1e3 * med
        out['us_' + k + '_min_max'] = [1e3 * lo, 1e3 * hi]
        line = '%s %s: B = %d, T = %d, %.1f us per pass (min %.1f, max %.1f)' % (shape, k, B, T, 1e3 * med, 1e3 * lo, 1e3 * hi)
        if 'loop' in k:
            got = [r['bufs'][i].download((T * n * ld,)) for i, n in ((0, D), (1, D * D))]
            dev = max(float(np.max(np.abs(g - f)) / np.max(np.abs(f))) for g, f in zip(got, ref))
            if k != 'k_ekf_loop':
                out['max_rel_dev_' + k] = dev
                line += ', largest norm-wise deviation from k_ekf_loop %.2g' % dev
        print(line, flush=True)
    fused = out['us_k_ekf_loop']
    out['gbps_fused'] = B * T * step_bytes / (fused * 1e-6) / 1e9
    out['ratio_launch_loop_over_fused'] = out['us_launch_loop'] / fused
    if parent is not None:
        out['ratio_parent_over_fused'] = out['us_parent_launch_loop'] / fused
        out['fused_faster_than_parent_beyond_spread'] = bool(out['us_k_ekf_loop_min_max'][1] < out['us_parent_launch_loop_min_max'][0])
    if 'us_gpq_kalman_fused' in out:
        out['ratio_fused_over_gpq_kalman'] = fused / out['us_gpq_kalman_fused']
    results.append(out)
    for r in routes.values():
        for b in r['bufs']:
            b.free()
    for b in (d_y, d_m0, d_P0):
        b.free()
for r in results:
    print(json.dumps(r), flush=True)
