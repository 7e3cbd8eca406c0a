#!/usr/bin/env python3
"""BootstrapParticleFilter.forward_pass_dev (k_particle_filter<D>, csrc/ssmq_particle.hip) on device-resident planes, with the
UnscentedKalman's forward_pass_dev on the same data beside it as the scale: UNGM at B = 1e4, T = 100 with N = 256 and 1024, and the
reentry 5-D + radar pair at B = 1e4, T = 50 with N = 1024.  With --variant NAME=PATH (repeatable) the same passes run in another build
of the library as well, called through the C ABI in the same process - e.g. csrc/ssmq_particle.hip compiled with -DSSMQ_PF_NO_RNG
(no Philox / Box-Muller) or -DSSMQ_PF_NO_MODEL (no model evaluations), which is how the time is split; ess_threshold = 0 against 1
gives the cost of the resampling itself.  --heavy adds the Student-t passes (k_particle_filter<D, QK=1>): the UNGM of the README's
heavy-tailed example (StudentRV initial state, process noise of scale 10 and measurement noise, dof 4) at the UNGM shapes and the
pendulum with Student-t process noise (dof 3) at B = 1e4, T = 100, N = 1024, each at ess_threshold = 0.5; a variant library that lacks
the *_rv entry points (a build of an earlier commit) is skipped for them.

hipEvent timing around blocks of passes after a warm-up, every buffer allocated outside the timed blocks; the routes alternate block by
block and the median over the rounds is reported with the smallest and the largest block.  The variants
(tools/build_variant.sh NAME "-DSSMQ_PF_NO_RNG" ssmq_particle.hip) run at ess_threshold = 0.5.

    python tools/particle_time.py [--variant NAME=PATH ...] [--rounds N] [--heavy]     ->  one JSON line per shape"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--variant', action='append', default=[])
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--per-block', type=int, default=2)
ap.add_argument('--heavy', action='store_true')
ap.add_argument('--shapes', default='', help='comma-separated shape names to run (default: all)')
opt = ap.parse_args()

amd.set_device(0)
lib = _lib.load()
variants = {}
for spec in opt.variant:
    name, path = spec.split('=', 1)
    v = ctypes.CDLL(os.path.abspath(path))
    for fn_name, (res, args) in _lib._PROTOTYPES.items():
        if hasattr(v, fn_name):
            fn = getattr(v, fn_name)
            fn.restype, fn.argtypes = res, args
    _lib.check(v.ssmq_set_device(0), 'variant ssmq_set_device')
    variants[name] = v


class Events:
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


def ungm():
    return sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), sm.UNGMMeasurement(sm.GaussRV(1), 1)


def reentry():
    m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
    P0 = np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1.0])
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, P0), sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6])), dt=0.1)
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-6])), 5, state_index=[0, 1], radar_loc=[6374.0, 0.0])
    return dyn, obs


def ungm_t():
    return (sm.UNGMTransition(sm.StudentRV(1, dof=4.0), sm.StudentRV(1, scale=np.array([[10.0]]), dof=4.0)),
            sm.UNGMMeasurement(sm.StudentRV(1, dof=4.0), 1))


def pendulum_t():
    dt = 0.01
    q = 0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]])
    return (sm.Pendulum2DTransition(sm.GaussRV(2, np.array([1.0, 0.0]), 0.05 * np.eye(2)), sm.StudentRV(2, scale=q, dof=3.0), dt=dt),
            sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.002]])), 2))


SHAPES = [('UNGM', ungm, 10000, 100, (256, 1024)), ('reentry5_radar', reentry, 10000, 50, (1024,))]
if opt.heavy:
    SHAPES += [('UNGM_t', ungm_t, 10000, 100, (256, 1024)), ('pendulum_t', pendulum_t, 10000, 100, (1024,))]
if opt.shapes:
    SHAPES = [s for s in SHAPES if s[0] in opt.shapes.split(',')]

results = []
for shape, models, B, T, counts in SHAPES:
    dyn, obs = models()
    D = dyn.dim_state
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=1)
    heavy = shape.endswith('_t')
    # the scale beside it: the UKF, the Studentian filter for the all-Student UNGM, none for a pair that mixes GaussRV and StudentRV
    from ssmtoybox_amd.ssmod import StudentRV
    all_t = all(isinstance(rv, StudentRV) for rv in (dyn.init_rv, dyn.noise_rv, obs.noise_rv))
    ukf = (ssinf.FullySymmetricStudent(dyn, obs, dof=4.0) if all_t else None) if heavy else ssinf.UnscentedKalman(dyn, obs)
    routes = {}

    def add(name, fn, l):
        routes[name] = {'run': fn, 'ev': Events(l), 'ms': []}

    # every buffer of a pass is allocated once, outside the timed blocks: the figures are the launches alone
    outs = [_lib.DeviceBuffer(8 * T * D * ld), _lib.DeviceBuffer(8 * T * D * D * ld), _lib.DeviceBuffer(8 * (T + 1) * ld),
            _lib.DeviceBuffer(8 * T * ld), _lib.DeviceBuffer(4 * ld)]
    stage = _lib.Staging()
    d_m0, d_P0 = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=counts[0])._initial_planes(stage, B, ld)

    def run_ukf():
        ukf._launch(lib, B, ld, T, d_y, d_m0, d_P0, outs[0], outs[1], outs[4])
    if ukf is not None:
        add('ukf', run_ukf, lib)
    for N in counts:
        for thr in ((0.5,) if heavy else (0.5, 0.0, 1.0)):
            pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=thr, seed=7)
            for vname, vlib in [('', lib)] + (list(variants.items()) if thr == 0.5 else []):
                if heavy and not hasattr(vlib, 'ssmq_particle_filter_rv_dev'):
                    continue
                def run_pf(pf=pf, vlib=vlib):
                    pf._launch(vlib, B, ld, T, 0, d_y, d_m0, d_P0, outs[0], outs[1], outs[2], outs[3], outs[4])
                add('pf_N%d_ess%g%s' % (N, thr, '_' + vname if vname else ''), run_pf, vlib)
    for r in routes.values():
        r['run']()
    _lib.sync()
    for _ in range(opt.rounds):
        for r in routes.values():
            r['ev'].record(0)
            for _ in range(opt.per_block):
                r['run']()
            r['ev'].record(1)
            r['ms'].append(r['ev'].ms() / opt.per_block)
    out = {'shape': shape, 'D': D, 'B': B, 'T': T, 'rounds': opt.rounds, 'passes_per_block': opt.per_block}
    for k, r in routes.items():
        out['ms_' + k] = float(np.median(r['ms']))
        out['ms_' + k + '_min_max'] = [min(r['ms']), max(r['ms'])]
        print('%s %s: %.3f ms per pass (min %.3f, max %.3f)' % (shape, k, out['ms_' + k], min(r['ms']), max(r['ms'])), flush=True)
    results.append(out)
    for b in outs + [d_x, d_y]:
        b.free()
    stage.free()
for r in results:
    print(json.dumps(r), flush=True)
