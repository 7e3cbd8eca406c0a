#!/usr/bin/env python3
"""ssmq_particle_smoother_dev (k_particle_smooth<D>, k_particle_lineage<D>; csrc/ssmq_particle_smooth.hip) on a cloud that is already
on the device, with the forward pass that writes the cloud (ssmq_particle_filter_dev with d_part, d_logw, d_anc) beside it as the scale:
UNGM at B = 256, T = 20 with N = 512 and 1024, and the coordinated turn (D = 5, full 5 x 5 Q) + radar at B = 256, T = 20 with N = 1024.

hipEvent timing around blocks of passes after a warm-up, every buffer allocated outside the timed blocks; the routes alternate block by
block and the median over the rounds is reported with the smallest and the largest block.  The marginal smoother evaluates
2 (T - 1) B N^2 exponentials per pass (two sweeps per step): the line also gives the time per pair and sweep.

    python tools/particle_smoother_time.py [--rounds N] [--per-block N]     ->  one JSON line per shape"""
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
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--per-block', type=int, default=2)
opt = ap.parse_args()

amd.set_device(0)
lib = _lib.load()


class Events:
    def __init__(self):
        self.e = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.e:
            _lib.check(lib.ssmq_event_create(ctypes.byref(e)), 'ssmq_event_create')

    def record(self, i):
        _lib.check(lib.ssmq_event_record(self.e[i]), 'ssmq_event_record')

    def ms(self):
        _lib.check(lib.ssmq_sync(), 'ssmq_sync')
        out = ctypes.c_float(0)
        _lib.check(lib.ssmq_event_elapsed_ms(self.e[0], self.e[1], ctypes.byref(out)), 'ssmq_event_elapsed_ms')
        return out.value


def ungm():
    return sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), sm.UNGMMeasurement(sm.GaussRV(1), 1)


def coordinated_turn():
    s = np.sqrt(np.array([0.05, 0.1, 0.05, 0.1, 0.002]))
    q = s[:, None] * 0.4 ** np.abs(np.subtract.outer(np.arange(5), np.arange(5))) * s[None, :]
    m0, P0 = np.array([10.0, 3.0, 5.0, -2.0, 0.3]), np.diag([1.0, 0.25, 1.0, 0.25, 0.01])
    dyn = sm.CoordinatedTurnTransition(sm.GaussRV(5, m0, P0), sm.GaussRV(5, cov=q), dt=0.2)
    return dyn, sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.array([[0.25, 1e-3], [1e-3, 4e-3]])), 5, state_index=[0, 2])


results = []
for shape, models, B, T, counts in (('UNGM', ungm, 256, 20, (512, 1024)), ('coordinated_turn_radar', coordinated_turn, 256, 20, (1024,))):
    dyn, obs = models()
    D = dyn.dim_state
    d_x, d_y, ld = sm.simulate_dev(dyn, obs, T, B, seed=1)
    routes = {}
    held = [d_x, d_y]
    stage = _lib.Staging()
    for N in counts:
        pf = ssinf.BootstrapParticleFilter(dyn, obs, num_particles=N, ess_threshold=0.5, seed=7)
        d_m0, d_P0 = pf._initial_planes(stage, B, ld)
        # every buffer of a pass is allocated once, outside the timed blocks: the figures are the launches alone
        o = dict(fm=8 * T * D * ld, fP=8 * T * D * D * ld, ll=8 * (T + 1) * ld, ess=8 * T * ld, st=4 * ld, sm=8 * T * D * ld,
                 sP=8 * T * D * D * ld, ess_s=8 * T * ld, unique=4 * T * ld, part=8 * T * D * B * N, logw=8 * T * B * N, anc=4 * T * B * N)
        o = {k: _lib.DeviceBuffer(v) for k, v in o.items()}
        held += list(o.values())
        o['st'].zero()
        f_dyn, f_obs, r, qm, qL, keep = pf._c_args()

        def run_filter(pf=pf, o=o, d_m0=d_m0, d_P0=d_P0):
            pf._launch(lib, B, ld, T, 0, d_y, d_m0, d_P0, o['fm'], o['fP'], o['ll'], o['ess'], o['st'], o['part'], o['logw'], o['anc'])

        def run_smoother(code, pf=pf, o=o, N=N, args=(f_dyn, qm, qL, keep)):
            vp, dp = _lib.vp, _lib.dp
            _lib.check(lib.ssmq_particle_smoother_dev(ctypes.byref(args[0]), D, args[1].size, N, B, ld, T, dp(args[1]), dp(args[2]), dp(pf.G),
                                                      code, vp(o['part']), vp(o['logw']), vp(o['anc']), vp(o['fm']), vp(o['fP']),
                                                      vp(o['ess']), vp(o['st']), vp(o['sm']), vp(o['sP']), vp(o['ess_s']), None, None,
                                                      vp(o['unique']) if code == 1 else None), 'ssmq_particle_smoother_dev')

        routes['filter_with_cloud_N%d' % N] = dict(run=run_filter, ev=Events(), ms=[], N=N)
        routes['marginal_N%d' % N] = dict(run=lambda f=run_smoother: f(0), ev=Events(), ms=[], N=N)
        routes['genealogy_N%d' % N] = dict(run=lambda f=run_smoother: f(1), ev=Events(), ms=[], N=N)
    for r in routes.values():        # warm-up; the filter of each N runs before its smoothers
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
        med = float(np.median(r['ms']))
        out['ms_' + k] = med
        out['ms_' + k + '_min_max'] = [min(r['ms']), max(r['ms'])]
        line = '%s %s: %.3f ms per pass (min %.3f, max %.3f)' % (shape, k, med, min(r['ms']), max(r['ms']))
        if k.startswith('marginal'):
            out['ns_per_pair_sweep_' + k] = med * 1e6 / (2.0 * (T - 1) * B * r['N'] ** 2)
            line += ', %.4f ns per pair and sweep' % out['ns_per_pair_sweep_' + k]
        print(line, flush=True)
    results.append(out)
    for b in held:
        b.free()
    stage.free()
for r in results:
    print(json.dumps(r), flush=True)
