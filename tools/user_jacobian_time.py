#!/usr/bin/env python3
"""The run-time compiled Jacobian kernels of user models (k_linearize_fn / k_taylor_gpqd_fn, csrc/ssmq_jacobian_kernel.h)
against the built-in kernels on device-resident planes, B = 1e6:

  pendulum 2-D          the built-in model restated as device_code + device_jacobian against k_linearize<2, 2> / k_taylor_gpqd<2, 2>
  constant velocity 4-D restated likewise, against k_linearize<4, 4> / k_taylor_gpqd<4, 4> and against the run-time-size bodies
                        <0, 0> (SSMQ_LINEAR_GENERIC / SSMQ_TAYLOR_GPQD_GENERIC) - the largest shape both routes can run: no built-in
                        model with a Jacobian is wider than that
  polynomial 6-D        a (D, E, DIN) = (6, 6, 6) user model, the shape the <0, 0> bodies would have been the only home of: rates alone

Time per launch and the HBM rate on the algorithmic bytes 8 (D + D^2 + E + E^2 + E D) per trajectory.  hipEvent timing around
blocks of launches after a warm-up; the launches rotate through buffer sets larger than the last-level cache; the variants
alternate block by block and the median over the rounds is reported (tools/taylor_gpqd_time.py).

    python tools/user_jacobian_time.py [B] [rounds]     ->  one JSON line per shape (also the last lines of the output)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssmod as sm  # noqa: E402

amd.set_device(0)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
PER_BLOCK = 12
CACHE_BYTES = 1 << 30          # rotate through at least this much: four times the last-level cache


class UserPendulum(sm.TransitionModel):
    dim_state, dim_noise, noise_additive = 2, 2, True
    device_code = 'o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]);'
    device_jacobian = 'double sn, cs; sincos_nr(x[0], &sn, &cs); J[0] = 1.0; J[1] = p[0]; J[ldj] = -9.81 * p[0] * cs; J[ldj + 1] = 1.0;'

    def _par(self):
        return (0.01,)


class UserCV(sm.TransitionModel):
    """ConstantVelocity with the Jacobian the reference returns for it (the transpose of the transition matrix)."""
    dim_state, dim_noise, noise_additive = 4, 4, True
    device_code = 'o[0] = x[0] + p[0] * x[1]; o[1] = x[1]; o[2] = x[2] + p[0] * x[3]; o[3] = x[3];'
    device_jacobian = 'for (int i = 0; i < 4; ++i) J[i * ldj + i] = 1.0; J[ldj] = p[0]; J[3 * ldj + 2] = p[0];'

    def _par(self):
        return (0.5,)


class UserPoly6(sm.TransitionModel):
    dim_state, dim_noise, noise_additive = 6, 6, True
    device_code = ' '.join('o[{e}] = sin_nr(x[{e}]) + 0.3*x[{b}]*x[{c}];'.format(e=e, b=(e + 1) % 6, c=(e + 2) % 6) for e in range(6))
    device_jacobian = ' '.join('{{ double sn, cs; sincos_nr(x[{e}], &sn, &cs); J[{e}*ldj + {e}] = cs; J[{e}*ldj + {b}] = 0.3*x[{c}]; '
                               'J[{e}*ldj + {c}] = 0.3*x[{b}]; }}'.format(e=e, b=(e + 1) % 6, c=(e + 2) % 6) for e in range(6))


CASES = (('pendulum 2-D', UserPendulum(sm.GaussRV(2), sm.GaussRV(2)), sm.Pendulum2DTransition(sm.GaussRV(2), sm.GaussRV(2), dt=0.01), False),
         ('constant velocity 4-D', UserCV(sm.GaussRV(4), sm.GaussRV(4)), sm.ConstantVelocity(sm.GaussRV(4), sm.GaussRV(2), dt=0.5), True),
         ('polynomial 6-D', UserPoly6(sm.GaussRV(6), sm.GaussRV(6)), None, False))
GENERIC = {'linearize': 'SSMQ_LINEAR_GENERIC', 'taylor_gpqd': 'SSMQ_TAYLOR_GPQD_GENERIC'}

results = []
for name, user, builtin, with_generic in CASES:
    D = E = user.dim_state
    tfs = {'linearize': amd.LinearizationTransform(D),
           'taylor_gpqd': amd.TaylorGPQDTransform(D, np.array([[1.5] + [2.0 + 0.5 * d for d in range(D)]]))}
    # variant -> (transform, integrand, switch to set while it is launched)
    variants = {}
    for k, tf in tfs.items():
        variants[k + ' user'] = (tf, user.dyn_eval, None)
        if builtin is not None:
            variants[k + ' built-in'] = (tf, builtin.dyn_eval, None)
            if with_generic:
                variants[k + ' built-in <0, 0>'] = (tf, builtin.dyn_eval, GENERIC[k])
    nbytes = 8.0 * B * (D + D * D + E + E * E + E * D)
    n_sets = max(2, int(np.ceil(CACHE_BYTES / nbytes)))
    rng = np.random.default_rng(1)
    means = rng.standard_normal((B, D))
    a = rng.standard_normal((B, D, D)) / np.sqrt(D)
    covs = np.einsum('bij,bkj->bik', a, a) + 0.2 * np.eye(D)
    sets = []
    for s in range(n_sets):
        mean, cov = _lib.SoA.from_host(means), _lib.SoA.from_host(covs)
        sets.append((mean, cov, _lib.SoA(E, B), _lib.SoA(E * E, B), _lib.SoA(E * D, B), _lib.DeviceBuffer(4 * mean.ld)))
    tbuf = _lib.DeviceBuffer(8)
    tbuf.upload(np.zeros(1))

    def block(variant, n, start):
        tf, f, switch = variant
        if switch:
            os.environ[switch] = '1'
        try:
            for i in range(n):
                mean, cov, mf, cf, cfx, st = sets[(start + i) % n_sets]
                tf.apply_batch_dev(f, mean, cov, tbuf, mf, cf, cfx, st, 0)
        finally:
            if switch:
                del os.environ[switch]

    for v in variants.values():          # warm-up: compiles, code objects, clocks
        block(v, 2 * n_sets, 0)
    _lib.sync()
    times = {k: [] for k in variants}
    for r in range(ROUNDS):
        for k, v in variants.items():
            e0, e1 = _lib.Event(), _lib.Event()
            e0.record()
            block(v, PER_BLOCK, r)
            e1.record()
            _lib.sync()
            times[k].append(e0.elapsed_ms(e1) / PER_BLOCK)
    med = {k: float(np.median(v)) for k, v in times.items()}
    row = {'shape': name, 'D': D, 'E': E, 'B': B, 'buffer_sets': n_sets}
    for k in variants:
        print('%s %s (%s): %.1f us per launch (min %.1f, max %.1f), %.0f GB/s on %d algorithmic bytes per trajectory' % (
            name, k, variants[k][0].kernel_name(variants[k][1]), 1e3 * med[k], 1e3 * min(times[k]), 1e3 * max(times[k]),
            nbytes / (med[k] * 1e-3) / 1e9, int(nbytes / B)), flush=True)
        row['us ' + k] = 1e3 * med[k]
        row['gbps ' + k] = nbytes / (med[k] * 1e-3) / 1e9
    for k in tfs:
        if builtin is not None:
            row['ratio ' + k + ' user / built-in'] = med[k + ' user'] / med[k + ' built-in']
        if with_generic:
            row['ratio ' + k + ' built-in <0, 0> / user'] = med[k + ' built-in <0, 0>'] / med[k + ' user']
    results.append(row)
    for s in sets:
        for b in s:
            (b.buf if hasattr(b, 'buf') else b).free()
    tbuf.free()
for r in results:
    print(json.dumps(r), flush=True)
