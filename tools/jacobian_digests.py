#!/usr/bin/env python3
"""One SHA-256 per output array of the linearisation and the Taylor-GPQD transform (mean_f, cov_f, cov_fx, status, and for
Taylor-GPQD the per-item model_var / integ_var) through apply_batch, for comparing two builds of libssmq.so bit by bit
(SSMQ_LIBRARY selects the library):

  g21       every block and parameter row of tests/golden/g21_taylor_gpqd.npz (Taylor-GPQD)
  linear    the eight models of test_linearization_transform_golden on its batch of 3000 (linearisation)
  index     the two state-index cases of test_state_index_against_the_oracle (Taylor-GPQD, B = 193)
  user      the user models of tests/test_user_jacobian_gpu.py: the pendulum restated, Van der Pol, shapes (3,2,3), (6,4,5), (6,6,6)
            (both transforms)

each as routed, under SSMQ_LINEAR_GENERIC=1 and under SSMQ_TAYLOR_GPQD_GENERIC=1.

    python tools/jacobian_digests.py > listing.txt"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import ssmod  # noqa: E402
from tests import _taylor_oracle as to, _user_jac_oracle as uo, _jacobian_cases as jc  # noqa: E402

amd.set_device(0)
NAMES = ('mean_f', 'cov_f', 'cov_fx', 'status', 'model_var', 'integ_var')


def digests(case, tf, f, mean, cov, time):
    kw = {'return_variances': True} if isinstance(tf, amd.TaylorGPQDTransform) else {}
    for route, switch in (('routed', None), ('linear-generic', 'SSMQ_LINEAR_GENERIC'), ('taylor-generic', 'SSMQ_TAYLOR_GPQD_GENERIC')):
        if switch:
            os.environ[switch] = '1'
        try:
            out = tf.apply_batch(f, mean, cov, time, return_status=True, **kw)
        finally:
            if switch:
                del os.environ[switch]
        for name, arr in zip(NAMES, out):
            print('{} | {} | {} | {} | {}'.format(case, tf.kernel_name(f).split('<')[0], route, name,
                                                  hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()), flush=True)


g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g21_taylor_gpqd.npz'))
models = jc.package_models()
for tag in to.CASES:
    for r in range(to.N_PAR):
        digests('g21 {} row {}'.format(tag, r), amd.TaylorGPQDTransform(to.CASES[tag][2], g[tag + '_par'][r:r + 1]), models[tag],
                g[tag + '_mean'], g[tag + '_cov'], g[tag + '_time'])

for tag, (mod, kind, _, _, _) in jc.linear_models().items():
    D = mod.dim_in
    rng = np.random.default_rng(5)
    means = rng.standard_normal((3000, D))
    a = rng.standard_normal((3000, D, D))
    digests('linear ' + tag, amd.LinearizationTransform(D), mod.dyn_eval if kind == 'dyn' else mod.meas_eval, means,
            np.einsum('bij,bkj->bik', a, a) + 0.2 * np.eye(D), np.arange(3000, dtype=float) % 50)

for tag, (mod, _, D, _) in jc.index_cases().items():
    rng = np.random.default_rng(22)
    mean = rng.standard_normal((193, D))
    a = rng.standard_normal((193, D, D))
    for alpha in (1.0, 2.5):
        par = np.hstack(([alpha], rng.uniform(0.5, 5.0, D)))[None, :]
        digests('index {} alpha {}'.format(tag, alpha), amd.TaylorGPQDTransform(D, par), mod.meas_eval, mean,
                np.einsum('bij,bkj->bik', a, a) + 0.2 * np.eye(D), 0.0)

rv = ssmod.GaussRV
vdp = uo.transition('VdP', 2, uo.VDP_CODE, uo.VDP_JAC, (0.1, 1.0))(rv(2, mean=np.array([1.0, 0.5]), cov=0.1 * np.eye(2)), rv(2, cov=0.01 * np.eye(2)))
vdp_meas = uo.measurement('VdPMeas', 1, uo.VDP_MEAS_CODE, uo.VDP_MEAS_JAC)(rv(1, cov=np.array([[0.05]])), 2)
user = [('pendulum', 2, uo.transition('Pend', 2, uo.PEND_CODE, uo.PEND_JAC, (0.01,))(rv(2), rv(2)).dyn_eval),
        ('pendulum meas', 2, uo.measurement('PendMeas', 1, uo.PEND_MEAS_CODE, uo.PEND_MEAS_JAC)(rv(1), 2).meas_eval),
        ('van der pol', 2, vdp.dyn_eval), ('van der pol meas', 2, vdp_meas.meas_eval)]
for D, E, DIN in ((3, 2, 3), (6, 4, 5), (6, 6, 6)):
    code, jac, _, _ = uo.poly_model(E, DIN)
    if E == D:
        f = uo.transition('Poly{}'.format(D), D, code, jac)(rv(D), rv(D)).dyn_eval
    else:
        f = uo.measurement('Poly{}{}'.format(D, E), E, code, jac, dim_substate=DIN if DIN < D else None)(rv(E), D).meas_eval
    user.append(('poly ({}, {}, {})'.format(D, E, DIN), D, f))
for name, D, f in user:
    rng = np.random.default_rng(10 + D)          # the inputs of tests/test_user_jacobian_gpu.py: inputs(D, seed, spread=0.6)
    mean = 0.6 * rng.uniform(-2.0, 2.0, (193, D))
    a = rng.standard_normal((193, D, D)) / np.sqrt(D)
    cov, time = np.einsum('bij,bkj->bik', a, a) + 0.05 * np.eye(D), rng.integers(0, 20, 193).astype(float)
    par = np.array([[1.3] + list(np.linspace(1.5, 4.0, D))])
    for tf in (amd.LinearizationTransform(D), amd.TaylorGPQDTransform(D, par)):
        digests('user ' + name, tf, f, mean, cov, time)
