#!/usr/bin/env python3
"""One SHA-256 per output array (raw bytes, status included) of the five likelihood-scoring entry points - kernel-parameter sweep,
t-process / Studentian scores and sweep, noise sweep, IMM over noise modes, innovation scores - on the cases of their tests, for
comparing two builds of libssmq.so bit by bit (SSMQ_LIBRARY selects the library):

  sweep      tests/_sweep_cases.py: ungm_gp (B = 70, ld = 128), pend_bs, reentry_gp (5 states), with and without per-step planes;
             a row whose weights fail; a NaN measurement planted at one step of one trajectory; T = 0 with a failed row
  student    tests/_student_score_cases.py: student_scores_batch of the sigma-point and the t-process form (STU = 1, per-step NIS),
             the t-process sweep with the Gaussian (STU = 0) and the Studentian recursion, a failed row, a NaN measurement, T = 0 (sweep, and
             student_scores_dev with P = 1)
  noise      tests/_noise_sweep_cases.py: all four cases (sigma-point, BQ, t-process BQ; ct_tp has 5 states), with and without
             per-step planes; an indefinite Q row; a non-PD P0 row; T = 0 through the C entry point
  imm        tests/_imm_cases.py: all four cases (M = 2, 3, 2, 4; ct_tp has 5 states), M = 1, a NaN measurement, an indefinite R mode,
             T = 0
  innov      the one-launch cases of tests/test_innovation_gpu.py (k_innovation<>; reentry and ct_bearing have 5 states; user_pend
             is compiled at run time from the embedded source)

A one-off comparison tool, not an interface: it imports the test modules for their case builders and reaches past the public API
(`_sweep_setup`, `_sweep_launch`, `_pair`, the raw C entry point) to get at T = 0, which the Python layer refuses; when those
internals move it has to move with them.

    python tools/score_digests.py > listing.txt"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, ssinf  # noqa: E402
from tests import _sweep_cases as sc, _noise_sweep_cases as nc, _student_score_cases as ssc, _imm_cases as ic  # noqa: E402
from tests import test_innovation_gpu as tig, test_student_scores_gpu as tss  # noqa: E402

amd.set_device(0)


def digests(case, kernel, out):
    for name in sorted(out):
        arr = np.ascontiguousarray(out[name])
        print('{} | {} | {} {} | {}'.format(case, kernel.split('<')[0], name, arr.shape, hashlib.sha256(arr.tobytes()).hexdigest()), flush=True)


def empty_sweep(case, alg, s, Y, B):
    """T = 0 of a likelihood sweep: past the Python layer, which asks for a step."""
    ld, P = _lib.padded(B), s['P']
    with _lib.Staging() as stage:
        d_y = stage.scratch(8 * Y * ld)
        d_tot, d_nis, _, d_st, ts = alg._sweep_launch(stage, s, d_y, B, ld, 0, False, False)
        digests(case, alg.likelihood_sweep_kernel_name(P), dict(
            theta_status=ts, loglik_total=d_tot.download((P, ld)), nis_mean=d_nis.download((P, ld)), status=d_st.download((P, ld), dtype=np.int32)))


# ---- kernel-parameter sweep (k_filter_sweep<>) ------------------------------------------------------------------------------
for name in sc.SHAPES:
    c = sc.case(name)
    alg = sc.make_filter(name, c['par'][0], c['par'][0])
    kn = alg.likelihood_sweep_kernel_name(len(c['par']))
    digests('sweep {} steps'.format(name), kn, alg.likelihood_sweep_batch(c['y'], c['par'], c['par'], steps=True))
    digests('sweep {} bare'.format(name), kn, alg.likelihood_sweep_batch(c['y'], c['par'], c['par']))
c = sc.case('ungm_gp')
alg = sc.make_filter('ungm_gp', c['par'][0], c['par'][0])
grid = np.insert(c['par'], 2, sc.BAD_ROW, axis=0)
digests('sweep ungm_gp failed row', 'k_filter_sweep<', alg.likelihood_sweep_batch(c['y'], grid, grid, steps=True))
yn = c['y'].copy()
yn[0, 2, 5] = np.nan
digests('sweep ungm_gp NaN measurement', 'k_filter_sweep<', alg.likelihood_sweep_batch(yn, c['par'], c['par'], steps=True))
empty_sweep('sweep ungm_gp T=0 failed row', alg, alg._sweep_setup(grid, grid), 1, c['B'])

# ---- t-process and Studentian scores and sweeps (k_filter_score<>) ------------------------------------------------------------
for name in ssc.SHAPES:
    y = tss.data(amd, name)
    for kind in ('fs', 'tps'):
        alg = ssc.make_filter(name, kind, False)
        digests('student_scores {} {}'.format(name, kind), alg.student_scores_kernel_name(), alg.student_scores_batch(y))
    yn = y.copy()
    yn[0, 2, 3] = np.nan
    digests('student_scores {} tps NaN measurement'.format(name), alg.student_scores_kernel_name(), alg.student_scores_batch(yn))
    B0, ld0 = y.shape[2], _lib.padded(y.shape[2])
    d_y0 = _lib.DeviceBuffer(8 * y.shape[0] * ld0)
    try:
        bufs = alg.student_scores_dev(d_y0, B0, ld0, 0)      # (d_nis, d_ll, d_tot, d_nm, d_st): no step, so no per-step plane to read
        digests('student_scores {} tps T=0'.format(name), alg.student_scores_kernel_name(), dict(
            loglik_total=bufs[2].download((ld0,)), nis_mean=bufs[3].download((ld0,)), status=bufs[4].download((ld0,), dtype=np.int32)))
        for buf in bufs:
            buf.free()
    except Exception as e:      # a layer above the library refuses an empty plane: the same text from both builds
        print('student_scores {} tps T=0 | refused | {}'.format(name, str(e)[:80]), flush=True)
    d_y0.free()
    par, nu, dof = ssc.ROWS[name]
    for kind, kw in (('tpk', dict(nu=nu)), ('tps', dict(nu=nu, dof=dof))):
        alg = ssc.make_filter(name, kind, False)
        digests('sweep_t {} {} steps'.format(name, kind), 'k_filter_score<', alg.likelihood_sweep_batch(y, par, par, steps=True, **kw))
        digests('sweep_t {} {} bare'.format(name, kind), 'k_filter_score<', alg.likelihood_sweep_batch(y, par, par, **kw))
        if name in ssc.BAD_ROW:
            grid = np.insert(par, 1, ssc.BAD_ROW[name], axis=0)
            kwb = {k: np.insert(v, 1, v[0]) for k, v in kw.items()}
            digests('sweep_t {} {} failed row'.format(name, kind), 'k_filter_score<', alg.likelihood_sweep_batch(y, grid, grid, steps=True, **kwb))
            empty_sweep('sweep_t {} {} T=0 failed row'.format(name, kind), alg, alg._sweep_setup(grid, grid, **kwb), y.shape[0], y.shape[2])

# ---- noise sweep (k_noise_sweep<>) --------------------------------------------------------------------------------------------
for name in nc.NAMES:
    c = nc.case(name)
    alg = nc.make_filter(name)
    kn = alg.noise_sweep_kernel_name(c['P'])
    digests('noise {} steps'.format(name), kn, alg.noise_sweep_batch(c['y'], c['q_cov'], c['r_cov'], c['x0_cov'], steps=True))
    digests('noise {} bare'.format(name), kn, alg.noise_sweep_batch(c['y'], c['q_cov'], c['r_cov'], c['x0_cov']))
c = nc.case('ungm_ukf')
alg = nc.make_filter('ungm_ukf')
digests('noise ungm_ukf indefinite Q row', 'k_noise_sweep<', alg.noise_sweep_batch(c['y'], nc.failing_q(c), c['r_cov'], steps=True))
x0 = np.array([[[1.0]], [[-2.0]], [[0.5]], [[1.0]], [[2.0]]])
try:
    digests('noise ungm_ukf non-PD P0 row', 'k_noise_sweep<', alg.noise_sweep_batch(c['y'], c['q_cov'], c['r_cov'], x0, steps=True))
except ValueError as e:      # refused before the device: the same text from both builds
    print('noise ungm_ukf non-PD P0 row | refused | {}'.format(str(e)[:80]), flush=True)
lib, P, B, ld = _lib.load(), 2, 70, 128
outs = [_lib.DeviceBuffer(8 * P * ld), _lib.DeviceBuffer(8 * P * ld), _lib.DeviceBuffer(4 * P * ld)]
d_y = _lib.DeviceBuffer(8 * ld)
rc = lib.ssmq_filter_noise_sweep_dev(*alg._pair(), 0, B, ld, 0, _lib.vp(d_y), P, _lib.dp(np.ones((2, 1))), 1, _lib.dp(np.ones((2, 1))), 1,
                                     _lib.dp(np.ones((2, 2))), 2, _lib.vp(outs[0]), _lib.vp(outs[1]), None, _lib.vp(outs[2]))
digests('noise ungm_ukf T=0 rc {}'.format(rc), 'k_noise_sweep<', dict(loglik_total=outs[0].download((P, ld)), nis_mean=outs[1].download((P, ld)),
                                                                       status=outs[2].download((P, ld), dtype=np.int32)))
for buf in outs + [d_y]:
    buf.free()

# ---- IMM over noise modes (k_imm_loop<>) --------------------------------------------------------------------------------------
for name in ic.NAMES:
    c = ic.get(name)
    alg = nc.make_filter(name)
    digests('imm {} M={}'.format(name, c['M']), alg.imm_kernel_name(c['M']), alg.imm_pass_batch(c['y'], **ic.args(c)))
c = ic.get('ungm_ukf')
alg = nc.make_filter('ungm_ukf')
digests('imm ungm_ukf M=1', alg.imm_kernel_name(1), alg.imm_pass_batch(c['y'], pi=np.ones((1, 1)), mu0=np.ones(1), q_cov=c['q_cov'][:1]))
yn = c['y'].copy()
yn[0, ic.FAIL_STEP, ic.FAIL_LANE] = np.nan
digests('imm ungm_ukf NaN measurement', alg.imm_kernel_name(2), alg.imm_pass_batch(yn, raise_on_failure=False, **ic.args(c)))
digests('imm ungm_ukf indefinite R mode', alg.imm_kernel_name(2),
        alg.imm_pass_batch(c['y'], raise_on_failure=False, **dict(ic.args(c), r_cov=ic.failing_r(c))))
B0, ld0 = c['y'].shape[2], _lib.padded(c['y'].shape[2])
d_y0 = _lib.DeviceBuffer(8 * ld0)
try:
    bufs = alg.imm_pass_dev(d_y0, B0, ld0, 0, c['pi'], mu0=c['mu0'], q_cov=c['q_cov'])      # (fm, fP, mode_prob, loglik, total, status)
    digests('imm ungm_ukf T=0', alg.imm_kernel_name(2), dict(loglik_total=bufs[4].download((ld0,)), status=bufs[5].download((ld0,), dtype=np.int32)))
    for buf in bufs:
        buf.free()
except Exception as e:      # a layer above the library refuses an empty plane: the same text from both builds
    print('imm ungm_ukf T=0 | refused | {}'.format(str(e)[:80]), flush=True)
d_y0.free()

# ---- innovation scores (k_innovation<>) ---------------------------------------------------------------------------------------
for name in tig.ONE_LAUNCH:
    alg, B, T = tig.make_case(amd, name)
    y = tig.simulate(tig.make_case(amd, 'pend_ukf')[0] if name == 'user_pend' else alg, B, T, 3)
    fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
    digests('innov {}'.format(name), alg.innovations_kernel_name(), alg.innovations_batch(y, fi_mean=fm, fi_cov=fP, return_moments=True))
    digests('innov {} bare'.format(name), alg.innovations_kernel_name(), alg.innovations_batch(y, fi_mean=fm, fi_cov=fP))
