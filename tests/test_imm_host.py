"""The IMM filter over noise modes, the parts that need no device: the two symbols, properties of the CPU restatement
(tests/_imm_oracle.py) that tie it to the oracles that exist, its long-double twin, the refusals of the Python methods before the library
is loaded, the conditions the GPU cases rest on, and the cross-compile check of k_imm_loop<> for gfx950 at the four case shapes."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _imm_cases as ic
from tests import _imm_oracle as imo
from tests import _noise_sweep_cases as nc
from tests import _noise_sweep_oracle as nso
from tests.test_innovation_host import pendulum_user
from tests.test_noise_sweep_host import bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)
METHODS = ('imm_pass_dev', 'imm_pass_batch', 'imm_pass', 'imm_kernel_name')


def test_library_exports_and_declares_the_entry_points():
    from ssmtoybox_amd import _lib, ssinf
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_filter_imm_dev', 'ssmq_filter_imm_kernel_name'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert 'int ' + name + '(' in header
    for name in METHODS:
        assert callable(getattr(ssinf.GaussianInference, name))
    pi = ssinf.mode_transition(4, 0.85)
    assert pi.shape == (4, 4) and np.all(np.diag(pi) == 0.85) and np.all(pi[~np.eye(4, dtype=bool)] == (1.0 - 0.85) / 3)
    assert np.array_equal(ssinf.mode_transition(1, 0.3), [[1.0]])
    with pytest.raises(ValueError, match='mode_transition'):
        ssinf.mode_transition(0, 0.5)


@pytest.mark.parametrize('name', ic.NAMES)
def test_cases_succeed_on_the_oracle_and_mode_probabilities_sum_to_one(name):
    c, ref = ic.get(name), ic.reference(name)
    assert not ref['status'].any() and all(np.isfinite(ref[k]).all() for k in ('mean', 'cov', 'mode_prob', 'loglik', 'loglik_total'))
    assert ref['mode_prob'].shape == (c['M'], c['T'], c['B']) and (ref['mode_prob'] >= 0).all()
    assert np.max(np.abs(ref['mode_prob'].sum(axis=0) - 1.0)) <= 4 * c['M'] * EPS
    assert np.array_equal(ref['cov'], ref['cov'].transpose(1, 0, 2, 3))


@pytest.mark.parametrize('name', ic.NAMES)
def test_oracle_against_its_long_double_twin(name):
    """The figures the GPU bounds are built on (tests/_imm_cases.py: TWIN), measured here."""
    d = imo.twin_difference(ic.reference(name), ic.reference(name, np.longdouble))
    print('imm {}: float64 oracle against its long-double twin, max |difference| / max(1, |value|) = {}; recorded {}'.format(
        name, {k: float('{:.3g}'.format(v)) for k, v in d.items()}, ic.TWIN[name]))
    assert not ic.reference(name, np.longdouble)['status'].any()
    for k, v in d.items():
        assert 0.0 < v <= ic.TWIN[name][k], (k, v)


@pytest.mark.parametrize('name', ('ungm_ukf', 'pend_ckf'))
def test_one_mode_is_the_plain_filter_oracle(name):
    c = ic.get(name)
    y = c['y'][..., :3]
    got = imo.imm(c, y, c['q_rows'][:1], c['r_rows'][:1], c['x0_rows'][:1], np.ones((1, 1)), np.ones(1))
    tfd, tfo = nso.transforms(c)
    sweep = nso.sweep(c, y, c['q_rows'][:1], c['r_rows'][:1], c['x0_rows'][:1])
    assert not got['status'].any() and np.array_equal(got['loglik'], sweep['loglik'][0]) and np.array_equal(got['loglik_total'], sweep['loglik_total'][0])
    assert (got['mode_prob'] == 1.0).all()
    D = c['m0'].shape[0]
    low = np.tril_indices(D)
    for b in range(y.shape[2]):
        fm, fP = orc.gaussian_filter(y[..., b], c['m0'], c['x0_rows'][0], c['q_rows'][0], c['r_rows'][0], c['G'], tfd, tfo)[:2]
        assert np.array_equal(got['mean'][..., b], fm)
        assert np.array_equal(got['cov'][..., b][low], fP[low])        # (the IMM writes both triangles from the lower one)


def test_identity_transitions_are_the_noise_sweep_rows():
    c = ic.get('pend_ckf')
    M, y, LD = c['M'], c['y'], np.longdouble
    mu0 = np.array([0.5, 0.3, 0.2])
    got = ic.oracle(c, pi=np.eye(M), mu0=mu0)
    twin = ic.oracle(c, pi=np.eye(M), mu0=mu0, dtype=LD)
    sweep = nso.sweep(c, y, c['q_rows'], c['r_rows'], c['x0_rows'])
    assert not got['status'].any() and np.array_equal(got['mode_ll'], sweep['loglik'])       # no mode ever reads another's moments
    a = np.log(mu0.astype(LD))[:, None] + sweep['loglik'].astype(LD).sum(axis=1)
    amax = a.max(axis=0)
    lse = amax + np.log(np.exp(a - amax).sum(axis=0))
    soft = np.exp(a - lse)
    tol_l = np.maximum(8 * np.abs(got['loglik_total'] - twin['loglik_total']), 8 * c['T'] * EPS * np.maximum(1.0, np.abs(lse)))
    tol_p = np.maximum(8 * np.abs(got['mode_prob'][:, -1] - twin['mode_prob'][:, -1]), 8 * c['T'] * EPS * np.maximum(1.0, np.abs(lse)))
    print('imm identity: |loglik_total - logsumexp| max {:.3g} (tolerance {:.3g}), |mode_prob - softmax| max {:.3g} (tolerance {:.3g})'.format(
        float(np.max(np.abs(got['loglik_total'] - lse))), float(tol_l.min()), float(np.max(np.abs(got['mode_prob'][:, -1] - soft))), float(tol_p.min())))
    assert np.all(np.abs(got['loglik_total'] - lse) <= tol_l) and np.all(np.abs(got['mode_prob'][:, -1] - soft) <= tol_p)


def test_permuting_the_modes_permutes_the_mode_probabilities():
    c, ref = ic.get('pend_ckf'), ic.reference('pend_ckf')
    perm = np.array([2, 0, 1])
    mu0 = np.array([0.5, 0.3, 0.2])
    pi = np.array([[0.9, 0.06, 0.04], [0.1, 0.8, 0.1], [0.02, 0.08, 0.9]])
    a = imo.imm(c, c['y'], c['q_rows'], c['r_rows'], c['x0_rows'], pi, mu0)
    b = imo.imm(c, c['y'], c['q_rows'][perm], c['r_rows'][perm], c['x0_rows'][perm], pi[np.ix_(perm, perm)], mu0[perm])
    tw = ic.TWIN['pend_ckf']
    for key, fig in (('mean', tw['mean']), ('cov', tw['cov']), ('loglik', tw['mode_prob'])):
        assert np.all(np.abs(a[key] - b[key]) <= ic.MARGIN * fig * np.maximum(1.0, np.abs(a[key]))), key
    assert np.all(np.abs(a['mode_prob'][perm] - b['mode_prob']) <= ic.MARGIN * tw['mode_prob'])
    assert not np.array_equal(a['mode_prob'], b['mode_prob'])


def test_an_unreachable_mode_keeps_its_moments():
    """c_j == 0: w_ij = delta_ij, a_j = -inf, mu_j = 0 - and nothing is NaN."""
    c = ic.get('pend_ckf')
    pi = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 1.0]])
    got = imo.imm(c, c['y'][..., :2], c['q_rows'], c['r_rows'], c['x0_rows'], pi, np.array([0.5, 0.5, 0.0]))
    assert not got['status'].any() and (got['mode_prob'][2] == 0.0).all() and np.isfinite(got['mean']).all()
    cc, m0, P0 = imo.mix(pi, np.array([0.5, 0.5, 0.0]), np.arange(6.0).reshape(3, 2), np.stack([np.eye(2)] * 3))
    assert cc[2] == 0.0 and np.array_equal(m0[2], [4.0, 5.0]) and np.array_equal(P0[2], np.eye(2))


def test_failure_cases_hold_on_the_oracle():
    """What tests/test_imm_gpu.py::test_failures_stay_local rests on."""
    c, ref = ic.get('ungm_ukf'), ic.reference('ungm_ukf')
    y = c['y'].copy()
    y[0, ic.FAIL_STEP, ic.FAIL_LANE] = np.nan
    got = ic.oracle(c, y=y[..., :8])
    assert got['status'][ic.FAIL_LANE] == 1 + ic.FAIL_STEP and np.count_nonzero(got['status']) == 1
    assert np.isnan(got['mean'][:, ic.FAIL_STEP:, ic.FAIL_LANE]).all() and np.array_equal(got['mean'][:, :ic.FAIL_STEP, ic.FAIL_LANE], ref['mean'][:, :ic.FAIL_STEP, ic.FAIL_LANE])
    # the planted R: a pattern of failures at several steps that a relative change of 1e-6 of the planted variance does not move
    r = ic.failing_r(c)
    fail = ic.oracle(c, r_rows=r)
    st = fail['status']
    print('imm planted R: status counts', np.bincount(st, minlength=c['T'] + 1))
    assert 0 < np.count_nonzero(st) < c['B'] and len(np.unique(st)) >= 3
    for rel in (1.0 - 1e-6, 1.0 + 1e-6):
        r2 = r.copy()
        r2[ic.FAIL_MODE] *= rel
        assert np.array_equal(ic.oracle(c, r_rows=r2)['status'], st)


def test_python_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm, mtran, _lib
    g1, t4 = (lambda: sm.GaussRV(1)), (lambda d: sm.StudentRV(d, dof=4.0))
    ungm = lambda: (sm.UNGMTransition(g1(), g1()), sm.UNGMMeasurement(g1(), 1))      # noqa: E731
    UP, UM = pendulum_user()
    cases = ((ssinf.FullySymmetricStudent(sm.UNGMTransition(t4(1), t4(1)), sm.UNGMMeasurement(t4(1), 1)), 'Studentian recursion'),
             (ssinf.UnscentedKalman(sm.UNGMNATransition(g1(), g1()), sm.UNGMNAMeasurement(g1(), 1)), 'non-additive noise'),
             (ssinf.ExtendedKalman(*ungm()), 'LinearizationTransform'),
             (ssinf.UnscentedKalman(UP(sm.GaussRV(2), sm.GaussRV(2)), UM(g1(), 2)), 'user models'),
             (bare(ssinf.UnscentedKalman, sm.UNGMTransition(g1(), t4(1)), sm.UNGMMeasurement(g1(), 1), mtran.UnscentedTransform), 'StudentRV'))

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    y = np.zeros((1, 4, 3))
    pi = ssinf.mode_transition(2, 0.9)
    for alg, what in cases:
        q = ssinf.noise_grid(np.atleast_2d(alg.q_cov), [0.5, 2.0])
        for call in (lambda a: a.imm_pass_batch(y, pi, q_cov=q), lambda a: a.imm_pass(y[..., 0], pi, q_cov=q),
                     lambda a: a.imm_pass_dev(None, 3, 64, 4, pi, q_cov=q), lambda a: a.imm_kernel_name(2)):
            with pytest.raises(NotImplementedError, match=what) as info:
                call(alg)
            assert 'IMM' in str(info.value) and 'noise sweeps cover UnscentedKalman' in str(info.value) and 'D <= 6, Y <= 4' in str(info.value), what
    ok = ssinf.UnscentedKalman(*nc.models('pend_ckf'))
    R = ok.r_cov
    nine = ssinf.noise_grid(R, np.arange(1.0, 10.0))
    for call in (lambda: ok.imm_pass_batch(y, ssinf.mode_transition(9, 0.9), r_cov=nine), lambda: ok.imm_kernel_name(9),
                 lambda: ok.imm_pass_dev(None, 3, 64, 4, ssinf.mode_transition(9, 0.9), r_cov=nine)):
        with pytest.raises(NotImplementedError, match='1 <= M <= 8 modes; got M = 9'):
            call()
    two = ssinf.noise_grid(R, [1.0, 2.0])
    for kwargs, what in ((dict(pi=np.array([[0.9, 0.1], [0.2, 0.7]])), 'row 1 of pi does not sum to 1'),
                         (dict(pi=np.array([[0.9, 0.1 + 1e-11], [0.2, 0.8]])), 'row 0 of pi does not sum to 1'),
                         (dict(pi=np.array([[1.1, -0.1], [0.2, 0.8]])), 'row 0 of pi has an entry that is not finite or is negative'),
                         (dict(pi=np.array([[0.9, 0.1], [np.nan, 0.8]])), 'row 1 of pi has an entry'),
                         (dict(pi=pi, mu0=np.array([0.5, 0.4])), 'mu0 does not sum to 1'), (dict(pi=pi, mu0=np.ones(3) / 3), 'mu0 is None'),
                         (dict(pi=np.ones(2) / 2), 'square'), (dict(pi=ssinf.mode_transition(3, 0.9)), '2 rows and pi has M = 3')):
        for call in (lambda: ok.imm_pass_batch(y, r_cov=two, **kwargs), lambda: ok.imm_pass_dev(None, 3, 64, 4, r_cov=two, **kwargs)):
            with pytest.raises(ValueError, match=what):
                call()
    with pytest.raises(ValueError, match='at least one of'):
        ok.imm_pass_batch(y, pi)                                   # two modes and nothing varied
    with pytest.raises(ValueError, match='dim_y, T, B'):
        ok.imm_pass_batch(np.zeros((2, 4, 3)), pi, r_cov=two)
    with pytest.raises(ValueError, match='multiple of 64'):
        ok.imm_pass_dev(None, 3, 70, 4, pi, r_cov=two)
    # M = 1 with nothing varied is the plain filter; the arrays of the entry point
    s = ok._imm_setup(np.ones((1, 1)), None, None, None, None, None)
    assert s['M'] == 1 and s['gqg'].shape == (1, 4) and np.array_equal(s['mu0'], [1.0])
    s = ok._imm_setup(pi, None, None, two, None, np.array([[1.0, 0.0], [2.0, 0.5]]))
    assert s['M'] == 2 and s['x0'].shape == (2, 6) and np.array_equal(s['x0'][:, :2], [[1.0, 0.0], [2.0, 0.5]]) and np.array_equal(s['mu0'], [0.5, 0.5])


# the four case shapes: (D, Y, N, integrand of the dynamics, of the measurement, SELO, form, tp)
def _compile_shapes():
    from ssmtoybox_amd import _lib
    return {'ungm_ukf': (1, 1, 3, _lib.F_UNGM_DYN, _lib.F_UNGM_MEAS, 0, _lib.FORM_SIGMA, 0),
            'pend_ckf': (2, 1, 4, _lib.F_PENDULUM_DYN, _lib.F_PENDULUM_MEAS, 0, _lib.FORM_SIGMA, 0),
            'cv_gp': (4, 2, 9, _lib.F_CV_DYN, _lib.F_RADAR2D_MEAS, 0, _lib.FORM_BQ, 0),
            'ct_tp': (5, 4, 11, _lib.F_CT_DYN, _lib.F_BEARING_MEAS, 1, _lib.FORM_BQ, 1)}


@pytest.mark.parametrize('name', ic.NAMES)
def test_compile_check_gfx950(name):
    """k_imm_loop<> of the case's shape compiles for gfx950; registers, scratch and LDS from the compiler's remarks (the LDS of the
    slots is dynamic: the remark counts static LDS only, the slots of the case's M modes are printed next to it)."""
    from ssmtoybox_amd import _lib
    D, Y, N, fd, fo, selo, form, tp = _compile_shapes()[name]
    rc, log = _lib.rtc_compile_check(fd, _lib.RTC_IMM, D, Y, N, form, tp=tp, opt=selo, fid_obs=fo, N_obs=N)
    assert rc == 0, log
    assert 'k_imm_loop' in log.splitlines()[0]
    res = {k: int(v) for k, v in re.findall(r'(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)', log)}
    M = ic.MODES[name]
    slots = 8 * M * (D + D * (D + 1) // 2 + 1) * 64
    print('k_imm_loop {}: {} | dynamic LDS of M = {} modes: {} bytes (M = 8: {})'.format(name, res, M, slots, slots // M * 8))
    assert res['VGPRs'] <= 256 and slots // M * 8 <= 160 * 1024 - 64
    if D <= 4:
        assert res['ScratchSize [bytes/lane]'] == 0, res
    assert _lib.rtc_compile_check(fd, _lib.RTC_IMM, 7, Y, N, form, fid_obs=fo, N_obs=N)[0] == -1
