"""Noise sweeps by measurement likelihood, the parts that need no device: the two symbols, the refusals of the Python methods (before the
library is loaded, each naming the range), what the C entry points refuse without a transform handle (a handle needs a device: the
refusals that read one are in tests/test_noise_sweep_gpu.py), `noise_grid`, `fit_noise_covariances` on an oracle table, and the
conditions the GPU cases rest on, established on the CPU restatement alone."""
import ctypes
import os

import numpy as np
import pytest

from tests import _noise_sweep_cases as nc
from tests import _noise_sweep_oracle as nso
from tests._cases import RTOL
from tests.test_innovation_host import pendulum_user

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -3
METHODS = ('noise_sweep_batch', 'noise_sweep_dev', 'noise_sweep_kernel_name', 'fit_noise_covariances')


def test_library_exports_and_declares_the_entry_points():
    from ssmtoybox_amd import _lib, ssinf
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_filter_noise_sweep_dev', 'ssmq_filter_noise_sweep_kernel_name'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert 'int ' + name + '(' in header
    for name in METHODS:
        assert callable(getattr(ssinf.GaussianInference, name))
    assert callable(ssinf.noise_grid)


def test_c_abi_refuses_null_handles_and_leaves_the_outputs_untouched():
    from ssmtoybox_amd import _lib, ssmod as sm
    from ssmtoybox_amd.mtran import resolve_integrand
    lib = _lib.load()
    f = [resolve_integrand(fn)[0] for fn in (sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1)).dyn_eval, sm.UNGMMeasurement(sm.GaussRV(1), 1).meas_eval)]
    P, ld, T = 2, 64, 2
    outs = [np.full(P * ld, 7.0), np.full(P * ld, 7.0), np.full(P * T * ld, 7.0), np.full(P * ld, 7, dtype=np.int32)]
    y, one = np.zeros(T * ld), np.ones((P, 2))
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    rc = lib.ssmq_filter_noise_sweep_dev(None, f[0], None, f[1], 0, 3, ld, T, vp(y), P, _lib.dp(one), 1, _lib.dp(one), 1, _lib.dp(one), 2,
                                         vp(outs[0]), vp(outs[1]), vp(outs[2]), vp(outs[3]))
    msg = _lib.last_error()
    assert rc == E_ARG and 'bad argument' in msg and 'D <= 6, Y <= 4' in msg and all((o == 7).all() for o in outs)
    buf = ctypes.create_string_buffer(256)
    assert lib.ssmq_filter_noise_sweep_kernel_name(None, f[0], None, f[1], 0, buf, 256) == E_ARG and 'D <= 6, Y <= 4' in _lib.last_error()
    assert lib.ssmq_filter_noise_sweep_kernel_name(None, f[0], None, f[1], 0, None, 0) == E_ARG


def bare(cls, dyn, obs, tf_cls):
    """A filter of class `cls` around the models without its constructor (which may compute weights on the device), its transforms
    objects of `tf_cls` that are never applied."""
    alg = object.__new__(cls)
    alg.mod_dyn, alg.mod_obs, alg.tf_dyn, alg.tf_obs = dyn, obs, object.__new__(tf_cls), object.__new__(tf_cls)
    alg.x0_mean, alg.x0_cov = dyn.init_rv.get_stats()[:2]
    alg.q_mean, alg.q_cov = dyn.noise_rv.get_stats()[:2]
    alg.r_mean, alg.r_cov = obs.noise_rv.get_stats()[:2]
    alg.G = dyn.noise_gain
    return alg


def test_python_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm, mtran, _lib
    from ssmtoybox_amd.bq import bqmtran
    g1, t4 = (lambda: sm.GaussRV(1)), (lambda d: sm.StudentRV(d, dof=4.0))
    ungm = lambda: (sm.UNGMTransition(g1(), g1()), sm.UNGMMeasurement(g1(), 1))      # noqa: E731
    UP, UM = pendulum_user()
    mix = sm.GaussianMixtureRV(1, (np.zeros(1), np.ones(1)), (np.eye(1), np.eye(1)), (0.5, 0.5))
    cases = ((ssinf.UnscentedKalman(UP(sm.GaussRV(2), sm.GaussRV(2)), UM(g1(), 2)), 'user models'),
             (ssinf.UnscentedKalman(sm.UNGMNATransition(g1(), g1()), sm.UNGMNAMeasurement(g1(), 1)), 'non-additive noise'),
             (bare(ssinf.UnscentedKalman, sm.UNGMTransition(g1(), t4(1)), sm.UNGMMeasurement(g1(), 1), mtran.UnscentedTransform), 'StudentRV'),
             (bare(ssinf.UnscentedKalman, sm.UNGMTransition(t4(1), g1()), sm.UNGMMeasurement(g1(), 1), mtran.UnscentedTransform), 'StudentRV'),
             (bare(ssinf.CubatureKalman, sm.UNGMTransition(g1(), g1()), sm.UNGMMeasurement(mix, 1), mtran.SphericalRadialTransform), 'GaussianMixtureRV'),
             (ssinf.FullySymmetricStudent(sm.UNGMTransition(t4(1), t4(1)), sm.UNGMMeasurement(t4(1), 1)), 'Studentian recursion'),
             (bare(ssinf.StudentProcessStudent, *ungm(), bqmtran.StudentTProcessTransform), 'Studentian recursion'),
             (bare(ssinf.MarginalizedGaussianProcessKalman, *ungm(), bqmtran.GaussianProcessTransform), 'marginalised filters'),
             (ssinf.ExtendedKalman(*ungm()), 'LinearizationTransform'),
             (bare(ssinf.ExtendedKalmanGPQD, *ungm(), mtran.TaylorGPQDTransform), 'TaylorGPQDTransform'),
             (bare(ssinf.GaussianProcessDerKalman, *ungm(), bqmtran.GaussianProcessDerTransform), 'GaussianProcessDerTransform'),
             (bare(ssinf.TruncatedUnscentedKalman, *ungm(), mtran.TruncatedUnscentedTransform), 'TruncatedUnscentedTransform'),
             (bare(ssinf.MultiOutputGaussianProcessKalman, *ungm(), bqmtran.MultiOutputGaussianProcessTransform), 'MultiOutputGaussianProcessTransform'),
             (ssinf.GaussianInference(*ungm(), mtran.UnscentedTransform(1), bare(ssinf.GaussianInference, *ungm(), bqmtran.GaussianProcessTransform).tf_obs),
              'UnscentedTransform / GaussianProcessTransform'),
             (ssinf.UnscentedKalman(sm.Smooth10DTransition(sm.GaussRV(10), sm.GaussRV(10)), sm.UNGMMeasurement(g1(), 10)), 'got D = 10'))

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    y = np.zeros((1, 4, 3))
    for alg, what in cases:
        q = ssinf.noise_grid(np.atleast_2d(alg.q_cov), [0.5, 2.0])
        for call in (lambda a: a.noise_sweep_batch(y, q_cov=q), lambda a: a.fit_noise_covariances(y, q_cov=q),
                     lambda a: a.noise_sweep_dev(None, 3, 64, 4, q_cov=q), lambda a: a.noise_sweep_kernel_name(2)):
            with pytest.raises(NotImplementedError, match=what) as info:
                call(alg)
            assert 'noise sweeps cover UnscentedKalman' in str(info.value) and 'D <= 6, Y <= 4' in str(info.value), what
    # the arguments, on a filter in the range: still before the library
    ok = ssinf.UnscentedKalman(*nc.models('pend_ckf'))
    Q, R, P0 = ok.q_cov, ok.r_cov, ok.x0_cov
    bad = lambda a, v: np.array([a, np.where(np.eye(len(a)) > 0, v, a)])      # noqa: E731   (row 1: the diagonal replaced)
    skew = np.array([Q, Q + np.array([[0.0, 1e-9], [0.0, 0.0]])])
    for kwargs, what in ((dict(), 'at least one of'), (dict(q_cov=Q, r_cov=R), 'at least one of'),
                         (dict(q_cov=ssinf.noise_grid(Q, [1, 2]), r_cov=ssinf.noise_grid(R, [1, 2, 3])), 'the same P'),
                         (dict(q_cov=ssinf.noise_grid(Q, [1, 2]), x0_cov=ssinf.noise_grid(P0, [1, 2, 3])), 'the same P'),
                         (dict(q_cov=np.ones((2, 3, 3))), r'q_cov is None, one \(2, 2\) matrix or a stack'),
                         (dict(r_cov=np.ones((0, 1, 1))), 'r_cov is None'), (dict(x0_cov=np.ones(4)), 'x0_cov is None'),
                         (dict(q_cov=bad(Q, np.nan)), 'row 1 of q_cov is not finite'), (dict(r_cov=bad(R, np.inf)), 'row 1 of r_cov is not finite'),
                         (dict(q_cov=skew), 'row 1 of q_cov is not symmetric'),
                         (dict(r_cov=ssinf.noise_grid(R, [1, 2]), x0_cov=np.array([[1.0, 0.5], [0.0, 1.0]])), 'row 0 of x0_cov is not symmetric')):
        for call in (lambda: ok.noise_sweep_batch(np.zeros((1, 4, 3)), **kwargs), lambda: ok.noise_sweep_dev(None, 3, 64, 4, **kwargs),
                     lambda: ok.fit_noise_covariances(np.zeros((1, 4, 3)), **kwargs)):
            with pytest.raises(ValueError, match=what):
                call()
    stack = ssinf.noise_grid(R, [1, 2])
    with pytest.raises(ValueError, match='dim_y, T, B'):
        ok.noise_sweep_batch(np.zeros((2, 4, 3)), r_cov=stack)
    with pytest.raises(ValueError, match='at least one step'):
        ok.noise_sweep_batch(np.zeros((1, 0, 3)), r_cov=stack)
    with pytest.raises(ValueError, match='multiple of 64'):
        ok.noise_sweep_dev(None, 3, 70, 4, r_cov=stack)
    # point counts are the table's to answer (five points at D = 1 are in it, nine at D = 2 are not): no Python check stops them
    for alg in (ssinf.GaussHermiteKalman(*ungm(), deg=5), ssinf.GaussHermiteKalman(*nc.models('pend_ckf'), deg=3)):
        assert alg._noise_sweep_setup(ssinf.noise_grid(alg.q_cov, [1.0, 2.0]), None, None)['P'] == 2
    # an indefinite row is no host error: it is for the device to report
    s = ok._noise_sweep_setup(ssinf.noise_grid(Q, [1.0, -1.0]), None, None)
    assert s['P'] == 2 and s['gqg'].shape == (2, 4) and s['rr'].shape == (1, 1) and s['x0'].shape == (1, 6)
    # row p's additive term is the expression of `_noise`, bit for bit
    row = nc.make_filter('pend_ckf', q_cov=ssinf.noise_grid(Q, [1.0, 0.3])[1])
    s = ok._noise_sweep_setup(ssinf.noise_grid(Q, [1.0, 0.3]), None, None)
    assert np.array_equal(s['gqg'][1].reshape(2, 2), row._noise()[0]) and np.array_equal(s['rr'][0].reshape(1, 1), row._noise()[1])


def test_noise_grid():
    from ssmtoybox_amd import ssinf
    Q = np.array([[2.0, 0.5], [0.5, 1.0]])
    g = ssinf.noise_grid(Q, [0.1, 1.0, 10.0])
    assert g.shape == (3, 2, 2) and g.flags['C_CONTIGUOUS'] and g.dtype == np.float64
    assert np.array_equal(g, np.array([0.1, 1.0, 10.0])[:, None, None] * Q)
    assert ssinf.noise_grid(3.0, np.array([2.0])).shape == (1, 1, 1) and ssinf.noise_grid([[3.0]], (2.0, 4.0))[1, 0, 0] == 12.0
    for cov, scales in ((Q, []), (Q, [[1.0, 2.0]]), (np.ones((2, 3)), [1.0]), (np.ones((2, 2, 2)), [1.0])):
        with pytest.raises(ValueError, match='noise_grid'):
            ssinf.noise_grid(cov, scales)


def test_fit_noise_covariances_is_the_oracle_argmax(monkeypatch):
    c, ref = nc.case('ungm_ukf'), nc.reference('ungm_ukf')
    alg = nc.make_filter('ungm_ukf')
    monkeypatch.setattr(alg, '_noise_sweep_run', lambda s, data, steps: {k: ref[k] for k in ('loglik_total', 'nis_mean', 'status')})
    index, q, r, table = alg.fit_noise_covariances(c['y'], c['q_cov'], c['r_cov'])
    want = ref['loglik_total'].sum(axis=1)
    assert index == int(np.argmax(want)) == 2 and np.allclose(table, want, rtol=1e-13, atol=0.0)      # (fit_table sums a copy: another order)
    assert np.array_equal(q, c['q_cov'][2]) and np.array_equal(r, c['r_cov'][2])
    # a shared argument is returned as it is; a failed item drops its trajectory from every row
    st = ref['status'].copy()
    st[4, 7] = 3
    monkeypatch.setattr(alg, '_noise_sweep_run', lambda s, data, steps: dict(loglik_total=ref['loglik_total'], status=st))
    index, q, r, table = alg.fit_noise_covariances(c['y'], c['q_cov'], None)
    assert np.array_equal(r, c['R']) and np.allclose(table, np.delete(ref['loglik_total'], 7, axis=1).sum(axis=1), rtol=1e-13, atol=0.0)


def test_case_conditions_hold_on_the_oracle():
    """What tests/test_noise_sweep_gpu.py rests on: every item of the four cases succeeds; the UNGM table has an interior maximum that
    leads the runner-up by more than 100 x the bound of its GPU comparison; the rows of cv_gp are no multiples of one another; the
    planted Q row fails in exactly the pattern below, which a relative change of 1e-6 of the planted variance - ten orders above the
    rounding of a step - does not move; a NaN measurement gives status 1 + step."""
    eps = float(np.finfo(float).eps)
    for name in nc.NAMES:
        ref = nc.reference(name)
        assert not ref['status'].any() and np.isfinite(ref['loglik']).all() and np.isfinite(ref['nis_mean']).all(), name
    c, ref = nc.case('ungm_ukf'), nc.reference('ungm_ukf')
    assert c['P'] == 5 and c['B'] == 70 and c['x0_cov'] is None
    table = ref['loglik_total'].sum(axis=1)
    order = np.argsort(table)
    margin = table[order[-1]] - table[order[-2]]
    P, T, B = ref['loglik'].shape
    bound = max(sum(max(RTOL, 64.0 * np.linalg.cond(ref['S'][p][b][..., k]) * eps) * max(1.0, abs(ref['loglik'][p, k, b]))
                    for b in range(B) for k in range(T)) for p in range(P))
    print('UNGM noise table {}: margin {:.4g}, bound of the GPU comparison {:.3g}'.format(table, margin, bound))
    assert order[-1] == 2 and margin > 100.0 * bound and margin > 10.0
    cv = nc.case('cv_gp')
    assert cv['r_cov'] is None and all(np.linalg.matrix_rank(np.stack([cv['q_cov'][i].ravel(), cv['q_cov'][j].ravel()])) == 2
                                        for i in range(3) for j in range(i))
    assert nc.case('pend_ckf')['q_cov'] is None and nc.case('pend_ckf')['x0_cov'] is None
    # the planted row: a negative process-noise variance
    q = nc.failing_q(c)
    fail = nso.sweep(c, c['y'], q, c['r_rows'], c['x0_rows'])
    st = fail['status']
    assert np.array_equal(np.bincount(st[nc.FAIL_ROW], minlength=T + 1), [1, 0, 40, 5, 2, 15, 7])
    keep = np.arange(P) != nc.FAIL_ROW
    assert not st[keep].any() and np.array_equal(fail['loglik'][keep], ref['loglik'][keep])
    bad = st[nc.FAIL_ROW] != 0
    assert np.isnan(fail['loglik_total'][nc.FAIL_ROW, bad]).all() and np.isfinite(fail['loglik_total'][nc.FAIL_ROW, ~bad]).all()
    for rel in (1.0 - 1e-6, 1.0 + 1e-6):
        q2 = q.copy()
        q2[nc.FAIL_ROW] *= rel
        assert np.array_equal(nso.sweep(c, c['y'], q2[nc.FAIL_ROW:nc.FAIL_ROW + 1], c['r_rows'][nc.FAIL_ROW:nc.FAIL_ROW + 1],
                                        c['x0_rows'][:1])['status'][0], st[nc.FAIL_ROW])
    # the oracle's own failure rule: a NaN measurement gives status 1 + step and NaN from there on
    y = c['y'][..., :2].copy()
    y[0, 2, 1] = np.nan
    r = nso.sweep(c, y, c['q_rows'][:2], c['r_rows'][:2], c['x0_rows'][:2])
    assert (r['status'][:, 1] == 3).all() and not r['status'][:, 0].any() and np.isnan(r['loglik_total'][:, 1]).all()
    assert np.isnan(r['loglik'][:, 2:, 1]).all() and np.array_equal(r['loglik'][:, :2, 1], ref['loglik'][:2, :2, 1])
