"""Kernel-parameter sweeps by measurement likelihood, the parts that need no device: the refusals of the C entry points (code,
message naming the range, outputs untouched) and of the Python methods (before the library is loaded), the bookkeeping of
`par_grid` / `fit_table`, and the conditions the GPU cases rest on, established on the CPU restatement alone."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _sweep_cases as sc
from tests import _sweep_oracle as swo
from tests._cases import RTOL
from tests.test_innovation_host import pendulum_user

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -3


def test_library_exports_and_declares_the_entry_points():
    from ssmtoybox_amd import _lib, ssinf
    header = open(os.path.join(ROOT, 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_filter_sweep_dev', 'ssmq_filter_sweep_kernel_name'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert 'int ' + name + '(' in header
    for cls in (ssinf.GaussianProcessKalman, ssinf.BayesSardKalman):
        for name in ('likelihood_sweep_dev', 'likelihood_sweep_batch', 'likelihood_sweep_kernel_name', 'fit_kernel_parameters'):
            assert callable(getattr(cls, name))
    assert not hasattr(ssinf.StudentProcessKalman, 'likelihood_sweep_batch')
    assert not hasattr(ssinf.MultiOutputGaussianProcessKalman, 'likelihood_sweep_batch')


def sweep_call(lib, f_dyn, f_obs, kind=(0, 0), N=(3, 3), D=1, Y=1, P=2, B=3, ld=64, T=2):
    """ssmq_filter_sweep_dev with host arrays full of a sentinel in the place of every output: (rc, message, outputs untouched)."""
    from ssmtoybox_amd import _lib
    xi = [np.ascontiguousarray(orc.points_ut(D)[:, :n] if n <= 2 * D + 1 else np.zeros((D, n))) for n in N]
    par = np.ones((max(P, 1), 1 + D))
    outs = [np.full(max(P, 1) * ld, 7.0), np.full(max(P, 1) * ld, 7.0), np.full(max(P * T * ld, 1), 7.0), np.full(max(P, 1) * ld, 7, dtype=np.int32), np.full(max(P, 1), 7, dtype=np.int32)]
    y = np.zeros(max(T, 1) * Y * ld)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    rc = lib.ssmq_filter_sweep_dev(f_dyn, f_obs, kind[0], kind[1], _lib.dp(xi[0]), N[0], _lib.dp(xi[1]), N[1], None, 0, None, 0, _lib.dp(par),
                                   _lib.dp(par), P, 1e-8, 1e-8, D, Y, B, ld, T, vp(y), _lib.dp(np.zeros(D)), _lib.dp(np.eye(D)),
                                   _lib.dp(np.eye(D)), _lib.dp(np.eye(Y)), vp(outs[0]), vp(outs[1]), vp(outs[2]), vp(outs[3]),
                                   outs[4].ctypes.data_as(_lib.c_int32_p))
    return rc, _lib.last_error(), all((o == 7).all() for o in outs)


def test_c_abi_refusals_leave_the_outputs_untouched():
    from ssmtoybox_amd import _lib, ssmod as sm
    from ssmtoybox_amd.mtran import resolve_integrand
    lib = _lib.load()
    ungm = [resolve_integrand(f)[0] for f in (sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1)).dyn_eval, sm.UNGMMeasurement(sm.GaussRV(1), 1).meas_eval)]
    ungmna = [resolve_integrand(f)[0] for f in (sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)).dyn_eval,
                                                sm.UNGMNAMeasurement(sm.GaussRV(1), 1).meas_eval)]
    UP, UM = pendulum_user()
    user = [resolve_integrand(UP(sm.GaussRV(2), sm.GaussRV(2)).dyn_eval)[0], resolve_integrand(UM(sm.GaussRV(1), 2).meas_eval)[0]]
    rng = 'D <= 6, Y <= 4, 2 <= N <= 2 D + 1'
    for kwargs, code, what in ((dict(f=user, D=2, N=(5, 5)), E_UNSUPPORTED, 'user-defined models'),
                               (dict(f=ungmna), E_UNSUPPORTED, 'non-additive noise'),
                               (dict(kind=(2, 0)), E_UNSUPPORTED, 't-process and multi-output'),
                               (dict(kind=(0, 3)), E_UNSUPPORTED, 't-process and multi-output'),
                               (dict(N=(5, 5)), E_UNSUPPORTED, 'point count out of range'),
                               (dict(N=(3, 1)), E_UNSUPPORTED, 'point count out of range'),
                               (dict(N=(3, 2)), E_UNSUPPORTED, 'no kernel for this pair'),
                               (dict(ld=70), E_ARG, 'multiple of 64'), (dict(B=65), E_ARG, 'ld a multiple of 64 and >= B'),
                               (dict(P=0), E_ARG, 'P >= 1'), (dict(T=-1), E_ARG, 'bad argument')):
        f = kwargs.pop('f', ungm)
        rc, msg, untouched = sweep_call(lib, f[0], f[1], **kwargs)
        assert rc == code and what in msg and rng in msg and untouched, (kwargs, rc, msg)
    buf = ctypes.create_string_buffer(256)
    assert lib.ssmq_filter_sweep_kernel_name(ungm[0], ungm[1], 0, 0, 3, 3, 1, 1, buf, 256) == 0
    assert buf.value.decode() == 'k_filter_sweep<D=1,Y=1,ND=3,NO=3,SSMQ_F_UNGM_DYN,SSMQ_F_UNGM_MEAS,SELO=0>'
    assert lib.ssmq_filter_sweep_kernel_name(ungmna[0], ungmna[1], 0, 0, 3, 3, 1, 1, buf, 256) == E_UNSUPPORTED


def test_python_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm, _lib
    from ssmtoybox_amd.bq import bqkern
    y, par = np.zeros((1, 4, 3)), np.ones((2, 2))

    def bare(dyn, obs, points=None, kernel=None):
        """A GaussianProcessKalman around the models without its constructor (which computes weights on the device)."""
        alg = object.__new__(ssinf.GaussianProcessKalman)

        class Tf:
            pass
        tfs = []
        for _ in range(2):
            tf, tf.model = Tf(), Tf()
            tf.model.points = orc.points_ut(dyn.dim_state) if points is None else points
            tf.model.kernel = object.__new__(kernel or bqkern.RBFGauss)
            tf.model.kernel.jitter = 1e-8
            tfs.append(tf)
        alg.mod_dyn, alg.mod_obs, alg.tf_dyn, alg.tf_obs = dyn, obs, tfs[0], tfs[1]
        alg.x0_mean, alg.x0_cov = dyn.init_rv.get_stats()[:2]
        alg.q_mean, alg.q_cov = dyn.noise_rv.get_stats()[:2]
        alg.r_mean, alg.r_cov = obs.noise_rv.get_stats()[:2]
        alg.G = dyn.noise_gain
        return alg
    g1 = lambda: sm.GaussRV(1)      # noqa: E731
    UP, UM = pendulum_user()
    cases = ((bare(sm.UNGMNATransition(g1(), g1()), sm.UNGMNAMeasurement(g1(), 1)), NotImplementedError, 'non-additive'),
             (bare(UP(sm.GaussRV(2), sm.GaussRV(2)), UM(g1(), 2)), NotImplementedError, 'user model'),
             (bare(sm.UNGMTransition(g1(), sm.StudentRV(1, dof=4.0)), sm.UNGMMeasurement(g1(), 1)), NotImplementedError, 'StudentRV'),
             (bare(sm.UNGMTransition(g1(), g1()), sm.UNGMMeasurement(sm.GaussianMixtureRV(1, (np.zeros(1), np.ones(1)), (np.eye(1), np.eye(1)),
                                                                                            (0.5, 0.5)), 1)), NotImplementedError, 'GaussianMixtureRV'),
             (bare(sm.UNGMTransition(g1(), g1()), sm.UNGMMeasurement(g1(), 1), kernel=bqkern.RBFStudent), NotImplementedError, "'rbf' kernel"),
             (bare(sm.UNGMTransition(g1(), g1()), sm.UNGMMeasurement(g1(), 1), points=orc.points_gh(1, 5)), NotImplementedError, '2 D \\+ 1 points'))

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    for alg, err, what in cases:
        for call in (lambda a: a.likelihood_sweep_batch(y, par, par), lambda a: a.fit_kernel_parameters(y, par, par),
                     lambda a: a.likelihood_sweep_dev(None, 3, 64, 4, par, par), lambda a: a.likelihood_sweep_kernel_name(2)):
            with pytest.raises(err, match=what):
                call(alg)
    ok = bare(sm.UNGMTransition(g1(), g1()), sm.UNGMMeasurement(g1(), 1))
    for pd, po in ((par, np.ones((3, 2))), (np.ones((2, 3)), par), (np.ones((0, 2)), np.ones((0, 2)))):
        with pytest.raises(ValueError, match='same P'):
            ok.likelihood_sweep_batch(y, pd, po)
    with pytest.raises(ValueError, match='dim_y, T, B'):
        ok.likelihood_sweep_batch(np.zeros((2, 4, 3)), par, par)
    with pytest.raises(ValueError, match='multiple of 64'):
        ok.likelihood_sweep_dev(None, 3, 70, 4, par, par)


def test_par_grid_and_fit_table():
    from ssmtoybox_amd import ssinf
    g = ssinf.par_grid([1.0, 2.0], [0.1, 0.3, 1.0], [5.0])
    assert g.shape == (6, 3) and g.flags['C_CONTIGUOUS']
    assert np.array_equal(g, [[1, .1, 5], [1, .3, 5], [1, 1, 5], [2, .1, 5], [2, .3, 5], [2, 1, 5]])
    assert np.array_equal(ssinf.par_grid(1.0, (3.0, 10.0)), [[1, 3], [1, 10]])
    with pytest.raises(ValueError):
        ssinf.par_grid([1.0], [])
    nan = np.nan
    ll = np.array([[-1.0, -2.0, -3.0, -4.0], [nan, nan, nan, nan], [-1.5, nan, -0.5, -0.25], [-9.0, -9.0, -9.0, 50.0]])
    st = np.array([[0, 0, 0, 0], [-1, -1, -1, -1], [0, 2, 0, 0], [0, 0, 0, 0]], dtype=np.int32)
    ts = np.array([0, 1, 0, 0], dtype=np.int32)
    # row 1 (failed weights) is skipped and does not drop trajectories; trajectory 1 failed in row 2: dropped from every row
    index, table = ssinf.fit_table(ll, st, ts)
    assert index == 3 and np.array_equal(table[[0, 2, 3]], [-8.0, -2.25, 32.0]) and np.isnan(table[1])
    st[0, 3] = 1                    # ... and trajectory 3 in row 0: the winner changes
    index, table = ssinf.fit_table(ll, st, ts)
    assert index == 2 and np.array_equal(table[[0, 2, 3]], [-4.0, -2.0, -18.0])
    st[3, 0] = st[2, 2] = 4
    with pytest.raises(ValueError, match='no trajectory is left'):
        ssinf.fit_table(ll, st, ts)
    with pytest.raises(ValueError, match='every parameter row failed'):
        ssinf.fit_table(ll, st, np.ones(4, dtype=np.int32))


def test_case_conditions_hold_on_the_oracle():
    """What tests/test_sweep_gpu.py rests on: every item of every case succeeds; the UNGM table has an interior maximum that leads the
    runner-up by more than 100 x the bound its GPU comparison allows; the planted row fails in the weights oracle."""
    eps = float(np.finfo(float).eps)
    for name in sc.SHAPES:
        ref = sc.reference(name)
        assert not ref['status'].any() and not ref['theta_status'].any(), name
        assert np.isfinite(ref['loglik']).all() and np.isfinite(ref['nis_mean']).all(), name
    c, ref = sc.case('ungm_gp'), sc.reference('ungm_gp')
    assert tuple(c['par'][:, 1]) == (0.3, 1.0, 3.0, 10.0, 30.0, 100.0)
    table = ref['loglik_total'].sum(axis=1)
    order = np.argsort(table)
    assert order[-1] == 4 and 0 < order[-1] < len(table) - 1
    margin = table[order[-1]] - table[order[-2]]
    P, T, B = ref['loglik'].shape
    bound = max(sum(max(RTOL, 64.0 * np.linalg.cond(ref['S'][p][b][..., k]) * eps) * max(1.0, abs(ref['loglik'][p, k, b]))
                    for b in range(B) for k in range(T)) for p in range(P))
    print('UNGM likelihood table {}: margin {:.4g}, bound of the GPU comparison {:.3g}'.format(table, margin, bound))
    assert margin > 100.0 * bound and margin > 10.0
    assert swo.row_weights('gp', sc.BAD_ROW, c['pts']) is None and swo.row_weights('gp', c['par'][0], c['pts']) is not None
    # the oracle's own failure rule: a NaN measurement gives status 1 + step and NaN from there on
    y = c['y'][..., :2].copy()
    y[0, 2, 1] = np.nan
    r = swo.sweep(c, y, c['par'][:2], c['par'][:2])
    assert (r['status'][:, 1] == 3).all() and not r['status'][:, 0].any() and np.isnan(r['loglik_total'][:, 1]).all()
    assert np.isnan(r['loglik'][:, 2:, 1]).all() and np.array_equal(r['loglik'][:, :2, 1], ref['loglik'][:2, :2, 1])
