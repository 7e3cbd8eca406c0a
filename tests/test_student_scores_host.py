"""Student-t measurement likelihood and the sweeps of the t-process filters, the parts that need no device: the oracle's density
against scipy, the mean of nis under the predictive t, every refusal before the library is loaded, argument validation and the
`fit_table` bookkeeping."""
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _student_score_cases as ssc
from tests import _student_score_oracle as sso
from tests.test_innovation_host import pendulum_user


@pytest.mark.parametrize('Y', (1, 2))
def test_oracle_density_is_scipys_multivariate_t(Y):
    from scipy import stats
    rng = np.random.default_rng(11)
    worst = 0.0
    for dof in (2.5, 4.0, 6.0, 30.0):
        for _ in range(20):
            a = rng.standard_normal((Y, Y))
            S, loc, y = a.dot(a.T) + 0.3 * np.eye(Y), rng.standard_normal(Y), 3.0 * rng.standard_normal(Y)
            nis, ll = sso.score(y - loc, S, dof)
            want = stats.multivariate_t(loc=loc, shape=S, df=dof).logpdf(y)
            worst = max(worst, abs(ll - want))
            assert abs(nis - (y - loc).dot(np.linalg.solve(S, y - loc))) <= 1e-12 * max(1.0, nis)
            # the long-double form is the same function
            nl, ld = sso.score(y - loc, S, dof, ld=True)
            assert abs(float(ld) - ll) <= 1e-12 * max(1.0, abs(ll)) and abs(float(nl) - nis) <= 1e-12 * max(1.0, nis)
    print('largest |oracle - scipy| logpdf, Y = {}: {:.3g}'.format(Y, worst))
    assert worst <= 1e-12
    # dof None: the Gaussian
    S, e = np.array([[2.0, 0.3], [0.3, 1.0]])[:Y, :Y], np.array([0.4, -1.1])[:Y]
    assert abs(sso.score(e, S)[1] - stats.multivariate_normal(np.zeros(Y), S).logpdf(e)) <= 1e-12


@pytest.mark.parametrize('Y', (1, 2))
def test_mean_nis_under_the_predictive_t(Y):
    """nis over 2e5 draws of the oracle's own predictive density t_6(y_mean, S_y): mean Y dof / (dof - 2) within five standard errors of
    that sample mean."""
    dof, n = 6.0, 200000
    rng = np.random.default_rng(5)
    S, loc = np.array([[2.0, 0.3], [0.3, 1.0]])[:Y, :Y], np.array([0.4, -1.1])[:Y]
    ys = sso.predictive_draws(rng, n, loc, S, dof)
    L = np.linalg.cholesky(S)
    v = np.linalg.solve(L, (ys - loc).T)
    nis = np.sum(v * v, axis=0)
    assert abs(nis[0] - sso.score(ys[0] - loc, S, dof)[0]) <= 1e-12 * max(1.0, nis[0])
    mean, se = nis.mean(), nis.std(ddof=1) / np.sqrt(n)
    print('mean nis {:.5f}, expected {:.5f}, standard error {:.5f}'.format(mean, Y * dof / (dof - 2), se))
    assert abs(mean - Y * dof / (dof - 2)) <= 5.0 * se


def no_library(monkeypatch):
    from ssmtoybox_amd import _lib

    def fail(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', fail)


def bare(kind, dyn, obs, kernel=None, points=None, dof=4.0):
    """A StudentProcessStudent ('tps') / StudentProcessKalmanSweep ('tpk') around the models without its constructor (which computes weights
    on the device): real transform objects, a stand-in for their model."""
    from ssmtoybox_amd import ssinf
    from ssmtoybox_amd.bq import bqkern, bqmtran
    alg = object.__new__(ssinf.StudentProcessStudent if kind == 'tps' else ssinf.StudentProcessKalmanSweep)

    class Model:
        pass
    tfs = []
    for _ in range(2):
        tf, tf.model = object.__new__(bqmtran.StudentTProcessTransform), Model()
        tf.model.points = orc.points_fs(dyn.dim_state, 3) if points is None else points
        tf.model.kernel = object.__new__(kernel or bqkern.RBFGauss)
        tf.model.kernel.jitter = 1e-8
        tf.model.nu = 4.0
        tfs.append(tf)
    alg.mod_dyn, alg.mod_obs, alg.tf_dyn, alg.tf_obs = dyn, obs, tfs[0], tfs[1]
    alg.x0_mean, alg.x0_cov = dyn.init_rv.get_stats()[:2]
    alg.q_mean, alg.q_cov = dyn.noise_rv.get_stats()[:2]
    alg.r_mean, alg.r_cov = obs.noise_rv.get_stats()[:2]
    alg.x0_dof = alg.q_dof = alg.r_dof = 4.0
    alg.G = dyn.noise_gain
    if kind == 'tps':
        c = (dof - 2) / dof
        alg.x_smat_0, alg.q_smat, alg.r_smat, alg.dof, alg.fixed_dof = c * alg.x0_cov, c * alg.q_cov, c * alg.r_cov, dof, True
    return alg


def test_refusals_come_before_the_library(monkeypatch):
    from ssmtoybox_amd import ssinf, ssmod as sm
    from ssmtoybox_amd.bq import bqkern
    from ssmtoybox_amd import mtran
    dyn, obs = ssc.models('ungm')
    gdyn, gobs = ssc.models('ungm', student=False)
    fs = ssinf.FullySymmetricStudent(dyn, obs, degree=3)
    tps, tpk = bare('tps', dyn, obs), bare('tpk', gdyn, gobs)
    y, par = np.zeros((1, 4, 3)), np.ones((2, 2))
    t4 = lambda d: sm.StudentRV(d, dof=4.0)      # noqa: E731
    UP, UM = pendulum_user()
    user = ssinf.FullySymmetricStudent(UP(t4(2), t4(2)), UM(t4(1), 2))
    user_tp = bare('tps', UP(t4(2), t4(2)), UM(t4(1), 2))
    na = bare('tpk', sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
    trunc = ssinf.StudentianInference(dyn, obs, mtran.TruncatedUnscentedTransform(1, 1), mtran.TruncatedUnscentedTransform(1, 1))
    other = ssinf.StudentianInference(dyn, obs, mtran.UnscentedTransform(1), mtran.UnscentedTransform(1))
    m5 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
    big = bare('tpk', sm.ReentryVehicle2DTransition(sm.GaussRV(5, m5, np.eye(5)), sm.GaussRV(3)),
               sm.Radar2DMeasurement(sm.GaussRV(2), 5, radar_loc=np.array([6374.0, 0.0])))
    big_s = bare('tps', sm.ReentryVehicle2DTransition(t4(5), t4(3)), sm.Radar2DMeasurement(t4(2), 5, radar_loc=np.array([6374.0, 0.0])))
    no_library(monkeypatch)
    # innovations* of a Studentian filter: the old error
    for alg in (fs, tps):
        for call in (lambda: alg.innovations(y[..., 0]), lambda: alg.innovations_batch(y), alg.innovations_kernel_name,
                     lambda: alg.innovations_dev(None, None, None, 3, 64, 4)):
            with pytest.raises(NotImplementedError, match='innovation scores cover the additive-noise Gaussian recursion; not implemented for the '
                                                          'Studentian recursion'):
                call()
    # user models
    for call in (lambda: user.student_scores_batch(np.zeros((1, 4, 3))), user.student_scores_kernel_name, lambda: user.student_scores_dev(None, 3, 64, 4),
                 lambda: user_tp.likelihood_sweep_batch(y, np.ones((2, 3)), np.ones((2, 3))), user_tp.likelihood_sweep_kernel_name):
        with pytest.raises(NotImplementedError, match='device_code'):
            call()
    # models that take their noise as an argument
    for call in (lambda: na.likelihood_sweep_batch(y, np.ones((2, 3)), np.ones((2, 3))), na.likelihood_sweep_kernel_name,
                 lambda: na.fit_kernel_parameters(y, np.ones((2, 3)), np.ones((2, 3)))):
        with pytest.raises(NotImplementedError, match='non-additive noise'):
            call()
    # truncated transforms, other transforms, the 'rbf-student' kernel
    with pytest.raises(NotImplementedError, match='truncated transforms'):
        trunc.student_scores_batch(y)
    with pytest.raises(NotImplementedError, match='fully-symmetric .* and t-process transforms'):
        other.student_scores_batch(y)
    for kind, models in (('tps', (dyn, obs)), ('tpk', (gdyn, gobs))):
        alg = bare(kind, *models, kernel=bqkern.RBFStudent)
        calls = [lambda: alg.likelihood_sweep_batch(y, par, par), lambda: alg.fit_kernel_parameters(y, par, par), alg.likelihood_sweep_kernel_name,
                 lambda: alg.likelihood_sweep_dev(None, 3, 64, 4, par, par)]
        if kind == 'tps':
            calls += [lambda: alg.student_scores_batch(y), alg.student_scores_kernel_name, lambda: alg.student_scores(y[..., 0])]
        for call in calls:
            with pytest.raises(NotImplementedError, match="the 'rbf' kernel; not implemented for RBFStudent"):
                call()
    # shapes without an instantiation, with the range named
    for call in (lambda: big.likelihood_sweep_batch(np.zeros((2, 3, 2)), np.ones((2, 6)), np.ones((2, 6))), big.likelihood_sweep_kernel_name,
                 lambda: big_s.likelihood_sweep_batch(np.zeros((2, 3, 2)), np.ones((2, 6)), np.ones((2, 6))),
                 lambda: big_s.student_scores_batch(np.zeros((2, 3, 2)))):
        with pytest.raises(NotImplementedError, match='D <= 4,? Y <= 2'):
            call()
    seven = bare('tps', dyn, obs, points=orc.points_gh(1, 5))
    for call in (lambda: seven.likelihood_sweep_batch(y, par, par), lambda: seven.student_scores_batch(y)):
        with pytest.raises(NotImplementedError, match='2 D \\+ 1 points'):
            call()
    # the Gaussian recursion takes Gaussian laws
    with pytest.raises(NotImplementedError, match='Gaussian initial state and noise'):
        bare('tpk', dyn, obs).likelihood_sweep_batch(y, par, par)


def test_argument_validation(monkeypatch):
    tps, tpk = bare('tps', *ssc.models('ungm')), bare('tpk', *ssc.models('ungm', student=False))
    from ssmtoybox_amd import ssinf
    fs = ssinf.FullySymmetricStudent(*ssc.models('ungm'), degree=3)
    no_library(monkeypatch)
    y, par = np.zeros((1, 4, 3)), np.ones((3, 2))
    for alg in (tps, tpk):
        with pytest.raises(ValueError, match=r'nu is a scalar or has one entry per parameter row, \(3,\)'):
            alg.likelihood_sweep_batch(y, par, par, nu=np.array([3.0, 4.0]))
        with pytest.raises(ValueError, match=r'nu is a scalar or has one entry'):
            alg.likelihood_sweep_batch(y, par, par, nu=np.ones((3, 1)))
        with pytest.raises(ValueError, match='nu of row 1 is 1.5'):
            alg.likelihood_sweep_batch(y, par, par, nu=np.array([3.0, 1.5, 4.0]))
        with pytest.raises(ValueError, match=r'\(P, 1 \+ D\)'):
            alg.likelihood_sweep_batch(y, par, np.ones((2, 2)))
    with pytest.raises(ValueError, match=r'dof is a scalar or has one entry per parameter row, \(3,\)'):
        tps.likelihood_sweep_batch(y, par, par, dof=np.array([3.0, 4.0]))
    for bad in (2.0, 1.0, np.nan):
        with pytest.raises(ValueError, match='dof of row 2 is'):
            tps.likelihood_sweep_batch(y, par, par, dof=np.array([4.0, 4.0, bad]))
    with pytest.raises(ValueError, match='dof of row 0 is 2.0'):
        tps.fit_kernel_parameters(y, par, par, dof=2.0)
    with pytest.raises(ValueError, match='dof is the Studentian filters'):
        tpk.likelihood_sweep_batch(y, par, par, dof=4.0)
    with pytest.raises(ValueError, match='dof is the Studentian filters'):
        tpk.likelihood_sweep_dev(None, 3, 64, 4, par, par, dof=np.full(3, 4.0))
    with pytest.raises(ValueError, match=r'data is \(dim_y, T, B\)'):
        fs.student_scores_batch(np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match='multiple of 64'):
        fs.student_scores_dev(None, 3, 70, 4)
    # the rows' scale matrices are the constructor's: (dof - 2) / dof times the laws' scale matrices
    s = tps._sweep_setup(par, par, nu=np.array([3.0, 4.0, 5.0]), dof=np.array([4.0, 6.0, 8.0]))
    assert np.array_equal(s['nu'][0], [3.0, 4.0, 5.0]) and np.array_equal(s['nu'][1], [3.0, 4.0, 5.0]) and np.array_equal(s['dof'], [4.0, 6.0, 8.0])
    S0, gqg, rr = s['keep'][-3:]
    for p, d in enumerate((4.0, 6.0, 8.0)):
        c = (d - 2) / d
        assert np.array_equal(S0[p], c * tps.x0_cov) and np.array_equal(gqg[p], tps.G.dot(c * tps.q_cov).dot(tps.G.T)) and np.array_equal(rr[p], c * tps.r_cov)
    s = tpk._sweep_setup(par, par)
    assert s['dof'] is None and np.array_equal(s['nu'][0], np.full(3, 4.0)) and np.array_equal(s['keep'][-3][2], tpk.x0_cov)


def test_where_the_methods_live():
    """`StudentProcessKalman` keeps no sweep of its own (tests/test_sweep_host.py); `StudentProcessKalmanSweep` is that filter with one."""
    import ctypes
    import os
    from ssmtoybox_amd import _lib, ssinf
    sweep = ('likelihood_sweep_dev', 'likelihood_sweep_batch', 'likelihood_sweep_kernel_name', 'fit_kernel_parameters')
    scores = ('student_scores', 'student_scores_batch', 'student_scores_dev', 'student_scores_kernel_name')
    for cls in (ssinf.StudentProcessKalmanSweep, ssinf.StudentProcessStudent):
        assert all(callable(getattr(cls, name)) for name in sweep)
    for cls in (ssinf.FullySymmetricStudent, ssinf.StudentProcessStudent):
        assert all(callable(getattr(cls, name)) for name in scores)
    assert not any(hasattr(ssinf.StudentProcessKalman, name) for name in sweep + scores)
    assert not any(hasattr(ssinf.FullySymmetricStudent, name) for name in sweep)
    assert issubclass(ssinf.StudentProcessKalmanSweep, ssinf.StudentProcessKalman)
    assert ssinf.StudentProcessKalmanSweep.__init__ is ssinf.StudentProcessKalman.__init__
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ssmq.h')).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ('ssmq_student_scores_dev', 'ssmq_student_scores_kernel_name', 'ssmq_filter_sweep_t_dev', 'ssmq_filter_sweep_t_kernel_name'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and 'int ' + name + '(' in header


def test_fit_table_with_a_failed_row():
    from ssmtoybox_amd.ssinf import fit_table, par_grid
    ll = np.array([[1.0, 2.0, 3.0], [np.nan, np.nan, np.nan], [4.0, np.nan, 0.5], [0.0, 9.0, 1.0]])
    st = np.array([[0, 0, 0], [-1, -1, -1], [0, 2, 0], [0, 0, 0]])
    index, table = fit_table(ll, st, np.array([0, 1, 0, 0]))
    # trajectory 1 failed in row 2: every row is summed over trajectories 0 and 2; the failed row is NaN and never chosen
    assert index == 2 and np.isnan(table[1]) and np.array_equal(table[[0, 2, 3]], [4.0, 4.5, 1.0])
    assert par_grid([1.0, 1.2], [1.0, 3.0, 10.0]).shape == (6, 2)


def test_the_bad_row_fails_on_the_cpu():
    """The row the GPU test expects to fail: the oracle's kernel matrix is not positive definite at the case's jitter."""
    from tests import _sweep_oracle as swo
    assert swo.row_weights('gp', ssc.BAD_ROW['ungm'], orc.points_fs(1, 3)) is None
    for row in ssc.ROWS['ungm'][0]:
        assert swo.row_weights('gp', row, orc.points_fs(1, 3)) is not None
