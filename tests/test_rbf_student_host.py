"""The 'rbf-student' kernel without a device: the public surface (kernel, model, filter keyword), the range refusals raised in
Python before the library is loaded, and the exact mixture oracle (tests/_student_oracle.py) against the reference's recorded
Monte Carlo (tests/golden/g18_rbf_student.npz)."""
import os

import numpy as np
import pytest

from tests import _student_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g18_rbf_student.npz')
Z = 6.0


def test_get_kernel_builds_rbf_student():
    from ssmtoybox_amd.bq.bqkern import RBFStudent, RBFGauss
    from ssmtoybox_amd.bq.bqmod import Model
    par = np.array([[1.5, 3.0, 3.0]])
    k = Model.get_kernel(2, 'rbf-student', par)
    assert isinstance(k, RBFStudent) and isinstance(k, RBFGauss)
    # the reference's attributes with the constructor's defaults (bq/bqkern.py:463-474)
    assert k.dof == 4.0 and k.num_samples == 2000000 and k.num_batches == 1000 and k.batch_size == 2000
    assert np.array_equal(k.scale_mat, np.eye(2)) and np.array_equal(k.mean, np.zeros(2))
    assert k.seed == 0 and k.jitter == 1e-8 and np.array_equal(k.par, par)
    assert k.supports_parameter_estimation is False
    assert k.exp_x_kxx(par) == 2.25
    k2 = RBFStudent(2, par, 1e-8, 6.0, 1e5, 10, seed=7)
    assert (k2.dof, k2.num_samples, k2.num_batches, k2.batch_size, k2.seed) == (6.0, 100000, 10, 10000, 7)


def test_rbf_student_is_a_supported_kernel():
    from ssmtoybox_amd.bq.bqmod import Model
    assert 'rbf-student' in Model._supported_kernels_ and 'rbf' in Model._supported_kernels_
    assert 'rq' not in Model._supported_kernels_


def test_student_process_student_accepts_kernel_keyword():
    import inspect
    from ssmtoybox_amd import ssinf
    sig = inspect.signature(ssinf.StudentProcessStudent.__init__)
    names = list(sig.parameters)
    assert names[-2:] == ['kernel', 'mc']
    assert sig.parameters['kernel'].default == 'rbf' and sig.parameters['mc'].default is None
    from ssmtoybox_amd import ssmod
    dyn = ssmod.UNGMTransition(ssmod.StudentRV(1), ssmod.StudentRV(1))
    obs = ssmod.UNGMMeasurement(ssmod.StudentRV(1), 1)
    par = np.array([[1.0, 1.0]])
    with pytest.raises(ValueError):
        ssinf.StudentProcessStudent(dyn, obs, par, par, kernel='rq')
    with pytest.raises(ValueError):
        ssinf.StudentProcessStudent(dyn, obs, par, par, mc={'seed': 1})


def test_range_refusals_before_the_library_is_loaded(monkeypatch):
    from ssmtoybox_amd import _lib
    from ssmtoybox_amd.bq.bqkern import RBFStudent

    def no_load():
        raise AssertionError('the library was loaded before the range check')

    monkeypatch.setattr(_lib, 'load', no_load)
    k = RBFStudent(17, np.ones((1, 18)))
    with pytest.raises(NotImplementedError, match='D <= 16'):
        k.exp_x_kx(k.par, np.zeros((17, 3)))
    with pytest.raises(NotImplementedError, match='D <= 16'):
        k.exp_xy_kxy(k.par)
    k = RBFStudent(2, np.ones((1, 3)))
    with pytest.raises(NotImplementedError, match='N <= 128'):
        k.exp_x_kxkx(k.par, k.par, np.zeros((2, 129)))
    with pytest.raises(NotImplementedError, match='N <= 128'):
        k.exp_x_xkx(k.par, np.zeros((2, 129)))
    for bad in (0, 2 ** 31):
        k.num_samples = bad
        with pytest.raises(NotImplementedError, match='num_samples'):
            k.exp_x_kx(k.par, np.zeros((2, 5)))
        with pytest.raises(NotImplementedError, match='num_samples'):
            k.exp_xy_kxy(k.par)
    k.num_samples = 1000
    for bad in (0.0, -1.0, float('nan')):
        k.dof = bad
        with pytest.raises(NotImplementedError, match='dof > 0'):
            k.expectations(k.par, np.zeros((2, 5)))


def test_optimize_refused_for_rbf_student(monkeypatch):
    from ssmtoybox_amd import _lib
    from ssmtoybox_amd.bq.bqmod import GaussianProcessModel, StudentTProcessModel
    monkeypatch.setattr(_lib, 'load', lambda: (_ for _ in ()).throw(AssertionError('library loaded')))
    for cls in (GaussianProcessModel, StudentTProcessModel):
        m = cls(1, np.array([[1.0, 1.0]]), 'rbf-student', 'fs', {'degree': 3})
        assert np.array_equal(m.points, np.array([[0.0, 3.0, -3.0]])) or m.points.shape == (1, 3)
        with pytest.raises(NotImplementedError, match='parameter estimation'):
            m.optimize(np.zeros(2), np.zeros(3), m.points)
        with pytest.raises(NotImplementedError, match='parameter estimation'):
            m.optimize_batch(np.zeros(2), np.zeros((1, 3, 1)), m.points)


@pytest.mark.parametrize('case', so.CASES, ids=[c[0] for c in so.CASES])
def test_oracle_against_reference_monte_carlo(case):
    """Every entry of the reference's recorded q, R, Q within 6 standard errors of the oracle, the standard error from the
    oracle's exact per-sample variance and the fixture's sample count; the recorded batch sums of exp_xy_kxy likewise, with
    their own recorded variance."""
    name, D, ell, deg, N, alpha, dof = case
    g = np.load(GOLDEN)
    x, par, S = g[name + '_x'], g[name + '_par'], int(g[name + '_num_samples'])
    assert x.shape == (D, N) and float(g[name + '_dof']) == dof and np.array_equal(par, [alpha] + [ell] * D)
    assert np.array_equal(x, so.fs_points(D, deg))
    if name == 'd1_fs3':
        assert np.array_equal(x, [[0.0, 3.0, -3.0]])
    o = so.expectations(x, par, dof)
    worst = {}
    for key in ('q', 'R', 'Q'):
        var = o['var_' + key]
        assert np.all(var >= -1e-12)
        bound = Z * np.sqrt(np.maximum(var, 0.0) / S)
        # an entry whose term is constant (x_d k_i with xi_id = 0 has variance > 0; only exact zeros) needs no slack
        ratio = np.abs(g[name + '_' + key] - o[key]) / np.where(bound > 0, bound, 1.0)
        worst[key] = float(ratio.max())
        print('{} {}: worst entry at {:.3f} of the 6-sigma bound, 1/sqrt(S) = {:.2e}'.format(name, key, worst[key], S ** -0.5))
        assert np.all(np.abs(g[name + '_' + key] - o[key]) <= bound), (key, worst[key])
    mean_t, var_t = float(g[name + '_kxy_mean']), float(g[name + '_kxy_var'])
    exact = so.kxy_batch_mean(par, dof)
    bound = Z * np.sqrt(var_t / so.KXY_BATCHES)
    print('{} kxy: batch mean {:.4f} exact {:.4f} bound {:.4f}'.format(name, mean_t, exact, bound))
    assert abs(mean_t - exact) <= bound


def test_oracle_tells_gaussian_and_other_dof_apart():
    """The oracle's own resolution: at 2e6 samples the Gaussian closed form and the nu = 5 expectation lie outside the 6-sigma
    bound of the nu = 4 oracle (D = 2 case), so a test with this bound can fail."""
    name, D, ell, deg, N, alpha, dof = so.CASES[1]
    x, par = so.fs_points(D, deg), np.array([alpha] + [ell] * D)
    o4, o5 = so.expectations(x, par, 4.0), so.expectations(x, par, 5.0)
    bound = Z * np.sqrt(o4['var_q'] / 2e6)
    h = par[1:] ** 2
    gauss = np.prod(np.sqrt(h[:, None] / (h[:, None] + 1.0)) * np.exp(-0.5 * x ** 2 / (h[:, None] + 1.0)), axis=0)
    assert np.all(np.abs(gauss - o4['q']) > bound)
    assert np.max(np.abs(o5['q'] - o4['q']) / bound) > 1.0
