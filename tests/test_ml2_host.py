"""
ML-II (type-II maximum likelihood of the RBF kernel's parameters) without a device: the analytic-gradient mode of the
BFGS state machine (csrc/ssmq_bfgs.h, bfgs_advance_jac) against scipy.optimize.minimize(method='BFGS', jac=True) on host
objectives with exact gradients, and the refusals and warnings of Model.optimize, which all come before any device call.
"""
import ctypes
import warnings

import numpy as np
import pytest
from scipy.optimize import minimize

from ssmtoybox_amd import _lib
from ssmtoybox_amd.bq.bqmod import GaussianProcessModel, StudentTProcessModel

OBJG = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double))


def lockstep_jac(fgs, x0, gtol=1e-5, maxiter=-1):
    """fgs[b](theta) -> (value, gradient); x0 (B, P).  Returns a dict of the per-run results."""
    lib = _lib.load()
    B, P = x0.shape

    def cb(ctx, n, p, traj, rows, vals, grads):
        r = np.ctypeslib.as_array(rows, shape=(n, p))
        t = np.ctypeslib.as_array(traj, shape=(n,))
        v = np.ctypeslib.as_array(vals, shape=(n,))
        g = np.ctypeslib.as_array(grads, shape=(n, p))
        for i in range(n):
            v[i], g[i] = fgs[int(t[i])](r[i].copy())
        return 0
    theta = np.ascontiguousarray(x0, dtype=np.float64).copy()
    fun, jac, hinv = np.empty(B), np.empty((B, P)), np.empty((B, P, P))
    st, nit, nfev = (np.zeros(B, dtype=np.int32) for _ in range(3))
    fn = OBJG(cb)
    rc = lib.ssmq_bfgs_jac_lockstep_host(ctypes.cast(fn, ctypes.c_void_p), None, B, P, float(gtol), int(maxiter),
                                         theta.ctypes.data_as(_lib.c_double_p), fun.ctypes.data_as(_lib.c_double_p),
                                         jac.ctypes.data_as(_lib.c_double_p), hinv.ctypes.data_as(_lib.c_double_p),
                                         st.ctypes.data_as(_lib.c_int32_p), nit.ctypes.data_as(_lib.c_int32_p),
                                         nfev.ctypes.data_as(_lib.c_int32_p))
    assert rc == 0
    return dict(x=theta, fun=fun, jac=jac, hess_inv=hinv, status=st, nit=nit, nfev=nfev)


def make_objectives(rng, B, P):
    """The objective families of test_bfgs_lockstep.py, each with its exact gradient."""
    fgs = []
    for b in range(B):
        kind = b % 4
        a = rng.standard_normal((P, P))
        A = a.dot(a.T) + 0.5 * np.eye(P)
        c = rng.standard_normal(P)
        if kind == 0:       # convex quadratic
            fgs.append(lambda x, A=A, c=c: (0.5 * (x - c).dot(A).dot(x - c), A.dot(x - c)))
        elif kind == 1:     # Rosenbrock chain
            def rosen(x):
                d = x[1:] - x[:-1] ** 2
                g = np.zeros_like(x)
                g[:-1] = -400.0 * x[:-1] * d - 2 * (1 - x[:-1])
                g[1:] += 200.0 * d
                return float(np.sum(100.0 * d ** 2 + (1 - x[:-1]) ** 2)), g
            fgs.append(rosen)
        elif kind == 2:     # log-sum-exp + quadratic
            def lse(x, A=A, c=c):
                z = A.dot(x) * 0.3
                w = np.exp(z - z.max())
                return (float(np.log(np.sum(np.exp(z))) + 0.05 * x.dot(x) + c.dot(x) * 0.1),
                        0.3 * A.T.dot(w / w.sum()) + 0.1 * x + 0.1 * c)
            fgs.append(lse)
        else:               # a negative Gaussian log-density in exp(theta) plus a prior
            def dens(x, c=c):
                e = np.exp(x)
                r = e - np.exp(0.3 * c)
                return float(0.5 * np.sum(r ** 2) + 0.5 * x.dot(x)), r * e + x
            fgs.append(dens)
    return fgs


@pytest.mark.parametrize('P', [1, 2, 4, 6, 8, 12, 17])
def test_jac_lockstep_follows_scipy(P):
    rng = np.random.default_rng(300 + P)
    B = 12
    fgs = make_objectives(rng, B, P)
    if P == 1:
        fgs = [f for i, f in enumerate(fgs) if i % 4 != 1]          # (the Rosenbrock chain needs two variables)
        B = len(fgs)
    x0 = 0.5 * rng.standard_normal((B, P))
    r = lockstep_jac(fgs, x0)
    for b in range(B):
        ref = minimize(fgs[b], x0[b], method='BFGS', jac=True)
        assert r['status'][b] == ref.status, (b, r['status'][b], ref.status, ref.message)
        if P > 6 and b % 4 == 1:
            # the Rosenbrock chains at P = 8 .. 17 (ML-II's P = D + 1 up to 17), 50 - 110 iterations: the two roundings of
            # the updates part after tens of iterations (measured: nit +-1, x to 2.5e-7 of its largest entry, hess_inv to
            # 0.14 of its largest entry, fun to 6e-14) - the same minimiser, not the same path
            assert abs(r['nit'][b] - ref.nit) <= 1 and r['nfev'][b] >= ref.nfev - 1, (b, r['nit'][b], ref.nit)
            assert np.abs(r['x'][b] - ref.x).max() <= 1e-6 * max(1.0, np.abs(ref.x).max()), b
            assert np.abs(r['hess_inv'][b] - ref.hess_inv).max() <= 0.5 * np.abs(ref.hess_inv).max(), b
            assert abs(r['fun'][b] - ref.fun) <= 1e-12 * max(1.0, abs(ref.fun))
            continue
        assert r['nit'][b] == ref.nit, (b, r['nit'][b], ref.nit)
        assert r['nfev'][b] >= ref.nfev - 1
        # the same path (above); x to the last bits (measured: <= 4e-12 of its largest entry).  hess_inv: numpy's dot
        # (OpenBLAS, fused multiply-adds) and this code's loops round differently, and the last updates divide differences
        # of near-equal gradients by yk'sk: measured up to 5e-8 of the largest entry on the Rosenbrock chains and the
        # log-sum-exp family at P >= 4, <= 2e-12 on the other families
        assert np.abs(r['x'][b] - ref.x).max() <= 2e-11 * max(1.0, np.abs(ref.x).max()), b
        # P = 8 .. 17 (measured): <= 3.3e-8 on the log-sum-exp family, <= 3.6e-10 on the others
        hbar = 1e-6 if b % 4 in (1, 2) else (1e-10 if P <= 6 else 2e-9)
        assert np.abs(r['hess_inv'][b] - ref.hess_inv).max() <= hbar * np.abs(ref.hess_inv).max(), b
        assert abs(r['fun'][b] - ref.fun) <= 1e-12 * max(1.0, abs(ref.fun))


def test_jac_lockstep_options_and_maxiter():
    # gtol and maxiter are honoured as minimize(options=...) honours them, maxiter = 0 included (status 1 at the start)
    rng = np.random.default_rng(7)
    fgs = make_objectives(rng, 4, 3)
    x0 = 0.5 * rng.standard_normal((4, 3))
    for gtol, maxiter in ((1e-3, -1), (1e-5, 3), (1e-5, 0)):
        r = lockstep_jac(fgs, x0, gtol=gtol, maxiter=maxiter)
        opts = {'gtol': gtol} if maxiter < 0 else {'gtol': gtol, 'maxiter': maxiter}
        for b in range(4):
            ref = minimize(fgs[b], x0[b], method='BFGS', jac=True, options=opts)
            assert (r['status'][b], r['nit'][b]) == (ref.status, ref.nit), (gtol, maxiter, b, ref.message)
            assert np.abs(r['x'][b] - ref.x).max() <= 2e-11 * max(1.0, np.abs(ref.x).max()), (gtol, maxiter, b)


def test_jac_lockstep_nan_objective():
    fgs = [lambda x: (float('nan'), np.full_like(x, np.nan)), lambda x: (float(x.dot(x)), 2 * x)]
    x0 = np.array([[0.3, -0.2], [0.5, 0.5]])
    r = lockstep_jac(fgs, x0)
    ref = minimize(fgs[0], x0[0], method='BFGS', jac=True)
    assert r['status'][0] == ref.status == _lib.BFGS_NAN and r['nit'][0] == ref.nit == 0
    assert r['status'][1] == 0 and np.abs(r['x'][1]).max() < 1e-6


def _gp(D):
    return GaussianProcessModel(D, np.ones((1, D + 1)), 'rbf', 'ut')


def test_refusals_name_the_range():
    m = _gp(1)
    for x, y, x0 in ((np.zeros((1, 129)), np.zeros((129, 1)), np.zeros(2)),       # N = 129
                     (np.zeros((17, 5)), np.zeros((5, 1)), np.zeros(18)),          # D = 17
                     (np.zeros((1, 5)), np.zeros((5, 17)), np.zeros(2))):          # E = 17
        with pytest.raises(NotImplementedError, match='N <= 128'):
            m.optimize(x0, y, x)
        with pytest.raises(NotImplementedError, match='D <= 16'):
            m.neg_log_marginal_likelihood(x0, y, x, 1e-8 * np.eye(x.shape[1]))
        with pytest.raises(NotImplementedError, match='E <= 16'):
            m.optimize_batch(x0, y[None], x)
    with pytest.raises(NotImplementedError, match='BFGS'):
        m.optimize(np.zeros(2), np.zeros((3, 1)), np.zeros((1, 3)), method='L-BFGS-B')
    with pytest.raises(NotImplementedError):
        StudentTProcessModel(1, np.ones((1, 2)), 'rbf', 'ut').optimize(np.zeros(2), np.zeros((3, 1)), np.zeros((1, 3)),
                                                                       method='Nelder-Mead')


def test_two_dimensional_start_is_refused_as_scipy_refuses_it():
    # the reference's tests pass (1, P) starts (tests/test_bqmod.py:167, 581); SciPy 1.15 refuses them
    with pytest.raises(ValueError) as ref:
        minimize(lambda x: (float(x.dot(x)), 2 * x), np.zeros((1, 2)), method='BFGS', jac=True)
    with pytest.raises(ValueError) as mine:
        _gp(1).optimize(np.zeros((1, 2)), np.zeros((3, 1)), np.zeros((1, 3)))
    assert str(mine.value) == str(ref.value)


def test_constraints_and_bounds_warn_as_scipy():
    con = {'type': 'eq', 'fun': lambda lp: np.exp(lp[0]) ** 2 - 1}
    bnd = ((None, None), (None, None))
    with warnings.catch_warnings(record=True) as ref:
        warnings.simplefilter('always')
        minimize(lambda x: (float(x.dot(x)), 2 * x), np.ones(2), method='BFGS', jac=True, constraints=con, bounds=bnd)
    ref = [(w.category, str(w.message)) for w in ref if issubclass(w.category, RuntimeWarning)]
    assert ('Method BFGS cannot handle constraints.' in [m for _, m in ref])
    with warnings.catch_warnings(record=True) as mine:
        warnings.simplefilter('always')
        with pytest.raises(NotImplementedError):        # the range refusal comes after the warnings, before the device
            _gp(1).optimize(np.zeros(2), np.zeros((129, 1)), np.zeros((1, 129)), method='BFGS', constraints=con,
                            bounds=bnd)
    mine = [(w.category, str(w.message)) for w in mine if issubclass(w.category, RuntimeWarning)]
    assert mine == ref


def test_bayes_sard_has_no_likelihood():
    from ssmtoybox_amd.bq.bqmod import BayesSardModel
    m = BayesSardModel(1, np.ones((1, 2)))
    assert m.neg_log_marginal_likelihood(np.zeros(2), np.zeros((3, 1)), np.zeros((1, 3)), 0.0) is None
    with pytest.raises(NotImplementedError):
        m.optimize(np.zeros(2), np.zeros((3, 1)), np.zeros((1, 3)))
