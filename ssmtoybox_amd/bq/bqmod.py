"""
Integrand models of Bayesian quadrature: kernel + point set -> quadrature weights (reference: ssmtoybox/bq/bqmod.py).

The weights are computed on the device (`ssmq_weights_gp` / `ssmq_weights_bs`, ssmtoybox_amd/csrc/ssmq_weights.hip);
this module keeps the reference's attribute surface: `points`, `kernel`, `dim_in`, `num_pts`, `q`, `Q`, `R`, `iK`,
`model_var`, `integral_var`, `nu`, `mulind` (bq/bqmod.py:85-106) and the `bq_weights(par, *args)` /
`exp_model_variance` / `integral_variance` methods the reference's tests and research scripts call.
Type-II maximum likelihood of the kernel parameters - `neg_log_marginal_likelihood` and `optimize` (bq/bqmod.py:250-285,
537-596, 1191-1245) - runs on the device too (`ssmq_gp_nlml_batch` / `ssmq_gp_ml2_batch`), with batched forms that fit
many data sets in one launch.  Prediction - `predict` of the three model families (bq/bqmod.py:454-493, 840-891,
1090-1130) and `predict_batch`, which takes the layout of `optimize_batch` so that fits chain into predictions - runs on
the device as well (`ssmq_gp_predict_batch`).  The multi-output models (bq/bqmod.py:1248-1560: one kernel-parameter row per
output) get their weights from `ssmq_weights_gp_mo`.  `plot_model` (matplotlib, host-only) is out of scope.
"""
import warnings

import numpy as np

from .. import _lib
from ..mtran import (SphericalRadialTransform, UnscentedTransform, GaussHermiteTransform,
                     FullySymmetricStudentTransform)
from .bqkern import (RBFGauss, RBFStudent, RBFGaussDer, device_gp_weights, device_student_weights, device_gpqd_weights,
                     check_which_der)


def n_sum_k(n, k):
    """Multi-indices of total degree k as columns of an (n, .) integer array, in the column order the reference's
    `utils.n_sum_k` produces (utils.py:459-475) - the order fixes the column order of the Vandermonde matrix and with
    it the Bayes-Sard weights.  Built degree by degree: level 1 is e_0 .. e_{n-1}; level d + 1 raises the first n - 1
    columns of level d by every e_j with j >= the column's position, then raises every remaining column by e_{n-1}.
    For k <= 2 that enumerates all n-tuples summing to k in lexicographic order of the index pair; for k >= 3 it is the
    reference's (incomplete) set, kept as is (pinned by tests/golden/g1_points.npz: nsumk_*)."""
    if k < 0:
        raise ValueError('k must be non-negative')
    if k == 0:
        return np.zeros((n, 1), dtype=int)
    unit = [tuple(int(r == j) for r in range(n)) for j in range(n)]
    level = list(unit)
    for _ in range(k - 1):
        head = [tuple(a + b for a, b in zip(level[i], unit[j])) for i in range(n - 1) for j in range(i, n)]
        tail = [tuple(a + b for a, b in zip(col, unit[n - 1])) for col in level[n - 1:]]
        level = head + tail
    return np.array(level, dtype=int).T.reshape(n, -1)


ML2_MAX_DIM, ML2_MAX_PTS, ML2_MAX_OUT = 16, 128, 16
_ML2_RANGE = 'ML-II on the device supports D <= 16 inputs, N <= 128 data points and E <= 16 outputs'
# scipy.optimize._optimize._status_message for the BFGS warnflags 0 .. 3
_BFGS_MESSAGES = ('Optimization terminated successfully.', 'Maximum number of iterations has been exceeded.',
                  'Desired error not necessarily achieved due to precision loss.', 'NaN result encountered.')


def _ml2_inputs(log_par, fcn_obs, x_obs, jitter=None):
    """Shapes and range checks shared by the ML-II entry points, before any device call.  log_par (B, P); fcn_obs (B, N, E);
    x_obs (D, N) or (B, D, N).  Returns C-contiguous float64 arrays and (D, N, E, B, x_per_fit)."""
    lp = np.ascontiguousarray(log_par, dtype=np.float64)
    y = np.asarray(fcn_obs, dtype=np.float64)
    x = np.asarray(x_obs, dtype=np.float64)
    if lp.ndim != 2 or y.ndim != 3 or x.ndim not in (2, 3):
        raise ValueError('log_par must be (B, P), fcn_obs (B, N, E) and x_obs (D, N) or (B, D, N)')
    B, P = lp.shape
    D, N = x.shape[-2:]
    E = y.shape[2]
    if D > ML2_MAX_DIM or N > ML2_MAX_PTS or E > ML2_MAX_OUT:
        raise NotImplementedError('{}; got D = {}, N = {}, E = {}'.format(_ML2_RANGE, D, N, E))
    if P != D + 1:
        raise ValueError('log_par needs 1 + dim = {} entries per row, got {}'.format(D + 1, P))
    if y.shape[:2] != (B, N) or (x.ndim == 3 and x.shape[0] != B):
        raise ValueError('fcn_obs must be ({0}, {1}, E) and x_obs ({2}, {1}) or ({0}, {2}, {1})'.format(B, N, D))
    if jitter is None:
        jitter = 1e-8 * np.eye(N)
    jit = np.ascontiguousarray(np.broadcast_to(np.asarray(jitter, dtype=np.float64), (N, N)))
    return lp, np.ascontiguousarray(y), np.ascontiguousarray(x), jit, (D, N, E, B, int(x.ndim == 3))


def _nlml_batch(log_par, fcn_obs, x_obs, jitter, nu):
    """(B,) values, (B, P) gradients and (B,) status (1: K not positive definite, value and gradient NaN)."""
    lp, y, x, jit, (D, N, E, B, per_fit) = _ml2_inputs(log_par, fcn_obs, x_obs, jitter)
    f, pf = _lib.out_c((B,))
    g, pg = _lib.out_c((B, D + 1))
    st = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.load().ssmq_gp_nlml_batch(D, N, E, B, _lib.as_c(x)[1], per_fit, _lib.as_c(y)[1], _lib.as_c(jit)[1],
                                              float(nu), _lib.as_c(lp)[1], pf, pg, st.ctypes.data_as(_lib.c_int32_p)),
               'ssmq_gp_nlml_batch')
    return f, g, st


def _ml2_options(options):
    """gtol and maxiter of scipy's BFGS (the only options the device optimiser takes); norm must stay inf."""
    options = dict(options or {})
    gtol = float(options.pop('gtol', 1e-5))
    maxiter = options.pop('maxiter', None)
    norm = options.pop('norm', np.inf)
    options.pop('disp', None)
    if norm != np.inf:
        raise NotImplementedError('ML-II on the device uses the max-norm of the gradient (norm=inf)')
    if options:
        raise NotImplementedError('BFGS options other than gtol, maxiter, norm=inf and disp are not supported on the device: '
                                  '{}'.format(sorted(options)))
    return gtol, (-1 if maxiter is None else int(maxiter))


def _ml2_batch(log_par_0, fcn_obs, x_obs, nu, gtol, maxiter, jitter=None):
    lp, y, x, jit, (D, N, E, B, per_fit) = _ml2_inputs(log_par_0, fcn_obs, x_obs, jitter)
    P = D + 1
    out = {k: _lib.out_c(sh) for k, sh in (('x', (B, P)), ('fun', (B,)), ('jac', (B, P)), ('hess_inv', (B, P, P)))}
    st, nit, nfev = (np.zeros(B, dtype=np.int32) for _ in range(3))
    _lib.check(_lib.load().ssmq_gp_ml2_batch(D, N, E, B, _lib.as_c(x)[1], per_fit, _lib.as_c(y)[1], _lib.as_c(jit)[1],
                                             float(nu), float(gtol), int(maxiter), _lib.as_c(lp)[1], out['x'][1],
                                             out['fun'][1], out['jac'][1], out['hess_inv'][1],
                                             st.ctypes.data_as(_lib.c_int32_p), nit.ctypes.data_as(_lib.c_int32_p),
                                             nfev.ctypes.data_as(_lib.c_int32_p)), 'ssmq_gp_ml2_batch')
    res = {k: v[0] for k, v in out.items()}
    res.update(status=st, success=st == 0, nit=nit, nfev=nfev, njev=nfev.copy())
    return res


def _predict_batch(model, test_data, fcn_obs, x_obs, par, nu=0.0, mulind=None):
    """Shapes and range checks of `predict_batch`, before any device call, then `ssmq_gp_predict_batch`.  Returns the dict of
    `predict_batch`."""
    y = np.asarray(fcn_obs, dtype=np.float64)
    if y.ndim == 2:
        y = y[..., None]
    x = np.asarray(model.points if x_obs is None else x_obs, dtype=np.float64)
    t = np.asarray(test_data, dtype=np.float64)
    p = model.kernel.get_parameters(par)
    if y.ndim != 3 or x.ndim not in (2, 3) or t.ndim not in (2, 3) or p.ndim != 2:
        raise ValueError('fcn_obs must be (B, N, E), x_obs (D, N) or (B, D, N), test_data (D, M) or (B, D, M) and par '
                         '(1 + D,) or (B, 1 + D)')
    B, N, E = y.shape
    D, M = t.shape[-2:]
    NB = 0
    if mulind is not None:
        mulind = np.asarray(mulind)
        if mulind.ndim != 2:
            raise ValueError('the multi-index matrix must be (dim, num_basis), got {}'.format(mulind.shape))
        NB = mulind.shape[1]
    if D > ML2_MAX_DIM or x.shape[-2] > ML2_MAX_DIM or x.shape[-1] > ML2_MAX_PTS or N > ML2_MAX_PTS or E > ML2_MAX_OUT:
        raise NotImplementedError('{} (prediction has the range of ML-II); got D = {}, N = {}, E = {}'.format(
            _ML2_RANGE.replace('ML-II', 'prediction'), max(D, x.shape[-2]), max(N, x.shape[-1]), E))
    if M < 1 or M > 2 ** 31 - 1:
        raise NotImplementedError('prediction on the device needs 1 <= M <= 2^31 - 1 test points, got M = {}'.format(M))
    if NB > x.shape[-1]:
        raise NotImplementedError('Bayes-Sard prediction on the device needs num_basis <= N; got {} basis functions on {} '
                                  'points'.format(NB, x.shape[-1]))
    if nu != 0.0 and E != 1:
        # the reference's fcn_obs.T.dot(iK) fails for more than one output (bq/bqmod.py:1129)
        raise ValueError('the Student-t process predicts one output: fcn_obs must be (N,) or (1, N), got E = {}'.format(E))
    if x.shape[-2:] != (D, N) or (x.ndim == 3 and x.shape[0] != B) or (t.ndim == 3 and t.shape[0] != B):
        raise ValueError('x_obs must be ({0}, {1}) or ({2}, {0}, {1}) and test_data ({0}, M) or ({2}, {0}, M)'.format(D, N, B))
    if NB and mulind.shape[0] != D:
        raise ValueError('the multi-index matrix must be (dim, num_basis) = ({}, .), got {}'.format(D, mulind.shape))
    if p.shape[1] != D + 1 or p.shape[0] not in (1, B):
        raise ValueError('par needs 1 + dim = {} entries per row and 1 or {} rows, got {}'.format(D + 1, B, p.shape))
    if nu != 0.0 and not nu > 2.0:
        raise ValueError('the Student-t process needs nu > 2, got {}'.format(nu))
    p = np.ascontiguousarray(np.broadcast_to(p, (B, D + 1)), dtype=np.float64)
    mean, pm = _lib.out_c((B, M, E))
    var, pv = _lib.out_c((B, M))
    st = np.zeros(B, dtype=np.int32)
    mi = np.ascontiguousarray(mulind, dtype=np.int32) if NB else None
    _lib.check(_lib.load().ssmq_gp_predict_batch(
        D, N, E, B, _lib.as_c(x)[1], int(x.ndim == 3), _lib.as_c(y)[1], float(model.kernel.jitter), float(nu),
        int(model.num_pts), _lib.as_c(p)[1], mi.ctypes.data_as(_lib.c_int32_p) if NB else None, NB, M, _lib.as_c(t)[1],
        int(t.ndim == 3), pm, pv, st.ctypes.data_as(_lib.c_int32_p)), 'ssmq_gp_predict_batch')
    return {'mean': mean, 'var': var, 'status': st}


def _predict_one(model, test_data, fcn_obs, x_obs, par, **model_args):
    """The reference's single prediction through the batch entry point: fcn_obs (E, N) or (N,), outputs first."""
    y = np.asarray(fcn_obs, dtype=np.float64)
    if y.ndim == 1:
        y = y[None, :]
    if y.ndim != 2 or np.asarray(test_data).ndim != 2:
        raise ValueError('fcn_obs must be (E, N) or (N,) and test_data (D, M)')
    r = _predict_batch(model, test_data, y.T[None], x_obs, par, **model_args)
    if r['status'][0] == 1:
        raise np.linalg.LinAlgError('Matrix is not positive definite')
    if r['status'][0]:
        raise np.linalg.LinAlgError('Bayes-Sard prediction: V\' iK V is not positive definite')
    return np.squeeze(r['mean'][0]), np.squeeze(r['var'][0])


class Model:
    """Kernel + point set (bq/bqmod.py:15-106)."""

    _supported_points_ = ['sr', 'ut', 'gh', 'fs']
    _supported_kernels_ = ['rbf', 'rbf-student']

    def __init__(self, dim, kern_par, kern_str, point_str, point_par, estimate_par):
        self.kernel = Model.get_kernel(dim, kern_str, kern_par)
        self.points = Model.get_points(dim, point_str, point_par)
        self.estimate_par = estimate_par
        self.str_pts = point_str
        self.str_pts_par = str(point_par)
        self.dim_in, self.num_pts = self.points.shape
        self.eye_d, self.eye_n = np.eye(self.dim_in), np.eye(self.num_pts)
        self.q, self.Q, self.R, self.iK = None, None, None, None
        self.model_var = None
        self.integral_var = None

    def __str__(self):
        return '{} {}\n{} {}'.format(type(self.kernel).__name__, self.kernel.par, self.str_pts, self.str_pts_par)

    @staticmethod
    def get_points(dim, points, point_par):
        """bq/bqmod.py:340-382; unknown strings print a message and return None, as the reference does."""
        points = points.lower()
        if points not in Model._supported_points_:
            print('Points {} not supported. Supported points are {}.'.format(points, Model._supported_points_))
            return None
        point_par = {} if point_par is None else point_par
        if points == 'sr':
            return SphericalRadialTransform.unit_sigma_points(dim)
        if points == 'ut':
            return UnscentedTransform.unit_sigma_points(dim, **point_par)
        if points == 'gh':
            return GaussHermiteTransform.unit_sigma_points(dim, **point_par)
        return FullySymmetricStudentTransform.unit_sigma_points(dim, **point_par)

    @staticmethod
    def get_kernel(dim, kernel, par):
        """bq/bqmod.py:384-423 ('rq' is not on this path).  'rbf-student' is built with the constructor's defaults, as in the
        reference (:420-421): dof = 4.0 whatever the noise's or the transform's nu is, 2e6 samples, seed 0; change them by
        assigning the kernel's attributes and computing the weights again."""
        kernel = kernel.lower()
        if kernel not in Model._supported_kernels_:
            print('Kernel {} not supported. Supported kernels are {}.'.format(kernel, Model._supported_kernels_))
            return None
        if kernel == 'rbf-student':
            return RBFStudent(dim, par)
        return RBFGauss(dim, par)

    def neg_log_marginal_likelihood(self, log_par, fcn_obs, x_obs, jitter):
        """Objective of `optimize` (bq/bqmod.py:214-248); the base model has none, as in the reference."""
        pass

    def _ml2_nu(self):
        raise NotImplementedError('{} has no marginal likelihood'.format(type(self).__name__))

    def _check_estimation(self):
        if not getattr(self.kernel, 'supports_parameter_estimation', True):
            raise NotImplementedError('{} does not support parameter estimation (supports_parameter_estimation = False, as in '
                                      'the reference)'.format(type(self.kernel).__name__))

    def optimize(self, log_par_0, fcn_obs, x_obs, method='BFGS', **kwargs):
        """Kernel log-parameters by type-II maximum likelihood (bq/bqmod.py:250-285): scipy.optimize.minimize(
        self.neg_log_marginal_likelihood, log_par_0, args=(fcn_obs, x_obs, 1e-8 I), method='BFGS', jac=True, **kwargs),
        with the whole optimisation on the device (`ssmq_gp_ml2_batch`: SciPy's BFGS and line searches restated).
        Returns a scipy.optimize.OptimizeResult.  `options` takes gtol and maxiter (and `tol` stands for gtol, as in
        minimize); bounds and constraints are ignored with SciPy's warning; other methods are not implemented.  Where K is
        not positive definite at a trial point, the objective is +inf there (the reference raises LinAlgError)."""
        from scipy.optimize import OptimizeResult
        self._check_estimation()
        if not isinstance(method, str) or method.lower() != 'bfgs':
            raise NotImplementedError('ML-II on the device implements method=\'BFGS\' only, not {!r}'.format(method))
        kwargs = dict(kwargs)
        options = dict(kwargs.pop('options', None) or {})
        tol = kwargs.pop('tol', None)
        if tol is not None:
            options.setdefault('gtol', tol)
        for key in ('hess', 'hessp'):
            if kwargs.pop(key, None) is not None:
                warnings.warn('Method BFGS does not use Hessian{} information ({}).'.format(
                    '-vector product' if key == 'hessp' else '', key), RuntimeWarning, stacklevel=2)
        if np.any(kwargs.pop('constraints', ())):
            warnings.warn('Method BFGS cannot handle constraints.', RuntimeWarning, stacklevel=2)
        if kwargs.pop('bounds', None) is not None:
            warnings.warn('Method BFGS cannot handle bounds.', RuntimeWarning, stacklevel=2)
        if kwargs.pop('callback', None) is not None:
            raise NotImplementedError('ML-II on the device takes no callback')
        if kwargs:
            raise TypeError('optimize() got unexpected keyword arguments {}'.format(sorted(kwargs)))
        x0 = np.asarray(log_par_0, dtype=np.float64)
        if x0.ndim != 1:
            raise ValueError("'x0' must only have one dimension.")
        y = np.asarray(fcn_obs, dtype=np.float64)
        if y.ndim == 1:
            y = y[:, None]
        x = np.asarray(x_obs, dtype=np.float64)
        gtol, maxiter = _ml2_options(options)
        r = _ml2_batch(x0[None, :], y[None], x, self._ml2_nu(), gtol, maxiter)
        st = int(r['status'][0])
        return OptimizeResult(x=r['x'][0], fun=float(r['fun'][0]), jac=r['jac'][0], hess_inv=r['hess_inv'][0],
                              nit=int(r['nit'][0]), nfev=int(r['nfev'][0]), njev=int(r['njev'][0]), status=st,
                              success=st == 0, message=_BFGS_MESSAGES[st] if 0 <= st < 4 else 'status {}'.format(st))

    def optimize_batch(self, log_par_0, fcn_obs, x_obs, **options):
        """B independent `optimize` runs in one launch, one workgroup per fit: log_par_0 (B, P) or (P,) for all, fcn_obs
        (B, N, E), x_obs (D, N) shared or (B, D, N); options gtol, maxiter.  Returns a dict of arrays with a leading B axis:
        x, fun, jac, hess_inv, nit, nfev, njev, status (scipy's warnflag), success.  Row b equals optimize() on row b's
        data, bit for bit."""
        self._check_estimation()
        y = np.asarray(fcn_obs, dtype=np.float64)
        if y.ndim == 2:
            y = y[..., None]
        x0 = np.asarray(log_par_0, dtype=np.float64)
        if x0.ndim == 1:
            x0 = np.broadcast_to(x0, (y.shape[0], x0.shape[0]))
        gtol, maxiter = _ml2_options(options)
        return _ml2_batch(x0, y, x_obs, self._ml2_nu(), gtol, maxiter)


    def predict_batch(self, test_data, fcn_obs, x_obs=None, par=None, **model_args):
        """B independent predictions in one call, in the layout of `optimize_batch`: fcn_obs (B, N, E) (or (B, N)), par
        (B, 1 + D) natural parameters or one row for all (default: the kernel's own), x_obs (D, N) shared or (B, D, N)
        (default: self.points), test_data (D, M) shared or (B, D, M).  Returns a dict: mean (B, M, E), var (B, M), status (B,)
        int32 - 0 ok, 1 = K + jitter I not positive definite, 2 = the Bayes-Sard V' iK V not positive definite; rows with a
        non-zero status are NaN, the others are unaffected.  Row b equals predict() on row b's data, bit for bit.  After a
        fit: model.predict_batch(xt, Y, x, par=np.exp(model.optimize_batch(lp0, Y, x)['x']))."""
        return _predict_batch(self, test_data, fcn_obs, x_obs, par, **self._predict_args(**model_args))

    def _predict_args(self, **model_args):
        raise NotImplementedError('{} has no predict'.format(type(self).__name__))


class GaussianProcessModel(Model):
    """GP quadrature weights (bq/bqmod.py:426-535)."""

    def __init__(self, dim, kern_par, kern_str, point_str, point_par=None, estimate_par=False):
        super().__init__(dim, kern_par, kern_str, point_str, point_par, estimate_par)

    def _device_weights(self, par):
        """All quantities of one parameter row: the Gaussian closed forms, or the kernel's Monte-Carlo expectations ('rbf-student',
        with the kernel's current dof / num_samples / seed) through the same weight algebra."""
        if isinstance(self.kernel, RBFStudent):
            return device_student_weights(self.points, par[:1], self.kernel)
        return device_gp_weights(self.points, par[:1], self.kernel.jitter)

    def bq_weights(self, par, *args):
        """wm = q iK, Wc = iK Q iK (symmetrised), Wcc = R iK and the model / integral variances (bq/bqmod.py:495-523)."""
        par = self.kernel.get_parameters(par)
        w = self._device_weights(par)
        self.q, self.Q, self.R, self.iK = w['q'][0], w['Q'][0], w['R'][0], w['iK'][0]
        self.model_var = float(w['model_var'][0])
        self.integral_var = float(w['integral_var'][0])
        return w['wm'][0], w['Wc'][0], w['Wcc'][0], self.model_var, self.integral_var

    def _ml2_nu(self):
        return 0.0

    def neg_log_marginal_likelihood(self, log_par, fcn_obs, x_obs, jitter):
        """Negative log marginal likelihood and its gradient at the kernel log-parameters (bq/bqmod.py:537-596), on the
        device: (float, (P,) array).  fcn_obs (N, E), x_obs (D, N), jitter added to K (an (N, N) matrix, as `optimize`
        passes it).  The gradient's first entry is taken with respect to alpha, not log alpha (RBFGauss.der_par)."""
        return self._nlml_one(log_par, fcn_obs, x_obs, jitter)

    def _nlml_one(self, log_par, fcn_obs, x_obs, jitter):
        y = np.asarray(fcn_obs, dtype=np.float64)
        if y.ndim == 1:
            y = y[:, None]
        f, g, st = _nlml_batch(np.atleast_1d(np.asarray(log_par, dtype=np.float64)).reshape(1, -1), y[None], x_obs, jitter,
                               self._ml2_nu())
        if st[0]:
            raise np.linalg.LinAlgError('kernel matrix not positive definite')
        return float(f[0]), g[0]

    def neg_log_marginal_likelihood_batch(self, log_par, fcn_obs, x_obs, jitter=None):
        """B objective evaluations in one launch: log_par (B, P), fcn_obs (B, N, E), x_obs (D, N) or (B, D, N), jitter
        (N, N) (default 1e-8 I).  Returns values (B,) and gradients (B, P); rows whose K is not positive definite are NaN."""
        y = np.asarray(fcn_obs, dtype=np.float64)
        if y.ndim == 2:
            y = y[..., None]
        f, g, _ = _nlml_batch(np.atleast_2d(log_par), y, x_obs, jitter, self._ml2_nu())
        return f, g

    def predict(self, test_data, fcn_obs, x_obs=None, par=None):
        """GP posterior mean and variance at the test inputs (bq/bqmod.py:454-493), on the device.  test_data (D, M);
        fcn_obs (E, N) or (N,) - OUTPUTS FIRST, as the reference's predict takes them, not the (N, E) of `optimize`; x_obs
        (D, N) training inputs (default: self.points); par natural kernel parameters [alpha, ell_1 .. ell_D] (default: the
        kernel's own).  With iK = sym((K(x_obs) + jitter I)^-1), kx = K(test, x_obs), kxx = alpha^2: mean = squeeze(kx iK
        fcn_obs.T), (M,) for one output and (M, E) otherwise; var = squeeze(kxx - diag(kx iK kx')), (M,).  At a training
        input the variance is a jitter-sized number that rounding may push below zero, here as in the reference.  Raises
        numpy.linalg.LinAlgError where K + jitter I is not positive definite."""
        return _predict_one(self, test_data, fcn_obs, x_obs, par, **self._predict_args())

    def _predict_args(self):
        return {}

    def bq_weights_batch(self, pars):
        """theta-batched weights: pars (P, 1 + D) -> dict with a leading P axis (one workgroup per row).  Gaussian expectations
        only."""
        if isinstance(self.kernel, RBFStudent):
            raise NotImplementedError("theta-batched weights are not implemented for the 'rbf-student' kernel")
        return device_gp_weights(self.points, np.atleast_2d(pars), self.kernel.jitter)

    def exp_model_variance(self, par, *args):
        """alpha^2 (1 - tr(Q iK)) with iK the inverse of the SCALED kernel matrix (bq/bqmod.py:525-528: eval_inv_dot is
        called with its default scaling=True there) and Q the unscaled expectation - both from the device, the trace of
        their product on the host."""
        par = self.kernel.get_parameters(par)
        iK = self.kernel.eval_inv_dot(par, self.points)
        Q = self.kernel.exp_x_kxkx(par, par, self.points)
        return float(self.kernel.exp_x_kxx(par) * (1 - np.trace(Q.dot(iK))))

    def integral_variance(self, par, *args):
        """bq/bqmod.py:530-535."""
        par = self.kernel.get_parameters(par)
        return float(self._device_weights(par)['integral_var'][0])


class GaussianProcessDerModel(GaussianProcessModel):
    """GP model with derivative observations at the points `which_der` (research/gpqd/gpqd_base.py: GaussianProcessDerModel): a
    strictly increasing index array into the sigma points, None = all of them, empty = none (the plain GP quadrature weights).
    `bq_weights` takes any subset - the reference's is consistent for all points only.  D <= 6, 2 <= N <= 2 D + 1."""

    _supported_kernels_ = ['rbf-d']

    def __init__(self, dim, kern_par, point_str, point_par=None, estimate_par=False, which_der=None):
        super().__init__(dim, kern_par, 'rbf', point_str, point_par, estimate_par)
        self.which_der = check_which_der(self.dim_in, self.num_pts, which_der)
        self.kernel = RBFGaussDer(dim, kern_par)

    def bq_weights(self, par, *args):
        """(wm (M,), Wc (M, M) symmetrised, Wcc (D, M), model_var, integral_var), M = N + Nd D, on the device (`ssmq_weights_gpqd`)."""
        par = self.kernel.get_parameters(par)
        w = device_gpqd_weights(self.points, par, self.which_der, self.kernel.jitter)
        self.q, self.Q, self.R, self.iK = w['q'], w['Q'], w['R'], w['iK']
        self.model_var, self.integral_var = w['model_var'], w['integral_var']
        return w['wm'], w['Wc'], w['Wcc'], self.model_var, self.integral_var

    def exp_model_variance(self, par, *args):
        """alpha^2 (1 - tr(Q~ iK)) with iK the inverse of the SCALED joint kernel matrix, as GaussianProcessModel's."""
        par = self.kernel.get_parameters(par)
        iK = self.kernel.eval_inv_dot(par, self.points, which_der=self.which_der)
        Q = device_gpqd_weights(self.points, par, self.which_der, self.kernel.jitter)['Q']
        return float(self.kernel.exp_x_kxx(par) * (1 - np.trace(Q.dot(iK))))

    def integral_variance(self, par, *args):
        par = self.kernel.get_parameters(par)
        return device_gpqd_weights(self.points, par, self.which_der, self.kernel.jitter)['integral_var']

    def _not_implemented(self, what):
        raise NotImplementedError('GaussianProcessDerModel.{} is not implemented (nor in the reference: its marginal likelihood and '
                                  'predictive moments are those of the model without derivatives)'.format(what))

    def optimize(self, *args, **kwargs):
        self._not_implemented('optimize')

    def predict(self, *args, **kwargs):
        self._not_implemented('predict')


class StudentTProcessModel(GaussianProcessModel):
    """Student-t process: GP weights, data-dependent model variance (bq/bqmod.py:1060-1190)."""

    def __init__(self, dim, kern_par, kern_str, point_str, point_par=None, estimate_par=False, nu=4.0):
        super().__init__(dim, kern_par, kern_str, point_str, point_par, estimate_par)
        self.nu = 3.0 if nu < 2 else nu

    def _ml2_nu(self):
        return float(self.nu)

    def neg_log_marginal_likelihood(self, log_par, fcn_obs, x_obs, jitter):
        """Student-t process negative log marginal likelihood and its gradient (bq/bqmod.py:1191-1245), on the device; the
        log Gamma terms of its constant as the reference forms them (the log of Gamma itself)."""
        return self._nlml_one(log_par, fcn_obs, x_obs, jitter)

    def predict(self, test_data, fcn_obs, x_obs=None, par=None, nu=None):
        """Student-t process prediction (bq/bqmod.py:1090-1130): the GP's mean, and the GP's variance times (nu - 2 +
        y' iK y) / (nu - 2 + self.num_pts).  Two quirks of the reference are kept: the denominator counts the MODEL's points,
        not the columns of x_obs, and there is one output only - fcn_obs (N,) or (1, N); more raise ValueError."""
        return _predict_one(self, test_data, fcn_obs, x_obs, par, **self._predict_args(nu=nu))

    def _predict_args(self, nu=None):
        return {'nu': float(self.nu if nu is None else nu)}

    def exp_model_variance(self, par, *args):
        """(nu - 2 + fx iK fx') / (nu - 2 + N) * model_var with the cached scaling=False inverse
        (bq/bqmod.py:1132-1160, estimate_par=False branch).  Host arithmetic on (E, N) data for callers that ask for the
        number; `apply()` computes the same quantity inside the device kernel."""
        fcn_obs = np.squeeze(args[0])
        scale = (self.nu - 2 + fcn_obs.dot(self.iK).dot(fcn_obs.T)) / (self.nu - 2 + self.num_pts)
        return scale * self.model_var

    def integral_variance(self, par, *args):
        fcn_obs = np.squeeze(args[0])
        scale = (self.nu - 2 + fcn_obs.dot(self.iK).dot(fcn_obs.T)) / (self.nu - 2 + self.num_pts)
        return scale * self.integral_var


class BayesSardModel(Model):
    """GP with a multivariate polynomial prior mean (bq/bqmod.py:599-1057)."""

    def __init__(self, dim, kern_par, multi_ind=2, point_str='ut', point_par=None, estimate_par=False):
        super().__init__(dim, kern_par, 'rbf', point_str, point_par, estimate_par)
        if type(multi_ind) is int:
            self.mulind = np.hstack([n_sum_k(dim, td) for td in range(multi_ind + 1)])
        elif type(multi_ind) is np.ndarray:
            self.mulind = multi_ind
        else:
            raise ValueError('Multi-index error: multi-index has to be either int or ndarray')

    def bq_weights(self, par, multi_ind=None):
        """bq/bqmod.py:893-992.  NOTE the reference crashes when handed an int multi-index here (SURVEY.md appendix
        B-2); this build falls back to the expanded `self.mulind` for anything that is not an ndarray."""
        if not isinstance(multi_ind, np.ndarray):
            multi_ind = self.mulind
        par = self.kernel.get_parameters(par)
        if multi_ind.shape[0] != self.dim_in:
            raise ValueError('Dimension mismatch {:d} != {:d}. Dimension of monomials must be equal to the dimension'
                             ' of the sigma-points.'.format(multi_ind.shape[0], self.dim_in))
        nb = multi_ind.shape[1]
        if nb > self.num_pts:
            raise ValueError('Number of basis functions needs to be lower than or equal to the number of points.'
                             'You supplied {:d} basis functions and {:d} points.'.format(nb, self.num_pts))
        lib = _lib.load()
        x, px = _lib.as_c(self.points)
        p, pp = _lib.as_c(par[:1])
        mi = np.ascontiguousarray(multi_ind, dtype=np.int32)
        D, N = x.shape
        out = {k: _lib.out_c(s) for k, s in (('wm', (N,)), ('Wc', (N, N)), ('Wcc', (D, N)), ('iK', (N, N)),
                                             ('q', (N,)), ('Q', (N, N)), ('R', (D, N)), ('mv', (1,)), ('iv', (1,)))}
        st = np.zeros(1, dtype=np.int32)
        rc = _lib.check(lib.ssmq_weights_bs(D, N, px, pp, 1, float(self.kernel.jitter),
                                            mi.ctypes.data_as(_lib.c_int32_p), nb, out['wm'][1], out['Wc'][1],
                                            out['Wcc'][1], out['iK'][1], out['q'][1], out['Q'][1], out['R'][1],
                                            out['mv'][1], out['iv'][1], st.ctypes.data_as(_lib.c_int32_p)),
                        'ssmq_weights_bs')
        if rc > 0:
            raise np.linalg.LinAlgError('Bayes-Sard weights: matrix not positive definite / singular (code {})'.format(
                int(st[0])))
        self.q, self.iK = out['q'][0], out['iK'][0]
        if nb < N:
            self.Q, self.R = out['Q'][0], out['R'][0]
        self.model_var = float(out['mv'][0][0])
        self.integral_var = float(out['iv'][0][0])
        return out['wm'][0], out['Wc'][0], out['Wcc'][0], self.model_var, self.integral_var

    def predict(self, test_data, fcn_obs, x_obs=None, par=None, mulind=None):
        """GP prediction with the polynomial prior mean (bq/bqmod.py:840-891, term by term), on the device: V =
        vandermonde(mulind, x_obs), Z = V' iK, iViKV = (Z V)^-1 by Cholesky, A = iViKV V', b = Z kx' - vx', mean = (kx -
        b' A) iK fcn_obs.T, var = kxx - diag(kx iK kx') + diag(b' iViKV b).  Arguments and shapes as
        GaussianProcessModel.predict (fcn_obs (E, N) or (N,), outputs first); mulind (dim, num_basis), default self.mulind.
        Needs num_basis <= N (NotImplementedError otherwise) and Z V positive definite (numpy.linalg.LinAlgError, as the
        reference)."""
        return _predict_one(self, test_data, fcn_obs, x_obs, par, **self._predict_args(mulind=mulind))

    def _predict_args(self, mulind=None):
        return {'mulind': self.mulind if mulind is None else mulind}

    def _moments(self, multi_ind, x=None, par=None, want=('px',)):
        """The polynomial expectations behind the weights (`ssmq_bs_moments`), one array per name in `want`."""
        mi = np.ascontiguousarray(multi_ind, dtype=np.int32)
        if mi.ndim != 2:
            raise ValueError('multi-index matrix must be (dim, num_basis)')
        D, NB = mi.shape
        N = 0 if x is None else np.atleast_2d(x).shape[1]
        shapes = {'px': (NB,), 'xpx': (D, NB), 'pxpx': (NB, NB), 'kxpx': (N, NB)}
        out = {k: _lib.out_c(shapes[k]) for k in want}
        xs = _lib.as_c(np.atleast_2d(np.asarray(x, dtype=np.float64)))[1] if x is not None else None
        pp = _lib.as_c(self.kernel.get_parameters(par)[:1])[1] if par is not None else None
        ptr = lambda k: out[k][1] if k in out else None          # noqa: E731
        _lib.check(_lib.load().ssmq_bs_moments(D, N, xs, pp, mi.ctypes.data_as(_lib.c_int32_p), NB, ptr('px'), ptr('xpx'),
                                               ptr('pxpx'), ptr('kxpx'), None), 'ssmq_bs_moments')
        return [out[k][0] for k in want]

    def _exp_x_px(self, multi_ind):
        """bq/bqmod.py:635-662: E[p_q(x)], (Q,)."""
        return self._moments(multi_ind, want=('px',))[0]

    def _exp_x_xpx(self, multi_ind):
        """bq/bqmod.py:664-698: E[x p(x)'], (D, Q)."""
        return self._moments(multi_ind, want=('xpx',))[0]

    def _exp_x_pxpx(self, multi_ind):
        """bq/bqmod.py:700-731: E[p(x) p(x)'], (Q, Q)."""
        return self._moments(multi_ind, want=('pxpx',))[0]

    def _exp_x_kxpx(self, par, multi_ind, x):
        """bq/bqmod.py:733-797: E[k(x, x_n) p_q(x)], (N, Q), on the device."""
        return self._moments(multi_ind, x=x, par=par, want=('kxpx',))[0]

    def _variances(self, pars, multi_ind=None):
        """theta-batched (model_var, integral_var) with the semantics of the reference's stand-alone methods
        (`ssmq_variances_bs`): pars (P, 1 + D)."""
        if not isinstance(multi_ind, np.ndarray):
            multi_ind = self.mulind
        lib = _lib.load()
        x, px = _lib.as_c(self.points)
        p, pp = _lib.as_c(np.atleast_2d(np.asarray(pars, dtype=np.float64)))
        mi = np.ascontiguousarray(multi_ind, dtype=np.int32)
        D, N = x.shape
        P = p.shape[0]
        if p.shape[1] != D + 1:
            raise ValueError('kernel parameters must have 1 + dim entries per row')
        mv, pmv = _lib.out_c((P,))
        iv, piv = _lib.out_c((P,))
        st = np.zeros(P, dtype=np.int32)
        rc = _lib.check(lib.ssmq_variances_bs(D, N, px, pp, P, float(self.kernel.jitter),
                                              mi.ctypes.data_as(_lib.c_int32_p), mi.shape[1], pmv, piv,
                                              st.ctypes.data_as(_lib.c_int32_p)), 'ssmq_variances_bs')
        if rc > 0:
            raise np.linalg.LinAlgError('Bayes-Sard variances: matrix not positive definite (parameter row {}, code {})'
                                        .format(rc - 1, int(st[rc - 1])))
        return mv, iv

    def exp_model_variance(self, par, mulind=None):
        """bq/bqmod.py:995-1026 (not the value bq_weights() returns: no jitter on V' iK V, general formula always)."""
        return float(self._variances(self.kernel.get_parameters(par)[:1], mulind)[0][0])

    def integral_variance(self, par, mulind=None):
        """bq/bqmod.py:1028-1050."""
        return float(self._variances(self.kernel.get_parameters(par)[:1], mulind)[1][0])

    def exp_model_variance_batch(self, pars, mulind=None):
        """Length-scale sweeps (research/bsq/bsq_ungm.py:244-282) in one launch: pars (P, 1 + D) -> (P,)."""
        return self._variances(pars, mulind)[0]

    def integral_variance_batch(self, pars, mulind=None):
        return self._variances(pars, mulind)[1]



MO_MAX_DIM, MO_MAX_OUT, MO_MAX_PTS = 16, 8, 64
_MO_RANGE = ("the multi-output models run on the device for D <= 16 inputs, E <= 8 outputs and N <= 64 points, with the 'rbf' "
             "kernel and the built-in models")


def check_mo_range(D, E, N, kern_str='rbf'):
    """NotImplementedError naming the range, before anything reaches the library."""
    if str(kern_str).lower() != 'rbf':
        raise NotImplementedError('{}; got kernel {!r}'.format(_MO_RANGE, kern_str))
    if D > MO_MAX_DIM or E > MO_MAX_OUT or N > MO_MAX_PTS:
        raise NotImplementedError('{}; got D = {}, E = {}, N = {}'.format(_MO_RANGE, D, E, N))


class MultiOutputModel(Model):
    """Kernel + point set with one parameter row [alpha, ell_1 .. ell_D] per output (bq/bqmod.py:1248-1478).  The reference's
    class is unfinished; this is the finished model around the parts of it that work: `bq_weights`,
    `exp_model_variance`, `integral_variance` and `optimize` as the reference defines them, `predict` (`pass` there) raises
    NotImplementedError."""

    def __init__(self, dim_in, dim_out, kern_par, kern_str, point_str, point_par=None, estimate_par=False):
        kern_par = np.asarray(kern_par, dtype=np.float64)
        if kern_par.ndim != 2 or kern_par.shape != (dim_out, dim_in + 1):
            raise ValueError('kern_par must be (dim_out, 1 + dim_in) = ({}, {}), got {}'.format(dim_out, dim_in + 1, kern_par.shape))
        check_mo_range(dim_in, dim_out, 0, kern_str)
        super().__init__(dim_in, kern_par, kern_str, point_str, point_par, estimate_par)
        self.dim_out = dim_out
        check_mo_range(self.dim_in, dim_out, self.num_pts, kern_str)

    def _rows(self, par):
        par = self.kernel.get_parameters(par)
        if par.shape != (self.dim_out, self.dim_in + 1):
            raise ValueError('par must be (dim_out, 1 + dim_in) = ({}, {}), got {}'.format(self.dim_out, self.dim_in + 1, par.shape))
        return np.ascontiguousarray(par, dtype=np.float64)

    def _device_weights(self, par):
        par = self._rows(par)
        D, N, E = self.dim_in, self.num_pts, self.dim_out
        out = {k: _lib.out_c(sh) for k, sh in (('wm', (E, N)), ('Wcc', (E, D, N)), ('iK', (E, N, N)), ('q', (E, N)), ('R', (E, D, N)),
                                               ('Wc', (E, E, N, N)), ('Q', (E, E, N, N)), ('model_var', (E,)),
                                               ('integral_var', (E,)))}
        st = np.zeros(E, dtype=np.int32)
        rc = _lib.check(_lib.load().ssmq_weights_gp_mo(D, N, E, _lib.as_c(self.points)[1], _lib.as_c(par)[1], float(self.kernel.jitter),
                                                       out['wm'][1], out['Wcc'][1], out['iK'][1], out['q'][1], out['R'][1],
                                                       out['Wc'][1], out['Q'][1], out['model_var'][1], out['integral_var'][1],
                                                       st.ctypes.data_as(_lib.c_int32_p)), 'ssmq_weights_gp_mo')
        if rc > 0:
            raise np.linalg.LinAlgError('kernel matrix of output {} is not positive definite'.format(rc - 1))
        return {k: v[0] for k, v in out.items()}

    def bq_weights(self, par):
        """(wm (N, E), Wc (N, N, E, E), Wcc (D, N, E)) in the reference's layouts (bq/bqmod.py:1254-1315); caches q (N, E), Q
        (N, N, E, E), R (D, N, E), iK (N, N, E), model_var (E,) and integral_var (E,).  Wc[..., i, j] = Wc[..., j, i] =
        sym(iK_i Q_ij iK_j), as the reference's symmetrisation leaves it."""
        w = self._device_weights(par)
        self.q, self.R = w['q'].T.copy(), w['R'].transpose(1, 2, 0).copy()
        self.iK, self.Q = w['iK'].transpose(1, 2, 0).copy(), w['Q'].transpose(2, 3, 0, 1).copy()
        self.model_var, self.integral_var = w['model_var'], w['integral_var']
        return w['wm'].T.copy(), w['Wc'].transpose(2, 3, 0, 1).copy(), w['Wcc'].transpose(1, 2, 0).copy()

    def optimize(self, log_par_0, fcn_obs, x_obs, method='BFGS', **kwargs):
        """One ML-II fit per output (bq/bqmod.py:1317-1372), the E fits as ONE `optimize_batch` launch: log_par_0 (E, P), fcn_obs
        (E, N).  Returns (par (E, P) - the stacked r.x - and the list of scipy.optimize.OptimizeResult), as the reference."""
        from scipy.optimize import OptimizeResult
        if not isinstance(method, str) or method.lower() != 'bfgs':
            raise NotImplementedError('ML-II on the device implements method=\'BFGS\' only, not {!r}'.format(method))
        kwargs = dict(kwargs)
        options = dict(kwargs.pop('options', None) or {})
        tol = kwargs.pop('tol', None)
        if tol is not None:
            options.setdefault('gtol', tol)
        if kwargs:
            raise TypeError('optimize() got unexpected keyword arguments {}'.format(sorted(kwargs)))
        lp0 = np.asarray(log_par_0, dtype=np.float64)
        y = np.asarray(fcn_obs, dtype=np.float64)
        if lp0.ndim != 2 or y.ndim != 2 or lp0.shape[0] != self.dim_out or y.shape[0] != self.dim_out:
            raise ValueError('log_par_0 must be (dim_out, P) and fcn_obs (dim_out, N) with dim_out = {}'.format(self.dim_out))
        r = self.optimize_batch(lp0, y[:, :, None], x_obs, **options)
        results = []
        for e in range(self.dim_out):
            st = int(r['status'][e])
            results.append(OptimizeResult(x=r['x'][e], fun=float(r['fun'][e]), jac=r['jac'][e], hess_inv=r['hess_inv'][e],
                                          nit=int(r['nit'][e]), nfev=int(r['nfev'][e]), njev=int(r['njev'][e]), status=st,
                                          success=st == 0, message=_BFGS_MESSAGES[st] if 0 <= st < 4 else 'status {}'.format(st)))
        return np.vstack([res.x for res in results]), results

    def predict(self, test_data, fcn_obs, par=None):
        raise NotImplementedError('the multi-output models have no predict (`pass` in the reference, bq/bqmod.py:1509-1530)')


class GaussianProcessMO(MultiOutputModel):
    """Multi-output GP model (bq/bqmod.py:1481-1560)."""

    def __init__(self, dim_in, dim_out, kern_par, kern_str, point_str, point_par=None):
        super().__init__(dim_in, dim_out, kern_par, kern_str, point_str, point_par)

    def _ml2_nu(self):
        return 0.0

    def exp_model_variance(self, fcn_obs):
        """(E,): alpha_e^2 (1 - tr(Q_ee iK_e)) of the last `bq_weights` (bq/bqmod.py:1532-1537).  alpha_e is taken from the rows
        given to `bq_weights`; the reference reads the constructor's rows (`kernel.scale`) - the same in every use it makes."""
        return np.array(self.model_var, dtype=np.float64)

    def integral_variance(self, fcn_obs, par=None):
        """(E,): kbar_e - q_e' iK_e q_e (bq/bqmod.py:1539-1548)."""
        return self._device_weights(par)['integral_var']


class StudentTProcessMO(MultiOutputModel):
    """Multi-output Student-t process model (bq/bqmod.py:1563-1640): the GP's weights, the model variance of every output scaled
    with that output's integrand values."""

    def __init__(self, dim_in, dim_out, kern_par, kern_str, point_str, point_par=None, nu=3.0):
        super().__init__(dim_in, dim_out, kern_par, kern_str, point_str, point_par)
        self.nu = 3.0 if nu < 2 else nu

    def _ml2_nu(self):
        return float(self.nu)

    def exp_model_variance(self, fcn_obs):
        """(E,): (nu - 2 + fx_e iK_e fx_e') / (nu - 2 + N) * model_var_e for fcn_obs (E, N).  Host arithmetic for callers that ask
        for the numbers; `apply()` computes them inside the device kernel."""
        fx = np.asarray(fcn_obs, dtype=np.float64).reshape(self.dim_out, self.num_pts)
        quad = np.array([fx[e].dot(self.iK[..., e]).dot(fx[e]) for e in range(self.dim_out)])
        return (self.nu - 2 + quad) / (self.nu - 2 + self.num_pts) * self.model_var

    def integral_variance(self, fcn_obs, par=None):
        raise NotImplementedError('only the multi-output GP model has an integral variance (bq/bqmod.py:1539-1548)')
