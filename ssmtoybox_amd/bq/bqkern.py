"""
Kernels of the integrand model: attribute carrier + device-computed expectations (reference: ssmtoybox/bq/bqkern.py).

The RBF kernel with Gaussian expectations (`RBFGauss`, bq/bqkern.py:295-454) and with Monte-Carlo Student-t expectations
(`RBFStudent`, bq/bqkern.py:457-536) are on the accelerated path.  The approximate `RQ` kernel of the reference is out of
scope.

`RBFGauss`: all numbers come from one device kernel (`ssmq_weights_gp`, ssmtoybox_amd/csrc/ssmq_weights.hip), which evaluates
the kernel matrix, its Cholesky-based inverse and the expectations q, R, Q together; the methods below select from it.
`RBFStudent`: the expectations come from the Monte-Carlo kernels of ssmtoybox_amd/csrc/ssmq_student_mc.hip, the weights from
`ssmq_weights_gp_given` - the algebra of `ssmq_weights_gp` on given expectations.
"""
import numpy as np

from .. import _lib


def device_gp_weights(points, par, jitter=1e-8):
    """All GP-quadrature quantities for P parameter rows.  points (D, N); par (P, 1 + D).
    Returns dict of arrays with a leading P axis: wm, Wc, Wcc, iK, q, Q, R, model_var, integral_var, status."""
    lib = _lib.load()
    x, px = _lib.as_c(points)
    par = np.atleast_2d(np.asarray(par, dtype=np.float64))
    par, pp = _lib.as_c(par)
    D, N = x.shape
    P = par.shape[0]
    if par.shape[1] != D + 1:
        raise ValueError('kernel parameters must have 1 + dim entries per row')
    out = {k: _lib.out_c(s) for k, s in (('wm', (P, N)), ('Wc', (P, N, N)), ('Wcc', (P, D, N)), ('iK', (P, N, N)),
                                         ('q', (P, N)), ('Q', (P, N, N)), ('R', (P, D, N)), ('model_var', (P,)),
                                         ('integral_var', (P,)))}
    st = np.zeros(P, dtype=np.int32)
    rc = _lib.check(lib.ssmq_weights_gp(D, N, px, pp, P, float(jitter), out['wm'][1], out['Wc'][1], out['Wcc'][1],
                                        out['iK'][1], out['q'][1], out['Q'][1], out['R'][1], out['model_var'][1],
                                        out['integral_var'][1], st.ctypes.data_as(_lib.c_int32_p)), 'ssmq_weights_gp')
    res = {k: v[0] for k, v in out.items()}
    res['status'] = st
    if rc > 0:
        raise np.linalg.LinAlgError('kernel matrix not positive definite for parameter row {}'.format(rc - 1))
    return res


class Kernel:
    """Base class (bq/bqkern.py:11-36): `par` is forced to a 2-D float array (dim_out, 1 + dim)."""

    def __init__(self, dim, par, jitter):
        self.par = np.atleast_2d(par).astype(float)
        assert self.par.ndim == 2
        self.scale = self.par[:, 0]
        self.dim = dim
        self.jitter = jitter
        self.eye_d = np.eye(dim)

    def get_parameters(self, par=None):
        if par is None:
            return self.par
        par = np.atleast_2d(par).astype(float)
        assert par.ndim == 2
        return par


class RBFGauss(Kernel):
    """k(x, x') = s^2 exp(-(x - x')' Lam^-1 (x - x') / 2), parameters [s, ell_1, ..., ell_D] (bq/bqkern.py:295-454)."""

    def __init__(self, dim, par, jitter=1e-8):
        par = np.atleast_2d(par)
        assert par.shape[1] == dim + 1
        super().__init__(dim, par, jitter)

    def _all(self, par, x):
        return device_gp_weights(x, np.atleast_2d(par)[:1], self.jitter)

    @staticmethod
    def _row(par):
        return np.ascontiguousarray(np.atleast_2d(np.asarray(par, dtype=np.float64))[:1])

    def eval(self, par, x1, x2=None, diag=False, scaling=True):
        """Kernel matrix K[i, j] = alpha^2 exp(-maha(Lam^-1/2 x1_i, Lam^-1/2 x2_j) / 2) (bq/bqkern.py:329-343), computed
        on the device with the reference's algebra (`ssmq_rbf_eval`)."""
        lib = _lib.load()
        par = self._row(par)
        x1, p1 = _lib.as_c(x1)
        if x2 is None:
            x2, p2 = x1, p1
        else:
            x2, p2 = _lib.as_c(x2)
        D, N1, N2 = x1.shape[0], x1.shape[1], x2.shape[1]
        if diag:
            assert x1.shape == x2.shape
        K, pk = _lib.out_c((N1,) if diag else (N1, N2))
        _lib.check(lib.ssmq_rbf_eval(D, N1, p1, N2, p2, _lib.as_c(par)[1], 1, int(bool(scaling)), int(bool(diag)), pk),
                   'ssmq_rbf_eval')
        return K

    def _factor(self, par, x, scaling, want_chol, want_inv, rhs=None):
        lib = _lib.load()
        par = self._row(par)
        x, px = _lib.as_c(x)
        D, N = x.shape
        L, pl = _lib.out_c((N, N)) if want_chol else (None, None)
        iK, pi = _lib.out_c((N, N)) if want_inv else (None, None)
        pb = None
        if rhs is not None:
            rhs, pb = _lib.as_c(rhs)
            if rhs.shape != (N, N):
                # the reference fails here too: _cho_inv symmetrises its result (bq/bqkern.py:63)
                raise ValueError('eval_inv_dot: the right-hand side has to be (N, N), got {}'.format(rhs.shape))
        rc = _lib.check(lib.ssmq_rbf_factor(D, N, px, _lib.as_c(par)[1], 1, int(bool(scaling)), float(self.jitter), pb, pl,
                                            pi, None), 'ssmq_rbf_factor')
        if rc > 0:
            raise np.linalg.LinAlgError('Matrix is not positive definite')
        return L, iK

    def eval_chol(self, par, x, scaling=True):
        """Lower Cholesky factor of K + jitter I (bq/bqkern.py:122-142)."""
        return self._factor(par, x, scaling, True, False)[0]

    def eval_inv_dot(self, par, x, b=None, scaling=True):
        """sym((K + jitter I)^-1 b) (bq/bqkern.py:96-120 with _cho_inv :38-64; b = None: the inverse itself).  The
        reference symmetrises whatever it solved for, so a right-hand side has to be square there; the same here."""
        return self._factor(par, x, scaling, False, True, b)[1]

    def exp_x_kx(self, par, x, scaling=False):
        """Kernel mean (bq/bqkern.py:345-356)."""
        q = self._all(par, x)['q'][0]
        return q * float(np.atleast_2d(par)[0, 0]) ** 2 if scaling else q

    def exp_x_xkx(self, par, x):
        """bq/bqkern.py:358-364."""
        return self._all(par, x)['R'][0]

    def exp_x_kxkx(self, par_0, par_1, x, scaling=False):
        """E[k(x, x_i; theta_0) k(x, x_j; theta_1)] (bq/bqkern.py:366-415); the two parameter rows may differ."""
        lib = _lib.load()
        x, px = _lib.as_c(x)
        D, N = x.shape
        Q, pq = _lib.out_c((N, N))
        _lib.check(lib.ssmq_rbf_exp_kxkx(D, N, px, _lib.as_c(self._row(par_0))[1], _lib.as_c(self._row(par_1))[1],
                                         int(bool(scaling)), pq), 'ssmq_rbf_exp_kxkx')
        return Q

    def der_par(self, par_0, x):
        """Derivatives of K (no jitter) with respect to the parameters, (N, N, 1 + D) (bq/bqkern.py:426-436): 2 K / alpha
        (with respect to alpha itself, a quirk of the reference the ML-II gradient inherits), then (x_i - x_j)^2 / ell^2 K
        (with respect to log ell).  K comes from the device (`eval`); the elementwise factors are formed here."""
        p = np.asarray(par_0, dtype=np.float64).squeeze()
        x = np.asarray(x, dtype=np.float64)
        alpha, el = p[0], p[1:]
        K = self.eval(p, x)
        d_alpha = 2 * alpha ** -1 * K
        d_el = (x[:, None, :] - x[:, :, None]) ** 2 * (el ** -2)[:, None, None] * K[None, :, :]
        return np.concatenate((d_alpha[..., None], d_el.T), axis=2)

    def exp_x_kxx(self, par):
        """bq/bqkern.py:417-419."""
        return float(np.atleast_2d(par)[0, 0]) ** 2

    def exp_xy_kxy(self, par):
        """bq/bqkern.py:421-424."""
        p = np.atleast_2d(par).astype(float)[0]
        return p[0] ** 2 * np.prod(2 * p[1:] ** -2 + 1.0) ** -0.5


GPQD_MAX_DIM = 6
_GPQD_RANGE = ('GP quadrature with derivative observations supports D <= 6 inputs, 2 <= N <= 2 D + 1 points and a strictly increasing '
               'which_der within the points')


def check_which_der(D, N, which_der):
    """The index array of the points that carry a derivative observation (None: all), checked against the supported range;
    NotImplementedError / ValueError before the library is touched."""
    if not (1 <= int(D) <= GPQD_MAX_DIM and 2 <= int(N) <= 2 * int(D) + 1):
        raise NotImplementedError('{} (got D = {}, N = {})'.format(_GPQD_RANGE, D, N))
    wd = np.arange(N, dtype=np.int32) if which_der is None else np.asarray(which_der).reshape(-1)
    if wd.size and (not np.issubdtype(wd.dtype, np.integer) or wd.min() < 0 or wd.max() >= N or np.any(np.diff(wd) <= 0)):
        raise ValueError('which_der must be strictly increasing integer indices into the {} points, got {}'.format(N, which_der))
    return np.ascontiguousarray(wd, dtype=np.int32)


def device_gpqd_weights(points, par, which_der=None, jitter=1e-8, scaling=False):
    """Every quantity of GP quadrature with derivative observations for one parameter row (`ssmq_weights_gpqd`): points (D, N), par
    [alpha, ell_1 .. ell_D], which_der the points with a derivative observation (None: all).  M = N + Nd D.  Returns a dict: wm (M,),
    Wc (M, M), Wcc (D, M), model_var, integral_var, K (M, M; joint kernel matrix without jitter), L (its lower factor with jitter),
    iK (symmetrised inverse), q (M,), Q (M, M), R (D, M) (the joint kernel expectations, scaling=False) and which_der.  `scaling`
    evaluates K, L and iK with alpha; the weights are the reference's for scaling=False."""
    x, px = _lib.as_c(points)
    D, N = x.shape
    wd = check_which_der(D, N, which_der)
    par = np.ascontiguousarray(np.atleast_2d(np.asarray(par, dtype=np.float64))[0])
    if par.shape != (D + 1,):
        raise ValueError('kernel parameters must have 1 + dim entries')
    M = N + wd.size * D
    out = {k: _lib.out_c(s) for k, s in (('wm', (M,)), ('Wc', (M, M)), ('Wcc', (D, M)), ('model_var', (1,)), ('integral_var', (1,)),
                                         ('K', (M, M)), ('L', (M, M)), ('iK', (M, M)), ('q', (M,)), ('Q', (M, M)), ('R', (D, M)))}
    rc = _lib.check(_lib.load().ssmq_weights_gpqd(D, N, px, _lib.as_c(par)[1], int(wd.size), wd.ctypes.data_as(_lib.c_int32_p),
                                                  float(jitter), int(bool(scaling)), *[out[k][1] for k in out]), 'ssmq_weights_gpqd')
    if rc > 0:
        raise np.linalg.LinAlgError('Matrix is not positive definite')
    res = {k: v[0] for k, v in out.items()}
    res['model_var'], res['integral_var'] = float(res['model_var'][0]), float(res['integral_var'][0])
    res['which_der'] = wd
    return res


class RBFGaussDer(RBFGauss):
    """RBF kernel "with derivatives" (research/gpqd/gpqd_base.py: RBFGaussDer): the joint kernel of the integrand's values at all
    points x (D, N) and of its D partial derivatives at the points `which_der` (None: all), M = N + Nd D rows in the order
    [values | derivatives at which_der[0] | derivatives at which_der[1] | ..], and its expectations under N(0, I).  Everything
    comes from one device kernel (`ssmq_weights_gpqd`).  Unlike the reference, EVERY method takes `which_der`: there only
    `exp_x_dkx` honours the one `bq_weights` passes, so a proper subset fails with mismatched shapes.  Jitter (1e-8) goes on the
    whole diagonal of the joint matrix."""

    def __init__(self, dim, par, jitter=1e-8):
        super().__init__(dim, par, jitter)

    def _der(self, par, x, which_der, scaling=False):
        return device_gpqd_weights(x, par, which_der, self.jitter, scaling)

    def eval(self, par, x1, x2=None, diag=False, scaling=True, which_der=None):
        """The (M, M) joint kernel matrix of the points x1 (no jitter).  Two different point sets or `diag` are the plain kernel's
        business: NotImplementedError."""
        if x2 is not None or diag:
            raise NotImplementedError('RBFGaussDer.eval: the joint kernel matrix of one point set (x2=None, diag=False); for two point '
                                      'sets use RBFGauss.eval')
        return self._der(par, x1, which_der, scaling)['K']

    def eval_chol(self, par, x, scaling=True, which_der=None):
        """Lower Cholesky factor of K + jitter I, (M, M)."""
        return self._der(par, x, which_der, scaling)['L']

    def eval_inv_dot(self, par, x, b=None, scaling=True, which_der=None):
        """sym((K + jitter I)^-1 b), (M, M); b = None: the inverse itself."""
        iK = self._der(par, x, which_der, scaling)['iK']
        if b is None:
            return iK
        b = np.asarray(b, dtype=np.float64)
        if b.shape != iK.shape:
            raise ValueError('eval_inv_dot: the right-hand side has to be (M, M), got {}'.format(b.shape))
        r = iK.dot(b)
        return 0.5 * (r + r.T)

    def _scaled(self, par, scaling, power=1):
        return float(np.atleast_2d(par)[0, 0]) ** (2 * power) if scaling else 1.0

    def exp_x_dkx(self, par, x, scaling=False, which_der=None):
        """E_x[k_fd(x, x_n)], (Nd D,)."""
        N = np.shape(x)[1]
        return self._der(par, x, which_der)['q'][N:] * self._scaled(par, scaling)

    def exp_x_xdkx(self, par, x, scaling=False, which_der=None):
        """E_x[x k_fd(x, x_m)], (D, Nd D)."""
        N = np.shape(x)[1]
        return np.ascontiguousarray(self._der(par, x, which_der)['R'][:, N:]) * self._scaled(par, scaling)

    def exp_x_kxdkx(self, par, x, scaling=False, which_der=None):
        """E_x[k_ff(x_n, x) k_fd(x, x_m)], (N, Nd D)."""
        N = np.shape(x)[1]
        return np.ascontiguousarray(self._der(par, x, which_der)['Q'][:N, N:]) * self._scaled(par, scaling, 2)

    def exp_x_dkxdkx(self, par, x, scaling=False, which_der=None):
        """E_x[k_df(x_n, x) k_fd(x, x_m)], (Nd D, Nd D)."""
        N = np.shape(x)[1]
        return np.ascontiguousarray(self._der(par, x, which_der)['Q'][N:, N:]) * self._scaled(par, scaling, 2)


STUDENT_MC_MAX_DIM, STUDENT_MC_MAX_PTS = 16, 128
_STUDENT_MC_RANGE = ("the 'rbf-student' expectations on the device support D <= 16 inputs, N <= 128 points, "
                     "1 <= num_samples < 2^31 and dof > 0")


class RBFStudent(RBFGauss):
    """RBF kernel whose expectations are taken under a standard multivariate Student-t density with `dof` degrees of freedom
    and estimated by Monte Carlo over `num_samples` samples (bq/bqkern.py:457-536), on the device.  `eval`, `eval_chol` and
    `eval_inv_dot` are RBFGauss's.  Constructor as in the reference plus `seed`; `num_batches` is accepted and ignored - it
    only shaped the reference's NumPy memory use (`batch_size` is still derived from it, as an attribute).

    Differences from the reference, both deliberate:
      * the random numbers are a function of (seed, sample index) alone, so repeated calls with the same `seed` return the
        same numbers, bit for bit; the reference advances NumPy's global stream with every call.  Change `seed` (or `dof`,
        `num_samples`) by assigning the attribute and computing the weights again;
      * `expectations()` - and with it the model's `bq_weights` - estimates q, R and Q from ONE sample set in one pass (the
        reference draws three independent sets).  Every estimate is still unbiased, and Q - q q' is then a sample covariance,
        hence positive semi-definite.  The single-quantity methods below draw the same samples, so exp_x_kxkx(p, p, x) is
        bit-equal to the Q of expectations(p, x).
    `exp_xy_kxy` reproduces the reference's estimator including its normalisation quirk (see there).  Parameter estimation
    is not supported (`supports_parameter_estimation = False`, as in the reference)."""
    supports_parameter_estimation = False

    def __init__(self, dim, par, jitter=1e-8, dof=4.0, num_samples=2e6, num_batches=1000, seed=0):
        # parameters of the standard Student's density
        self.mean = np.zeros((dim, ))
        self.scale_mat = np.eye(dim)
        self.dof = dof
        # parameters of the Monte-Carlo approximation
        self.num_samples = int(num_samples)
        self.num_batches = int(num_batches)
        self.batch_size = int(num_samples // num_batches)
        self.seed = int(seed)
        super().__init__(dim, par, jitter)

    def _check_range(self, D, N=1):
        """Raised in Python, before the library is loaded."""
        S = int(self.num_samples)
        if not (1 <= D <= STUDENT_MC_MAX_DIM and 1 <= N <= STUDENT_MC_MAX_PTS and 1 <= S < 2 ** 31 and self.dof > 0
                and np.isfinite(self.dof)):
            raise NotImplementedError('{}; got D = {}, N = {}, num_samples = {}, dof = {}'.format(
                _STUDENT_MC_RANGE, D, N, S, self.dof))
        return S

    def expectations(self, par_0, x, par_1=None):
        """(q (N,), R (D, N), Q (N, N)) with scaling=False from one pass over one sample set (`ssmq_rbf_student_expect`):
        q = E[k0], R = E[x k0'], Q[i, j] = E[k1_i k0_j] with k0 / k1 the kernel at par_0 / par_1 (default: par_0)."""
        x = np.asarray(x, dtype=np.float64)
        D, N = x.shape
        S = self._check_range(D, N)
        p0 = self._row(par_0)
        p1 = p0 if par_1 is None else self._row(par_1)
        if p0.shape[1] != D + 1 or p1.shape[1] != D + 1:
            raise ValueError('kernel parameters must have 1 + dim entries per row')
        lib = _lib.load()
        x, px = _lib.as_c(x)
        q, pq = _lib.out_c((N,))
        R, pr = _lib.out_c((D, N))
        Q, pQ = _lib.out_c((N, N))
        _lib.check(lib.ssmq_rbf_student_expect(D, N, px, _lib.as_c(p0)[1], _lib.as_c(p1)[1], float(self.dof), S,
                                               int(self.seed) & (2 ** 64 - 1), pq, pr, pQ), 'ssmq_rbf_student_expect')
        return q, R, Q

    def exp_x_kx(self, par, x, scaling=False):
        """Kernel mean E[k(x, x_i)], (N,) (bq/bqkern.py:476-482)."""
        q = self.expectations(par, x)[0]
        return q * float(np.atleast_2d(par)[0, 0]) ** 2 if scaling else q

    def exp_x_xkx(self, par, x, scaling=False):
        """E[x k(x, x_i)], (D, N) (bq/bqkern.py:484-491)."""
        R = self.expectations(par, x)[1]
        return R * float(np.atleast_2d(par)[0, 0]) ** 2 if scaling else R

    def exp_x_kxkx(self, par_0, par_1, x, scaling=False):
        """Q[i, j] = E[k(x, x_i; par_1) k(x, x_j; par_0)], both kernels on the same samples (bq/bqkern.py:493-524); the two
        parameter rows may differ."""
        Q = self.expectations(par_0, x, par_1)[2]
        if scaling:
            Q = Q * (float(np.atleast_2d(par_0)[0, 0]) * float(np.atleast_2d(par_1)[0, 0])) ** 2
        return Q

    def exp_x_kxx(self, par):
        """bq/bqkern.py:526-527."""
        return float(np.atleast_2d(par)[0, 0]) ** 2

    def exp_xy_kxy(self, par, batch_sums=False):
        """The reference's estimator as it is (bq/bqkern.py:529-536): 10 000 batches of 200 samples (hard-coded there), per
        batch the sum of eval(par, xs, xs) over all 200 x 200 pairs, the diagonal included, scaling=True; the total divided
        by `num_samples`.  That is NOT the pair mean E[k(x, y)]: at the default 2e6 samples it is alpha^2 (199 E[k] + 1), about
        200 times it - a quirk of the reference that its integral variance inherits, kept here.
        `batch_sums=True` also returns the (10000,) per-batch sums."""
        p = self._row(par)
        D = p.shape[1] - 1
        S = self._check_range(D)
        out, po = _lib.out_c((1,))
        sums, ps = _lib.out_c((10000,)) if batch_sums else (None, None)
        _lib.check(_lib.load().ssmq_rbf_student_kxy(D, _lib.as_c(p)[1], float(self.dof), S, int(self.seed) & (2 ** 64 - 1), po,
                                                    ps), 'ssmq_rbf_student_kxy')
        return (float(out[0]), sums) if batch_sums else float(out[0])


def device_student_weights(points, par, kernel):
    """GP-quadrature quantities of one parameter row with the Monte-Carlo expectations of an `RBFStudent` kernel: the dict of
    `device_gp_weights` (leading axis of length 1).  The expectations and the weights are computed on the device
    (`ssmq_rbf_student_expect`, `ssmq_rbf_student_kxy`, `ssmq_weights_gp_given`)."""
    par = np.atleast_2d(np.asarray(par, dtype=np.float64))[:1]
    x, px = _lib.as_c(points)
    D, N = x.shape
    kernel._check_range(D, N)
    if par.shape[1] != D + 1:
        raise ValueError('kernel parameters must have 1 + dim entries per row')
    q, R, Q = kernel.expectations(par, x)
    kbar = kernel.exp_xy_kxy(par)
    out = {k: _lib.out_c(s) for k, s in (('wm', (1, N)), ('Wc', (1, N, N)), ('Wcc', (1, D, N)), ('iK', (1, N, N)),
                                         ('model_var', (1,)), ('integral_var', (1,)))}
    st = np.zeros(1, dtype=np.int32)
    rc = _lib.check(_lib.load().ssmq_weights_gp_given(
        D, N, px, _lib.as_c(par)[1], float(kernel.jitter), _lib.as_c(q)[1], _lib.as_c(R)[1], _lib.as_c(Q)[1], float(kbar),
        out['wm'][1], out['Wc'][1], out['Wcc'][1], out['iK'][1], out['model_var'][1], out['integral_var'][1],
        st.ctypes.data_as(_lib.c_int32_p)), 'ssmq_weights_gp_given')
    res = {k: v[0] for k, v in out.items()}
    res.update(q=q[None], R=R[None], Q=Q[None], status=st, kbar=kbar)
    if rc > 0:
        raise np.linalg.LinAlgError('kernel matrix not positive definite for parameter row {}'.format(rc - 1))
    return res
