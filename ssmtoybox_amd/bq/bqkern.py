"""
Kernels of the integrand model: attribute carrier + device-computed expectations (reference: ssmtoybox/bq/bqkern.py).

Only the RBF kernel with Gaussian expectations is on the accelerated path (`RBFGauss`, bq/bqkern.py:295-454).  The
Monte-Carlo `RBFStudent` and the approximate `RQ` kernels of the reference are out of scope (SURVEY.md section 2, row
3b): their weights are RNG-dependent and enter this build as injected data (assign tf.wm / tf.Wc / tf.Wcc).

All numbers come from one device kernel (`ssmq_weights_gp`, ssmtoybox_amd/csrc/ssmq_weights.hip), which evaluates the
kernel matrix, its Cholesky-based inverse and the expectations q, R, Q together; the methods below select from it.
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
