"""
Bayesian-quadrature moment transforms (reference: ssmtoybox/bq/bqmtran.py).

Constructor signatures, the `wm` / `Wc` / `Wcc` / `I_out` / `model` attributes and `apply()` / `weights()` follow the
reference (bq/bqmtran.py:55-130, 285-415) so that code written against it runs unchanged; weights and moments are
computed by HIP kernels.  `apply_batch()` (many trajectories per launch) is this build's addition.
"""
import ctypes

import numpy as np

from .. import _lib
from ..mtran import MomentTransform, _DeviceApply, DeviceTransform, resolve_integrand
from .._lib import FORM_BQ, EMV_DIAG, EMV_BROADCAST
from ..ssmod import user_unsupported, is_user_model, has_device_jacobian
from .bqmod import (GaussianProcessModel, StudentTProcessModel, BayesSardModel, GaussianProcessMO, StudentTProcessMO,
                    GaussianProcessDerModel, check_mo_range)


class BQTransform(_DeviceApply, MomentTransform):
    """Base class (bq/bqmtran.py:11-130)."""

    _supported_models_ = ['gp', 'tp', 'bs', 'gp-mo', 'tp-mo']

    def __init__(self, dim_in, dim_out, kern_par, model, kern_str, point_str, point_par, estimate_par, **kwargs):
        self.model = BQTransform._get_model(dim_in, dim_out, model, kern_str, point_str, kern_par, point_par,
                                            estimate_par, **kwargs)
        self.I_out = np.eye(dim_out)
        self._dev = {}

    @staticmethod
    def _get_model(dim_in, dim_out, model, kern_str, point_str, kern_par, point_par, estimate_par, **kwargs):
        """bq/bqmtran.py:226-279.  NB: as in the reference, `nu` is NOT forwarded to the 'tp' model (appendix B-1 of
        SURVEY.md): the effective degrees of freedom are always 4.0."""
        if model.lower() not in BQTransform._supported_models_:
            print('Model {} not supported. Supported models are {}.'.format(model, BQTransform._supported_models_))
            return None
        if model == 'gp':
            return GaussianProcessModel(dim_in, kern_par, kern_str, point_str, point_par, estimate_par)
        if model == 'tp':
            return StudentTProcessModel(dim_in, kern_par, kern_str, point_str, point_par, estimate_par)
        if model == 'gp-mo':
            return GaussianProcessMO(dim_in, dim_out, kern_par, kern_str, point_str, point_par)
        if model == 'tp-mo':      # unlike 'tp', `nu` is forwarded here (bq/bqmtran.py:278-279)
            return StudentTProcessMO(dim_in, dim_out, kern_par, kern_str, point_str, point_par, **kwargs)
        return BayesSardModel(dim_in, kern_par, point_str=point_str, point_par=point_par, estimate_par=estimate_par,
                              **kwargs)

    def _set_kernel_attributes(self, kern_attr):
        """Attributes of the model's kernel (the 'rbf-student' kernel's dof, num_samples, seed) set before the weights are
        first computed; afterwards assign them to `model.kernel` and call `weights()` again."""
        for key, value in (kern_attr or {}).items():
            if not hasattr(self.model.kernel, key):
                raise AttributeError('{} has no attribute {!r}'.format(type(self.model.kernel).__name__, key))
            setattr(self.model.kernel, key, value)

    def weights(self, par, *args):
        """bq/bqmtran.py:111-130."""
        wm, wc, wcc, emv, ivar = self.model.bq_weights(par, *args)
        return wm, wc, wcc

    def apply(self, f, mean, cov, fcn_par, kern_par=None):
        """bq/bqmtran.py:60-109: weights are re-computed only when `kern_par` is given (:93-95)."""
        if kern_par is not None:
            self.wm, self.Wc, self.Wcc = self.weights(kern_par)
        return _DeviceApply.apply(self, f, mean, cov, fcn_par)

    # ---- device plumbing ------------------------------------------------------------------------------------------
    def _tp(self):
        return 0.0, None

    def _num_points(self):
        return self.model.points.shape[1]

    def _handle_for(self, E):
        D, N = self.model.points.shape
        mv = self.model.model_var
        emv = np.asarray(mv, dtype=float) * np.ones((E, E)) if np.ndim(mv) == 0 else np.asarray(mv, dtype=float)
        if emv.shape != (E, E):
            emv = np.broadcast_to(emv, (E, E)).copy()
        # `model_var * I_out` (bq/bqmtran.py:198): eye(E) keeps the diagonal; eye(1) with E > 1 broadcasts everything
        mode = EMV_DIAG if (self.I_out.shape[0] == E or E == 1) else EMV_BROADCAST
        nu, iK = self._tp()
        dt = self._dev.setdefault(E, DeviceTransform())
        return dt.get(D, E, N, FORM_BQ, self.model.points, self.wm, self.Wc, self.Wcc, emv, mode, nu, iK)


class GaussianProcessTransform(BQTransform):
    """GP quadrature moment transform (bq/bqmtran.py:285-310).  kern_str 'rbf' or 'rbf-student'; kern_attr (this build's
    addition): a dict of kernel attributes set before the weights are computed."""

    def __init__(self, dim_in, dim_out, kern_par, kern_str='rbf', point_str='ut', point_par=None, estimate_par=False,
                 kern_attr=None):
        super().__init__(dim_in, dim_out, kern_par, 'gp', kern_str, point_str, point_par, estimate_par)
        self._set_kernel_attributes(kern_attr)
        self.wm, self.Wc, self.Wcc = self.weights(kern_par)


class GaussianProcessDerTransform(BQTransform):
    """GP quadrature with derivative observations at the sigma points (research/gpqd/gpqd_base.py: GaussianProcessDerTransform,
    the MLSP-2016 moment transform): the GP is conditioned on the integrand's values at all N sigma points and on its Jacobians
    at the points `which_der` (strictly increasing indices, None = all, empty = none).  With L = chol(cov), x_n = mean + L xi_n
    the observation vector of output e is

        [f_e(x_1) .. f_e(x_N) | (J(x) L)[e, :] at which_der[0] | (J(x) L)[e, :] at which_der[1] | ..],     M = N + Nd D entries,

    and the moments are BQTransform's on that (E, M) matrix: mean_f = fx wm, cov_f = fx Wc fx' - mean_f mean_f' + model_var I,
    cov_fx = fx Wcc' L' - (E, D).  Three deliberate departures from the reference: the derivative observation is
    J L, the derivative in the unit coordinates the GP lives in (the reference takes J, right for cov = I only); row e of the
    observation matrix holds output e (the reference's reshape is right for one output only); every kernel expectation honours
    `which_der` (the reference's weights fail on a proper subset).  At one output, cov = I and all derivatives the two agree.

    One launch per batch: `k_apply_gpqd` (dim_in <= 2, observations in registers) or `k_apply_gpqd_lds` (observations in LDS).
    Supported: dim_in <= 6, 2 <= N <= 2 dim_in + 1 points ('ut', 'sr', 'gh' where it fits), outputs <= max(dim_in, 4); `f` the
    bound dyn_eval / meas_eval of a built-in model that has a Jacobian and additive noise (UNGM, pendulum, constant velocity,
    coordinated turn and the UNGM, pendulum, radar and bearing measurement models) or of a model of your own with `device_code`
    and `device_jacobian` (compiled at run time).
    Everything else raises NotImplementedError naming this range, before the library is touched.  `wm`, `Wc`, `Wcc` and
    `model.model_var` may be replaced after construction; the next call picks them up."""

    _RANGE = ('GaussianProcessDerTransform supports dim_in <= 6, 2 <= N <= 2 dim_in + 1 points, 1 <= outputs <= max(dim_in, 4) and the '
              'bound dyn_eval / meas_eval of a built-in model with a Jacobian and additive noise (UNGM, pendulum, constant velocity, '
              'coordinated turn, radar, bearings) or '
              'of a model with device_code and device_jacobian')
    _BUILTIN = (_lib.F_UNGM_DYN, _lib.F_UNGM_MEAS, _lib.F_PENDULUM_DYN, _lib.F_PENDULUM_MEAS, _lib.F_CV_DYN, _lib.F_CT_DYN,
                _lib.F_RADAR2D_MEAS, _lib.F_BEARING_MEAS)

    def __init__(self, dim_in, dim_out, kern_par, point_str='ut', point_par=None, estimate_par=False, which_der=None):
        if not (1 <= int(dim_in) <= 6 and 1 <= int(dim_out) <= max(int(dim_in), 4)):
            raise NotImplementedError('{} (got dim_in = {}, dim_out = {})'.format(self._RANGE, dim_in, dim_out))
        try:
            self.model = GaussianProcessDerModel(dim_in, kern_par, point_str, point_par, estimate_par, which_der)
        except NotImplementedError as e:
            raise NotImplementedError('{} ({})'.format(self._RANGE, e))
        self.e = int(dim_out)
        self.I_out = np.eye(dim_out)
        self._dev = {}
        self.wm, self.Wc, self.Wcc = self.weights(kern_par)

    def _device_integrand(self, f):
        """(Integrand, E) of a supported `f`; every refusal is raised here, before the library is touched."""
        owner = getattr(f, '__self__', None)
        if is_user_model(owner) and not has_device_jacobian(owner):
            raise user_unsupported('GaussianProcessDerTransform (model Jacobians: give the model a device_jacobian)')
        dev = resolve_integrand(f)
        if dev is None:
            raise NotImplementedError('not an arbitrary Python callable: ' + self._RANGE)
        if not getattr(owner, 'noise_additive', True):
            raise NotImplementedError('not a model with non-additive noise: ' + self._RANGE)
        integ, E = dev
        if integ.id < _lib.F_USER_FIRST and integ.id not in self._BUILTIN:
            raise NotImplementedError('{} has no Jacobian on the device: {}'.format(type(owner).__name__, self._RANGE))
        if not 1 <= E <= max(self.model.dim_in, 4):
            raise NotImplementedError('{} (got {} outputs)'.format(self._RANGE, E))
        return integ, E

    def _handle_for(self, E):
        D, N = self.model.points.shape
        wd = self.model.which_der
        M = N + wd.size * D
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (self.wm, self.Wc, self.Wcc)]
        if arrs[0].shape != (M,) or arrs[1].shape != (M, M) or arrs[2].shape != (D, M):
            raise ValueError('wm / Wc / Wcc must be (M,), (M, M), (D, M) with M = N + Nd D = {}'.format(M))
        mv = float(self.model.model_var)
        snap = (mv, wd.tobytes()) + tuple(a.tobytes() for a in arrs)
        have = self._dev.get(E)
        if have is not None and have[1] == snap:
            return have[0]
        lib = _lib.load()
        ptr = [a.ctypes.data_as(_lib.c_double_p) for a in arrs]
        pwd = wd.ctypes.data_as(_lib.c_int32_p)
        if have is not None:
            _lib.check(lib.ssmq_transform_gpqd_set(ctypes.c_void_p(have[0]), int(wd.size), pwd, ptr[0], ptr[1], ptr[2], mv),
                       'ssmq_transform_gpqd_set')
            h = have[0]
        else:
            h = lib.ssmq_transform_create_gpqd(D, int(E), N, _lib.as_c(self.model.points)[1], int(wd.size), pwd, ptr[0], ptr[1], ptr[2], mv)
            if not h:
                raise _lib.SsmqError('ssmq_transform_create_gpqd failed: ' + _lib.last_error())
        self._dev[E] = (h, snap)
        return h

    def kernel_name(self, f):
        self._device_integrand(f)
        return super().kernel_name(f)

    def apply_batch(self, f, mean, cov, time=None, fcn_pars=None, return_status=False):
        """B transforms in one launch: mean (B, D), cov (B, D, D), time scalar or (B,) -> (B, E), (B, E, E), (B, E, D)."""
        self._device_integrand(f)
        if np.ndim(mean) != 2 or np.shape(mean)[1] != self.model.dim_in:
            raise ValueError('mean must have shape (B, dim_in) with dim_in = {}'.format(self.model.dim_in))
        return super().apply_batch(f, mean, cov, time=0.0 if time is None else time, fcn_pars=fcn_pars, return_status=return_status)

    def apply_batch_dev(self, f, *args, **kwargs):
        self._device_integrand(f)
        return super().apply_batch_dev(f, *args, **kwargs)

    def _fixed_outputs(self):
        return self.e

    def __del__(self):
        try:
            lib = _lib.load()
            for h, _ in getattr(self, '_dev', {}).values():
                lib.ssmq_transform_destroy(ctypes.c_void_p(h))
            self._dev = {}
        except Exception:
            pass


class BayesSardTransform(BQTransform):
    """Bayes-Sard quadrature moment transform (bq/bqmtran.py:313-360)."""

    def __init__(self, dim_in, dim_out, kern_par, multi_ind=2, point_str='ut', point_par=None, estimate_par=False):
        super().__init__(dim_in, dim_out, kern_par, 'bs', 'rbf', point_str, point_par, estimate_par,
                         multi_ind=multi_ind)
        self.wm, self.Wc, self.Wcc = self.weights(kern_par, multi_ind)

    def weights(self, par, *args):
        multi_ind = args[0] if args else None
        wm, wc, wcc, emv, ivar = self.model.bq_weights(par, multi_ind)
        return wm, wc, wcc


class StudentTProcessTransform(BQTransform):
    """Student-t process quadrature moment transform (bq/bqmtran.py:363-415).  kern_str 'rbf' or 'rbf-student'; kern_attr
    (this build's addition): a dict of kernel attributes set before the weights are computed."""

    def __init__(self, dim_in, dim_out, kern_par, kern_str='rbf', point_str='ut', point_par=None, estimate_par=False,
                 nu=3.0, kern_attr=None):
        super().__init__(dim_in, dim_out, kern_par, 'tp', kern_str, point_str, point_par, estimate_par, nu=nu)
        self._set_kernel_attributes(kern_attr)
        self.wm, self.Wc, self.Wcc = self.weights(kern_par)

    def _tp(self):
        return float(self.model.nu), self.model.iK


class _MoDeviceTransform:
    """Owner of one multi-output `ssmq_transform` handle (`ssmq_transform_create_mo`); constants that were replaced on the Python
    side go up again through `ssmq_transform_update_mo`."""

    def __init__(self):
        self._handle = None
        self._key = None
        self._snap = None

    def get(self, D, E, N, xi, wm, Wc, Wcc, emv, tp_nu, iK):
        lib = _lib.load()
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (xi, wm, Wc, Wcc, emv, iK)]
        key = (D, E, N, float(tp_nu) > 0.0)
        snap = (float(tp_nu),) + tuple(None if a is None else a.tobytes() for a in arrs)
        if self._handle is not None and key == self._key and snap == self._snap:
            return self._handle
        ptr = [None if a is None else a.ctypes.data_as(_lib.c_double_p) for a in arrs]
        if self._handle is not None and key == self._key:
            _lib.check(lib.ssmq_transform_update_mo(ctypes.c_void_p(self._handle), ptr[0], ptr[1], ptr[2], ptr[3], ptr[4],
                                                    float(tp_nu), ptr[5]), 'ssmq_transform_update_mo')
        else:
            self.close()
            h = lib.ssmq_transform_create_mo(D, E, N, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], float(tp_nu), ptr[5])
            if not h:
                raise _lib.SsmqError('ssmq_transform_create_mo failed: ' + _lib.last_error())
            self._handle = h
        self._key, self._snap = key, snap
        return self._handle

    def close(self):
        if self._handle is not None:
            _lib.load().ssmq_transform_destroy(ctypes.c_void_p(self._handle))
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _MultiOutputTransform(BQTransform):
    """What the two multi-output transforms share (bq/bqmtran.py:425-602).  Deliberate departures from the reference, whose
    classes are unfinished: the constructor computes and sets wm (N, E), Wc (N, N, E, E), Wcc (D, N, E);
    `weights(par)` returns the three arrays (the reference unpacks five values from three and raises); the model variance goes on
    the DIAGONAL of the covariance, as the single-output `model_var * I_out` (the reference adds the (E,) vector to whole
    columns, which leaves cov_f unsymmetric); `apply` returns fresh arrays (the reference returns its scratch buffers).
    Moments: mean_f[i] = fx_i . wm[:, i]; cov_f[i, j] = fx_i' Wc[..., i, j] fx_j - mean_f[i] mean_f[j] + delta_ij emv_i;
    cov_fx[i] = fx_i Wcc[..., i]' L' - one kernel, k_apply_mo.  Runs for D <= 16, E <= 8, N <= 64, the 'rbf' kernel and the
    built-in models (NotImplementedError otherwise, before anything reaches the library)."""

    def __init__(self, dim_in, dim_out, kern_par, model, kern_str, point_str, point_par, estimate_par, **kwargs):
        kern_par = np.asarray(kern_par, dtype=np.float64)
        if kern_par.ndim != 2 or kern_par.shape != (dim_out, dim_in + 1):
            raise ValueError('kern_par must be (dim_out, 1 + dim_in) = ({}, {}), got {}'.format(dim_out, dim_in + 1, kern_par.shape))
        check_mo_range(dim_in, dim_out, 0, kern_str)
        super().__init__(dim_in, dim_out, kern_par, model, kern_str, point_str, point_par, estimate_par, **kwargs)
        self.e = dim_out
        self._mo = _MoDeviceTransform()
        self.wm, self.Wc, self.Wcc = self.weights(kern_par)

    def weights(self, par, *args):
        return self.model.bq_weights(par)

    def _check_user(self, integ, D):
        if integ.id >= _lib.F_USER_FIRST:
            raise user_unsupported('the multi-output transforms (D <= 16, E <= 8, N <= 64, built-in models)')

    def _refuse_user_model(self, f):
        """A user model (device_code) is refused before its code is registered with the library."""
        if is_user_model(getattr(f, '__self__', None)):
            raise user_unsupported('the multi-output transforms (D <= 16, E <= 8, N <= 64, built-in models)')

    def apply_batch(self, f, mean, cov, time=0.0, fcn_pars=None, return_status=False):
        self._refuse_user_model(f)
        return super().apply_batch(f, mean, cov, time=time, fcn_pars=fcn_pars, return_status=return_status)

    def apply_batch_dev(self, f, *args, **kwargs):
        self._refuse_user_model(f)
        return super().apply_batch_dev(f, *args, **kwargs)

    def kernel_name(self, f):
        self._refuse_user_model(f)
        return super().kernel_name(f)

    def _fixed_outputs(self):
        return self.e

    def _handle_for(self, E):
        if E not in (1, self.e):      # (1: the sigma points of a Python integrand, which do not depend on E)
            raise ValueError('the integrand has {} outputs, the transform was built for {}'.format(E, self.e))
        D, N = self.model.points.shape
        e = self.e
        wm, Wc, Wcc = np.asarray(self.wm), np.asarray(self.Wc), np.asarray(self.Wcc)
        if wm.shape != (N, e) or Wc.shape != (N, N, e, e) or Wcc.shape != (D, N, e):
            raise ValueError('wm / Wc / Wcc must be (N, E), (N, N, E, E), (D, N, E)')
        nu, iK = self._tp()
        return self._mo.get(D, e, N, self.model.points, wm.T, Wc.transpose(2, 3, 0, 1), Wcc.transpose(2, 0, 1),
                            np.broadcast_to(np.asarray(self.model.model_var, dtype=np.float64), (e,)), nu,
                            None if iK is None else np.asarray(iK).transpose(2, 0, 1))


class MultiOutputGaussianProcessTransform(_MultiOutputTransform):
    """Multi-output GP quadrature moment transform (bq/bqmtran.py:425-523): one kernel-parameter row per output, kern_par
    (dim_out, 1 + dim_in)."""

    def __init__(self, dim_in, dim_out, kern_par, kern_str='rbf', point_str='ut', point_par=None, estimate_par=False):
        super().__init__(dim_in, dim_out, kern_par, 'gp-mo', kern_str, point_str, point_par, estimate_par)


class MultiOutputStudentTProcessTransform(_MultiOutputTransform):
    """Multi-output Student-t process quadrature moment transform (bq/bqmtran.py:526-602): the model variance of output i is
    scaled by (nu - 2 + fx_i iK_i fx_i') / (nu - 2 + N).  `nu` reaches the model (unlike the single-output 'tp')."""

    def __init__(self, dim_in, dim_out, kern_par, kern_str='rbf', point_str='ut', point_par=None, estimate_par=False,
                 nu=3.0):
        super().__init__(dim_in, dim_out, kern_par, 'tp-mo', kern_str, point_str, point_par, estimate_par, nu=nu)

    def _tp(self):
        return float(self.model.nu), self.model.iK
