"""
Bayesian-quadrature moment transforms (reference: ssmtoybox/bq/bqmtran.py).

Constructor signatures, the `wm` / `Wc` / `Wcc` / `I_out` / `model` attributes and `apply()` / `weights()` follow the
reference (bq/bqmtran.py:55-130, 285-415) so that code written against it runs unchanged; weights and moments are
computed by HIP kernels.  `apply_batch()` (many trajectories per launch) is this build's addition.
"""
import numpy as np

from ..mtran import MomentTransform, _DeviceApply, DeviceTransform
from .._lib import FORM_BQ, EMV_DIAG, EMV_BROADCAST
from .bqmod import GaussianProcessModel, StudentTProcessModel, BayesSardModel


class BQTransform(_DeviceApply, MomentTransform):
    """Base class (bq/bqmtran.py:11-130)."""

    _supported_models_ = ['gp', 'tp', 'bs']

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
