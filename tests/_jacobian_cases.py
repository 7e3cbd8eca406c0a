"""Model tables of the linearisation and Taylor-GPQD tests, shared with tools/jacobian_digests.py."""
import numpy as np

from oracle import ssmq_oracle as orc


def linear_models():
    """tag -> (model, 'dyn' / 'meas', fid, integrand constants, state index) of test_linearization_transform_golden."""
    from ssmtoybox_amd import ssmod as sm
    dt = 0.01
    q2 = sm.GaussRV(2, cov=0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]]))
    return {
        'ungm_dyn': (sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), 'dyn', orc.F_UNGM_DYN, (), None),
        'ungmna_dyn': (sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))), 'dyn', orc.F_UNGMNA_DYN, (), None),
        'pend_dyn': (sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0]), cov=0.01 * np.eye(2)), q2, dt=dt), 'dyn',
                     orc.F_PENDULUM_DYN, (dt,), None),
        'cv_dyn': (sm.ConstantVelocity(sm.GaussRV(4), sm.GaussRV(2), dt=0.5), 'dyn', orc.F_CV_DYN, (0.5,), None),
        'ungm_meas': (sm.UNGMMeasurement(sm.GaussRV(1), 1), 'meas', orc.F_UNGM_MEAS, (), None),
        'ungmna_meas': (sm.UNGMNAMeasurement(sm.GaussRV(1), 1), 'meas', orc.F_UNGMNA_MEAS, (), None),
        'pend_meas': (sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2), 'meas', orc.F_PENDULUM_MEAS, (), None),
        'pend_meas_idx': (sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2, state_index=[0]), 'meas',
                          orc.F_PENDULUM_MEAS, (), [0]),
    }


def package_models():
    """g21 block -> the package's dyn_eval / meas_eval."""
    from ssmtoybox_amd import ssmod as sm
    dt = 0.01
    q2 = sm.GaussRV(2, cov=0.01 * np.array([[(dt ** 3) / 3, (dt ** 2) / 2], [(dt ** 2) / 2, dt]]))
    return {
        'ungm_dyn': sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))).dyn_eval,
        'ungm_meas': sm.UNGMMeasurement(sm.GaussRV(1), 1).meas_eval,
        'pend_dyn': sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0]), cov=0.01 * np.eye(2)), q2, dt=dt).dyn_eval,
        'pend_meas': sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2).meas_eval,
        'cv_dyn': sm.ConstantVelocity(sm.GaussRV(4), sm.GaussRV(2), dt=0.5).dyn_eval,
        'ungmna_dyn': sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))).dyn_eval,
    }


def index_cases():
    """tag -> (model, fid, D, state index): a non-leading index on the <2, 1> body, a reversed one on a shape that has only <0, 0>."""
    from ssmtoybox_amd import ssmod as sm
    from ssmtoybox_amd import _lib

    class ReversedUNGMNA(sm.UNGMNAMeasurement):
        """Both inputs [x, r] of the model picked from a 3-D input, in reverse order (the class itself appends the noise index)."""

        def device_integrand(self):
            return _lib.Integrand.make(_lib.F_UNGMNA_MEAS, (), [2, 0]), 1

    return {
        'pend_meas_idx1': (sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2, state_index=[1]), orc.F_PENDULUM_MEAS, 2, [1]),
        'ungmna_meas_idx20': (ReversedUNGMNA(sm.GaussRV(1), 2), orc.F_UNGMNA_MEAS, 3, [2, 0]),
    }
