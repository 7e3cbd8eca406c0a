"""Truncated sigma-point transforms and their filters, the parts that need no device: the NumPy restatement
(tests/_truncated_oracle.py) against the reference's outputs (tests/golden/g22_truncated.npz), the refusals that come before the
library is touched, the exported constructor and the default of dim_eff."""
import ctypes

import numpy as np
import pytest

from tests._cases import rel_err
from tests import _truncated_oracle as tro


@pytest.fixture(scope='module')
def g22(golden):
    return golden('g22_truncated')


def ctor(g22, rule, dim, de):
    return {a: g22['ctor_%s_%d_%d_%s' % (rule, dim, de, a)] for a in ('wm', 'Wc', 'Wcc', 'unit_sp_eff', 'unit_sp')}


@pytest.mark.parametrize('rule', tro.RULES)
@pytest.mark.parametrize('tag', list(tro.CASES))
def test_oracle_agrees_with_the_reference(g22, tag, rule):
    """Every apply case to 1e-13 relative (max |a - b| / max |b| per item): NumPy against NumPy, the same formulas."""
    fid, p, D, de, E = tro.CASES[tag]
    c = ctor(g22, rule, D, de)
    f = tro.integrand(fid, p)
    for i in range(tro.N_ITEMS):
        got = tro.apply(f, g22[tag + '_mean'][i], g22[tag + '_cov'][i], de, c['unit_sp_eff'], c['wm'], np.diag(c['Wc']), c['unit_sp'],
                        np.diag(c['Wcc']))
        for k, key in enumerate(('mf', 'cf', 'cfx')):
            ref = g22['%s_%s_%s' % (tag, rule, key)][i]
            assert got[k].shape == ref.shape
            e = rel_err(got[k], ref)
            assert e <= 1e-13, (tag, rule, i, key, e)


def _models():
    from ssmtoybox_amd import ssmod as sm

    class UserMeas(sm.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
        device_code = 'o[0] = sin(x[0]);'

    class UserDyn(sm.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, True
        device_code = 'o[0] = x[0] + p[0] * x[1]; o[1] = x[1] - 9.81 * p[0] * sin(x[0]);'

        def _par(self):
            return (0.01,)

    return sm, UserMeas, UserDyn


def test_refusals_come_before_the_library(monkeypatch):
    import ssmtoybox_amd as amd
    from ssmtoybox_amd import ssinf, _lib
    sm, UserMeas, UserDyn = _models()

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', no_library)
    m5, P5 = np.ones((1, 5)), np.eye(5)[None]
    radar = sm.Radar2DMeasurement(sm.GaussRV(2), 5)
    for tf in (amd.TruncatedUnscentedTransform(5, 2), amd.TruncatedSphericalRadialTransform(5, 2), amd.TruncatedGaussHermiteTransform(5, 2)):
        assert isinstance(tf, amd.TruncatedSigmaPointTransform) and (tf.dim, tf.dim_eff) == (5, 2)
        for call in (lambda f: tf.apply(f, m5[0], P5[0], np.atleast_1d(0.0)), lambda f: tf.apply_batch(f, m5, P5), tf.kernel_name,
                     lambda f: tf.apply_batch_dev(f, None, None, None, None, None, None, None)):
            with pytest.raises(NotImplementedError, match='Python callable'):
                call(lambda x, p: x[:2])
            with pytest.raises(NotImplementedError, match='user model'):
                call(UserMeas(sm.GaussRV(1), 5).meas_eval)
            with pytest.raises(NotImplementedError, match='non-additive'):
                call(sm.UNGMNAMeasurement(sm.GaussRV(1), 5).meas_eval)
            # models that read beyond dim_eff: a 5-input transition model, a state index that reaches entry 2
            with pytest.raises(NotImplementedError, match='beyond dim_eff'):
                call(sm.ReentryVehicle2DTransition(sm.GaussRV(5), sm.GaussRV(3)).dyn_eval)
            with pytest.raises(NotImplementedError, match='beyond dim_eff'):
                call(sm.Radar2DMeasurement(sm.GaussRV(2), 5, state_index=[0, 2]).meas_eval)
    with pytest.raises(NotImplementedError, match='beyond dim_eff'):
        amd.TruncatedUnscentedTransform(5, 1).apply_batch(radar.meas_eval, m5, P5)
    # the range, named in the message: dim > 6, more than 4 outputs, more than 729 points
    with pytest.raises(NotImplementedError, match='dim <= 6'):
        amd.TruncatedUnscentedTransform(7, 2).apply_batch(sm.Radar2DMeasurement(sm.GaussRV(2), 7).meas_eval, np.ones((1, 7)), np.eye(7)[None])
    with pytest.raises(NotImplementedError, match='outputs <= 4'):
        bearing = sm.BearingMeasurement(sm.GaussRV(5), 5, sensor_pos=np.arange(10.0).reshape(5, 2))
        amd.TruncatedUnscentedTransform(5, 2).apply_batch(bearing.meas_eval, m5, P5)
    with pytest.raises(NotImplementedError, match='729 points'):
        amd.TruncatedGaussHermiteTransform(5, 2, degree=5).apply_batch(radar.meas_eval, m5, P5)
    # the filters
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, cov=np.eye(5)), sm.GaussRV(3))
    for make in (lambda d, o, **k: ssinf.TruncatedUnscentedKalman(d, o, **k), lambda d, o, **k: ssinf.TruncatedCubatureKalman(d, o, **k),
                 lambda d, o, **k: ssinf.TruncatedGaussHermiteKalman(d, o, 3, **k)):
        with pytest.raises(NotImplementedError, match='user model'):
            make(UserDyn(sm.GaussRV(2), sm.GaussRV(2)), UserMeas(sm.GaussRV(1), 2))
        with pytest.raises(NotImplementedError, match='user model'):
            make(sm.Pendulum2DTransition(sm.GaussRV(2), sm.GaussRV(2)), UserMeas(sm.GaussRV(1), 2))
        with pytest.raises(NotImplementedError, match='additive'):
            make(sm.UNGMNATransition(sm.GaussRV(1), sm.GaussRV(1)), sm.UNGMNAMeasurement(sm.GaussRV(1), 1))
        with pytest.raises(NotImplementedError, match='beyond dim_eff'):
            make(dyn, radar, dim_eff=1)
    flt = ssinf.TruncatedUnscentedKalman(dyn, radar)
    monkeypatch.undo()          # (run_filters loads the library before it looks at its filters)
    with pytest.raises(NotImplementedError, match='truncated'):
        ssinf.run_filters([flt], np.zeros((2, 3, 2)))


def test_dim_eff_defaults_to_the_substate_dimension():
    import ssmtoybox_amd as amd
    from ssmtoybox_amd import ssinf
    sm = amd.ssmod
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, cov=np.eye(5)), sm.GaussRV(3))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2), 5)
    pend = (sm.Pendulum2DTransition(sm.GaussRV(2), sm.GaussRV(2)), sm.Pendulum2DMeasurement(sm.GaussRV(1), 2))
    for cls, args, plain, trunc in ((ssinf.TruncatedUnscentedKalman, (), amd.UnscentedTransform, amd.TruncatedUnscentedTransform),
                                    (ssinf.TruncatedCubatureKalman, (), amd.SphericalRadialTransform, amd.TruncatedSphericalRadialTransform),
                                    (ssinf.TruncatedGaussHermiteKalman, (3,), amd.GaussHermiteTransform, amd.TruncatedGaussHermiteTransform)):
        flt = cls(dyn, obs, *args)
        assert isinstance(flt, ssinf.GaussianInference) and type(flt.tf_dyn) is plain and type(flt.tf_obs) is trunc
        assert flt.dim_eff == obs.dim_substate == 2 and (flt.tf_obs.dim, flt.tf_obs.dim_eff) == (5, 2)
        assert flt.tf_obs.unit_sp_eff.shape[0] == 2 and flt.tf_obs.unit_sp.shape[0] == 5
        assert cls(*pend, *args).tf_obs.dim_eff == 1
        full = cls(dyn, obs, *args, dim_eff=obs.dim_state)          # the reference's behaviour
        assert full.dim_eff == 5 and full.tf_obs.unit_sp_eff.shape == full.tf_obs.unit_sp.shape
        for name in ('forward_pass', 'forward_pass_batch', 'forward_pass_dev', 'backward_pass', 'backward_pass_batch', 'kernel_name'):
            assert callable(getattr(flt, name))


@pytest.mark.parametrize('rule', tro.RULES)
def test_constructors_reproduce_the_reference_on_the_host(g22, rule):
    """Host arithmetic only: the attributes within 1e-14 of the reference's (the GPU test states where they are bit-equal)."""
    import ssmtoybox_amd as amd
    cls = {'ut': amd.TruncatedUnscentedTransform, 'sr': amd.TruncatedSphericalRadialTransform, 'gh': amd.TruncatedGaussHermiteTransform}[rule]
    for dim, de in tro.DIMS:
        tf, ref = cls(dim, de), ctor(g22, rule, dim, de)
        for a, r in ref.items():
            got = np.asarray(getattr(tf, a), dtype=float)
            assert got.shape == r.shape and np.max(np.abs(got - r)) <= 1e-14 * max(1.0, np.max(np.abs(r))), (rule, dim, de, a)


def test_library_exports_the_constructor():
    from ssmtoybox_amd import _lib
    assert 'ssmq_transform_create_truncated' in _lib.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(_lib.library_path())
    assert hasattr(lib, 'ssmq_transform_create_truncated')
    assert _lib.FORM_TRUNC_SIGMA == 5
    import ssmtoybox_amd as amd
    for name in ('TruncatedSigmaPointTransform', 'TruncatedSphericalRadialTransform', 'TruncatedUnscentedTransform', 'TruncatedGaussHermiteTransform'):
        assert getattr(amd, name) is getattr(amd.mtran, name)
