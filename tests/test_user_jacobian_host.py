"""User models with a device Jacobian (device_code + device_jacobian): registration, validation and the run-time compilation of
k_linearize_fn / k_taylor_gpqd_fn for gfx950 - no device needed."""
import numpy as np
import pytest

from ssmtoybox_amd import _lib, ssinf, ssmod
from tests import _user_jac_oracle as uo

# (D, E, DIN) of the compile checks: the scalar case, a measurement of one state, and three shapes the built-in table never had
SHAPES = [(1, 1, 1), (2, 1, 1), (3, 2, 3), (6, 4, 5), (6, 6, 6)]


def test_define_dx_registry():
    a = _lib.define_integrand_dx(uo.VDP_CODE, uo.VDP_JAC, 2, 2, False)
    assert _lib.F_USER_FIRST <= a < _lib.F_USER_FIRST + _lib.F_USER_SLOTS
    assert _lib.define_integrand_dx(uo.VDP_CODE, uo.VDP_JAC, 2, 2, False) == a                  # idempotent
    plain = _lib.define_integrand(uo.VDP_CODE, 2, 2, False)
    assert plain != a and _lib.define_integrand(uo.VDP_CODE, 2, 2, False) == plain              # the plain id is another, and stays
    b = _lib.define_integrand_dx(uo.VDP_CODE, uo.VDP_JAC_FLIPPED, 2, 2, False)
    assert b not in (a, plain) and _lib.define_integrand_dx(uo.VDP_CODE, uo.VDP_JAC, 2, 2, False) == a


def test_define_dx_validates_the_jacobian_body():
    def error(jac, body='o[0] = x[0];'):
        with pytest.raises(_lib.SsmqError) as e:
            _lib.define_integrand_dx(body, jac, 1, 1, False)
        return str(e.value)
    assert 'Jacobian body' in error('J[0] = 1.0; }') and 'unbalanced' in error('J[0] = 1.0; }')
    assert 'unbalanced' in error('{ J[0] = 1.0;')
    assert 'preprocessor' in error('#define C }\nJ[0] = 1.0;')
    assert 'digraph' in error('J[0] = 1.0; %>')
    assert 'line continuations' in error('J[0] = 1.0; // \\\n}')
    assert 'longer than' in error('J[0] = 1.0;' + ' ' * _lib.USER_BODY_MAX)
    assert 'Jacobian body is empty' in error('')
    assert 'integrand body' in error('J[0] = 1.0;', body='o[0] = x[0]; }')                       # the function body is still checked
    with pytest.raises(_lib.SsmqError) as e:
        _lib.define_integrand_dx('o[0] = x[0];', 'J[0] = 1.0;', 0, 1, False)
    assert 'din and dout' in str(e.value)


@pytest.mark.parametrize('D,E,DIN', SHAPES)
def test_compile_check_gfx950_no_scratch(D, E, DIN):
    """Both kernels for every shape: the lowered name carries the id and the shape, and the compile-time bodies use no scratch
    memory - the point of compiling them for the shape."""
    code, jac, _, _ = uo.poly_model(E, DIN)
    fid = _lib.define_integrand_dx(code, jac, DIN, E, True)
    for kind, name in ((_lib.RTC_LINEAR, '_ZN4ssmq14k_linearize_fn'), (_lib.RTC_TAYLOR_GPQD, '_ZN4ssmq16k_taylor_gpqd_fn')):
        rc, log = _lib.rtc_compile_check(fid, kind, D, E, 0, 0)
        assert rc == 0, log
        lowered = log.splitlines()[0]
        assert lowered.startswith(name) and 'ILi{}ELi{}ELi{}ELi{}EE'.format(fid, D, E, DIN) in lowered, log
        remarks = [ln.strip() for ln in log.splitlines()]
        print(D, E, DIN, name[10:], [ln for ln in remarks if ln.startswith(('VGPRs:', 'ScratchSize', 'Occupancy'))])
        assert 'ScratchSize [bytes/lane]: 0' in remarks, log
        assert 'VGPRs Spill: 0' in remarks, log


def test_jacobian_compile_error_names_the_jacobian_body():
    fid = _lib.define_integrand_dx('o[0] = x[0];', 'J[0] = undeclared_slope;', 1, 1, False)
    for kind in (_lib.RTC_LINEAR, _lib.RTC_TAYLOR_GPQD):
        rc, log = _lib.rtc_compile_check(fid, kind, 1, 1, 0, 0)
        assert rc == -3
        err = _lib.last_error()
        assert 'undeclared_slope' in err and 'undeclared identifier' in err and 'user_jacobian_{}'.format(fid) in err
        assert 'user_integrand_{}'.format(fid) not in err
        assert 'undeclared_slope' in log
    # ... and an error in the function body of the same integrand still names the function body
    fid = _lib.define_integrand_dx('o[0] = undeclared_value;', 'J[0] = 1.0;', 1, 1, False)
    rc, _ = _lib.rtc_compile_check(fid, _lib.RTC_LINEAR, 1, 1, 0, 0)
    assert rc == -3 and 'user_integrand_{}'.format(fid) in _lib.last_error()


def test_new_kinds_need_a_jacobian_and_a_shape_in_range():
    plain = _lib.define_integrand(uo.VDP_CODE, 2, 2, False)
    for kind in (_lib.RTC_LINEAR, _lib.RTC_TAYLOR_GPQD):
        rc, _ = _lib.rtc_compile_check(plain, kind, 2, 2, 0, 0)
        assert rc == -3 and 'no Jacobian' in _lib.last_error()
        rc, _ = _lib.rtc_compile_check(_lib.F_PENDULUM_DYN, kind, 2, 2, 0, 0)           # a built-in id is no user integrand
        assert rc == -1
    code, jac, _, _ = uo.poly_model(2, 2)
    fid = _lib.define_integrand_dx(code, jac, 2, 2, True)
    rc, _ = _lib.rtc_compile_check(fid, _lib.RTC_LINEAR, 7, 2, 0, 0)
    assert rc == -3 and 'D <= 6' in _lib.last_error()
    rc, _ = _lib.rtc_compile_check(fid, _lib.RTC_TAYLOR_GPQD, 3, 3, 0, 0)               # the integrand has two outputs
    assert rc == -1 and 'dimensions' in _lib.last_error()
    rc, _ = _lib.rtc_compile_check(fid, _lib.RTC_LINEAR, 1, 2, 0, 0)                    # ... and reads two inputs
    assert rc == -1


def test_the_other_kernels_still_compile_for_an_integrand_with_a_jacobian():
    """k_apply_small for the same id: the wrapper with jac() serves every run-time kernel."""
    fid = _lib.define_integrand_dx(uo.VDP_CODE, uo.VDP_JAC, 2, 2, False)
    rc, log = _lib.rtc_compile_check(fid, _lib.RTC_APPLY, 2, 2, 5, _lib.FORM_SIGMA)
    assert rc == 0 and 'Li{}E'.format(fid) in log.splitlines()[0], log


def _systems():
    VdP = uo.transition('VdP', 2, uo.VDP_CODE, uo.VDP_JAC, (0.1, 1.0))
    VdPMeas = uo.measurement('VdPMeas', 1, uo.VDP_MEAS_CODE, uo.VDP_MEAS_JAC)
    NoJac = uo.transition('NoJac', 2, uo.VDP_CODE, None, (0.1, 1.0))
    NoJacMeas = uo.measurement('NoJacMeas', 1, uo.VDP_MEAS_CODE, None)
    return VdP, VdPMeas, NoJac, NoJacMeas


def test_python_registration_and_refusals():
    VdP, VdPMeas, NoJac, NoJacMeas = _systems()
    rv2, rv1 = ssmod.GaussRV(2), ssmod.GaussRV(1)
    dyn, obs = VdP(rv2, rv2), VdPMeas(rv1, 2)
    f, e = dyn.device_integrand()
    assert e == 2 and f.id == _lib.define_integrand_dx(uo.VDP_CODE, uo.VDP_JAC, 2, 2, False) and tuple(f.par[:2]) == (0.1, 1.0)
    assert NoJac(rv2, rv2).device_integrand()[0].id == _lib.define_integrand(uo.VDP_CODE, 2, 2, False) != f.id
    assert ssmod.has_device_jacobian(dyn) and not ssmod.has_device_jacobian(NoJac(rv2, rv2))
    assert not ssmod.has_device_jacobian(ssmod.Pendulum2DTransition(rv2, rv2))
    # device_jacobian without device_code: ValueError at class use
    Orphan = uo.transition('Orphan', 2, None, uo.VDP_JAC)
    OrphanMeas = uo.measurement('OrphanMeas', 1, None, uo.VDP_MEAS_JAC)
    with pytest.raises(ValueError) as err:
        Orphan(rv2, rv2)
    assert 'device_jacobian without device_code' in str(err.value)
    with pytest.raises(ValueError):
        OrphanMeas(rv1, 2)
    # the extended Kalman filters take the pair with Jacobians, and refuse a member without one - naming device_jacobian
    ssinf.ExtendedKalman(dyn, obs)
    ssinf.ExtendedKalmanGPQD(dyn, obs, np.array([[1.0, 3.0, 3.0]]), np.array([[1.0, 3.0, 3.0]]))
    for d, o in ((NoJac(rv2, rv2), obs), (dyn, NoJacMeas(rv1, 2))):
        for make in (lambda: ssinf.ExtendedKalman(d, o), lambda: ssinf.ExtendedKalmanGPQD(d, o, np.ones((1, 3)), np.ones((1, 3)))):
            with pytest.raises(NotImplementedError) as err:
                make()
            assert 'device_jacobian' in str(err.value) and 'dim_state <= 6' in str(err.value)
    from ssmtoybox_amd import mtran
    m, P = np.zeros((3, 2)), np.tile(np.eye(2), (3, 1, 1))
    for tf in (mtran.LinearizationTransform(2), mtran.TaylorGPQDTransform(2, np.array([[1.0, 3.0, 3.0]]))):
        with pytest.raises(NotImplementedError) as err:
            tf.apply_batch(NoJac(rv2, rv2).dyn_eval, m, P)
        assert 'device_jacobian' in str(err.value)


def test_state_index_non_additive_and_large_state_refusals_unchanged():
    code7 = 'for (int i = 0; i < 7; ++i) o[i] = x[i];'
    Big = uo.transition('Big', 7, code7, 'for (int i = 0; i < 7; ++i) J[i * ldj + i] = 1.0;')
    NonAdditive = type('NonAdditive', (uo.transition('NA', 2, uo.VDP_CODE, uo.VDP_JAC, (0.1, 1.0)),), dict(noise_additive=False))
    VdPMeas = uo.measurement('VdPMeas', 1, uo.VDP_MEAS_CODE, uo.VDP_MEAS_JAC)
    for model in (Big(ssmod.GaussRV(7), ssmod.GaussRV(7)), NonAdditive(ssmod.GaussRV(2), ssmod.GaussRV(2)),
                  VdPMeas(ssmod.GaussRV(1), 2, state_index=[1])):
        with pytest.raises(NotImplementedError) as e:
            model.device_integrand()
        assert 'dim_state <= 6' in str(e.value)
