"""User-defined models (device_code): registration, validation and run-time compilation for gfx950 - no device needed."""
import numpy as np
import pytest

from ssmtoybox_amd import _lib, ssinf, ssmod

PEND_DYN = 'o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]);'
PEND_MEAS = 'o[0] = sin_nr(x[0]);'
# three uncoupled pendulums: a 6-D state
PEND6_DYN = 'for (int i = 0; i < 3; ++i) { o[2 * i] = x[2 * i] + x[2 * i + 1] * p[0]; o[2 * i + 1] = x[2 * i + 1] - 9.81 * p[0] * sin_nr(x[2 * i]); }'
PEND6_MEAS = 'o[0] = sin_nr(x[0]); o[1] = sin_nr(x[2]) + x[4];'


def _error(body, din=1, dout=1):
    with pytest.raises(_lib.SsmqError) as e:
        _lib.define_integrand(body, din, dout, False)
    return str(e.value)


def test_define_validation():
    for din, dout in ((0, 1), (17, 1), (1, 0), (1, 17), (-1, 2)):
        assert 'din and dout' in _error('o[0] = x[0];', din, dout)
    assert 'unbalanced' in _error('o[0] = x[0]; }')
    assert 'unbalanced' in _error('{ o[0] = x[0];')
    assert 'unbalanced' in _error('/* { */ } void f() { o[0] = x[0];')      # a brace in a comment does not count
    assert 'unbalanced' in _error('o[0] = x[0]; } } void g() { {')            # balanced in total, but closes the function
    assert 'preprocessor' in _error('#define C }\no[0] = x[0];')
    assert 'digraph' in _error('o[0] = x[0]; %>')
    assert 'longer than' in _error('o[0] = x[0];' + ' ' * _lib.USER_BODY_MAX)
    assert 'empty' in _error('')
    assert 'empty' in _lib.last_error()
    with pytest.raises(ValueError):                                            # more than SSMQ_MAX_FPAR constants
        _lib.Integrand.make(_lib.F_USER_FIRST, range(_lib.SSMQ_MAX_FPAR + 1))


def test_define_idempotent():
    a = _lib.define_integrand(PEND_DYN, 2, 2, False)
    assert _lib.F_USER_FIRST <= a < _lib.F_USER_FIRST + _lib.F_USER_SLOTS
    assert _lib.define_integrand(PEND_DYN, 2, 2, False) == a
    assert _lib.define_integrand(PEND_DYN + ' ', 2, 2, False) != a
    assert _lib.define_integrand(PEND_MEAS, 1, 1, False) != a
    # braces inside literals and comments are not code
    assert _lib.define_integrand('o[0] = x[0]; // }', 1, 1, False) >= _lib.F_USER_FIRST


@pytest.mark.parametrize('D', [2, 6])
def test_compile_check_gfx950(D):
    dyn, meas = (PEND_DYN, PEND_MEAS) if D == 2 else (PEND6_DYN, PEND6_MEAS)
    Y = 1 if D == 2 else 2
    fd = _lib.define_integrand(dyn, D, D, False)
    fo = _lib.define_integrand(meas, 1 if D == 2 else 5, Y, False)
    N = 2 * D + 1
    for form in (_lib.FORM_SIGMA, _lib.FORM_BQ):
        rc, log = _lib.rtc_compile_check(fd, _lib.RTC_FILTER, D, Y, N, form, fid_obs=fo, N_obs=N)
        assert rc == 0, log
        name = log.splitlines()[0]
        assert name.startswith('_ZN4ssmq14k_filter_fused') and 'Li{}E'.format(fd) in name and 'Li{}E'.format(fo) in name, log
        assert 'VGPRs:' in log
    rc, log = _lib.rtc_compile_check(fd, _lib.RTC_APPLY, D, D, N, _lib.FORM_BQ, tp=1)
    assert rc == 0 and log.splitlines()[0].startswith('_ZN4ssmq13k_apply_small'), log
    rc, log = _lib.rtc_compile_check(fo, _lib.RTC_APPLY, D, Y, 2 * D, _lib.FORM_SIGMA)
    assert rc == 0 and log.splitlines()[0].startswith('_ZN4ssmq13k_apply_small'), log


def test_compile_check_refuses_shapes():
    fd = _lib.define_integrand(PEND_DYN, 2, 2, False)
    rc, _ = _lib.rtc_compile_check(fd, _lib.RTC_APPLY, 7, 7, 15, _lib.FORM_SIGMA)
    assert rc == -3 and 'D <= 6' in _lib.last_error()
    rc, _ = _lib.rtc_compile_check(fd, _lib.RTC_APPLY, 2, 2, 9, _lib.FORM_SIGMA)      # N > 2 D + 1
    assert rc == -3


def test_compile_error_reports_compiler_message():
    fid = _lib.define_integrand('o[0] = undeclared_thing * x[0];', 1, 1, False)
    rc, log = _lib.rtc_compile_check(fid, _lib.RTC_APPLY, 1, 1, 3, _lib.FORM_SIGMA)
    assert rc == -3
    err = _lib.last_error()
    assert 'undeclared_thing' in err and 'undeclared identifier' in err and 'user_integrand_{}'.format(fid) in err
    assert 'undeclared_thing' in log


class UserPendulum(ssmod.TransitionModel):
    dim_state, dim_noise, noise_additive = 2, 2, True
    device_code = PEND_DYN

    def __init__(self, init_rv=None, noise_rv=None, dt=0.01):
        super().__init__(init_rv, noise_rv)
        self.dt = dt

    def _par(self):
        return (self.dt,)


class UserPendulumMeas(ssmod.MeasurementModel):
    dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
    device_code = PEND_MEAS


def test_model_registration_once_per_class_and_body():
    m = UserPendulum(ssmod.GaussRV(2), ssmod.GaussRV(2), dt=0.05)
    f, e = m.device_integrand()
    assert e == 2 and f.id >= _lib.F_USER_FIRST and f.n_par == 1 and f.par[0] == 0.05
    assert UserPendulum(ssmod.GaussRV(2), ssmod.GaussRV(2)).device_integrand()[0].id == f.id
    g, e = UserPendulumMeas(ssmod.GaussRV(1), 2).device_integrand()
    assert e == 1 and g.id != f.id
    # built-in models are untouched
    assert ssmod.Pendulum2DTransition(ssmod.GaussRV(2), ssmod.GaussRV(2)).device_integrand()[0].id == _lib.F_PENDULUM_DYN


def test_model_refusals_name_what_is_supported():
    class Big(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 7, 7, True
        device_code = 'for (int i = 0; i < 7; ++i) o[i] = x[i];'

    class NonAdditive(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, False
        device_code = PEND_DYN

    for model in (Big(ssmod.GaussRV(7), ssmod.GaussRV(7)), NonAdditive(ssmod.GaussRV(2), ssmod.GaussRV(2)),
                  UserPendulumMeas(ssmod.GaussRV(1), 2, state_index=[1])):
        with pytest.raises(NotImplementedError) as e:
            model.device_integrand()
        assert 'dim_state <= 6' in str(e.value)
    dyn, obs = UserPendulum(ssmod.GaussRV(2), ssmod.GaussRV(2)), UserPendulumMeas(ssmod.GaussRV(1), 2)
    with pytest.raises(NotImplementedError):
        ssinf.ExtendedKalman(dyn, obs)
    with pytest.raises(NotImplementedError):
        dyn.simulate_discrete(10, 4)
    with pytest.raises(NotImplementedError):
        obs.simulate_measurements(np.zeros((2, 10, 4)))


def test_define_refuses_line_splices():
    # a backslash before a line break joins lines before comments end: the compiler would see braces the scan does not
    for body in ('// \\\n{{\n}} int m; __device__ void g() const { {\n// \\\n}}',   # `//` comment continued onto the next line
                 '/* { *\\\n/ } o[0] = x[0];',                                         # `*` + `/` spliced into a comment end
                 'o[0] = x[0]; // \\  \n}'):                                           # (clang splices across trailing blanks too)
        assert 'line continuations' in _error(body)
    assert _lib.define_integrand('o[0] = x[0]; // a \\ b', 1, 1, False) >= _lib.F_USER_FIRST


def test_user_point_count_refused_in_python():
    """Point sets beyond 2 D + 1 raise NotImplementedError naming the range, before anything reaches the library."""
    from ssmtoybox_amd import mtran
    dyn, obs = UserPendulum(ssmod.GaussRV(2), ssmod.GaussRV(2)), UserPendulumMeas(ssmod.GaussRV(1), 2)
    alg = ssinf.GaussHermiteKalman(dyn, obs, deg=3)                  # 3^2 = 9 points at D = 2
    for call in (lambda: alg.forward_pass_batch(np.zeros((1, 5, 4))), lambda: alg.kernel_name(4)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert '2 .. 2 D + 1' in str(e.value) and 'dim_state <= 6' in str(e.value)
    with pytest.raises(NotImplementedError):
        mtran.GaussHermiteTransform(2, 3).apply_batch(dyn.dyn_eval, np.zeros((3, 2)), np.tile(np.eye(2), (3, 1, 1)))


def test_compile_check_mixed_pair():
    """A built-in model next to a user model: one instantiation with both functors (UNGM's dynamics read its host time table)."""
    fo = _lib.define_integrand('o[0] = 0.05 * (x[0] * x[0]);', 1, 1, False)
    rc, log = _lib.rtc_compile_check(_lib.F_UNGM_DYN, _lib.RTC_FILTER, 1, 1, 3, _lib.FORM_SIGMA, fid_obs=fo, N_obs=3)
    assert rc == 0 and 'Li{}ELi{}E'.format(_lib.F_UNGM_DYN, fo) in log.splitlines()[0], log
