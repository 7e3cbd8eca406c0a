"""User-defined models (device_code) on the device: the run-time compiled whole-pass filter kernel and k_apply_small against
the reference (tests/golden/make_golden_user.py), bit for bit against the built-in route, time dependence, refusals, cache."""
import ctypes

import numpy as np
import pytest

from tests._cases import assert_moments_close, cov_err, rel_err, within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


def _models():
    from ssmtoybox_amd import ssmod

    class VanDerPol(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, True
        device_code = 'o[0] = x[0] + p[0] * x[1];  o[1] = x[1] + p[0] * (p[1] * (1.0 - x[0] * x[0]) * x[1] - x[0]);'

        def __init__(self, init_rv, noise_rv, dt=0.1, mu=1.0):
            super().__init__(init_rv, noise_rv)
            self.dt, self.mu = dt, mu

        def _par(self):
            return (self.dt, self.mu)

    class VdPMeasurement(ssmod.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 2, 1, True
        device_code = 'o[0] = x[0] + 0.5 * sin(x[1]);'

    class CoupledPendulums(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 4, 4, True
        device_code = '''const double dt = p[0], c = p[1], k = p[2];
            o[0] = x[0] + dt * x[1];  o[1] = x[1] + dt * (-sin(x[0]) - c * x[1] + k * (x[2] - x[0]));
            o[2] = x[2] + dt * x[3];  o[3] = x[3] + dt * (-sin(x[2]) - c * x[3] + k * (x[0] - x[2]));'''

        def _par(self):
            return (0.05, 0.2, 0.5)

    class CoupledMeasurement(ssmod.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 2, 4, 2, True
        device_code = 'o[0] = sin(x[0]) + 0.5 * x[2];  o[1] = 0.5 * x[0] + sin(x[2]);'

    return {'vdp': (VanDerPol, VdPMeasurement), 'cpl': (CoupledPendulums, CoupledMeasurement)}


def _system(g, tag, student=False):
    from ssmtoybox_amd import ssmod
    Dyn, Obs = _models()[tag]
    m0, P0, Q, R = g[tag + '_m0'], g[tag + '_P0'], g[tag + '_Q'], g[tag + '_R']
    D, Y = m0.shape[0], R.shape[0]
    if student:
        return Dyn(ssmod.StudentRV(D, m0, P0, 1000.0), ssmod.StudentRV(D, scale=Q, dof=1000.0)), \
            Obs(ssmod.StudentRV(Y, scale=R, dof=4.0), D)
    return Dyn(ssmod.GaussRV(D, m0, P0), ssmod.GaussRV(D, cov=Q)), Obs(ssmod.GaussRV(Y, cov=R), D)


def _filter(name, dyn, obs, D):
    from ssmtoybox_amd import ssinf
    par = np.array([[1.0] + [2.0] * D])
    mi = np.hstack((np.zeros((D, 1)), np.eye(D), 2 * np.eye(D))).astype(int)
    return {'ukf': lambda: ssinf.UnscentedKalman(dyn, obs), 'ckf': lambda: ssinf.CubatureKalman(dyn, obs),
            'gpqkf': lambda: ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
            'bsqkf': lambda: ssinf.BayesSardKalman(dyn, obs, par, par, mi, mi, 'ut'),
            'tpqkf': lambda: ssinf.StudentProcessKalman(dyn, obs, par, par, 'rbf', 'ut'),
            'fss': lambda: ssinf.FullySymmetricStudent(dyn, obs)}[name]()


@pytest.mark.parametrize('tag', ['vdp', 'cpl'])
@pytest.mark.parametrize('name', ['ukf', 'ckf', 'gpqkf', 'bsqkf', 'tpqkf', 'fss'])
def test_user_filter_golden(amd, golden, tag, name):
    """(a) every filter of the fixture on user models, through forward_pass_batch, against the reference."""
    g = golden('g15_user_models')
    dyn, obs = _system(g, tag, student=(name == 'fss'))
    D = dyn.dim_state
    alg = _filter(name, dyn, obs, D)
    assert 'k_filter_fused' in alg.kernel_name(8) and 'run-time compiled' in alg.kernel_name(8)
    y = g[tag + '_y']
    fm, fP = alg.forward_pass_batch(y)
    ref_fm = g['{}_{}_fm'.format(tag, name)]
    ref_fc = np.zeros((D, D) + ref_fm.shape[1:])
    il = np.tril_indices(D)
    ref_fc[il] = g['{}_{}_fcl'.format(tag, name)]
    ref_fc[il[1], il[0]] = g['{}_{}_fcl'.format(tag, name)]
    assert rel_err(fm, ref_fm) < 1e-8, (tag, name, rel_err(fm, ref_fm))
    assert within(cov_err(fP, ref_fc), 5e-9, 'user %s %s fP vs reference' % (tag, name)), (tag, name)


@pytest.mark.parametrize('tag', ['vdp', 'cpl'])
def test_user_transforms_golden(amd, golden, tag):
    """(a) UnscentedTransform / GaussianProcessTransform .apply_batch on the user model functions (k_apply_small, run-time
    compiled) against the reference's apply(), GP weights injected from the fixture."""
    g = golden('g15_user_models')
    dyn, obs = _system(g, tag)
    D = dyn.dim_state
    for fname, f, dout in ((tag + '_dyn', dyn.dyn_eval, D), (tag + '_meas', obs.meas_eval, obs.dim_out)):
        means, covs = g[fname + '_mean'], g[fname + '_cov']
        for tname in ('ut', 'gpq'):
            key = '{}_{}'.format(fname, tname)
            if tname == 'ut':
                tf = amd.UnscentedTransform(D)
            else:
                tf = amd.GaussianProcessTransform(D, dout, np.array([[1.0] + [2.0] * D]), 'rbf', 'ut')
                assert np.array_equal(tf.model.points, g[key + '_pts'])
                tf.wm, tf.Wc, tf.Wcc = g[key + '_wm'], g[key + '_Wc'], g[key + '_Wcc']
                tf.model.model_var = float(g[key + '_mv'])
            assert 'run-time compiled' in tf.kernel_name(f)
            got = tf.apply_batch(f, means, covs, np.zeros(means.shape[0]))
            ref = (g[key + '_mf'], g[key + '_cf'], g[key + '_cfx'])
            for i in range(means.shape[0]):
                assert_moments_close([a[i] for a in got], [a[i] for a in ref], covs[i], what=(key, i))


def _pendulum_user():
    from ssmtoybox_amd import ssmod

    class UserPendulum(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, True
        # Fn<SSMQ_F_PENDULUM_DYN> restated (csrc/ssmq_device.h): the same expressions and helpers
        device_code = 'o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]);'

        def __init__(self, init_rv, noise_rv, dt=0.01):
            super().__init__(init_rv, noise_rv)
            self.dt = dt

        def _par(self):
            return (self.dt,)

    class UserPendulumMeas(ssmod.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
        device_code = 'o[0] = sin_nr(x[0]);'

    return UserPendulum, UserPendulumMeas


@pytest.mark.parametrize('name', ['ukf', 'gpqkf'])
def test_user_pendulum_bit_identical_to_builtin(amd, monkeypatch, name):
    """(b) the pendulum restated as device code runs the built-in route's code: fm, fP and status bit for bit, B = 1e4, T = 100,
    both on the whole-pass kernel."""
    from ssmtoybox_amd import ssinf, ssmod
    monkeypatch.setenv('SSMQ_FUSED_QUAD', '0')
    B, T = 10000, 100
    m0, P0, Q = np.array([1.5, 0.0]), 0.01 * np.eye(2), 0.01 * np.array([[0.01 ** 3 / 3, 0.01 ** 2 / 2], [0.01 ** 2 / 2, 0.01]])
    UP, UM = _pendulum_user()
    rng = np.random.default_rng(11)
    y = np.sin(1.5 * np.cos(np.linspace(0, 3, T)))[None, :, None] + 0.1 * rng.standard_normal((1, T, B))
    par = np.array([[1.0, 2.0, 2.0]])
    res = []
    for Dyn, Obs in ((ssmod.Pendulum2DTransition, ssmod.Pendulum2DMeasurement), (UP, UM)):
        dyn, obs = Dyn(ssmod.GaussRV(2, m0, P0), ssmod.GaussRV(2, cov=Q)), Obs(ssmod.GaussRV(1, cov=np.array([[0.1]])), 2)
        alg = ssinf.UnscentedKalman(dyn, obs) if name == 'ukf' else ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut')
        kn = alg.kernel_name(B)
        assert kn.startswith('k_filter_fused<'), kn
        fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
        res.append((fm.copy(), fP.copy(), alg.status.copy(), kn))
    (fm0, fP0, st0, k0), (fm1, fP1, st1, k1) = res
    assert 'run-time compiled' in k1 and 'run-time compiled' not in k0
    assert np.all(np.isfinite(fm0)) and not st0.any()
    assert np.array_equal(fm0, fm1) and np.array_equal(fP0, fP1) and np.array_equal(st0, st1)


def test_user_time_dependence(amd, golden):
    """(c) UNGM with its time term cos(1.2 t) in the device code agrees with the built-in UNGM filter (host time table)."""
    from ssmtoybox_amd import ssinf, ssmod

    class UserUNGM(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 1, 1, True
        device_code = 'o[0] = 0.5 * x[0] + 25.0 * div_nr(x[0], 1.0 + x[0] * x[0]) + 8.0 * cos(1.2 * t);'

    class UserUNGMMeas(ssmod.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
        device_code = 'o[0] = 0.05 * (x[0] * x[0]);'

    y = golden('g4_filters')['ungm_y']
    out = []
    for Dyn, Obs in ((ssmod.UNGMTransition, ssmod.UNGMMeasurement), (UserUNGM, UserUNGMMeas)):
        dyn, obs = Dyn(ssmod.GaussRV(1), ssmod.GaussRV(1, cov=np.array([[10.0]]))), Obs(ssmod.GaussRV(1), 1)
        out.append(ssinf.UnscentedKalman(dyn, obs).forward_pass_batch(y))
    assert rel_err(out[1][0], out[0][0]) < 1e-12 and rel_err(out[1][1], out[0][1]) < 1e-12, (rel_err(out[1][0], out[0][0]),
                                                                                             rel_err(out[1][1], out[0][1]))


def test_user_refusals(amd, golden):
    """(d) every unsupported call on a user model raises and leaves its outputs untouched."""
    from ssmtoybox_amd import _lib, ssinf, ssmod
    g = golden('g15_user_models')
    dyn, obs = _system(g, 'vdp')
    alg = ssinf.UnscentedKalman(dyn, obs)
    y = g['vdp_y']
    alg.forward_pass_batch(y)
    fm = alg.fi_mean.copy()
    with pytest.raises(NotImplementedError):
        alg.backward_pass_batch()
    assert alg.sm_mean is None and np.array_equal(alg.fi_mean, fm)
    with pytest.raises(NotImplementedError):
        dyn.simulate_discrete(10, 4)
    with pytest.raises(NotImplementedError):
        ssinf.ExtendedKalman(dyn, obs)
    # the C ABI refuses with SSMQ_E_UNSUPPORTED before touching an output buffer
    lib = _lib.load()
    f_dyn, e_dyn = dyn.device_integrand()
    f_obs, e_obs = obs.device_integrand()
    h_dyn, h_obs = alg.tf_dyn._handle_for(e_dyn), alg.tf_obs._handle_for(e_obs)
    B, T, D, ld = 8, 50, 2, 64
    sentinel = np.full((T * D * D, ld), 7.25)
    bufs = [_lib.DeviceBuffer(sentinel.nbytes) for _ in range(7)]
    for b in bufs:
        b.upload(sentinel)
    d_y, d_m0, d_P0, d_fm, d_fP, d_sm, d_sP = bufs
    d_st = _lib.DeviceBuffer(4 * ld)
    d_st.upload(np.full(ld, 5, dtype=np.int32))
    gqg, pg = _lib.as_c(np.eye(2))
    rr, pr = _lib.as_c(np.eye(1))
    rc = lib.ssmq_filter_smooth_dev(ctypes.c_void_p(h_dyn), ctypes.byref(f_dyn), ctypes.c_void_p(h_obs), ctypes.byref(f_obs), B, ld, T,
                                    ctypes.c_void_p(d_y.ptr), ctypes.c_void_p(d_m0.ptr), ctypes.c_void_p(d_P0.ptr), pg, pr,
                                    ctypes.c_void_p(d_fm.ptr), ctypes.c_void_p(d_fP.ptr), ctypes.c_void_p(d_sm.ptr),
                                    ctypes.c_void_p(d_sP.ptr), ctypes.c_void_p(d_st.ptr))
    assert rc == -3 and 'user-defined integrands' in _lib.last_error()
    _lib.sync()
    for b in (d_fm, d_fP, d_sm, d_sP):
        assert np.array_equal(b.download(sentinel.shape), sentinel)
    assert np.array_equal(d_st.download((ld,), dtype=np.int32), np.full(ld, 5, dtype=np.int32))
    for b in bufs + [d_st]:
        b.free()

    class Big(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 7, 7, True
        device_code = 'for (int i = 0; i < 7; ++i) o[i] = x[i];'

    class BigMeas(ssmod.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
        device_code = 'o[0] = x[0];'

    class NonAdditive(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, False
        device_code = 'o[0] = x[0] + x[2]; o[1] = x[1] + x[3];'

    VdPMeas = type(obs)
    cases = [(Big(ssmod.GaussRV(7), ssmod.GaussRV(7)), BigMeas(ssmod.GaussRV(1), 7), np.zeros((1, 5, 3))),
             (NonAdditive(ssmod.GaussRV(2), ssmod.GaussRV(2)), VdPMeas(ssmod.GaussRV(1), 2), y),
             (dyn, VdPMeas(ssmod.GaussRV(1), 2, state_index=[1]), y)]
    for d, o, data in cases:
        a = ssinf.UnscentedKalman(d, o)
        with pytest.raises(NotImplementedError):
            a.forward_pass_batch(data)
        assert a.fi_mean is None


def test_user_cache_and_compile_errors(amd, golden):
    """(e) a second filter on the same model compiles nothing; a body that does not compile leaves the library working."""
    from ssmtoybox_amd import _lib, ssinf, ssmod
    g = golden('g15_user_models')
    dyn, obs = _system(g, 'vdp')
    y = g['vdp_y']
    fm0, _ = ssinf.UnscentedKalman(dyn, obs).forward_pass_batch(y)
    c0, h0, s0 = _lib.rtc_stats()
    fm1, _ = ssinf.UnscentedKalman(dyn, obs).forward_pass_batch(y)
    c1, h1, s1 = _lib.rtc_stats()
    assert c1 == c0 and h1 > h0 and np.array_equal(fm0, fm1)

    class Broken(ssmod.TransitionModel):
        dim_state, dim_noise, noise_additive = 2, 2, True
        device_code = 'o[0] = no_such_function(x[0]); o[1] = x[1];'

    bad = ssinf.UnscentedKalman(Broken(dyn.init_rv, dyn.noise_rv), obs)
    with pytest.raises(_lib.SsmqError) as e:
        bad.forward_pass_batch(y)
    assert 'no_such_function' in str(e.value)
    fm2, fP2 = ssinf.UnscentedKalman(dyn, obs).forward_pass_batch(y)
    assert np.array_equal(fm2, fm0) and np.all(np.isfinite(fP2))


@pytest.mark.parametrize('name', ['ukf', 'gpqkf'])
def test_mixed_pair_with_builtin_time_table(amd, golden, monkeypatch, name):
    """A built-in transition whose time term comes from a host table (UNGM) next to a user measurement: the run-time route
    uploads the table as the AOT route does, and the pair runs the built-in pair's code - the same bits."""
    from ssmtoybox_amd import ssinf, ssmod
    monkeypatch.setenv('SSMQ_FUSED_QUAD', '0')

    class UserUNGMMeas(ssmod.MeasurementModel):
        dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
        device_code = 'o[0] = 0.05 * (x[0] * x[0]);'          # Fn<SSMQ_F_UNGM_MEAS> restated

    y = np.ascontiguousarray(np.repeat(golden('g4_filters')['ungm_y'], 1250, axis=2))     # (1, 100, 10 000): whole-pass kernel
    par = np.array([[1.0, 3.0]])
    out = []
    for Obs in (ssmod.UNGMMeasurement, UserUNGMMeas):
        dyn, obs = ssmod.UNGMTransition(ssmod.GaussRV(1), ssmod.GaussRV(1, cov=np.array([[10.0]]))), Obs(ssmod.GaussRV(1), 1)
        alg = ssinf.UnscentedKalman(dyn, obs) if name == 'ukf' else ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut')
        kn = alg.kernel_name(y.shape[2])
        fm, fP = alg.forward_pass_batch(y)
        out.append((fm.copy(), fP.copy(), kn))
    assert 'run-time compiled' in out[1][2] and out[0][2].startswith('k_filter_fused<'), (out[0][2], out[1][2])
    assert np.all(np.isfinite(out[1][0]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize('launch_loop', [False, True], ids=['default-routes', 'launch-loop'])
def test_user_and_builtin_filters_share_one_constants_block(amd, golden, monkeypatch, launch_loop):
    """The run-time compiled route and the built-in route keep the pass's constants in ONE cached block per context.  B = 64:
    (a) UNGM GPQ-Kalman, T = 5 (built-in, time table), (b) the Van der Pol user pair, D = 2, its own Q and R, T = 5, (c) the
    built-in pendulum UKF, no time table, T = 3.  Each result from its first call; then a, b, c, a, c, b, a with a changed R in
    the second-to-last call: every repeat with the original arguments is the first call bit for bit (means, covariances,
    status) - a shorter T or smaller D after a larger one leaves nothing stale in sight - and the changed-R call differs and
    repeats itself bit for bit.  Once with the default routes and once with the built-in calls on the captured launch loop
    (SSMQ_NO_FUSED=1), whose graph reads the block."""
    from ssmtoybox_amd import ssinf, ssmod as sm
    from bench import simulate_ungm
    monkeypatch.setenv('SSMQ_NO_PIPED', '1')          # the device-resident entry point, not the pipelined host-array pass
    g = golden('g15_user_models')
    rng = np.random.default_rng(15)
    B = 64
    par = np.array([[1.0, 3.0]])
    ungm = ssinf.GaussianProcessKalman(sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]]))),
                                       sm.UNGMMeasurement(sm.GaussRV(1), 1), par, par, 'rbf', 'ut')
    vdp = _filter('ukf', *_system(g, 'vdp'), 2)
    pend = ssinf.UnscentedKalman(
        sm.Pendulum2DTransition(sm.GaussRV(2, mean=np.array([1.5, 0.0]), cov=0.01 * np.eye(2)), sm.GaussRV(2, cov=0.01 * np.eye(2)), 0.01),
        sm.Pendulum2DMeasurement(sm.GaussRV(1, cov=np.array([[0.1]])), 2))
    assert 'run-time compiled' in vdp.kernel_name(B)
    data = {'a': np.ascontiguousarray(simulate_ungm(B, 5, 15)[1][None]),
            'b': np.tile(g['vdp_y'][:, :5], (1, 1, 8)) + 0.01 * rng.standard_normal((1, 5, B)),
            'c': 1.0 + 0.3 * rng.standard_normal((1, 3, B))}
    algs = {'a': ungm, 'b': vdp, 'c': pend}
    r_b = vdp.r_cov.copy()

    def run(tag, r_cov=None):
        alg = algs[tag]
        if launch_loop and tag != 'b':
            monkeypatch.setenv('SSMQ_NO_FUSED', '1')
            assert alg.kernel_name(B).startswith('hipGraph')
        if r_cov is not None:
            alg.r_cov = r_cov
        try:
            fm, fP = alg.forward_pass_batch(data[tag], raise_on_failure=False)
        finally:
            monkeypatch.delenv('SSMQ_NO_FUSED', raising=False)
            if tag == 'b':
                alg.r_cov = r_b
        assert np.isfinite(fm).all() and np.isfinite(fP).all() and not alg.status.any(), tag
        return fm.copy(), fP.copy(), alg.status.copy()

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y))

    first = {tag: run(tag) for tag in 'abc'}
    assert first['a'][0].shape == (1, 5, B) and first['b'][1].shape == (2, 2, 5, B) and first['c'][0].shape == (2, 3, B)
    for i, tag in enumerate('abcacba'):
        if i == 5:
            changed = run('b', 2.0 * r_b)
            assert not np.array_equal(changed[0], first['b'][0]) and not np.array_equal(changed[1], first['b'][1])
        else:
            assert same(run(tag), first[tag]), (i, tag)
    assert same(run('b', 2.0 * r_b), changed)
    assert same(run('b'), first['b'])
