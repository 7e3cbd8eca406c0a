"""GP quadrature with derivative observations (GPQ+D) without a GPU: the NumPy oracle of tests/_gpqd_oracle.py against the
reference's numbers (tests/golden/g23_gpqd.npz), the oracle's own properties, the refusals and range messages, the run-time
compile checks for gfx950 and the ABI.

The oracle-to-reference bound.  Both are solves with the jittered joint kernel matrix, cond up to 2.6e4 here with weights that are
differences of numbers 1e4 times their size: two routes through it (the reference's float64 cho_solve, the oracle's longdouble
factorisation) differ by far more than an ulp.  Measured on the recording machine, as max |oracle - reference| / max |reference| per
array (the two variances against alpha^2): 2.44e-9 (Wc of 'd2_sr'; wm 7.6e-13, Wcc 5.1e-13, variances 4.1e-13, moments of apply()
2.2e-14).  The bound is 4 times that, as the issue sets it."""
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _gpqd_oracle as go
from tests._cases import rel_err
from tests._gpqd_cases import WEIGHT_CASES, APPLY_MEANS, APPLY_TIME

MEASURED = 2.44e-9
BOUND = 4 * MEASURED


@pytest.fixture(scope='module')
def g23():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_gpqd.npz'))


def weight_distance(w, ref, alpha):
    """Largest of the per-array distances between two weight sets (dicts wm, Wc, Wcc, model_var, integral_var)."""
    d = {k: rel_err(w[k], ref[k]) for k in ('wm', 'Wc', 'Wcc')}
    d['model_var'] = abs(w['model_var'] - ref['model_var']) / alpha ** 2
    d['integral_var'] = abs(w['integral_var'] - ref['integral_var']) / alpha ** 2
    return max(d.values()), d


def fixture_weights(g, tag):
    return dict(wm=g[tag + '_wm'], Wc=g[tag + '_Wc'], Wcc=g[tag + '_Wcc'], model_var=float(g[tag + '_mv']), integral_var=float(g[tag + '_iv']))


@pytest.mark.parametrize('tag', list(WEIGHT_CASES))
def test_oracle_weights_against_the_reference(g23, tag):
    D, _, _, par = WEIGHT_CASES[tag]
    w = go.weights(g23[tag + '_points'], par)
    e, parts = weight_distance(w, fixture_weights(g23, tag), par[0])
    print('{}: oracle against the reference {}'.format(tag, {k: '%.3g' % v for k, v in parts.items()}))
    assert e <= BOUND, parts


def test_oracle_apply_against_the_reference(g23):
    """UNGM dynamics, one output, cov = I, all derivatives: what the reference pins."""
    tag = list(WEIGHT_CASES)[0]
    par = WEIGHT_CASES[tag][3]
    pts = g23[tag + '_points']
    w = go.weights(pts, par)
    f = lambda x, t: orc.integrand(orc.F_UNGM_DYN, x, t, ())              # noqa: E731
    f_dx = lambda x, t: orc.jacobian(orc.F_UNGM_DYN, x, t, ())            # noqa: E731
    worst = 0.0
    for i, m in enumerate(APPLY_MEANS):
        mf, cf, cfx = go.apply(f, f_dx, np.array([m]), np.eye(1), APPLY_TIME, pts, None, w)
        e = max(rel_err(mf, g23['apply_mf'][i]), rel_err(cf, g23['apply_cf'][i]), rel_err(cfx, g23['apply_cfx'][i]))
        worst = max(worst, e)
    print('oracle apply() against the reference: {:.3g}'.format(worst))
    assert worst <= BOUND


def test_oracle_properties():
    pts = orc.points_ut(2)
    par = np.array([1.5, 2.0, 3.0])
    full, none = go.weights(pts, par), go.weights(pts, par, [])
    sub = go.weights(pts, par, [0, 2])
    for w in (full, none, sub):
        assert np.array_equal(w['Wc'], w['Wc'].T)
    assert sub['wm'].shape == (5 + 2 * 2,) and sub['Wcc'].shape == (2, 9)
    plain = orc.gp_weights(par[None], pts)
    e, parts = weight_distance(none, dict(wm=plain['wm'], Wc=plain['Wc'], Wcc=plain['Wcc'], model_var=float(np.ravel(plain['model_var'])[0]),
                                          integral_var=float(np.ravel(plain['integral_var'])[0])), par[0])
    print('which_der=[] against the plain GP quadrature weights: {:.3g}'.format(e))
    assert e <= BOUND, parts
    assert full['integral_var'] <= sub['integral_var'] <= none['integral_var']


def _user_model(D, E):
    from tests import _user_jac_oracle as uo
    if (D, E) == (2, 2):
        return uo.transition('GqPend', 2, uo.PEND_CODE, uo.PEND_JAC, (0.01,))
    code = ' '.join('o[{e}] = sin_nr(x[{a}]) + 0.3*x[{b}]*x[{c}];'.format(e=e, a=e % D, b=(e + 1) % D, c=(e + 2) % D) for e in range(E))
    jac = ' '.join('{{ double sn, cs; sincos_nr(x[{a}], &sn, &cs); J[{e}*ldj + {a}] += cs; J[{e}*ldj + {b}] += 0.3*x[{c}]; '
                   'J[{e}*ldj + {c}] += 0.3*x[{b}]; }}'.format(e=e, a=e % D, b=(e + 1) % D, c=(e + 2) % D) for e in range(E))
    return uo.measurement('GqWide{}x{}'.format(D, E), E, code, jac)


def test_refusals_and_range_messages():
    import ssmtoybox_amd as amd
    from ssmtoybox_amd import ssmod, ssinf
    from ssmtoybox_amd.bq.bqmod import GaussianProcessDerModel
    rv = ssmod.GaussRV
    with pytest.raises(NotImplementedError, match='dim_in <= 6'):
        amd.GaussianProcessDerTransform(7, 1, np.ones((1, 8)))
    with pytest.raises(NotImplementedError, match='2 dim_in \\+ 1'):
        amd.GaussianProcessDerTransform(2, 1, np.ones((1, 3)), point_str='gh')          # 9 points
    with pytest.raises(NotImplementedError, match='outputs'):
        amd.GaussianProcessDerTransform(2, 5, np.ones((1, 3)))
    for bad in ([2, 1], [0, 0], [5], [-1]):
        with pytest.raises(ValueError, match='strictly increasing'):
            GaussianProcessDerModel(2, np.ones((1, 3)), 'ut', which_der=bad)
    m = GaussianProcessDerModel(2, np.ones((1, 3)), 'ut', which_der=[])
    assert m.which_der.size == 0 and GaussianProcessDerModel._supported_kernels_ == ['rbf-d']
    for name in ('optimize', 'predict'):
        with pytest.raises(NotImplementedError, match='GaussianProcessDerModel'):
            getattr(m, name)()
    # the transform's refusals need no weights: an instance without __init__
    tf = amd.GaussianProcessDerTransform.__new__(amd.GaussianProcessDerTransform)
    tf.model = m
    with pytest.raises(NotImplementedError, match='Python callable'):
        tf._device_integrand(lambda x, t: x)
    with pytest.raises(NotImplementedError, match='no Jacobian'):
        tf._device_integrand(ssmod.ReentryVehicle2DTransition().dyn_eval)
    with pytest.raises(NotImplementedError, match='non-additive'):
        tf._device_integrand(ssmod.UNGMNATransition(rv(1), rv(1)).dyn_eval)
    with pytest.raises(NotImplementedError, match='additive'):
        ssinf.GaussianProcessDerKalman(ssmod.UNGMNATransition(rv(1), rv(1)), ssmod.UNGMNAMeasurement(rv(1), 1), np.ones((1, 3)), np.ones((1, 3)))


def test_rtc_compile_check_and_abi():
    from ssmtoybox_amd import _lib
    for name in ('ssmq_transform_create_gpqd', 'ssmq_transform_gpqd_set', 'ssmq_weights_gpqd'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    assert _lib.FORM_GPQD == 6 and _lib.RTC_GPQD == 5
    from ssmtoybox_amd import ssmod
    rv = ssmod.GaussRV
    for (D, E, N), kernel in (((2, 2, 5), 'k_apply_gpqdI'), ((6, 4, 13), 'k_apply_gpqd_ldsI')):
        cls = _user_model(D, E)
        mod = cls(rv(2), rv(2)) if D == 2 else cls(rv(E), D)
        fid = mod.device_integrand()[0].id
        rc, log = _lib.rtc_compile_check(fid, _lib.RTC_GPQD, D, E, N, 0)
        print(log)
        assert rc == 0, log
        assert kernel in log.splitlines()[0]
        assert 'ScratchSize [bytes/lane]: 0' in log, log
    # a shape outside the range
    rc, _ = _lib.rtc_compile_check(fid, _lib.RTC_GPQD, 7, 4, 0, 0)
    assert rc < 0 and 'D <= 6' in _lib.last_error()
