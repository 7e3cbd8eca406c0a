"""The filter entry points of ssinf.py hand every device buffer back, whichever way they are left: `_lib.scratch` and
`_lib.DeviceBuffer` are wrapped with a recorder, and after the call every recorded buffer has `ptr is None` - except, for a `*_dev`
call that succeeds, exactly the buffers it returns (and the two planes the particle filter keeps).

UNGM + UnscentedKalman, B = 130 (pitch 192: a partial last wave and padding lanes), T = 3.  SSMQ_NO_PIPED=1 throughout: on this pair
`forward_pass_batch` would otherwise take the pipelined route, which stages nothing on this side and hands a per-trajectory x0_mean
to the library as it is - the staged route is the one under test.  Every failure here is a host-side exception or an ordinary return
code of the library; nothing runs on the device after it.

The pair of the library refusal: a GP-quadrature Kalman filter on UNGM with 4 Gauss-Hermite points.  Its transforms are
GaussianProcessTransforms, which the Python refusals of the iterated smoother let through, and the dispatch table of k_ipls_pass<> has
UNGM with 2, 3 and 5 points (csrc/ssmq_filter_shapes.h): the library answers SSMQ_E_UNSUPPORTED (-3)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B, T = 130, 3


@pytest.fixture(scope='module')
def amd():
    import ssmtoybox_amd
    if ssmtoybox_amd.device_count() < 1:
        pytest.fail('no device: the GPU tests need an MI355X')
    ssmtoybox_amd.set_device(0)
    return ssmtoybox_amd


@pytest.fixture(scope='module')
def case(amd):
    """The filters, the measurements (1, T, B) and their planes on the device: made once, before any recorder, never modified."""
    from ssmtoybox_amd import _lib, ssinf, ssmod as sm
    dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
    obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
    par = np.array([[1.0, 3.0]])
    cv = sm.ConstantVelocity(sm.GaussRV(4, np.array([100.0, 5.0, 200.0, -3.0]), np.diag([1.0, 0.1, 1.0, 0.1])), sm.GaussRV(2, cov=0.1 * np.eye(2)))
    dyn_s = sm.UNGMTransition(sm.StudentRV(1, dof=4.0), sm.StudentRV(1, dof=4.0))
    c = dict(ukf=ssinf.UnscentedKalman(dyn, obs), ckf=ssinf.CubatureKalman(dyn, obs),
             student=ssinf.FullySymmetricStudent(dyn_s, sm.UNGMMeasurement(sm.StudentRV(1, dof=4.0), 1)),
             gh4=ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'gh', {'degree': 4}),
             radar=ssinf.UnscentedKalman(cv, sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.5, 1e-4])), 4)),
             pf=ssinf.BootstrapParticleFilter(dyn, obs, num_particles=64, seed=3))
    c['y'] = np.random.default_rng(11).standard_normal((1, T, B))
    c['ld'] = _lib.padded(B)
    assert c['ld'] == 192
    c['d_y'] = _lib.DeviceBuffer(8 * T * c['ld'])
    _lib.upload_study(c['y'], 1, c['ld'], c['d_y'])
    yield c
    c['d_y'].free()
    c['pf'].free_dev()


@pytest.fixture
def made(case, monkeypatch):
    """Every buffer `_lib.scratch` and `_lib.DeviceBuffer` hand out during the test, in order (a scratch block that the pool could not
    serve is there twice: it is a DeviceBuffer underneath)."""
    from ssmtoybox_amd import _lib
    made, scratch, Buffer = [], _lib.scratch, _lib.DeviceBuffer

    def recording_scratch(nbytes):
        made.append(scratch(nbytes))
        return made[-1]

    class RecordingBuffer(Buffer):
        def __init__(self, nbytes):
            Buffer.__init__(self, nbytes)
            made.append(self)

    monkeypatch.setattr(_lib, 'scratch', recording_scratch)
    monkeypatch.setattr(_lib, 'DeviceBuffer', RecordingBuffer)
    monkeypatch.setenv('SSMQ_NO_PIPED', '1')
    return made


def all_returned(made):
    return bool(made) and all(b.ptr is None for b in made)


BATCH_CALLS = {
    'forward_pass_batch': lambda a, y, **kw: a.forward_pass_batch(y, raise_on_failure=False, **kw),
    'innovations_batch': lambda a, y, **kw: a.innovations_batch(y, return_moments=True, **kw),
    'innovations_batch(fi_mean)': lambda a, y, **kw: a.innovations_batch(y, fi_mean=np.zeros((1, T, B)), fi_cov=np.ones((1, 1, T, B)), **kw),
    'iterated_pass_batch': lambda a, y, **kw: a.iterated_pass_batch(y, 2, raise_on_failure=False, **kw),
    'iterated_smoother_batch': lambda a, y, **kw: a.iterated_smoother_batch(y, 2, raise_on_failure=False, **kw),
}


@pytest.mark.parametrize('name', sorted(BATCH_CALLS))
def test_wrong_x0_mean_shape(case, made, name):
    """x0_mean (B + 1, D): a NumPy broadcasting error, raised after the measurement planes were allocated."""
    with pytest.raises(ValueError):
        BATCH_CALLS[name](case['ukf'], case['y'], x0_mean=np.zeros((B + 1, 1)))
    assert all_returned(made), [b.ptr for b in made]


def test_wrong_lin_mean_shape(case, made):
    with pytest.raises(ValueError, match='lin_mean'):
        case['ukf'].iterated_smoother_batch(case['y'], 2, lin_mean=np.zeros((1, T, B)), lin_cov=np.ones((1, 1, T, B)))
    assert all_returned(made), [b.ptr for b in made]


def test_library_refusal(case, made):
    """SSMQ_E_UNSUPPORTED from `ssmq_smoother_iterated_dev` (see the module docstring for the pair): NotImplementedError, nothing held -
    the batch call's planes and the eight output buffers of the `_dev` call."""
    alg = case['gh4']
    assert alg.tf_dyn._num_points() == 4
    with pytest.raises(NotImplementedError, match='smoother_iterated'):
        alg.iterated_smoother_batch(case['y'], 2)
    assert all_returned(made), [b.ptr for b in made]
    del made[:]
    with pytest.raises(NotImplementedError, match='smoother_iterated'):
        alg.iterated_smoother_dev(case['d_y'], B, case['ld'], T, 2)
    assert len(made) >= 10 and all_returned(made), [b.ptr for b in made]


def test_run_filters_mismatch(case, made):
    from ssmtoybox_amd import ssinf
    with pytest.raises(ValueError, match='same measurements'):       # the second filter takes dim_out = 2: before any allocation
        ssinf.run_filters([case['ukf'], case['radar']], case['y'])
    assert made == []
    with pytest.raises(ValueError):
        ssinf.run_filters([case['ukf'], case['ckf']], case['y'], x0_mean=np.zeros((B + 1, 1)))
    assert all_returned(made), [b.ptr for b in made]


@pytest.mark.parametrize('name', sorted(BATCH_CALLS))
def test_straight_path_batch(case, made, name):
    BATCH_CALLS[name](case['ukf'], case['y'])
    assert all_returned(made), [b.ptr for b in made]


def test_straight_path_other_entry_points(case, made):
    """`run_filters` over a Gaussian and a Studentian filter, the smoother, the Studentian and the particle filter's batch calls."""
    from ssmtoybox_amd import ssinf
    ssinf.run_filters([case['ukf'], case['student']], case['y'], raise_on_failure=False)
    case['ukf'].forward_pass_batch(case['y'], raise_on_failure=False, smooth=True)
    case['student'].forward_pass_batch(case['y'], raise_on_failure=False)
    case['pf'].forward_pass_batch(case['y'], raise_on_failure=False, return_particles=True)
    assert all_returned(made), [b.ptr for b in made]


def test_straight_path_dev(case, made):
    """A `*_dev` call that succeeds leaves exactly the buffers it returns alive; the particle filter's, those and the two it owns."""
    ukf, pf, d_y, ld = case['ukf'], case['pf'], case['d_y'], case['ld']

    def alive():
        return sorted(id(b) for b in made if b.ptr is not None)

    def check(out, extra=()):
        assert len(out) == len(set(id(b) for b in out)) and all(b.ptr for b in out)
        assert alive() == sorted(id(b) for b in tuple(out) + tuple(extra))
        for b in out:
            b.free()
        del made[:]

    fwd = ukf.forward_pass_dev(d_y, B, ld, T)
    assert len(fwd) == 3 and alive() == sorted(id(b) for b in fwd)
    del made[:]
    check(ukf.innovations_dev(d_y, fwd[0], fwd[1], B, ld, T))
    for b in fwd:
        b.free()
    out = ukf.iterated_pass_dev(d_y, B, ld, T, 2)
    assert len(out) == 4
    check(out)
    out = ukf.iterated_smoother_dev(d_y, B, ld, T, 2)
    assert len(out) == 8
    check(out)
    out = pf.forward_pass_dev(d_y, B, ld, T)
    assert len(out) == 3
    check(out, (pf.d_loglik, pf.d_ess))
    pf.free_dev()
