"""The cases of the IMM tests, built without a device on the models, measurements and rows of tests/_noise_sweep_cases.py (its seed: the
oracle's status is 0 everywhere on these four, tests/test_imm_host.py checks it) - the smallest shapes at which each thing can go wrong:

    ungm_ukf   sigma-point, D = Y = 1, N = 3, M = 2, B = 70 (a full and a partial 64-lane workgroup), T = 6: Q per mode, mu0 not uniform
    pend_ckf   sigma-point, D = 2, Y = 1, N = 4, M = 3 (no power of two), B = 5, T = 4: an R stack alone
    cv_gp      BQ, D = 4, Y = 2, N = 9, M = 2, B = 5, T = 4: full-matrix Q rows and a P0 stack
    ct_tp      t-process, D = 5, Y = 4, N = 11, SELO = 1, M = 4, B = 5, T = 4: Q scale rows"""
import numpy as np

from tests import _imm_oracle as imo
from tests import _noise_sweep_cases as nc

NAMES = nc.NAMES
MODES = {'ungm_ukf': 2, 'pend_ckf': 3, 'cv_gp': 2, 'ct_tp': 4}
STAY = 0.9
# the failure cases of ungm_ukf: a NaN measurement of trajectory FAIL_LANE at step FAIL_STEP; mode FAIL_MODE's measurement-noise variance
# replaced by FAIL_R (indefinite: the innovation variance of a trajectory whose predicted measurement variance is below 10 is not positive)
FAIL_STEP, FAIL_LANE = 2, 5
FAIL_MODE, FAIL_R = 1, -10.0


def case(name):
    """The noise-sweep case with the IMM's modes: M, pi, mu0, the arguments q_cov / r_cov / x0_cov of imm_pass_batch (None or (M, n, n)
    stacks) and the oracle's rows q_rows / r_rows / x0_rows (M, n, n).  Built once, never modified."""
    from ssmtoybox_amd import ssinf
    c = dict(nc.case(name))
    M = MODES[name]
    if name == 'ungm_ukf':
        q, r, x0 = c['q_cov'][[1, 3]], None, None
    elif name == 'pend_ckf':
        q, r, x0 = None, c['r_cov'], None
    elif name == 'cv_gp':
        q, r, x0 = c['q_cov'][:2], None, c['x0_cov'][:2]
    else:
        q, r, x0 = ssinf.noise_grid(c['Q'], [0.3, 1.0, 5.0, 20.0]), None, None
    c.update(M=M, q_cov=q, r_cov=r, x0_cov=x0, pi=ssinf.mode_transition(M, STAY), mu0=np.array([0.7, 0.3]) if name == 'ungm_ukf' else np.full(M, 1.0 / M))
    c['q_rows'], c['r_rows'], c['x0_rows'] = (np.broadcast_to(own, (M,) + own.shape) if a is None else a
                                              for a, own in ((q, c['Q']), (r, c['R']), (x0, c['P0'])))
    return c


_CASES, _REFS = {}, {}


def get(name):
    if name not in _CASES:
        _CASES[name] = case(name)
    return _CASES[name]


def oracle(c, y=None, weights=None, dtype=np.float64, pi=None, mu0=None, r_rows=None):
    return imo.imm(c, c['y'] if y is None else y, c['q_rows'], c['r_rows'] if r_rows is None else r_rows, c['x0_rows'],
                   c['pi'] if pi is None else pi, c['mu0'] if mu0 is None else mu0, weights=weights, dtype=dtype)


def reference(name, dtype=np.float64):
    """The oracle's IMM pass of the case on its own weights (float64, or the long-double twin), computed once."""
    key = (name, np.dtype(dtype).name)
    if key not in _REFS:
        _REFS[key] = oracle(get(name), dtype=dtype)
    return _REFS[key]


def failing_r(c):
    """The r rows of ungm_ukf with the planted mode: a negative measurement-noise variance."""
    r = np.array(c['r_rows'], dtype=float)
    r[FAIL_MODE] = FAIL_R
    return r


def args(c):
    return dict(pi=c['pi'], mu0=c['mu0'], q_cov=c['q_cov'], r_cov=c['r_cov'], x0_cov=c['x0_cov'])


# The float64 oracle against its long-double twin (tests/_imm_oracle.py), max |difference| / max(1, |value|) per case, measured on the
# CPU by tests/test_imm_host.py::test_oracle_against_its_long_double_twin, which asserts that the figures below still hold (each is the
# measured value rounded up to two digits).  The device gets MARGIN times the figure: another summation order, FMA contraction, div_nr.
TWIN = {'ungm_ukf': dict(mean=9.1e-14, cov=4.3e-13, mode_prob=6.4e-15), 'pend_ckf': dict(mean=4.5e-16, cov=2.0e-17, mode_prob=2.8e-16),
        'cv_gp': dict(mean=6.4e-15, cov=7.1e-13, mode_prob=9.7e-14), 'ct_tp': dict(mean=1.5e-13, cov=6.7e-12, mode_prob=1.1e-12)}
MARGIN = 64.0
