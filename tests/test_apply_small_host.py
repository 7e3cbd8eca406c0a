"""Host half of the k_apply_small pinning (tests/_apply_small_oracle.py): the table reader, the 50-digit integrands against the float64
ones, the measurement of K_REF - the worst ratio of the plain float64 NumPy restatement of the reference against the oracle, in units
of eps (A + S) - and the sanity of the scales.  The device half (tests/test_apply_small_gpu.py) holds every kernel to
K = max(16, 8 K_REF) on the same cases."""
import re

import mpmath as mp
import numpy as np
import pytest

from oracle import ssmq_oracle as orc
from tests import _apply_small_oracle as ao

ROWS = ao.table_rows()


def test_table_reader():
    assert len(ROWS) == ao.EXPECTED_ROWS == 168
    names = [r.name for r in ROWS]
    assert len(set(names)) == len(names)
    pat = re.compile(r'^k_apply_small<D=\d+,E=\d+,N=\d+,SSMQ_F_\w+,SSMQ_FORM_(BQ|SIGMA),TP=[01],SEL=[01],OPT=[01237]>$')
    assert all(pat.match(n) for n in names)
    shapes = {(r.F, r.D, r.E, r.N, r.sel) for r in ROWS}
    fast = {(r.F, r.D, r.E, r.N, r.sel) for r in ROWS if r.fast}
    assert len(shapes) == 46 and len(fast) == 6
    for s in shapes:
        got = sorted((r.form, r.tp, r.opt) for r in ROWS if (r.F, r.D, r.E, r.N, r.sel) == s)
        want = [(0, 0, 0), (0, 1, 0), (1, 0, 0)] + ([(0, 0, 1), (0, 0, 3), (0, 0, 7), (0, 1, 2), (1, 0, 2)] if s in fast else [])
        assert got == sorted(want), s
    for r in ROWS:                                 # every row has a model, an operating point, and a shape the model fits
        fid, _, g0, _, _ = ao.MODELS[r.F]
        assert (r.D, r.sel) in g0 and len(g0[(r.D, r.sel)]) == r.D
        idx = ao.state_index(r)
        assert max(idx if idx is not None else range(ao.DIN[fid])) < r.D


def test_rules_have_the_shape_their_kernel_needs():
    """What can be said of a rule without the device: unscented-type points exactly where the kernel wants them, a refused LDL' for the
    dense kernel of a fast-path shape, an accepted one for the LDL' kernels, bit-exact reflection symmetry for OPT = 7."""
    for r in ROWS:
        rule = ao.rule_for(r)
        D, N = r.D, r.N
        ut = N == 2 * D + 1 and np.array_equal(rule['xi'], ao.unscented_points(D, rule['xi'][0, 1] if N > 1 else 0.0)) and rule['xi'][0, 1] > 0
        assert ut == (r.opt in (7, 3, 2)), r.name
        assert np.all(np.isfinite(rule['wm'])) and np.all(rule['wm'] != 0.0), r.name
        if r.form == ao.FORM_SIGMA:
            assert rule['Wc'].shape == (N,) and rule['Wcc'] is None
            continue
        assert np.array_equal(rule['Wc'], rule['Wc'].T), r.name
        if r.opt in (7, 3, 1):
            assert ao._ldl_accepts(rule['Wc']), r.name
        if r.fast and r.opt == 0 and not r.tp:
            assert rule['Wc'][0, 0] == 0.0, r.name
        if r.tp:
            assert np.array_equal(rule['iK'], rule['iK'].T) and np.linalg.eigvalsh(rule['iK'])[0] > 0.0, r.name
        if r.opt == 7:
            W, q = rule['Wc'], [0] + list(range(1 + D, N)) + list(range(1, 1 + D))          # swap of every point pair
            assert np.array_equal(W, W[np.ix_(q, q)]) and np.array_equal(rule['wm'], rule['wm'][q]), r.name
            assert np.array_equal(rule['Wcc'], -rule['Wcc'][:, q]), r.name
        if r.opt == 3:
            W, q = rule['Wc'], [0] + list(range(1 + D, N)) + list(range(1, 1 + D))
            assert not np.allclose(W, W[np.ix_(q, q)], rtol=1e-6, atol=0.0), r.name


@pytest.mark.parametrize('F', sorted(ao.MODELS))
def test_hp_integrands_against_float64(F):
    """The 50-digit integrands agree with oracle.ssmq_oracle.integrand to a few ulp at the probes' own sigma points: 4 eps of the terms of
    f plus its first-order sensitivity to one rounding of each input (the float64 evaluation rounds its arguments' derived quantities)."""
    fid, p = ao.MODELS[F][:2]
    worst = 0.0
    for r in (r for r in ROWS if r.F == F and r.form == ao.FORM_BQ and r.tp == 0 and r.opt == 0):
        mean, cov, time = ao.probes_for(r.F, r.D, r.sel)
        sidx, xi = ao.state_index(r), ao.rule_for(r)['xi']
        idx = list(range(ao.DIN[fid])) if sidx is None else list(sidx)
        for k in range(ao.N_PROBES):
            if k == ao.BAD_PROBE:
                continue
            x = mean[k][:, None] + np.linalg.cholesky(cov[k]).dot(xi)
            for n in range(r.N):
                xs = x[idx, n]
                want = orc.integrand(fid, xs, time[k], p)
                with mp.workdps(ao.DPS):
                    xh, th = [mp.mpf(float(v)) for v in xs], mp.mpf(float(time[k]))
                    f, T = ao.integrand_hp(fid, xh, th, p)
                    J, Jt = ao._jacobian_hp(fid, xh, th, p)
                    f, T = np.array([float(v) for v in f]), np.array([float(v) for v in T])
                bar = ao.EPS * (T + J.dot(np.abs(xs)) + Jt * abs(time[k]))
                assert want.shape == f.shape
                q = float(np.max(np.where(want == f, 0.0, np.abs(want - f) / bar)))
                worst = max(worst, q)
    print('%s: worst |float64 - hp| / (eps (T + |J||x|)) = %.3g' % (F, worst))
    assert worst < 4.0, (F, worst)


@pytest.fixture(scope='module')
def f64_ratios():
    """(row, probe) -> ratios of the float64 restatement against the oracle, in units of eps (A + S)."""
    out = {}
    for r in ROWS:
        fid, p, sidx = ao.model_of(r)
        rule, ref = ao.rule_for(r), ao.reference(r)
        mean, cov, time = ao.probes_for(r.F, r.D, r.sel)
        for k in range(ao.N_PROBES):
            if ref[k] is not None:
                out[(r, k)] = ao.ratios(ao.transform_f64(fid, p, sidx, r.form, rule, mean[k], cov[k], time[k]), ref[k])
    return out


def test_float64_restatement_within_k_ref(f64_ratios):
    """K_REF: the worst ratio over all cases, per model and form; the constant in the oracle module is that measurement."""
    worst, by_model, by_form = (0.0, None), {}, {}
    for (r, k), q in f64_ratios.items():
        m = max(q)
        by_model[r.F] = max(by_model.get(r.F, 0.0), m)
        by_form[ao.form_tag(r)] = tuple(max(a, b) for a, b in zip(by_form.get(ao.form_tag(r), (0.0,) * 3), q))
        if m > worst[0]:
            worst = (m, (r.name, k, q))
    for F in sorted(by_model):
        print('K_ref %-28s %.3g' % (F, by_model[F]))
    for t in sorted(by_form):
        print('K_ref %-6s mean %.3g cov %.3g cross %.3g' % ((t,) + by_form[t]))
    print('K_ref worst', worst)
    assert max(by_model.values()) < 50.0, by_model          # (above that the scale S would be missing a term)
    assert worst[0] <= ao.K_REF, worst
    assert ao.K == max(16.0, 8.0 * ao.K_REF)


def test_scales_and_failures():
    """A + S is positive and finite for every entry of every case; the non-PD probe is the only one reported as failed."""
    for r in ROWS:
        ref = ao.reference(r)
        assert [k for k in range(ao.N_PROBES) if ref[k] is None] == [ao.BAD_PROBE], r.name
        for k in range(ao.N_PROBES):
            if ref[k] is None:
                continue
            for v, s in zip(ref[k][:3], ref[k][3:]):
                assert v.shape == s.shape and np.all(np.isfinite(v)) and np.all(np.isfinite(s)) and np.all(s > 0.0), (r.name, k)
            assert ref[k][0].shape == (r.E,) and ref[k][1].shape == (r.E, r.E) and ref[k][2].shape == (r.E, r.D)
        _, cov, time = ao.probes_for(r.F, r.D, r.sel)
        assert len(set(time.tolist())) == ao.N_PROBES
        assert [ao.lane_probe(b) for b in (0, 9, 10, 129, 130)] == [0, 9, 0, 9, 9]
