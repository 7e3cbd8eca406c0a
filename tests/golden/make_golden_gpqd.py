"""
Generate tests/golden/g23_gpqd.npz by running the REFERENCE's GP quadrature with derivative observations
(research/gpqd/gpqd_base.py: GaussianProcessDerModel.bq_weights and GaussianProcessDerTransform.apply); see make_golden.py for how
the reference is reached and for the shims.

What the reference pins: all derivatives (which_der=None), one output, cov = I.  Stored per weight case `tag`
(tests/_gpqd_cases.py: WEIGHT_CASES): the points, wm, Wc, Wcc, model_var, integral_var; and for UNGM dynamics with the first case's
model, cov = I and three means including 0: mean_f, cov_f and the (E, D) cov_fx of apply().

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_gpqd.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import make_golden as mg  # noqa: E402  (installs the shims, puts the reference on the path)
from tests._gpqd_cases import WEIGHT_CASES, APPLY_MEANS, APPLY_TIME  # noqa: E402

sys.path.insert(0, os.path.join(mg.REF, 'research', 'gpqd'))
from gpqd_base import GaussianProcessDerModel, GaussianProcessDerTransform  # noqa: E402
from ssmtoybox.utils import GaussRV  # noqa: E402
from ssmtoybox import ssmod  # noqa: E402


def main():
    out = {'names': np.array(list(WEIGHT_CASES))}
    for tag, (D, pts, ppar, par) in WEIGHT_CASES.items():
        model = GaussianProcessDerModel(D, np.array([par]), pts, ppar)
        wm, Wc, Wcc, mv, iv = model.bq_weights(np.array([par]))
        out.update({tag + '_points': model.points, tag + '_par': np.array(par), tag + '_wm': wm, tag + '_Wc': Wc, tag + '_Wcc': Wcc,
                    tag + '_mv': np.array(mv), tag + '_iv': np.array(iv)})
        print(tag, 'M =', wm.shape[0], 'cond(K + jitter I) = %.3g' % np.linalg.cond(np.linalg.inv(model.iK)))
    tag = list(WEIGHT_CASES)[0]
    D, pts, ppar, par = WEIGHT_CASES[tag]
    dyn = ssmod.UNGMTransition(GaussRV(1), GaussRV(1, cov=np.array([[10.0]])))
    g = lambda x, t, dx=False: np.atleast_1d(dyn.dyn_eval(x, float(np.asarray(t).reshape(-1)[0]), dx=dx))      # noqa: E731
    tf = GaussianProcessDerTransform(D, 1, np.array([par]), pts, ppar)
    res = [tf.apply(g, np.array([m]), np.eye(1), np.atleast_1d(APPLY_TIME)) for m in APPLY_MEANS]
    out['apply_mf'] = np.array([np.atleast_1d(r[0]) for r in res])
    out['apply_cf'] = np.array([np.atleast_2d(r[1]) for r in res])
    out['apply_cfx'] = np.array([np.atleast_2d(r[2]) for r in res])
    mg.save('g23_gpqd', **out)


if __name__ == '__main__':
    main()
