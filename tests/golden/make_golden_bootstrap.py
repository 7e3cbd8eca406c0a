"""
Golden values for the bootstrap variance: the reference's bootstrap_var (utils.py:223-244) run once per input at a recorded
NumPy seed.  Reuses the import shims of make_golden.py (importing that module installs them and loads the reference).

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_bootstrap.py  -> tests/golden/g20_bootstrap.npz

normal_data: 4096 standard normals of default_rng(20); the skewed input is their squares (not stored twice).
`normal_var`, `skewed_var`: np.random.seed(0); bootstrap_var(data, 4096).  The reference's value is itself a sample variance of S = 4096 near-normal means around
var(data) / n, so it lies within 5 sqrt(2 / (S - 1)) relative of that figure - asserted here; the device's value is held
to the same band, and to sqrt(2) times the band against the reference's (tests/test_bootstrap_gpu.py).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_golden as mg  # noqa: E402,F401  (installs the shims, imports the reference)
from ssmtoybox.utils import bootstrap_var  # noqa: E402

N, SAMPLES, SEED = 4096, 4096, 0


def main():
    normal = np.random.default_rng(20).standard_normal(N)
    out = {'samples': np.asarray(SAMPLES), 'seed': np.asarray(SEED)}
    for name, data in (('normal', normal), ('skewed', normal ** 2)):
        np.random.seed(SEED)
        var = float(bootstrap_var(data[None, :], SAMPLES))
        theory = np.var(data) / N
        band = 5.0 * np.sqrt(2.0 / (SAMPLES - 1))
        print('  {:7s} bootstrap_var {:.6e}  var(data)/n {:.6e}  ratio - 1 = {:+.4f}  (band {:.4f})'.format(
            name, var, theory, var / theory - 1.0, band))
        assert abs(var / theory - 1.0) <= band
        out[name + '_var'] = np.asarray(var)
    out['normal_data'] = normal
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g20_bootstrap.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
