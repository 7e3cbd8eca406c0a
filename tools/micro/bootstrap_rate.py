"""Times the streaming bootstrap (ssmq_bootstrap_var_dev: k_bootstrap_sums + k_boot_means, synchronous, the download of the
S means and the host-side variance included) and reports draws per second: a record, not a gate.

    python tools/micro/bootstrap_rate.py [--samples 10000] [--blocks 5] [--calls 3] [--out FILE]

Shapes: n = 1e4, 1e5, 1e6 included entries, S resamples, R = 1 and 4 rows, on the default route and with SSMQ_BOOT_NO_LDS=1
(the same route as the default where R n does not fit the LDS of a CU; the two are timed alternately).  Per shape: one warm-up
call, then `blocks` blocks of `calls` calls each, wall time around the synchronous call; the median over the blocks of the
per-call time is reported, with the spread.  A draw is one index and the R values it gathers: draws = n S.
Last, the reference's NumPy formula (utils.py:223-244: np.random.choice(data, (S, n)), mean, var) on the host at n = S = 1e4.
One JSON line per measurement.  Run under a time limit of its own (timeout -k 10 600 python tools/micro/bootstrap_rate.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import ssmtoybox_amd as amd  # noqa: E402
from ssmtoybox_amd import _lib, mcshard  # noqa: E402


def timed_blocks(fn, blocks, calls):
    per_call = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        per_call.append((time.perf_counter() - t0) / calls)
    return per_call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=10000)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert amd.device_count() >= 1, 'needs a GPU: there is no CPU fallback'
    out = open(a.out, 'w') if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    rng = np.random.default_rng(0)
    S = a.samples
    for n in (10 ** 4, 10 ** 5, 10 ** 6):
        ld = (n + 63) // 64 * 64
        for R in (1, 4):
            host = np.zeros((R, ld))
            host[:, :n] = rng.standard_normal((R, n))
            d = _lib.DeviceBuffer(host.nbytes)
            d.upload(host)
            fits = 8 * R * n + 8 * 8 * (1 if R == 1 else 4) <= 160 * 1024 - 64
            results = {}
            for route in ('default', 'no_lds'):
                if route == 'no_lds':
                    os.environ['SSMQ_BOOT_NO_LDS'] = '1'
                else:
                    os.environ.pop('SSMQ_BOOT_NO_LDS', None)
                fn = lambda: mcshard.bootstrap_var_dev(d, ld, R, n, samples=S, seed=1)       # noqa: E731
                results[route] = fn()                                                      # warm-up
                t = timed_blocks(fn, a.blocks, a.calls)
                med = float(np.median(t))
                emit({'what': 'ssmq_bootstrap_var_dev', 'n': n, 'S': S, 'R': R, 'route': route,
                      'values_in_lds': bool(fits and route == 'default'), 'blocks': a.blocks, 'calls_per_block': a.calls,
                      'median_ms': round(med * 1e3, 3), 'min_ms': round(min(t) * 1e3, 3), 'max_ms': round(max(t) * 1e3, 3),
                      'draws_per_s': round(n * S / med, 1), 'gathered_values_per_s': round(n * S * R / med, 1)})
            os.environ.pop('SSMQ_BOOT_NO_LDS', None)
            assert np.array_equal(results['default'], results['no_lds']), 'the two routes disagree'
            d.free()
    # the reference's formula on the host
    n = S = 10 ** 4
    data = rng.standard_normal(n)

    def ref():
        return np.var(np.mean(np.random.choice(data, (S, n)), 1))
    ref()
    t = timed_blocks(ref, a.blocks, 1)
    med = float(np.median(t))
    emit({'what': 'numpy reference formula (host)', 'n': n, 'S': S, 'R': 1, 'median_ms': round(med * 1e3, 1),
          'min_ms': round(min(t) * 1e3, 1), 'max_ms': round(max(t) * 1e3, 1), 'draws_per_s': round(n * S / med, 1)})
    if out:
        out.close()


if __name__ == '__main__':
    main()
