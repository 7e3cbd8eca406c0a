"""Times the iterated posterior linearisation smoother (ssmq_smoother_iterated_dev) for J = 1, 2, 4 next to the existing smoother
(ssmq_filter_smooth_dev: forward pass + RTS) and the iterated pass at J = 1 (k_iplf_loop<>: what the forward sweep alone costs) of the
same handles, in one process, everything on the device: simulate_dev, then warm-up and >= 30 calls of every entry point timed one by
one with events on the library stream, the median reported.  Both smoothers are synchronous and allocate their workspace per call;
the events include that.

    python tools/micro/ipls_rate.py [--shape ungm|reentry] [--calls 40]

ungm: GPQ Kalman filter, 3 unscented points, B = 1e4, T = 100;  reentry: 5-D reentry vehicle + radar, GPQ, B = 1e5, T = 50 (the shapes of
tools/micro/iterated_rate.py; on the device simulator's reentry data the plain filter itself fails in > 99 % of the trajectories within
7 steps, and a failed trajectory leaves the sweeps early: `failed_trajectories` is part of the record).
Prints one JSON line per shape.  Run under a time limit (timeout -k 10 300 python tools/micro/ipls_rate.py)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssmtoybox_amd import _lib, ssmod as sm  # noqa: E402
from tools.micro.iterated_rate import build, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='both', choices=('ungm', 'reentry', 'both'))
    ap.add_argument('--calls', type=int, default=40)
    a = ap.parse_args()
    lib = _lib.load()
    for shape in (('ungm', 'reentry') if a.shape == 'both' else (a.shape,)):
        alg, B, T = build(shape)
        D, Y = alg.mod_dyn.dim_state, alg.mod_obs.dim_out
        d_x, d_y, ld = sm.simulate_dev(alg.mod_dyn, alg.mod_obs, T, B, seed=1)
        stage = _lib.Staging()
        d_m0, d_P0 = alg._initial_planes(stage, B, ld)
        outs = alg._ipls_outputs(_lib.DeviceBuffer, D, T, ld)
        d_tdelta = _lib.DeviceBuffer(8 * T * ld)

        def rts():
            alg._launch_smooth(lib, B, ld, T, d_y, d_m0, d_P0, outs[0], outs[1], outs[2], outs[3], outs[7])

        def iplf():
            alg._launch_iterated(lib, B, ld, T, 1, 0, d_y, d_m0, d_P0, outs[0], outs[1], d_tdelta, outs[7])

        rec = {'shape': shape, 'D': D, 'Y': Y, 'B': B, 'T': T, 'calls': a.calls, 'kernel': alg.iterated_smoother_kernel_name(1)}
        rec['smooth_dev_ms_median'], rec['smooth_dev_ms_min'] = (round(v, 4) for v in timed(rts, a.calls))
        rec['iterated_pass_J1_ms_median'], rec['iterated_pass_J1_ms_min'] = (round(v, 4) for v in timed(iplf, a.calls))
        for J in (1, 2, 4):
            def ipls():
                alg._launch_ipls(lib, B, ld, T, J, d_y, d_m0, d_P0, None, None, outs)
            med, low = timed(ipls, a.calls)
            ok = outs[7].download((ld,), dtype=np.int32)[:B] == 0
            rec['J{}'.format(J)] = {'ms_median': round(med, 4), 'ms_min': round(low, 4), 'ratio_to_smooth_dev': round(med / rec['smooth_dev_ms_median'], 3),
                                    'failed_trajectories': int(B - np.count_nonzero(ok)),
                                    'delta_median': float(np.median(outs[6].download((ld,))[:B][ok]))}
        print(json.dumps(rec), flush=True)
        for buf in [d_x, d_y, d_tdelta] + outs:
            buf.free()
        stage.free()


if __name__ == '__main__':
    main()
