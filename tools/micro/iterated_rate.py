"""Times the iterated posterior linearisation pass (ssmq_filter_iterated_dev) for J = 1, 2, 4 next to the forward pass of the same
handles, in one process, everything on the device: simulate_dev, then warm-up and >= 30 calls of either entry point timed one by
one with events on the library stream, the median reported.

    python tools/micro/iterated_rate.py [--shape ungm|reentry] [--calls 40]

ungm: GPQ Kalman filter, 3 unscented points, B = 1e4, T = 100;  reentry: 5-D reentry vehicle + radar, GPQ, B = 1e5, T = 50.
Prints one JSON line per shape: kernel names, median (minimum) time of the forward pass and of the iterated pass per J, the ratio
to the forward pass, the largest delta of the last step.  Run under a time limit (timeout -k 10 300 python tools/micro/iterated_rate.py)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402


def build(shape):
    if shape == 'ungm':
        dyn = sm.UNGMTransition(sm.GaussRV(1), sm.GaussRV(1, cov=np.array([[10.0]])))
        obs = sm.UNGMMeasurement(sm.GaussRV(1), 1)
        par = np.array([[1.0, 3.0]])
        return ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'), 10000, 100
    m0 = np.array([6500.4, 349.14, -1.8093, -6.7967, 0.6932])
    dyn = sm.ReentryVehicle2DTransition(sm.GaussRV(5, m0, np.diag([1e-6, 1e-6, 1e-6, 1e-6, 1.0])),
                                        sm.GaussRV(3, cov=np.diag([2.4064e-5, 2.4064e-5, 1e-6])))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([1e-6, 0.17e-6])), 5)      # (the benchmark's reentry workload)
    par = np.array([[1.0] + [3.0] * 5])
    return ssinf.GaussianProcessKalman(dyn, obs, par, par, 'rbf', 'ut'), 100000, 50


def timed(fn, calls):
    for _ in range(5):
        fn()
    _lib.sync()
    ms = []
    for _ in range(calls):
        e0, e1 = _lib.Event(), _lib.Event()
        e0.record()
        fn()
        e1.record()
        ms.append(e0.elapsed_ms(e1))
    return float(np.median(ms)), float(min(ms))


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
        d_fm, d_fP = _lib.DeviceBuffer(8 * T * D * ld), _lib.DeviceBuffer(8 * T * D * D * ld)
        d_delta, d_st = _lib.DeviceBuffer(8 * T * ld), _lib.DeviceBuffer(4 * ld)

        def forward():
            alg._launch(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st)

        rec = {'shape': shape, 'D': D, 'Y': Y, 'B': B, 'T': T, 'calls': a.calls, 'filter_kernel': alg.kernel_name(B),
               'iterated_kernel': alg.iterated_kernel_name(1, B)}
        rec['forward_ms_median'], rec['forward_ms_min'] = (round(v, 4) for v in timed(forward, a.calls))
        for J in (1, 2, 4):
            def iterated():
                alg._launch_iterated(lib, B, ld, T, J, 0, d_y, d_m0, d_P0, d_fm, d_fP, d_delta, d_st)
            med, low = timed(iterated, a.calls)
            ok = d_st.download((ld,), dtype=np.int32)[:B] == 0
            rec['J{}'.format(J)] = {'ms_median': round(med, 4), 'ms_min': round(low, 4), 'ratio_to_forward': round(med / rec['forward_ms_median'], 3),
                                    'failed_trajectories': int(B - np.count_nonzero(ok)),
                                    'delta_last_step_max': float(np.max(d_delta.download((T, ld))[T - 1, :B][ok]))}
        print(json.dumps(rec), flush=True)
        for buf in (d_x, d_y, d_fm, d_fP, d_st, d_delta):
            buf.free()
        stage.free()


if __name__ == '__main__':
    main()
