"""Times the outlier-robust pass (ssmq_filter_robust_dev) for J = 1, 2, 4, 8 next to the forward pass of the same handles, in one
process, everything on the device: simulate_dev, then warm-up and >= 30 calls of either entry point timed one by one with events on the
library stream, the median reported.

    python tools/micro/robust_rate.py [--shape ungm|cv] [--calls 40]

ungm: GPQ Kalman filter, 3 unscented points, B = 1e4, T = 100;  cv: constant velocity + radar, UKF, 9 points, B = 1e5, T = 50.
The models are Gaussian; the pass is given dof = 4 and the measurement covariance as its scale.  Prints one JSON line per shape:
kernel names, median (minimum) time of the forward pass and of the robust pass per J, the ratio to the forward pass, the smallest
weight and the largest delta of the last step.  Run under a time limit (timeout -k 10 300 python tools/micro/robust_rate.py)."""
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
    dyn = sm.ConstantVelocity(sm.GaussRV(4, np.array([100.0, 5.0, 200.0, -3.0]), np.diag([1.0, 0.1, 1.0, 0.1])), sm.GaussRV(2, cov=0.1 * np.eye(2)))
    obs = sm.Radar2DMeasurement(sm.GaussRV(2, cov=np.diag([0.5, 1e-4])), 4)
    return ssinf.UnscentedKalman(dyn, obs), 100000, 50


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
    ap.add_argument('--shape', default='both', choices=('ungm', 'cv', 'both'))
    ap.add_argument('--calls', type=int, default=40)
    a = ap.parse_args()
    lib = _lib.load()
    for shape in (('ungm', 'cv') if a.shape == 'both' else (a.shape,)):
        alg, B, T = build(shape)
        D, Y = alg.mod_dyn.dim_state, alg.mod_obs.dim_out
        d_x, d_y, ld = sm.simulate_dev(alg.mod_dyn, alg.mod_obs, T, B, seed=1)
        stage = _lib.Staging()
        d_m0, d_P0 = alg._initial_planes(stage, B, ld)
        d_fm, d_fP = _lib.DeviceBuffer(8 * T * D * ld), _lib.DeviceBuffer(8 * T * D * D * ld)
        d_lam, d_delta, d_st = _lib.DeviceBuffer(8 * T * ld), _lib.DeviceBuffer(8 * T * ld), _lib.DeviceBuffer(4 * ld)

        def forward():
            alg._launch(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st)

        rec = {'shape': shape, 'D': D, 'Y': Y, 'B': B, 'T': T, 'calls': a.calls, 'filter_kernel': alg.kernel_name(B),
               'robust_kernel': alg.robust_kernel_name(1, B)}
        rec['forward_ms_median'], rec['forward_ms_min'] = (round(v, 4) for v in timed(forward, a.calls))
        dof, _, R = alg._robust_refusal(4.0, 1, None)
        for J in (1, 2, 4, 8):
            def robust():
                alg._launch_robust(lib, B, ld, T, dof, J, R, 0, d_y, d_m0, d_P0, d_fm, d_fP, d_lam, d_delta, d_st)
            med, low = timed(robust, a.calls)
            ok = d_st.download((ld,), dtype=np.int32)[:B] == 0
            rec['J{}'.format(J)] = {'ms_median': round(med, 4), 'ms_min': round(low, 4), 'ratio_to_forward': round(med / rec['forward_ms_median'], 3),
                                    'failed_trajectories': int(B - np.count_nonzero(ok)),
                                    'lam_last_step_min': float(np.min(d_lam.download((T, ld))[T - 1, :B][ok])),
                                    'delta_last_step_max': float(np.max(d_delta.download((T, ld))[T - 1, :B][ok]))}
        print(json.dumps(rec), flush=True)
        for buf in (d_x, d_y, d_fm, d_fP, d_st, d_lam, d_delta):
            buf.free()
        stage.free()


if __name__ == '__main__':
    main()
