"""Times the masked pass (ssmq_filter_masked_dev) with a full mask, a 50 % random mask (ssmq_detection_mask_dev, per component) and a
full mask behind a 99 % chi-square gate, next to the forward pass and the robust pass at one iteration of the same handles, in one
process, everything on the device: simulate_dev, then warm-up and >= 30 calls of every entry point timed one by one with events on the
library stream, the median reported.

    python tools/micro/masked_rate.py [--shape ungm|cv] [--calls 40]

ungm: GPQ Kalman filter, 3 unscented points, B = 1e4, T = 100;  cv: constant velocity + radar, UKF, 9 points, B = 1e5, T = 50.
Prints one JSON line per shape: kernel names, median (minimum) time of the three passes and of the masked pass per case, the ratios to
the forward pass and to the robust pass, the share of components used.  Run under a time limit (timeout -k 10 300 python
tools/micro/masked_rate.py)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssmtoybox_amd import _lib, ssinf, ssmod as sm  # noqa: E402
from micro.robust_rate import build, timed  # noqa: E402


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
        d_used = _lib.DeviceBuffer(4 * T * ld)
        d_full = sm.detection_mask_dev(B, ld, T, Y, 1.0, seed=2)
        d_half = sm.detection_mask_dev(B, ld, T, Y, 0.5, seed=2)

        def forward():
            alg._launch(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st)

        dof, _, R = alg._robust_refusal(4.0, 1, None)

        def robust():
            alg._launch_robust(lib, B, ld, T, dof, 1, R, 0, d_y, d_m0, d_P0, d_fm, d_fP, d_lam, d_delta, d_st)

        rec = {'shape': shape, 'D': D, 'Y': Y, 'B': B, 'T': T, 'calls': a.calls, 'filter_kernel': alg.kernel_name(B),
               'robust_kernel': alg.robust_kernel_name(1, B), 'masked_kernel': alg.masked_kernel_name(B)}
        rec['forward_ms_median'], rec['forward_ms_min'] = (round(v, 4) for v in timed(forward, a.calls))
        rec['robust_J1_ms_median'], rec['robust_J1_ms_min'] = (round(v, 4) for v in timed(robust, a.calls))
        gate = alg._masked_refusal(ssinf.gate_thresholds(Y, 0.99))
        for what, d_mask, g in (('full_mask', d_full, None), ('half_mask', d_half, None), ('full_mask_gate99', d_full, gate)):
            def masked():
                alg._launch_masked(lib, B, ld, T, 0, g, d_y, d_mask, d_m0, d_P0, d_fm, d_fP, d_used, d_lam, d_delta, d_st)
            med, low = timed(masked, a.calls)
            ok = d_st.download((ld,), dtype=np.int32)[:B] == 0
            uw = d_used.download((T, ld), dtype=np.uint32)[:, :B][:, ok]
            share = sum(int(np.count_nonzero((uw >> i) & 1)) for i in range(Y)) / max(uw.size * Y, 1)
            rec[what] = {'ms_median': round(med, 4), 'ms_min': round(low, 4), 'ratio_to_forward': round(med / rec['forward_ms_median'], 3),
                         'ratio_to_robust_J1': round(med / rec['robust_J1_ms_median'], 3),
                         'failed_trajectories': int(B - np.count_nonzero(ok)), 'share_of_components_used': round(share, 4)}
        print(json.dumps(rec), flush=True)
        for buf in (d_x, d_y, d_fm, d_fP, d_st, d_lam, d_delta, d_used, d_full, d_half):
            buf.free()
        stage.free()


if __name__ == '__main__':
    main()
