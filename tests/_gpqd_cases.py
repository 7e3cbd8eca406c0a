"""Case tables of the GPQ+D tests, shared with tests/golden/make_golden_gpqd.py."""
# tag -> (D, point set, point parameters, kernel parameters [alpha, ell_1 .. ell_D])
WEIGHT_CASES = {
    'd1_ut': (1, 'ut', {'kappa': 0.0}, [10.0, 0.7]),
    'd2_ut': (2, 'ut', None, [1.0, 2.0, 2.0]),
    'd2_sr': (2, 'sr', None, [10.0, 3.0, 3.0]),
}
APPLY_MEANS = (0.0, 0.8, -1.7)       # UNGM dynamics, cov = I
APPLY_TIME = 3.0
