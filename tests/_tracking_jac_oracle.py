"""The tracking models that have a Jacobian on the device without one in the reference - coordinated turn, radar, bearings
(csrc/ssmq_device.h: jac_integrand) - stated three times: in mpmath at 50 digits (function and analytic Jacobian;
the Jacobian is checked there against mpmath.diff of the function), in plain NumPy fp64 (the same formulas, the yardstick for
the error bound), and as host callables f(x, t), f_dx(x, t) for the NumPy recursions of tests/_user_jac_oracle.py (ekf, linearize).

Error scale of an entry: S = the sum of the absolute values of the terms of its formula as written here; a device or NumPy entry
is held to |err| <= K eps S, so that the cancellation of c_om, d_om at small theta = omega dt shows in S, not in a loose bar."""
import numpy as np

DPS = 50
EPS = 2.0 ** -52
DT = 0.1
RADAR_LOC = (100.0, -50.0)
SENSORS = ((1000.0, 0.0), (0.0, 1000.0), (-1000.0, 0.0), (0.0, -1000.0))


def _mp():
    import mpmath
    if mpmath.mp.dps < DPS:                 # (diff_jac_mp works at 2 DPS: left alone)
        mpmath.mp.dps = DPS
    return mpmath


# ---- mpmath: functions ---------------------------------------------------------------------------------------------------
def ct_f_mp(x, dt=DT):
    mp = _mp()
    x, dt = [mp.mpf(v) for v in x], mp.mpf(dt)
    om = x[4]
    a, b = mp.sin(om * dt), mp.cos(om * dt)
    c, d = a / om, (1 - b) / om
    return [x[0] + c * x[1] - d * x[3], b * x[1] - a * x[3], d * x[1] + x[2] + c * x[3], a * x[1] + b * x[3], x[4]]


def radar_f_mp(x, loc=RADAR_LOC):
    mp = _mp()
    dx, dy = mp.mpf(x[0]) - mp.mpf(loc[0]), mp.mpf(x[1]) - mp.mpf(loc[1])
    return [mp.sqrt(dx * dx + dy * dy), mp.atan2(dy, dx)]


def bearing_f_mp(x, sensors=SENSORS):
    mp = _mp()
    return [mp.atan2(mp.mpf(x[1]) - mp.mpf(s[1]), mp.mpf(x[0]) - mp.mpf(s[0])) for s in sensors]


# ---- mpmath: analytic Jacobians, each entry as the list of its terms (entry = sum, S = sum of |term|) -------------------------
def ct_terms_mp(x, dt=DT):
    mp = _mp()
    x, dt = [mp.mpf(v) for v in x], mp.mpf(dt)
    om = x[4]
    th = om * dt
    a, b = mp.sin(th), mp.cos(th)
    o2 = om * om
    one, z = [mp.mpf(1)], []
    # c = a / om, d = 1 / om - b / om, c_om = th b / om^2 - a / om^2, d_om = th a / om^2 - 1 / om^2 + b / om^2
    c, d, md = [a / om], [1 / om, -b / om], [-1 / om, b / om]
    x1, x3 = x[1], x[3]
    c_om = lambda s: [s * th * b / o2, -s * a / o2]                            # noqa: E731
    d_om = lambda s: [s * th * a / o2, -s / o2, s * b / o2]                    # noqa: E731
    return [[one, c, z, md, c_om(x1) + d_om(-x3)],
            [z, [b], z, [-a], [-dt * a * x1, -dt * b * x3]],
            [z, d, one, c, d_om(x1) + c_om(x3)],
            [z, [a], z, [b], [dt * b * x1, -dt * a * x3]],
            [z, z, z, z, one]]


def radar_terms_mp(x, loc=RADAR_LOC):
    mp = _mp()
    dx, dy = mp.mpf(x[0]) - mp.mpf(loc[0]), mp.mpf(x[1]) - mp.mpf(loc[1])
    r2 = dx * dx + dy * dy
    r = mp.sqrt(r2)
    return [[[dx / r], [dy / r]], [[-dy / r2], [dx / r2]]]


def bearing_terms_mp(x, sensors=SENSORS):
    mp = _mp()
    rows = []
    for s in sensors:
        dx, dy = mp.mpf(x[0]) - mp.mpf(s[0]), mp.mpf(x[1]) - mp.mpf(s[1])
        r2 = dx * dx + dy * dy
        rows.append([[-dy / r2], [dx / r2]])
    return rows


def collapse(terms):
    """terms[e][k] -> (J, S): the entries in mpmath and their error scales as floats."""
    mp = _mp()
    J = [[mp.fsum(t) for t in row] for row in terms]
    S = np.array([[float(mp.fsum([abs(v) for v in t])) for t in row] for row in terms])
    return J, S


def diff_jac_mp(f, x):
    """mpmath.diff of f's outputs in each input, at 2 DPS working digits."""
    mp = _mp()
    n = len(x)
    with mp.workdps(2 * DPS):
        xs = [mp.mpf(v) for v in x]
        E = len(f(xs))
        return [[mp.diff(lambda v, k=k, e=e: f(xs[:k] + [v] + xs[k + 1:])[e], xs[k]) for k in range(n)] for e in range(E)]


# ---- NumPy fp64: the same formulas ------------------------------------------------------------------------------------------
def ct_f(x, t=0.0, dt=DT):
    om = x[4]
    a, b = np.sin(om * dt), np.cos(om * dt)
    c, d = a / om, (1 - b) / om
    return np.array([x[0] + c * x[1] - d * x[3], b * x[1] - a * x[3], d * x[1] + x[2] + c * x[3], a * x[1] + b * x[3], x[4]])


def ct_dx(x, t=0.0, dt=DT):
    om = x[4]
    th = om * dt
    a, b = np.sin(th), np.cos(th)
    c, d = a / om, (1 - b) / om
    c_om, d_om = (th * b - a) / om ** 2, (th * a - (1 - b)) / om ** 2
    return np.array([[1, c, 0, -d, x[1] * c_om - x[3] * d_om], [0, b, 0, -a, -dt * (a * x[1] + b * x[3])],
                     [0, d, 1, c, x[1] * d_om + x[3] * c_om], [0, a, 0, b, dt * (b * x[1] - a * x[3])], [0, 0, 0, 0, 1.0]])


def radar_f(x, t=0.0, loc=RADAR_LOC):
    dx, dy = x[0] - loc[0], x[1] - loc[1]
    return np.array([np.sqrt(dx * dx + dy * dy), np.arctan2(dy, dx)])


def radar_dx(x, t=0.0, loc=RADAR_LOC):
    dx, dy = x[0] - loc[0], x[1] - loc[1]
    r2 = dx * dx + dy * dy
    r = np.sqrt(r2)
    return np.array([[dx / r, dy / r], [-dy / r2, dx / r2]])


def bearing_f(x, t=0.0, sensors=SENSORS):
    s = np.asarray(sensors)
    return np.arctan2(x[1] - s[:, 1], x[0] - s[:, 0])


def bearing_dx(x, t=0.0, sensors=SENSORS):
    s = np.asarray(sensors)
    dx, dy = x[0] - s[:, 0], x[1] - s[:, 1]
    r2 = dx * dx + dy * dy
    return np.stack((-dy / r2, dx / r2), axis=1)


def cv_f(x, t=0.0, dt=DT):
    return np.array([x[0] + dt * x[1], x[1], x[2] + dt * x[3], x[3]])


def cv_dx(x, t=0.0, dt=DT):
    """As the reference writes it (ssmod.py:848-852): the TRANSPOSE of the transition matrix."""
    return np.array([[1, dt, 0, 0], [0, 1, 0, 0], [0, 0, 1, dt], [0, 0, 0, 1.0]]).T


def indexed(f, f_dx, idx, D):
    """f, f_dx of a sub-state -> callables of the full state: the Jacobian's columns land at idx."""
    idx = list(idx)

    def g(x, t):
        return f(x[idx], t)

    def g_dx(x, t):
        js = f_dx(x[idx], t)
        J = np.zeros((js.shape[0], D), dtype=js.dtype)
        J[:, idx] = js
        return J
    return g, g_dx


# ---- test points ----------------------------------------------------------------------------------------------------------
THETAS = (np.deg2rad(3.0) * DT, 1e-2, 0.1, 1.0, 3.0)       # omega dt; the first: the reference's 3 deg / s at dt = 0.1 (5.2e-3)


def ct_points():
    """70 states [x, vx, y, vy, om]: positions of order 1e3, speeds of order 1e2, omega dt = +-THETAS."""
    rng = np.random.default_rng(5)
    pts = []
    for th in THETAS:
        for sgn in (1.0, -1.0):
            for _ in range(7):
                p = 1e3 * rng.uniform(-2.0, 2.0, 2)
                v = 1e2 * rng.uniform(-3.0, 3.0, 2)
                pts.append([p[0], v[0], p[1], v[1], sgn * th / DT])
    return np.array(pts)


_ANGLES = np.concatenate((np.pi * np.array([0.13, 0.37, 0.61, 0.87, -0.13, -0.37, -0.61, -0.87]),
                          [np.pi - 1e-3, -np.pi + 1e-3, np.pi - 0.02, -np.pi + 0.02, 1e-3, -1e-3, 0.5 * np.pi + 1e-3, -0.5 * np.pi - 1e-3]))
_RANGES = (1.0, 10.0, 100.0, 1e3, 1e4)
# (1e-3 rad from the +-pi cut at r = 1 is 1e-3 in y: ten central-difference steps of check_jacobian at rel_step = 1e-7 and
# coordinates of order 1e3 - closer, and the difference quotient itself would straddle the cut)


def radar_points():
    """80 positions around RADAR_LOC: every quadrant, both sides of the +-pi cut, r = 1 .. 1e4."""
    return np.array([[RADAR_LOC[0] + r * np.cos(a), RADAR_LOC[1] + r * np.sin(a)] for r in _RANGES for a in _ANGLES])


def bearing_points():
    """80 positions, the n-th placed around sensor n mod 4 as radar_points places its own; none within 1e-3 r of any sensor."""
    pts = []
    for n, (r, a) in enumerate((r, a) for r in _RANGES for a in _ANGLES):
        s = SENSORS[n % 4]
        pts.append([s[0] + r * np.cos(a), s[1] + r * np.sin(a)])
    pts = np.array(pts)
    for s in SENSORS:
        d = np.hypot(pts[:, 0] - s[0], pts[:, 1] - s[1])
        assert np.all(d > 0.5), 'a test point at a sensor'
    return pts


def embed(p2, D, idx):
    """(n, 2) positions -> (n, D) states with the positions at idx and unit-sized values elsewhere."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((p2.shape[0], D))
    x[:, list(idx)] = p2
    return x


_REF = {}


def reference(name):
    """(points (n, din), J (n, E, din) rounded from mpmath, S (n, E, din)) of 'ct' | 'radar' | 'bearing', computed once."""
    if name not in _REF:
        pts, terms = {'ct': (ct_points, ct_terms_mp), 'radar': (radar_points, radar_terms_mp), 'bearing': (bearing_points, bearing_terms_mp)}[name]
        pts = pts()
        Js, Ss = [], []
        for x in pts:
            J, S = collapse(terms(list(x)))
            Js.append([[float(v) for v in row] for row in J])
            Ss.append(S)
        _REF[name] = (pts, np.array(Js), np.array(Ss))
    return _REF[name]


def ratio(J, name):
    """worst |J - oracle| / (eps S) over the entries with S > 0; entries with S = 0 must be exactly 0."""
    _, Jr, S = reference(name)
    J = np.asarray(J, dtype=float)
    assert np.all(J[S == 0] == 0.0)
    return float(np.max(np.abs(J - Jr)[S > 0] / (EPS * S[S > 0])))


def twin_ratio(name):
    """The NumPy fp64 twin's worst ratio on the test points: what K is derived from (K = max(8, 4 x this))."""
    pts = reference(name)[0]
    f_dx = {'ct': ct_dx, 'radar': radar_dx, 'bearing': bearing_dx}[name]
    return ratio(np.array([f_dx(x) for x in pts]), name)


def bound_K(name):
    return max(8.0, 4.0 * twin_ratio(name))


# ---- the extended Kalman recursion in a chosen precision --------------------------------------------------------------------
def _chol(S):
    n = S.shape[0]
    L = np.zeros_like(S)
    for j in range(n):
        L[j, j] = np.sqrt(S[j, j] - np.sum(L[j, :j] * L[j, :j]))
        for i in range(j + 1, n):
            L[i, j] = (S[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    return L


def _solve_spd(S, Bm):
    """S^-1 Bm through the Cholesky factor, in the dtype of S."""
    L, n = _chol(S), S.shape[0]
    X = Bm.copy()
    for i in range(n):
        X[i] = (X[i] - L[i, :i].dot(X[:i])) / L[i, i]
    for i in range(n - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i].dot(X[i + 1:])) / L[i, i]
    return X


def ekf_in(dtype, fd, fd_dx, fo, fo_dx, y, m0, P0, gqg, rr):
    """The additive-noise extended Kalman recursion of tests/_user_jac_oracle.py::ekf (time index k in both transforms of step k)
    with every operation in `dtype` (np.float64, np.longdouble) from the float64 inputs: (fm (D, T, B), fP (D, D, T, B))."""
    Y, T, B = y.shape
    D = m0.shape[0]
    y, gqg, rr = y.astype(dtype), gqg.astype(dtype), rr.astype(dtype)
    fm, fP = np.zeros((D, T, B), dtype=dtype), np.zeros((D, D, T, B), dtype=dtype)
    for b in range(B):
        m, P = m0.astype(dtype), P0.astype(dtype)
        for k in range(T):
            F = fd_dx(m, float(k)).astype(dtype)
            mp, Pp = fd(m, float(k)), F.dot(P).dot(F.T) + gqg
            H = fo_dx(mp, float(k)).astype(dtype)
            Pyx = H.dot(Pp)
            S = Pyx.dot(H.T) + rr
            Kt = _solve_spd(S, Pyx)                       # (Y, D): gain'
            m = mp + Kt.T.dot(y[:, k, b] - fo(mp, float(k)))
            P = Pp - Kt.T.dot(S).dot(Kt)
            fm[:, k, b], fP[:, :, k, b] = m, P
    return fm, fP
