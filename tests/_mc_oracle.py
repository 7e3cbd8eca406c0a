"""
NumPy restatement of the streaming Monte-Carlo transform (csrc/ssmq_mc_moments.h, csrc/ssmq_mc_transform.hip) - the oracle of
tests/test_mc_transform_host.py and tests/test_mc_transform_gpu.py.

The draw (the header comment of csrc/ssmq_mc_moments.h): sample j has the unit point z_j, two coordinates per Philox call,
    (o0, o1, o2, o3) = Philox4x32-10(counter = (j, 0, p, MC_TAG), key = (seed & 0xffffffff, seed >> 32))
    u1 = (((o0 >> 5) << 26 | o1 >> 6) + 0.5) 2^-53,   u2 likewise from (o2, o3)
    r = sqrt(-2 log u1),   z_j[2 p] = r cos(2 pi u2),   z_j[2 p + 1] = r sin(2 pi u2)
with MC_TAG = 0x4D435446.  The moments are the reference's centred formulas (mtran.py:62-94), here in np.longdouble (the
oracle) and in float64 (what the reference itself would return on the same draws: the yardstick of the device's error).
"""
import numpy as np

from tests._bootstrap_oracle import philox4x32_10, M32

MC_TAG = 0x4D435446
CHUNK = 2048                  # kMcChunk
LD = np.longdouble
PI_LD = LD('3.14159265358979323846264338327950288')


def _cospi_sinpi(w):
    """cos(pi w), sin(pi w) for float64 w in (0, 2), rounded from long double.  The argument is reduced exactly first - w = k / 2
    + v with |v| <= 1 / 4 - so that the values near a zero of cos or sin keep their relative accuracy, as sincospi's do."""
    k = np.rint(2.0 * w)
    a = PI_LD * (w - 0.5 * k).astype(LD)
    c, s = np.cos(a).astype(np.float64), np.sin(a).astype(np.float64)
    q = k.astype(np.int64) % 4
    return np.choose(q, [c, -s, -c, s]), np.choose(q, [s, c, -s, -c])


def unit_points(seed, D, first, count):
    """(D, count) float64 unit samples first .. first + count - 1.  cos / sin of 2 pi u2 are taken in long double after an exact argument reduction and
    rounded (the device's sincospi is exact in its argument reduction); log, sqrt and the product are float64 as on the device."""
    j = np.arange(first, first + count, dtype=np.uint64)
    key = (seed & M32, (seed >> 32) & M32)
    z = np.empty((D, count))
    for p in range((D + 1) // 2):
        o = philox4x32_10((j, 0, p, MC_TAG), key)
        o = [np.asarray(v, dtype=np.uint64) for v in o]
        u1 = (((o[0] >> np.uint64(5)) << np.uint64(26) | (o[1] >> np.uint64(6))).astype(np.float64) + 0.5) * 2.0 ** -53
        u2 = (((o[2] >> np.uint64(5)) << np.uint64(26) | (o[3] >> np.uint64(6))).astype(np.float64) + 0.5) * 2.0 ** -53
        r = np.sqrt(-2.0 * np.log(u1))
        cs, sn = _cospi_sinpi(2.0 * u2)
        z[2 * p] = r * cs
        if 2 * p + 1 < D:
            z[2 * p + 1] = r * sn
    return z


# ---- the integrands, vectorised over the sample axis and in the dtype of x (float64 or longdouble) ------------------------------
def f_ungm(x, t):
    return (0.5 * x[0] + 25 * (x[0] / (1 + x[0] ** 2)) + 8 * np.cos(x.dtype.type(1.2) * x.dtype.type(t)))[None]


def f_pendulum(x, t, dt=0.01):
    return np.stack((x[0] + x[1] * dt, x[1] - 9.81 * dt * np.sin(x[0])))


def f_radar(x, t, idx=(0, 1)):
    dx, dy = x[idx[0]], x[idx[1]]
    return np.stack((np.sqrt(dx ** 2 + dy ** 2), np.arctan2(dy, dx)))


def f_reentry(x, t, dt=0.1):
    R0, H0, Gm0, b0 = 6374, 13.406, 3.9860e5, -0.59783
    b = b0 * np.exp(x[4])
    R = np.sqrt(x[0] ** 2 + x[1] ** 2)
    V = np.sqrt(x[2] ** 2 + x[3] ** 2)
    Dr = b * np.exp((R0 - R) / H0) * V
    G = -Gm0 / R ** 3
    return np.stack((x[0] + dt * x[2], x[1] + dt * x[3], x[2] + dt * (Dr * x[2] + G * x[0]), x[3] + dt * (Dr * x[3] + G * x[1]),
                     x[4]))


def f_reentry_bias(x, t, dt=0.1):
    return np.concatenate((f_reentry(x[:5], t, dt), x[5:6]))


def f_cv(x, t, dt=0.5):
    return np.stack((x[0] + dt * x[1], x[1], x[2] + dt * x[3], x[3]))


def cholesky(P):
    """Lower Cholesky factor in the dtype of P (numpy.linalg has no long double)."""
    n = P.shape[0]
    L = np.zeros_like(P)
    for j in range(n):
        L[j, j] = np.sqrt(P[j, j] - (L[j, :j] ** 2).sum())
        for i in range(j + 1, n):
            L[i, j] = (P[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def moments(f, mean, cov, z, t=0.0, dtype=LD):
    """The reference's MonteCarloTransform.apply (mtran.py:73-86) on the unit points z (D, n), two-pass, in `dtype`."""
    m, P, zz = np.asarray(mean, dtype=dtype), np.asarray(cov, dtype=dtype), np.asarray(z, dtype=dtype)
    n = zz.shape[1]
    x = m[:, None] + cholesky(P).dot(zz)
    fx = f(x, t)
    mean_f = fx.sum(axis=1) / dtype(n)
    dfx = fx - mean_f[:, None]
    cov_f = dfx.dot(dfx.T) / dtype(n - 1)
    cov_fx = dfx.dot((x - m[:, None]).T) / dtype(n - 1)
    return mean_f, cov_f, cov_fx


def scaled_errors(got, exact):
    """max |got - exact| of (mean_f, cov_f, cov_fx), each over the largest magnitude of its exact array."""
    out = []
    for g, e in zip(got, exact):
        s = np.max(np.abs(e))
        out.append(float(np.max(np.abs(np.asarray(g, dtype=LD) - e)) / (s if s > 0 else LD(1))))
    return out


def random_moments(rng, B, D, centre, spread):
    """B means around `centre` and B distinct random positive-definite covariances with standard deviations ~ `spread`."""
    centre, spread = np.asarray(centre, dtype=float), np.asarray(spread, dtype=float)
    mean = centre + 0.1 * spread * rng.standard_normal((B, D))
    a = rng.standard_normal((B, D, D)) / np.sqrt(D)
    cov = np.einsum('bij,bkj->bik', a, a) + 0.2 * np.eye(D)
    cov = cov * spread[:, None] * spread[None, :]
    return mean, cov
