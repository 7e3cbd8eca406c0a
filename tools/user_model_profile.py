"""
Kernel time of the pendulum UKF as device code against the built-in one (B = 1e5, T = 100, three passes each), and hiprtc wall
time per instantiation at D = 2 and D = 6.
  rocprofv3 --kernel-trace --stats -d OUT -o user -- python tools/user_model_profile.py OUT/user_models.json
  python tools/user_model_profile.py --summarize OUT/user_results.db OUT/user_models.json   -> profiles/r07_user_models_prof.txt format
"""
import os, sys, time, json, sqlite3
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) > 1 and sys.argv[1] == '--summarize':
    c = sqlite3.connect(sys.argv[2])
    print('# tools/user_model_profile.py: rocprofv3 --kernel-trace, kernel durations (us) of the whole-pass filter kernels')
    for name, n, avg, mn in c.execute("select name, count(*), avg(end - start), min(end - start) from kernels where name like "
                                      "'%k_filter_fused%' group by name order by name"):
        print('{:90s} n={} avg={:.1f} min={:.1f}'.format(name, n, avg / 1e3, mn / 1e3))
    print('# hiprtc (ssmq_rtc_stats around the first pass):', json.dumps(json.load(open(sys.argv[3]))))
    sys.exit(0)
import numpy as np
import ssmtoybox_amd as amd
from ssmtoybox_amd import ssinf, ssmod, _lib
amd.set_device(0)
os.environ['SSMQ_FUSED_QUAD'] = '0'
B, T = 100000, 100
m0, P0 = np.array([1.5, 0.0]), 0.01 * np.eye(2)
Q = 0.01 * np.array([[0.01 ** 3 / 3, 0.01 ** 2 / 2], [0.01 ** 2 / 2, 0.01]])
class UP(ssmod.TransitionModel):
    dim_state, dim_noise, noise_additive = 2, 2, True
    device_code = 'o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]);'
    def __init__(self, a, b, dt=0.01):
        super().__init__(a, b); self.dt = dt
    def _par(self): return (self.dt,)
class UM(ssmod.MeasurementModel):
    dim_out, dim_substate, dim_noise, noise_additive = 1, 1, 1, True
    device_code = 'o[0] = sin_nr(x[0]);'
class U6(ssmod.TransitionModel):
    dim_state, dim_noise, noise_additive = 6, 6, True
    device_code = 'for (int i = 0; i < 3; ++i) { o[2 * i] = x[2 * i] + x[2 * i + 1] * p[0]; o[2 * i + 1] = x[2 * i + 1] - 9.81 * p[0] * sin_nr(x[2 * i]); }'
    def _par(self): return (0.01,)
class U6M(ssmod.MeasurementModel):
    dim_out, dim_substate, dim_noise, noise_additive = 2, 6, 2, True
    device_code = 'o[0] = sin_nr(x[0]); o[1] = sin_nr(x[2]) + x[4];'
rng = np.random.default_rng(1)
y = np.sin(1.5 * np.cos(np.linspace(0, 3, T)))[None, :, None] + 0.1 * rng.standard_normal((1, T, B))
out = {}
for tag, Dyn, Obs in (('builtin', ssmod.Pendulum2DTransition, ssmod.Pendulum2DMeasurement), ('user', UP, UM)):
    dyn, obs = Dyn(ssmod.GaussRV(2, m0, P0), ssmod.GaussRV(2, cov=Q)), Obs(ssmod.GaussRV(1, cov=np.array([[0.1]])), 2)
    alg = ssinf.UnscentedKalman(dyn, obs)
    c0, _, s0 = _lib.rtc_stats()
    for r in range(3):
        fm, fP = alg.forward_pass_batch(y, raise_on_failure=False)
    c1, _, s1 = _lib.rtc_stats()
    out[tag] = dict(kernel=alg.kernel_name(B), compiles=c1 - c0, compile_s=s1 - s0)
# D = 6: one instantiation of the whole-pass kernel
m6 = np.array([0.5, 0, -0.3, 0, 0.2, 0])
dyn, obs = U6(ssmod.GaussRV(6, m6, 0.01 * np.eye(6)), ssmod.GaussRV(6, cov=1e-4 * np.eye(6))), U6M(ssmod.GaussRV(2, cov=0.01 * np.eye(2)), 6)
alg = ssinf.UnscentedKalman(dyn, obs)
c0, _, s0 = _lib.rtc_stats()
t0 = time.time()
alg.forward_pass_batch(np.zeros((2, 10, 64)), raise_on_failure=False)
c1, _, s1 = _lib.rtc_stats()
out['d6'] = dict(kernel=alg.kernel_name(64), compiles=c1 - c0, compile_s=s1 - s0, wall_s=time.time() - t0)
print(json.dumps(out, indent=1))
json.dump(out, open(sys.argv[1], 'w'), indent=1)
