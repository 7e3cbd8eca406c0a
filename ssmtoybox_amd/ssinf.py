"""
Callers of the moment-transform path kept on the device: Gaussian filters (reference:
ssmtoybox/ssinf.py:215-323, 347-552) running B independent trajectories per kernel launch.

`forward_pass(data)` keeps the reference's one-trajectory signature; `forward_pass_batch(data)` takes
data of shape (dim_y, T, B) - the reference's Monte-Carlo axis (`for imc in range(mc)` in its research scripts,
e.g. research/tpq/tpq_base.py:175-192) - and returns (D, T, B) / (D, D, T, B).

Per time step k = 1..T (both transforms use time index k - 1: ssinf.py:104, 276-288):
    dyn transform, + G Q G'   ->   obs transform, + R   ->   Kalman update (ssinf.py:297-323)
all inside `ssmq_filter_forward_dev` (ssmtoybox_amd/csrc); nothing is computed in NumPy.
`StudentianInference` (ssinf.py:555-736) runs the same loop with the reference's scale-matrix bookkeeping
(`ssmq_student_filter_forward_dev`); `backward_pass*` is the RTS smoother (`ssmq_filter_smooth_dev`).  Models that take
their noise as an argument (UNGMNA, CTRS; ssinf.py:271-295) go through `ssmq_filter_forward_aug_dev` / `ssmq_filter_smooth_aug_dev`.
`MarginalInference` (ssinf.py:1034-1292) evaluates its theta-conditioned steps on the device (`ssmq_gp_theta_step`); the
BFGS optimiser stays on the host as in the reference.
"""
import ctypes

import numpy as np

from . import _lib
from .mtran import (MomentTransform, LinearizationTransform, TaylorGPQDTransform, UnscentedTransform, SphericalRadialTransform, GaussHermiteTransform,
                    FullySymmetricStudentTransform, TruncatedUnscentedTransform, TruncatedSphericalRadialTransform,
                    TruncatedGaussHermiteTransform, resolve_integrand)
from .bq.bqmtran import (GaussianProcessTransform, BayesSardTransform, StudentTProcessTransform,
                         MultiOutputGaussianProcessTransform, GaussianProcessDerTransform)
from .ssmod import TransitionModel, MeasurementModel, is_user_model, has_device_jacobian, user_unsupported, check_user_points


_NOT_PD = 'Matrix is not positive definite (trajectory {}, step {})'


def _raise_failed(status, prefix='', message=_NOT_PD):
    """The LinAlgError of the first trajectory whose status is not 0 (1 + the step that failed), if there is one."""
    if status.any():
        b = int(np.flatnonzero(status)[0])
        raise np.linalg.LinAlgError(prefix + message.format(b, int(status[b]) - 1))


def _iteration_count(iterations):
    """`iterations` as an int, or the ValueError of a count outside 1 .. ITERATED_MAX."""
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= int(iterations) <= _lib.ITERATED_MAX:
        raise ValueError('iterations must be an integer in 1 .. {} (got {!r})'.format(_lib.ITERATED_MAX, iterations))
    return int(iterations)


def initial_planes(stage, D, mean, cov, B, ld, x0_mean=None, x0_cov=None, broadcast_on_device=False):
    """The initial moments of B trajectories as planes [D][ld], [D*D][ld], buffers of the staging scope `stage`: the model's
    (mean, cov) for every trajectory, or the per-trajectory x0_mean (B, D) / x0_cov (B, D, D), laid out on the host and uploaded
    (scratch blocks).  broadcast_on_device: the model's moments only, one 64-lane tile per plane uploaded and doubled on the device
    until the plane is full (DeviceBuffers; no host array of the size of the batch)."""
    if broadcast_on_device:
        assert x0_mean is None and x0_cov is None
        lib = _lib.load()
        planes = []
        for moment, n in ((mean, D), (cov, D * D)):
            tile = np.ascontiguousarray(np.repeat(np.asarray(moment, dtype=np.float64).reshape(n, 1), 64, axis=1))
            dev = stage.device(8 * n * ld)
            for e in range(n):
                dev.upload(tile[e], byte_offset=8 * e * ld)
                done = 64
                while done < ld:
                    step = min(done, ld - done)
                    _lib.check(lib.ssmq_memcpy_d2d(dev.at(8 * (e * ld + done)), dev.at(8 * e * ld), ctypes.c_size_t(8 * step)),
                               'ssmq_memcpy_d2d')
                    done += step
            planes.append(dev)
        return planes
    m0 = np.broadcast_to(mean, (B, D)) if x0_mean is None else np.asarray(x0_mean, dtype=np.float64)
    P0 = np.broadcast_to(cov, (B, D, D)) if x0_cov is None else np.asarray(x0_cov, dtype=np.float64)
    mbuf = np.zeros((D, ld))
    mbuf[:, :B] = m0.T
    Pbuf = np.zeros((D * D, ld))
    Pbuf[:, :B] = P0.reshape(B, D * D).T
    if ld > B:       # padding lanes are never read (b >= B), keep them PD anyway
        Pbuf[:, B:] = np.eye(D).reshape(-1, 1)
    d_m0, d_P0 = stage.scratch(mbuf.nbytes), stage.scratch(Pbuf.nbytes)
    d_m0.upload(mbuf)
    d_P0.upload(Pbuf)
    return d_m0, d_P0


_NOISE_SWEEP_RANGE = ('noise sweeps cover UnscentedKalman, CubatureKalman, GaussHermiteKalman, GaussianProcessKalman, BayesSardKalman and '
                      'StudentProcessKalman on the built-in additive-noise model pairs of the fused time loop, Gaussian noise and a '
                      'Gaussian initial state, D <= 6, Y <= 4 and the point counts that loop is instantiated for')


def noise_grid(cov, scales):
    """Rows of a noise sweep that are multiples of one covariance: cov (n, n) and scales (P,) -> (P, n, n) = scales[:, None, None] *
    cov."""
    cov, scales = np.atleast_2d(np.asarray(cov, dtype=np.float64)), np.asarray(scales, dtype=np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or scales.ndim != 1 or scales.size == 0:
        raise ValueError('noise_grid: cov is a square matrix and scales a non-empty one-dimensional sequence')
    return np.ascontiguousarray(scales[:, None, None] * cov)


def gate_thresholds(dim_y, prob):
    """The gate table of `masked_pass*` from a gate probability: the chi-square quantiles chi2.ppf(prob, o) for o = 1 .. dim_y
    observed components (SciPy), so that a measurement that fits the filter's model passes the gate with probability `prob`."""
    from scipy.stats import chi2
    prob = float(prob)
    if not 0.0 < prob <= 1.0:
        raise ValueError('gate_thresholds: prob must lie in (0, 1] (got {!r})'.format(prob))
    return chi2.ppf(prob, np.arange(1, int(dim_y) + 1))


def mode_transition(M, stay):
    """The transition matrix of M modes that keep their mode with probability `stay` and go to each of the others with equal
    probability: (M, M), `stay` on the diagonal and (1 - stay) / (M - 1) off it (M = 1: [[1]])."""
    M = int(M)
    if M < 1 or not 0.0 <= float(stay) <= 1.0:
        raise ValueError('mode_transition: M >= 1 and 0 <= stay <= 1')
    if M == 1:
        return np.ones((1, 1))
    pi = np.full((M, M), (1.0 - float(stay)) / (M - 1))
    np.fill_diagonal(pi, float(stay))
    return pi


IMM_MAX_MODES = 8


def _mode_probabilities(pi, mu0):
    """(pi (M, M), mu0 (M,)) of an IMM pass as C arrays, checked as the library checks them: 1 <= M <= IMM_MAX_MODES
    (NotImplementedError beyond), entries finite and non-negative, every row of pi and mu0 summing to 1 within 1e-12 (ValueError
    naming the row).  mu0 None: uniform."""
    pi = np.ascontiguousarray(pi, dtype=np.float64)
    if pi.ndim != 2 or pi.shape[0] != pi.shape[1] or pi.shape[0] < 1:
        raise ValueError('IMM: pi is a square (M, M) matrix with M >= 1; got shape {}'.format(pi.shape))
    M = pi.shape[0]
    if M > IMM_MAX_MODES:
        raise NotImplementedError('IMM: 1 <= M <= {} modes; got M = {}'.format(IMM_MAX_MODES, M))
    mu0 = np.full(M, 1.0 / M) if mu0 is None else np.ascontiguousarray(mu0, dtype=np.float64)
    if mu0.shape != (M,):
        raise ValueError('IMM: mu0 is None (uniform) or has shape ({},); got {}'.format(M, mu0.shape))
    for name, row in [('row {} of pi'.format(i), pi[i]) for i in range(M)] + [('mu0', mu0)]:
        if not np.isfinite(row).all() or (row < 0).any():
            raise ValueError('IMM: {} has an entry that is not finite or is negative'.format(name))
        total = 0.0
        for v in row:
            total += float(v)
        if not abs(total - 1.0) <= 1e-12:
            raise ValueError('IMM: {} does not sum to 1 within 1e-12 (sum {!r})'.format(name, total))
    return pi, mu0


def _cov_rows(value, own, name):
    """A covariance argument of a noise sweep - None (the model's own), one matrix (shared by all rows) or a stack (P, n, n) - as
    ((rows, n, n) float64, whether it is a stack); ValueError for another shape and for a row that is not finite or not symmetric,
    naming the row."""
    own = np.atleast_2d(np.asarray(own, dtype=np.float64))
    a = own if value is None else np.asarray(value, dtype=np.float64)
    n = own.shape[0]
    stacked = a.ndim == 3
    if a.shape[-2:] != (n, n) or a.ndim not in (2, 3) or a.shape[0] < 1:
        raise ValueError('noise sweep: {} is None, one ({n}, {n}) matrix or a stack (P, {n}, {n}) with P >= 1; got shape {}'.format(
            name, a.shape, n=n))
    a = a.reshape((-1, n, n))
    for p, row in enumerate(a):
        if not np.isfinite(row).all():
            raise ValueError('noise sweep: row {} of {} is not finite'.format(p, name))
        if not np.array_equal(row, row.T):
            raise ValueError('noise sweep: row {} of {} is not symmetric'.format(p, name))
    return a, stacked


class GaussianInference:
    """Gaussian filter (ssinf.py:215-323)."""

    def __init__(self, mod_dyn, mod_obs, tf_dyn, tf_obs):
        assert isinstance(mod_dyn, TransitionModel) and isinstance(mod_obs, MeasurementModel)
        assert isinstance(tf_dyn, MomentTransform) and isinstance(tf_obs, MomentTransform)
        self.mod_dyn, self.mod_obs, self.tf_dyn, self.tf_obs = mod_dyn, mod_obs, tf_dyn, tf_obs
        self.x0_mean, self.x0_cov = mod_dyn.init_rv.get_stats()
        self.q_mean, self.q_cov = mod_dyn.noise_rv.get_stats()
        # (a StudentRV measurement noise hands back its dof as well: its SCALE matrix stands in for R - what `robust_pass*` are for)
        self.r_mean, self.r_cov = mod_obs.noise_rv.get_stats()[:2]
        self.G = mod_dyn.noise_gain
        self.fi_mean = self.fi_cov = None
        self.sm_mean = self.sm_cov = None
        self.status = None
        self._data = None

    def reset(self):
        self.fi_mean = self.fi_cov = None
        self.sm_mean = self.sm_cov = None
        self.status = None
        self._data = None

    def _check_user_points(self):
        """Filters on user models (device_code) run the run-time compiled whole-pass kernel: 2 .. 2 D + 1 points per transform."""
        if is_user_model(self.mod_dyn) or is_user_model(self.mod_obs):
            for tf in (self.tf_dyn, self.tf_obs):
                if tf._num_points():                  # (the linearisation and Taylor-GPQD transforms have no points)
                    check_user_points(self.mod_dyn.dim_state, tf._num_points())

    @property
    def _additive(self):
        return self.mod_dyn.noise_additive and self.mod_obs.noise_additive

    # ---- what every entry point below is built from: the pair, the noise arguments, a staging scope (`_lib.Staging`), the status
    # check (`_raise_failed`) ------------------------------------------------------------------------------------------------------
    _recursion = 'gauss'         # 'student': the Studentian recursion (its own entry point, `scale` / `dof` in a `run_filters` job)

    def _pair(self):
        """(h_dyn, f_dyn, h_obs, f_obs): the transform handles and integrand descriptors every C entry point starts with (ctypes
        passes a descriptor by reference where the prototype says so)."""
        f_dyn, e_dyn = resolve_integrand(self.mod_dyn.dyn_eval)
        f_obs, e_obs = resolve_integrand(self.mod_obs.meas_eval)
        return self.tf_dyn._handle_for(e_dyn), f_dyn, self.tf_obs._handle_for(e_obs), f_obs

    def _noise(self):
        """The additive terms of the recursion as C arrays: G Q G' and R (None for a model that takes its noise as an argument)."""
        gqg = np.ascontiguousarray(self.G.dot(self.q_cov).dot(self.G.T), dtype=np.float64) if self.mod_dyn.noise_additive else None
        rr = np.ascontiguousarray(self.r_cov, dtype=np.float64) if self.mod_obs.noise_additive else None
        return gqg, rr

    def _noise_aug(self):
        """(q_mean, q_cov, dim_q, r_mean, r_cov, dim_r) of the augmented recursion: the moments of a noise that enters its model
        function (ssinf.py:271-272, 282-283, 294-295); (None, the term of `_noise`, 0) for an additive one."""
        def moments(mean, cov):
            mean = np.ascontiguousarray(np.atleast_1d(mean), dtype=np.float64)
            return mean, np.ascontiguousarray(np.atleast_2d(cov), dtype=np.float64), int(mean.shape[0])
        gqg, rr = self._noise()
        return ((None, gqg, 0) if gqg is not None else moments(self.q_mean, self.q_cov)) + \
               ((None, rr, 0) if rr is not None else moments(self.r_mean, self.r_cov))

    def _kernel_name(self, fn, *extra, unsupported=False):
        """`fn(pair..., extra..., buf, 512)` of the library, checked and decoded (unsupported: see `_lib.check`)."""
        buf = ctypes.create_string_buffer(512)
        _lib.check(getattr(_lib.load(), fn)(*self._pair(), *extra, buf, 512), fn, unsupported)
        return buf.value.decode()

    def _initial_planes(self, stage, B, ld, x0_mean=None, x0_cov=None, broadcast_on_device=False):
        """The initial moments of B trajectories as planes [D][ld], [D*D][ld], buffers of `stage` (`initial_planes`)."""
        return initial_planes(stage, self.mod_dyn.dim_state, self.x0_mean, self._initial_cov(), B, ld, x0_mean, x0_cov,
                              broadcast_on_device)

    def _initial_cov(self):
        return self.x0_cov

    def kernel_name(self, batch=0, ld=0, T=0):
        """Which kernel(s) the device filter loop runs for this filter (one fused kernel - k_filter_fused<..> and its schedules,
        k_ekf_loop<D=..,Y=..> for ExtendedKalman on built-in models - or a replayed hipGraph of 3 T launches) on a batch of
        `batch` trajectories (0: a batch that fills the device; small batches of some systems run k_filter_wsplit), in planes
        of pitch `ld` over `T` steps (0, 0: not given; k_filter_ungm_quad takes passes of 8 ld T < 2^31 bytes only)."""
        if not self._additive:
            return ('k_filter_fused_aug (one kernel for the time loop) where instantiated, else a launch loop of 5 T '
                    'launches (k_augment | apply dyn | k_augment | apply obs | k_kalman_update)')
        self._check_user_points()
        if ld or T:
            return self._kernel_name('ssmq_filter_kernel_name_shape', int(batch), int(ld), int(T))
        return self._kernel_name('ssmq_filter_kernel_name_batch', int(batch))

    def forward_pass(self, data):
        """data (dim_y, T) -> filtered means (D, T), covariances (D, D, T)  (ssinf.py:66-118)."""
        fm, fP = self.forward_pass_batch(np.asarray(data)[..., None])
        return fm[..., 0], fP[..., 0]

    def _launch(self, lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st):
        if not self._additive:
            return self._launch_aug(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st)
        gqg, rr = self._noise()
        vp, dp = _lib.vp, _lib.dp
        _lib.check(lib.ssmq_filter_forward_dev(*self._pair(), B, ld, T, vp(d_y), vp(d_m0), vp(d_P0), dp(gqg), dp(rr), vp(d_fm), vp(d_fP),
                                               vp(d_st)), 'ssmq_filter_forward_dev')

    def _launch_smooth(self, lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_sm, d_sP, d_st):
        """The forward pass and the RTS smoother in one call."""
        if not self._additive:
            return self._launch_aug(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st, d_sm, d_sP)
        gqg, rr = self._noise()
        vp, dp = _lib.vp, _lib.dp
        _lib.check(lib.ssmq_filter_smooth_dev(*self._pair(), B, ld, T, vp(d_y), vp(d_m0), vp(d_P0), dp(gqg), dp(rr), vp(d_fm), vp(d_fP),
                                              vp(d_sm), vp(d_sP), vp(d_st)), 'ssmq_filter_smooth_dev')

    def _launch_aug(self, lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st, d_sm=None, d_sP=None):
        """Noise enters the model functions: augmented moments per transform (ssinf.py:271-272, 282-283, 294-295).
        With d_sm / d_sP the RTS smoother runs as well (`ssmq_filter_smooth_aug_dev`)."""
        qm, qc, dq, rm, rc, dr = self._noise_aug()
        vp, dp = _lib.vp, _lib.dp
        args = (*self._pair(), self.mod_dyn.dim_state, B, ld, T, vp(d_y), vp(d_m0), vp(d_P0), dp(qm), dp(qc), dq, dp(rm), dp(rc), dr,
                vp(d_fm), vp(d_fP))
        if d_sm is not None:
            _lib.check(lib.ssmq_filter_smooth_aug_dev(*args, vp(d_sm), vp(d_sP), vp(d_st)), 'ssmq_filter_smooth_aug_dev')
        else:
            _lib.check(lib.ssmq_filter_forward_aug_dev(*args, vp(d_st)), 'ssmq_filter_forward_aug_dev')

    def backward_pass(self):
        """RTS smoothing of the trajectory given to the last forward_pass (ssinf.py:120-147)."""
        sm, sP = self.backward_pass_batch()
        return sm[..., 0], sP[..., 0]

    def backward_pass_batch(self):
        """RTS smoothing of the batch given to the last forward_pass_batch: (D, T, B), (D, D, T, B).  The reference's
        indexing is kept (the last two smoothed steps equal the filtered ones)."""
        assert self._data is not None, 'run forward_pass first'     # the reference asserts its 'filtered' flag
        if is_user_model(self.mod_dyn) or is_user_model(self.mod_obs):
            raise user_unsupported('the RTS smoother (backward_pass)')
        self.forward_pass_batch(self._data, smooth=True)
        return self.sm_mean, self.sm_cov

    def forward_pass_dev(self, d_y, B, ld, T):
        """Filter measurements that are already on the device (planes [T][dim_y][ld], e.g. from `ssmod.simulate_dev`)
        and leave the results there: returns DeviceBuffers (d_fm [T][D][ld], d_fP [T][D*D][ld], d_status [ld]) for
        `mcshard.device_error_sums`; the caller frees them.  Every trajectory starts from the model's initial moments."""
        self._check_user_points()
        lib = _lib.load()
        D = self.mod_dyn.dim_state
        with _lib.Staging() as stage:
            d_m0, d_P0 = self._initial_planes(stage, B, ld, broadcast_on_device=True)
            d_fm, d_fP, d_st = stage.device(8 * T * D * ld), stage.device(8 * T * D * D * ld), stage.device(4 * ld)
            self._launch(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st)
            _lib.sync()
            return stage.release(d_fm, d_fP, d_st)

    def _forward_pass_piped(self, lib, data, x0_mean, x0_cov, raise_on_failure):
        """The forward pass with its transfers overlapped (`ssmq_filter_forward_piped`: time blocks; the measurements of the next
        block go up and the moments of the previous one come down while a block runs).  None when the filter has no time-block
        kernel - the caller then takes the upload / pass / download path.  Results: the same bits either way."""
        if self._recursion != 'gauss':        # Studentian recursion: not pipelined
            return None
        Y, T, B = data.shape
        D = self.mod_dyn.dim_state
        pair = self._pair()
        flags = 0
        if x0_mean is None and x0_cov is None:
            m0, P0 = np.ascontiguousarray(self.x0_mean, dtype=np.float64), np.ascontiguousarray(self._initial_cov(), dtype=np.float64)
        else:
            m0 = np.ascontiguousarray(np.broadcast_to(self.x0_mean, (B, D)) if x0_mean is None else x0_mean, dtype=np.float64)
            P0 = np.ascontiguousarray(np.broadcast_to(self._initial_cov(), (B, D, D)) if x0_cov is None else x0_cov, dtype=np.float64)
            flags |= 2           # SSMQ_PIPED_X0_PER_TRAJECTORY
        fm, fP = _lib.pinned_empty((D, T, B)), _lib.pinned_empty((D, D, T, B))
        if fm is None or fP is None:
            fm, fP = np.empty((D, T, B)), np.empty((D, D, T, B))
        else:
            flags |= 1           # SSMQ_PIPED_OUT_PINNED
        st = np.empty(B, dtype=np.int32)
        gqg, rr = self._noise()
        yc = np.ascontiguousarray(data)
        dp = _lib.dp
        rc = lib.ssmq_filter_forward_piped(*pair, B, T, dp(yc), dp(m0), dp(P0), dp(gqg), dp(rr), ctypes.c_void_p(fm.ctypes.data),
                                           ctypes.c_void_p(fP.ctypes.data), ctypes.c_void_p(st.ctypes.data), flags, 0)
        if rc == -3:             # SSMQ_E_UNSUPPORTED
            return None
        _lib.check(rc, 'ssmq_filter_forward_piped')
        self.status = st
        if raise_on_failure:
            _raise_failed(st)
        self.fi_mean, self.fi_cov = fm, fP
        return fm, fP

    def forward_pass_batch(self, data, x0_mean=None, x0_cov=None, raise_on_failure=True, smooth=False):
        """data (dim_y, T, B).  Optional per-trajectory initial moments x0_mean (B, D), x0_cov (B, D, D)."""
        if smooth and (is_user_model(self.mod_dyn) or is_user_model(self.mod_obs)):
            raise user_unsupported('the RTS smoother (backward_pass)')
        self._check_user_points()
        lib = _lib.load()
        data = np.asarray(data, dtype=np.float64)
        self._data = data
        Y, T, B = data.shape
        D = self.mod_dyn.dim_state
        ld = _lib.padded(B)
        if not smooth and self._additive and B > 0 and T > 0:
            done = self._forward_pass_piped(lib, data, x0_mean, x0_cov, raise_on_failure)
            if done is not None:
                return done
        with _lib.Staging() as stage:
            # (dim_y, T, B) -> planes [T][Y][ld]: a row permutation, done between the caller's array and the library's pinned
            # staging block (`ssmq_upload_planes`)
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_m0, d_P0 = self._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d_fm, d_fP, d_st = stage.scratch(8 * T * D * ld), stage.scratch(8 * T * D * D * ld), stage.scratch(4 * ld)
            if smooth:
                d_sm, d_sP = stage.scratch(8 * T * D * ld), stage.scratch(8 * T * D * D * ld)
                self._launch_smooth(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_sm, d_sP, d_st)
                self.sm_mean = _lib.download_study(d_sm, (D,), T, B, ld)
                self.sm_cov = _lib.download_study(d_sP, (D, D), T, B, ld)
            else:
                self._launch(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st)
            fm = _lib.download_study(d_fm, (D,), T, B, ld)       # planes [T][D][ld] -> (D, T, B), via pinned staging
            fP = _lib.download_study(d_fP, (D, D), T, B, ld)
            self.status = d_st.download((ld,), dtype=np.int32)[:B]
        if raise_on_failure:
            _raise_failed(self.status)
        self.fi_mean, self.fi_cov = fm, fP
        return self.fi_mean, self.fi_cov

    # ---- innovation scores: what a filter run on measurements alone can be judged by -------------------------------------------
    def _innovations_refusal(self):
        """None, or the NotImplementedError of a filter outside the range of the innovation scores (additive-noise Gaussian
        recursion)."""
        if not self._additive:
            return NotImplementedError('innovation scores cover the additive-noise Gaussian recursion; not implemented for models '
                                       'that take their noise as an argument (non-additive noise)')
        return None

    def _additive_gauss_only(self, what='innovation scores cover'):
        """Raises what keeps a filter out of the passes that cover the range of the innovation scores (`what` names the pass) -
        before the library is touched."""
        err = self._innovations_refusal()
        if err is not None:
            raise NotImplementedError(str(err).replace('innovation scores cover', what))

    def innovations_kernel_name(self, batch=0):
        """Which kernel(s) `innovations_*` run for this filter: k_innovation<..> (all T B items in one launch) where the fused time
        loop has an instantiation, and for user models; else the launch loop apply dyn | apply obs | k_innovation_score."""
        self._additive_gauss_only()
        self._check_user_points()
        return self._kernel_name('ssmq_innovations_kernel_name', int(batch))

    def _launch_innovations(self, lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_ym, d_S, d_nis, d_ll, d_tot, d_st):
        gqg, rr = self._noise()
        vp, dp = _lib.vp, _lib.dp
        _lib.check(lib.ssmq_filter_innovations_dev(*self._pair(), B, ld, T, vp(d_y), vp(d_m0), vp(d_P0), vp(d_fm), vp(d_fP), dp(gqg),
                                                   dp(rr), vp(d_ym), vp(d_S), vp(d_nis), vp(d_ll), vp(d_tot), vp(d_st)),
                   'ssmq_filter_innovations_dev')

    def innovations_dev(self, d_y, d_fm, d_fP, B, ld, T):
        """Innovation scores of a pass whose measurements and filtered moments are on the device (what `ssmod.simulate_dev` /
        `forward_pass_dev` return): DeviceBuffers (d_nis [T][ld], d_ll [T][ld], d_total [2][ld]: sum of the log-likelihoods and mean
        NIS of every trajectory, d_status [ld] int32: 1 + the first step whose scores are NaN, or 0); the caller frees them.  Every
        trajectory starts from the model's initial moments, as in `forward_pass_dev`."""
        self._additive_gauss_only()
        self._check_user_points()
        lib = _lib.load()
        with _lib.Staging() as stage:
            d_m0, d_P0 = self._initial_planes(stage, B, ld)
            d_nis, d_ll = stage.device(8 * T * ld), stage.device(8 * T * ld)
            d_tot, d_st = stage.device(8 * 2 * ld), stage.device(4 * ld)
            self._launch_innovations(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, None, None, d_nis, d_ll, d_tot, d_st)
            _lib.sync()
            return stage.release(d_nis, d_ll, d_tot, d_st)

    def innovations_batch(self, data, x0_mean=None, x0_cov=None, fi_mean=None, fi_cov=None, return_moments=False):
        """Normalised innovation squared and measurement log-likelihood of every step, data (dim_y, T, B): with (m, P) the initial
        moments for k = 0, else the filtered moments of step k - 1,
            y_mean, S = predictive measurement moments of step k;  e = y_k - y_mean;
            nis[k] = e' S^-1 e;  loglik[k] = log N(y_k | y_mean, S) = log p(y_k | y_1..k-1).
        fi_mean (D, T, B) / fi_cov (D, D, T, B): the filtered moments of `data` (both or neither); without them
        `forward_pass_batch(data, x0_mean, x0_cov, raise_on_failure=False)` runs first.  Returns a dict: nis (T, B), loglik (T, B),
        loglik_total (B,), nis_mean (B,), status (B,) - 1 + the first step whose scores are NaN (the filter failed there or
        earlier, or a covariance is not positive definite), 0 if none; with return_moments also y_mean (dim_y, T, B) and y_cov
        (dim_y, dim_y, T, B)."""
        self._additive_gauss_only()
        if (fi_mean is None) != (fi_cov is None):
            raise ValueError('innovations_batch: give fi_mean and fi_cov, or neither')
        self._check_user_points()
        data = np.asarray(data, dtype=np.float64)
        if fi_mean is None:
            fi_mean, fi_cov = self.forward_pass_batch(data, x0_mean=x0_mean, x0_cov=x0_cov, raise_on_failure=False)
        lib = _lib.load()
        Y, T, B = data.shape
        D = self.mod_dyn.dim_state
        ld = _lib.padded(B)
        with _lib.Staging() as stage:
            d_y, d_fm, d_fP = stage.scratch(8 * T * Y * ld), stage.scratch(8 * T * D * ld), stage.scratch(8 * T * D * D * ld)
            _lib.upload_study(data, Y, ld, d_y)
            _lib.upload_study(np.asarray(fi_mean, dtype=np.float64).reshape(D, T, B), D, ld, d_fm)
            _lib.upload_study(np.asarray(fi_cov, dtype=np.float64).reshape(D * D, T, B), D * D, ld, d_fP)
            d_m0, d_P0 = self._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d_nis, d_ll, d_tot, d_st = stage.scratch(8 * T * ld), stage.scratch(8 * T * ld), stage.scratch(8 * 2 * ld), stage.scratch(4 * ld)
            d_ym = stage.scratch(8 * T * Y * ld) if return_moments else None
            d_S = stage.scratch(8 * T * Y * Y * ld) if return_moments else None
            self._launch_innovations(lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_ym, d_S, d_nis, d_ll, d_tot, d_st)
            out = {'nis': _lib.download_study(d_nis, (), T, B, ld), 'loglik': _lib.download_study(d_ll, (), T, B, ld)}
            tot = d_tot.download((2, ld))
            out['loglik_total'], out['nis_mean'] = tot[0, :B].copy(), tot[1, :B].copy()
            out['status'] = d_st.download((ld,), dtype=np.int32)[:B]
            if return_moments:
                out['y_mean'] = _lib.download_study(d_ym, (Y,), T, B, ld)
                out['y_cov'] = _lib.download_study(d_S, (Y, Y), T, B, ld)
        return out

    def innovations(self, data):
        """`innovations_batch` for one trajectory, data (dim_y, T): nis (T,), loglik (T,), loglik_total, nis_mean, status."""
        out = self.innovations_batch(np.asarray(data)[..., None])
        return {k: (v[..., 0] if v.ndim else v) for k, v in out.items()}

    # ---- noise sweeps: Q, R and P0 per row by measurement likelihood, the weights shared (`ssmq_filter_noise_sweep_dev`) ----------
    def _noise_sweep_setup(self, q_cov, r_cov, x0_cov):
        """The refusals of the noise sweeps that need no library - the class, the models, the noise, the kind of transform, D and Y -
        and the row arrays of the C entry point: G Q_p G', R_p and m0 | P0_p, each (rows, size) with rows = P for a stack and 1 for a
        shared matrix (stride 0).  Whether the pair of models and the point counts have a kernel is the table's to say: the C entry
        point answers that (NotImplementedError as well, after the library is loaded)."""
        from .ssmod import GaussRV
        what = _NOISE_SWEEP_RANGE
        if self._recursion != 'gauss':
            raise NotImplementedError(what + '; not implemented for the Studentian recursion ({})'.format(type(self).__name__))
        if isinstance(self, MarginalInference):
            raise NotImplementedError(what + '; not implemented for the marginalised filters ({})'.format(type(self).__name__))
        if is_user_model(self.mod_dyn) or is_user_model(self.mod_obs):
            raise NotImplementedError(what + '; not implemented for user models (device_code)')
        if not self._additive:
            raise NotImplementedError(what + '; not implemented for models that take their noise as an argument (non-additive noise)')
        for rv in (self.mod_dyn.init_rv, self.mod_dyn.noise_rv, self.mod_obs.noise_rv):
            if not isinstance(rv, GaussRV):
                raise NotImplementedError(what + '; not implemented for {}'.format(type(rv).__name__))
        families = ((UnscentedTransform, SphericalRadialTransform, GaussHermiteTransform), (GaussianProcessTransform, BayesSardTransform),
                    (StudentTProcessTransform,))
        family = [[type(tf) in fam for fam in families] for tf in (self.tf_dyn, self.tf_obs)]
        if not any(family[0]) or family[0] != family[1]:
            raise NotImplementedError(what + '; not implemented for the pair of transforms {} / {} (the extended, Taylor-GPQD, GPQ+D, '
                                      'truncated, multi-output, Monte-Carlo and fully-symmetric Student transforms have no sweep, and both '
                                      'transforms are of one form)'.format(type(self.tf_dyn).__name__, type(self.tf_obs).__name__))
        D, Y = self.mod_dyn.dim_state, self.mod_obs.dim_out
        if D > 6 or Y > 4:
            raise NotImplementedError(what + '; got D = {}, Y = {}'.format(D, Y))
        q, qs = _cov_rows(q_cov, self.q_cov, 'q_cov')
        r, rs = _cov_rows(r_cov, self.r_cov, 'r_cov')
        x, xs = _cov_rows(x0_cov, self._initial_cov(), 'x0_cov')
        stacks = [a.shape[0] for a, s in ((q, qs), (r, rs), (x, xs)) if s]
        if not stacks or len(set(stacks)) != 1:
            raise ValueError('noise sweep: at least one of q_cov, r_cov, x0_cov is a stack (P, n, n), and all stacks have the same P; got '
                             'leading axes {}'.format(stacks))
        G = self.G
        # row p: the very expression of `_noise`, so that a row can have the bits of the two-call path
        gqg = np.ascontiguousarray([np.ascontiguousarray(G.dot(qp).dot(G.T), dtype=np.float64).ravel() for qp in q], dtype=np.float64)
        rr = np.ascontiguousarray([np.ascontiguousarray(rp, dtype=np.float64).ravel() for rp in r], dtype=np.float64)
        m0 = np.ascontiguousarray(self.x0_mean, dtype=np.float64).ravel()
        x0 = np.ascontiguousarray([np.concatenate((m0, np.ascontiguousarray(xp, dtype=np.float64).ravel())) for xp in x], dtype=np.float64)
        return dict(P=stacks[0], D=D, Y=Y, gqg=gqg, rr=rr, x0=x0, q=q, r=r)

    def noise_sweep_kernel_name(self, P=1):
        """Which kernel `noise_sweep_*` run for this filter (the same for every number of rows P)."""
        self._noise_sweep_setup(noise_grid(self.q_cov, np.ones(int(P))), None, None)
        return self._kernel_name('ssmq_filter_noise_sweep_kernel_name', 0, unsupported=True)

    def _noise_sweep_launch(self, stage, s, d_y, B, ld, T, steps, device):
        alloc = stage.device if device else stage.scratch
        P = s['P']
        d_tot, d_nis, d_st = alloc(8 * P * ld), alloc(8 * P * ld), alloc(4 * P * ld)
        d_ll = alloc(8 * P * T * ld) if steps else None
        vp, dp = _lib.vp, _lib.dp
        rows = []
        for a in (s['gqg'], s['rr'], s['x0']):
            rows += [dp(a), a.shape[1] if a.shape[0] > 1 else 0]
        _lib.check(_lib.load().ssmq_filter_noise_sweep_dev(*self._pair(), 0, B, ld, T, vp(d_y), P, *rows, vp(d_tot), vp(d_nis), vp(d_ll),
                                                           vp(d_st)), 'ssmq_filter_noise_sweep_dev', True)
        return d_tot, d_nis, d_ll, d_st

    def noise_sweep_dev(self, d_y, B, ld, T, q_cov=None, r_cov=None, x0_cov=None, steps=False):
        """`noise_sweep_batch` on measurements that are already on the device (planes [T][dim_y][ld], ld a multiple of 64):
        DeviceBuffers d_loglik_total [P][ld], d_nis_mean [P][ld], d_loglik [P][T][ld] (None without `steps`), d_status [P][ld] int32;
        the caller frees them.  Every trajectory of row p starts from (x0_mean, x0_cov[p])."""
        s = self._noise_sweep_setup(q_cov, r_cov, x0_cov)
        if ld % 64 or ld < B:
            raise ValueError('noise sweep: ld is a multiple of 64 and at least B')
        with _lib.Staging() as stage:
            bufs = self._noise_sweep_launch(stage, s, d_y, B, ld, T, steps, True)
            stage.release(*[b for b in bufs if b is not None])
        return bufs

    def noise_sweep_batch(self, data, q_cov=None, r_cov=None, x0_cov=None, steps=False):
        """The measurement likelihood of `data` (dim_y, T, B) under P rows of noise covariances, in one kernel launch that stores no
        filtered moment (k_noise_sweep<>).  Each of q_cov (process noise, the dimension of `noise_rv`), r_cov (measurement noise) and
        x0_cov (initial state) is None - the model's own -, one matrix shared by all rows, or a stack (P, n, n); at least one is a
        stack and all stacks have the same P (ValueError otherwise, and for a row that is not finite or not symmetric, naming the
        row).  Positive definiteness is not checked here: an indefinite row fails on the device and shows in `status`.

        Row p is `type(self)` on the same models with noise_rv.cov = q_cov[p], r_cov[p] and initial covariance x0_cov[p], and the
        weights this object has now; its scores are that filter's forward_pass_batch followed by innovations_batch, computed by the
        dense kernels.  Returns a dict: loglik_total (P, B) = sum_k log p(y_k | y_1..k-1) under row p, nis_mean (P, B), status (P, B)
        int32 (0, or 1 + the first step whose scores are not numbers; the totals of such an item are NaN), and with `steps` loglik
        (P, T, B).  Touches neither fi_mean / fi_cov / status nor the weights.  Range: see `_NOISE_SWEEP_RANGE`.  A filter class, a
        kind of model, noise or transform, or a D or Y outside it raises NotImplementedError before the library is loaded; a built-in
        additive-noise pair of models or a point count for which the fused time loop has no instantiation passes those checks and is
        refused by the library's table - NotImplementedError too, but after the library is loaded."""
        return self._noise_sweep_run(self._noise_sweep_setup(q_cov, r_cov, x0_cov), data, steps)

    def _noise_sweep_run(self, s, data, steps):
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 3 or data.shape[0] != s['Y']:
            raise ValueError('noise sweep: data is (dim_y, T, B)')
        Y, T, B = data.shape
        if B < 1 or T < 1:
            raise ValueError('noise sweep: data holds at least one step of at least one trajectory')
        ld, P = _lib.padded(B), s['P']
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_tot, d_nis, d_ll, d_st = self._noise_sweep_launch(stage, s, d_y, B, ld, T, steps, False)
            out = {'loglik_total': d_tot.download((P, ld))[:, :B].copy(), 'nis_mean': d_nis.download((P, ld))[:, :B].copy(),
                   'status': d_st.download((P, ld), dtype=np.int32)[:, :B].copy()}
            if steps:
                out['loglik'] = d_ll.download((P, T, ld))[:, :, :B].copy()
        return out

    def fit_noise_covariances(self, data, q_cov=None, r_cov=None, x0_cov=None):
        """The row of `noise_sweep_batch` with the largest measurement likelihood: (index, q_cov[index], r_cov[index], table) with
        table[p] the sum of loglik_total[p] over the trajectories on which every row succeeded (`fit_table`); an argument that is
        shared (or None: the model's own) is returned as it is."""
        s = self._noise_sweep_setup(q_cov, r_cov, x0_cov)
        out = self._noise_sweep_run(s, data, False)
        index, table = fit_table(out['loglik_total'], out['status'], np.zeros(s['P'], dtype=np.int32))
        q, r = (rows[index if len(rows) > 1 else 0].copy() for rows in (s['q'], s['r']))      # (one row: shared by all)
        return index, q, r, table

    # ---- interacting multiple-model filter over noise modes: M rows of a noise sweep coupled every step (`ssmq_filter_imm_dev`) ---
    def _imm_setup(self, pi, mu0, q_cov, r_cov, x0_cov, x0_mean):
        """The refusals of the IMM pass that need no library - those of the noise sweeps (`_noise_sweep_setup`, naming the range),
        then the mode count and the probabilities (`_mode_probabilities`) - and the arrays of the C entry point.  The modes are the
        rows of a noise sweep: at least one of q_cov, r_cov, x0_cov is a stack (M, n, n), or M = 1 and none is."""
        pi_shape = np.shape(pi)
        M = pi_shape[0] if len(pi_shape) == 2 else 0
        stacked = any(a is not None and np.ndim(a) == 3 for a in (q_cov, r_cov, x0_cov))
        if not stacked and M == 1:     # one mode, nothing varied: a stack of one row of the model's own process noise
            q_cov = np.atleast_2d(np.asarray(self.q_cov if q_cov is None else q_cov, dtype=np.float64))[None]
        try:
            s = self._noise_sweep_setup(q_cov, r_cov, x0_cov)
        except NotImplementedError as e:
            raise NotImplementedError('IMM over noise modes has the range of the noise sweeps: ' + str(e)) from None
        pi, mu0 = _mode_probabilities(pi, mu0)
        if s['P'] != pi.shape[0]:
            raise ValueError('IMM: the stacks of q_cov / r_cov / x0_cov have {} rows and pi has M = {}'.format(s['P'], pi.shape[0]))
        if x0_mean is not None:
            x0_mean = np.asarray(x0_mean, dtype=np.float64)
            D = s['D']
            if x0_mean.shape not in ((D,), (s['P'], D)) or not np.isfinite(x0_mean).all():
                raise ValueError('IMM: x0_mean is None, one finite ({0},) vector or a stack (M, {0})'.format(D))
            rows = np.broadcast_to(s['x0'], (s['P'] if x0_mean.ndim == 2 else s['x0'].shape[0], D + D * D)).copy()
            rows[:, :D] = x0_mean
            s['x0'] = np.ascontiguousarray(rows)
        s.update(M=pi.shape[0], pi=pi, mu0=mu0)
        return s

    def imm_kernel_name(self, M=1):
        """Which kernel `imm_pass*` run for this filter (the same for every number of modes M)."""
        self._imm_setup(mode_transition(int(M), 0.9), None, noise_grid(self.q_cov, np.ones(int(M))), None, None, None)
        return self._kernel_name('ssmq_filter_imm_kernel_name', 0, unsupported=True)

    def _imm_launch(self, stage, s, d_y, B, ld, T, device):
        alloc = stage.device if device else stage.scratch
        D, M = s['D'], s['M']
        d_fm, d_fP, d_mp = alloc(8 * T * D * ld), alloc(8 * T * D * D * ld), alloc(8 * T * M * ld)
        d_ll, d_tot, d_st = alloc(8 * T * ld), alloc(8 * ld), alloc(4 * ld)
        vp, dp = _lib.vp, _lib.dp
        rows = []
        for a in (s['gqg'], s['rr'], s['x0']):
            rows += [dp(a), a.shape[1] if a.shape[0] > 1 else 0]
        _lib.check(_lib.load().ssmq_filter_imm_dev(*self._pair(), 0, B, ld, T, vp(d_y), M, *rows, dp(s['pi']), dp(s['mu0']), vp(d_fm), vp(d_fP),
                                                   vp(d_mp), vp(d_ll), vp(d_tot), vp(d_st)), 'ssmq_filter_imm_dev', True)
        return d_fm, d_fP, d_mp, d_ll, d_tot, d_st

    def imm_pass_dev(self, d_y, B, ld, T, pi, mu0=None, q_cov=None, r_cov=None, x0_cov=None, x0_mean=None):
        """`imm_pass_batch` on measurements that are already on the device (planes [T][dim_y][ld], ld a multiple of 64):
        DeviceBuffers d_fm [T][D][ld], d_fP [T][D*D][ld], d_mode_prob [T][M][ld], d_loglik [T][ld], d_loglik_total [ld], d_status [ld]
        int32; the caller frees them."""
        s = self._imm_setup(pi, mu0, q_cov, r_cov, x0_cov, x0_mean)
        if ld % 64 or ld < B:
            raise ValueError('IMM: ld is a multiple of 64 and at least B')
        with _lib.Staging() as stage:
            bufs = self._imm_launch(stage, s, d_y, B, ld, T, True)
            stage.release(*bufs)
        return bufs

    def imm_pass_batch(self, data, pi, mu0=None, q_cov=None, r_cov=None, x0_cov=None, x0_mean=None, raise_on_failure=True):
        """Interacting multiple-model filter (Blom & Bar-Shalom 1988) over M noise modes of this filter on `data` (dim_y, T, B), the
        whole pass in one kernel launch (k_imm_loop<>).  Mode j is `type(self)` on the same models and weights with noise_rv.cov =
        q_cov[j], r_cov[j], initial covariance x0_cov[j] and initial mean x0_mean[j]: each of q_cov / r_cov / x0_cov is None - the
        model's own -, one matrix shared by all modes, or a stack (M, n, n), as in `noise_sweep_batch`; at least one is a stack, or
        M = 1.  x0_mean: None, (D,) or (M, D).  pi (M, M): pi[i][j] the probability of going from mode i to mode j (`mode_transition`);
        mu0 (M,): the initial mode probabilities, None = uniform.  Rows of pi and mu0 sum to 1 within 1e-12 (ValueError naming the
        row); 1 <= M <= 8.

        Every step the modes' moments are mixed by the Markov probabilities, each mode runs its filter step, the modes are weighted
        by their measurement likelihood, and the combined moments are stored (the steps: include/ssmq.h, ssmq_filter_imm_dev).
        Returns a dict: mean (D, T, B), cov (D, D, T, B), mode_prob (M, T, B), loglik (T, B) = log p(y_k | y_1..k-1), loglik_total (B,),
        status (B,) int32 - 1 + the first step at which a mode's scores or a mixed quantity is not a finite number (every output of
        that trajectory is NaN from there on), or 0.  Sets fi_mean / fi_cov / status as `forward_pass_batch` does and raises
        LinAlgError for a failed trajectory unless raise_on_failure is False.  Touches neither the weights nor the noise of the
        object.  Range: that of the noise sweeps (`_NOISE_SWEEP_RANGE`; NotImplementedError before the library is loaded)."""
        s = self._imm_setup(pi, mu0, q_cov, r_cov, x0_cov, x0_mean)
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 3 or data.shape[0] != s['Y']:
            raise ValueError('IMM: data is (dim_y, T, B)')
        Y, T, B = data.shape
        if B < 1 or T < 1:
            raise ValueError('IMM: data holds at least one step of at least one trajectory')
        ld, D, M = _lib.padded(B), s['D'], s['M']
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_fm, d_fP, d_mp, d_ll, d_tot, d_st = self._imm_launch(stage, s, d_y, B, ld, T, False)
            out = {'mean': _lib.download_study(d_fm, (D,), T, B, ld), 'cov': _lib.download_study(d_fP, (D, D), T, B, ld),
                   'mode_prob': _lib.download_study(d_mp, (M,), T, B, ld), 'loglik': _lib.download_study(d_ll, (), T, B, ld),
                   'loglik_total': d_tot.download((ld,))[:B].copy(), 'status': d_st.download((ld,), dtype=np.int32)[:B].copy()}
        self._data = data
        self.status = out['status']
        if raise_on_failure:
            _raise_failed(self.status, message='a mode\'s scores or a mixed moment is not a finite number (trajectory {}, step {})')
        self.fi_mean, self.fi_cov = out['mean'], out['cov']
        return out

    def imm_pass(self, data, pi, **kwargs):
        """`imm_pass_batch` for one trajectory, data (dim_y, T): mean (D, T), cov (D, D, T), mode_prob (M, T), loglik (T,),
        loglik_total, status."""
        out = self.imm_pass_batch(np.asarray(data)[..., None], pi, **kwargs)
        return {k: (v[..., 0] if v.ndim else v) for k, v in out.items()}

    # ---- iterated posterior linearisation (IPLF): J measurement updates per step, each re-linearised around the posterior ------
    def _iterated_refusal(self, iterations):
        """Raises what keeps a filter or an iteration count out of the iterated pass - before the library is touched."""
        self._additive_gauss_only('the iterated pass covers')
        return _iteration_count(iterations)

    def iterated_kernel_name(self, iterations, batch=0, launch_loop=False):
        """Which kernel(s) `iterated_pass*` run for this filter: k_iplf_loop<..> (the whole pass in one launch) where the fused time
        loop has an instantiation, and for user models; else the launch loop apply dyn | J x (apply obs | k_iplf_update)."""
        iterations = self._iterated_refusal(iterations)
        self._check_user_points()
        return self._kernel_name('ssmq_iterated_kernel_name', int(batch), iterations, _lib.ITERATED_LAUNCH_LOOP if launch_loop else 0)

    def _launch_iterated(self, lib, B, ld, T, iterations, flags, d_y, d_m0, d_P0, d_fm, d_fP, d_delta, d_st):
        gqg, rr = self._noise()
        vp, dp = _lib.vp, _lib.dp
        _lib.check(lib.ssmq_filter_iterated_dev(*self._pair(), B, ld, T, iterations, flags, vp(d_y), vp(d_m0), vp(d_P0), dp(gqg), dp(rr),
                                                vp(d_fm), vp(d_fP), vp(d_delta), vp(d_st)), 'ssmq_filter_iterated_dev')

    def iterated_pass_dev(self, d_y, B, ld, T, iterations, launch_loop=False):
        """`forward_pass_dev` with `iterations` re-linearised measurement updates per step: measurements on the device (planes
        [T][dim_y][ld]), results left there - DeviceBuffers (d_fm [T][D][ld], d_fP [T][D*D][ld], d_delta [T][ld], d_status [ld]);
        the caller frees them.  Every trajectory starts from the model's initial moments."""
        iterations = self._iterated_refusal(iterations)
        self._check_user_points()
        lib = _lib.load()
        D = self.mod_dyn.dim_state
        with _lib.Staging() as stage:
            d_m0, d_P0 = self._initial_planes(stage, B, ld)
            d_fm, d_fP = stage.device(8 * T * D * ld), stage.device(8 * T * D * D * ld)
            d_delta, d_st = stage.device(8 * T * ld), stage.device(4 * ld)
            self._launch_iterated(lib, B, ld, T, iterations, _lib.ITERATED_LAUNCH_LOOP if launch_loop else 0, d_y, d_m0, d_P0, d_fm,
                                  d_fP, d_delta, d_st)
            _lib.sync()
            return stage.release(d_fm, d_fP, d_delta, d_st)

    def iterated_pass_batch(self, data, iterations, x0_mean=None, x0_cov=None, raise_on_failure=True, return_delta=False,
                            launch_loop=False):
        """The forward pass with the iterated posterior linearisation update (IPLF; the iterated EKF for `ExtendedKalman`), data
        (dim_y, T, B): per step the time update of `forward_pass_batch`, then `iterations` measurement updates of the PRIOR, each
        with the measurement moments taken around the current posterior (m_0, P_0 = the prior):
            y^, S_y, C = tf_obs(m_i, P_i);  A = C P_i^-1;  b = y^ - A m_i;  Omega = S_y - A P_i A';  S = A P- A' + Omega + R;
            K = P- A' S^-1;  m_{i+1} = m- + K (y - A m- - b);  P_{i+1} = P- - K S K'.
        iterations = 1 is the plain filter up to rounding.  Returns and sets fi_mean (D, T, B), fi_cov (D, D, T, B) and `status` as
        the forward pass does; with return_delta also delta (T, B) = max_d |m_J - m_{J-1}| / sqrt(P_J[d, d]), the convergence
        diagnostic (the iteration count is fixed: there is no stopping rule).  launch_loop=True forces the launch-loop route."""
        iterations = self._iterated_refusal(iterations)
        self._check_user_points()
        lib = _lib.load()
        data = np.asarray(data, dtype=np.float64)
        Y, T, B = data.shape
        D = self.mod_dyn.dim_state
        ld = _lib.padded(B)
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_m0, d_P0 = self._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d_fm, d_fP = stage.scratch(8 * T * D * ld), stage.scratch(8 * T * D * D * ld)
            d_delta, d_st = stage.scratch(8 * T * ld), stage.scratch(4 * ld)
            self._launch_iterated(lib, B, ld, T, iterations, _lib.ITERATED_LAUNCH_LOOP if launch_loop else 0, d_y, d_m0, d_P0, d_fm,
                                  d_fP, d_delta, d_st)
            fm = _lib.download_study(d_fm, (D,), T, B, ld)
            fP = _lib.download_study(d_fP, (D, D), T, B, ld)
            delta = _lib.download_study(d_delta, (), T, B, ld)
            self.status = d_st.download((ld,), dtype=np.int32)[:B]
        if raise_on_failure:
            _raise_failed(self.status)
        self.fi_mean, self.fi_cov = fm, fP
        return (fm, fP, delta) if return_delta else (fm, fP)

    def iterated_pass(self, data, iterations):
        """`iterated_pass_batch` for one trajectory, data (dim_y, T) -> filtered means (D, T), covariances (D, D, T)."""
        fm, fP = self.iterated_pass_batch(np.asarray(data)[..., None], iterations)
        return fm[..., 0], fP[..., 0]

    # ---- outlier-robust measurement update: Student-t measurement noise, the weight lambda_k found by a fixed point per step -----
    def _robust_refusal(self, dof, iterations, r_scale):
        """(dof, iterations, R) of a robust pass, or what keeps a filter or an argument out of it - before the library is touched.
        r_scale=None: the scale of a `StudentRV` measurement noise, the covariance of a `GaussRV`; dof=None: the `StudentRV`'s."""
        self._additive_gauss_only('the robust pass covers')
        from .ssmod import StudentRV
        iterations = _iteration_count(iterations)
        rv = self.mod_obs.noise_rv
        if dof is None:
            if not isinstance(rv, StudentRV):
                raise ValueError('robust pass: the measurement noise is not a StudentRV, so `dof` must be given')
            dof = rv.dof
        dof = float(dof)
        if not (dof > 0.0 and np.isfinite(dof)):
            raise ValueError('robust pass: dof must be a positive finite number (got {!r})'.format(dof))
        if r_scale is None:
            r_scale = rv.scale if isinstance(rv, StudentRV) else rv.cov
        Y = self.mod_obs.dim_out
        R = np.ascontiguousarray(np.atleast_2d(np.asarray(r_scale, dtype=np.float64)))
        if R.shape != (Y, Y) or not np.isfinite(R).all() or not np.array_equal(R, R.T):
            raise ValueError('robust pass: r_scale must be a finite symmetric ({0}, {0}) matrix'.format(Y))
        try:
            np.linalg.cholesky(R)
        except np.linalg.LinAlgError:
            raise ValueError('robust pass: r_scale is not positive definite') from None
        return dof, iterations, R

    def robust_kernel_name(self, iterations, batch=0, launch_loop=False):
        """Which kernel(s) `robust_pass*` run for this filter: k_robust_loop<..> (the whole pass in one launch) where the fused time
        loop has an instantiation, and for user models; else the launch loop apply dyn | apply obs | k_robust_update."""
        self._additive_gauss_only('the robust pass covers')
        iterations = _iteration_count(iterations)
        self._check_user_points()
        return self._kernel_name('ssmq_robust_kernel_name', int(batch), iterations, _lib.ROBUST_LAUNCH_LOOP if launch_loop else 0)

    def _launch_robust(self, lib, B, ld, T, dof, iterations, R, flags, d_y, d_m0, d_P0, d_fm, d_fP, d_lam, d_delta, d_st):
        gqg, _ = self._noise()
        vp, dp = _lib.vp, _lib.dp
        _lib.check(lib.ssmq_filter_robust_dev(*self._pair(), B, ld, T, iterations, flags, vp(d_y), vp(d_m0), vp(d_P0), dp(gqg), dp(R), dof,
                                              vp(d_fm), vp(d_fP), vp(d_lam), vp(d_delta), vp(d_st)), 'ssmq_filter_robust_dev')

    def robust_pass_dev(self, d_y, B, ld, T, dof=None, iterations=5, r_scale=None, launch_loop=False):
        """`forward_pass_dev` with the outlier-robust measurement update: measurements on the device (planes [T][dim_y][ld]), results
        left there - DeviceBuffers (d_fm [T][D][ld], d_fP [T][D*D][ld], d_lam [T][ld], d_delta [T][ld], d_status [ld]); the caller
        frees them.  Every trajectory starts from the model's initial moments."""
        dof, iterations, R = self._robust_refusal(dof, iterations, r_scale)
        self._check_user_points()
        lib = _lib.load()
        D = self.mod_dyn.dim_state
        with _lib.Staging() as stage:
            d_m0, d_P0 = self._initial_planes(stage, B, ld)
            d_fm, d_fP = stage.device(8 * T * D * ld), stage.device(8 * T * D * D * ld)
            d_lam, d_delta, d_st = stage.device(8 * T * ld), stage.device(8 * T * ld), stage.device(4 * ld)
            self._launch_robust(lib, B, ld, T, dof, iterations, R, _lib.ROBUST_LAUNCH_LOOP if launch_loop else 0, d_y, d_m0, d_P0, d_fm,
                                d_fP, d_lam, d_delta, d_st)
            _lib.sync()
            return stage.release(d_fm, d_fP, d_lam, d_delta, d_st)

    def robust_pass_batch(self, data, dof=None, iterations=5, r_scale=None, x0_mean=None, x0_cov=None, raise_on_failure=True,
                          return_weights=False, launch_loop=False):
        """The forward pass with the variational outlier-robust measurement update (Agamennoni et al. 2012; Piche, Sarkka,
        Hartikainen 2012), data (dim_y, T, B).  The measurement noise is Student-t with scale matrix `r_scale` and `dof` degrees of
        freedom, r_k | lambda_k ~ N(0, R / lambda_k), lambda_k ~ Gamma(dof / 2, dof / 2).  Per step the time update of
        `forward_pass_batch`, one measurement transform at the prior (y^, P_h without noise, C; e = y_k - y^, lambda_0 = 1), then
        `iterations` - 1 rounds of the fixed point in measurement space
            S_i = P_h + R / lambda_i;  r^ = (R / lambda_i) S_i^-1 e;  Psi = r^ r^' + P_h - P_h S_i^-1 P_h;
            lambda_{i+1} = (dof + dim_y) / (dof + trace(R^-1 Psi))
        and one state update with the last weight: S = P_h + R / lambda, K = C' S^-1, m = m- + K e, P = P- - K S K'.
        iterations = 1 is the plain filter with R = r_scale, up to rounding.  r_scale=None: the scale of a `StudentRV` measurement
        noise, the covariance of a `GaussRV`; dof=None: the `StudentRV`'s (a ValueError for a `GaussRV`).  Returns and sets fi_mean
        (D, T, B), fi_cov (D, D, T, B) and `status` as the forward pass does; with return_weights also lam (T, B), the weight every
        update used - the outlier indicator, near 1 for an unsurprising measurement, towards 0 for an outlier - and delta (T, B) =
        |lambda_{J-1} - lambda_{J-2}| / lambda_{J-1}, the convergence diagnostic (the iteration count is fixed: there is no stopping
        rule).  Neither the weights of the transforms nor the noise of the filter are touched.  launch_loop=True forces the
        launch-loop route."""
        dof, iterations, R = self._robust_refusal(dof, iterations, r_scale)
        self._check_user_points()
        lib = _lib.load()
        data = np.asarray(data, dtype=np.float64)
        Y, T, B = data.shape
        D = self.mod_dyn.dim_state
        ld = _lib.padded(B)
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_m0, d_P0 = self._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d_fm, d_fP = stage.scratch(8 * T * D * ld), stage.scratch(8 * T * D * D * ld)
            d_lam, d_delta, d_st = stage.scratch(8 * T * ld), stage.scratch(8 * T * ld), stage.scratch(4 * ld)
            self._launch_robust(lib, B, ld, T, dof, iterations, R, _lib.ROBUST_LAUNCH_LOOP if launch_loop else 0, d_y, d_m0, d_P0, d_fm,
                                d_fP, d_lam, d_delta, d_st)
            fm = _lib.download_study(d_fm, (D,), T, B, ld)
            fP = _lib.download_study(d_fP, (D, D), T, B, ld)
            lam = _lib.download_study(d_lam, (), T, B, ld)
            delta = _lib.download_study(d_delta, (), T, B, ld)
            self.status = d_st.download((ld,), dtype=np.int32)[:B]
        if raise_on_failure:
            _raise_failed(self.status)
        self.fi_mean, self.fi_cov = fm, fP
        return (fm, fP, lam, delta) if return_weights else (fm, fP)

    def robust_pass(self, data, dof=None, iterations=5, r_scale=None, return_weights=False):
        """`robust_pass_batch` for one trajectory, data (dim_y, T) -> filtered means (D, T), covariances (D, D, T); with
        return_weights also lam (T,) and delta (T,)."""
        out = self.robust_pass_batch(np.asarray(data)[..., None], dof=dof, iterations=iterations, r_scale=r_scale,
                                     return_weights=return_weights)
        return tuple(v[..., 0] for v in out)

    # ---- missing and gated measurements: a bit mask of the observed components per step, a chi-square gate in front of the update ----
    def _masked_refusal(self, gate):
        """The gate table [dim_y + 1] of a masked pass (None: no gate), or what keeps a filter or a gate out of it - before the library
        is touched.  gate: None, a scalar (the threshold for every number of observed components) or a sequence of dim_y thresholds
        (for o = 1 .. dim_y observed components; `gate_thresholds`); every threshold a positive number or +inf."""
        self._additive_gauss_only('the masked pass covers')
        if gate is None:
            return None
        Y = self.mod_obs.dim_out
        g = np.asarray(gate, dtype=np.float64)
        if g.ndim == 0:
            g = np.full(Y, float(g))
        if g.shape != (Y,) or not np.all(g > 0.0):
            raise ValueError('masked pass: gate must be a positive number (or +inf) or {} of them, for o = 1 .. {} observed components'
                             .format(Y, Y))
        return np.ascontiguousarray(np.concatenate(([np.inf], g)))

    def _mask_words(self, mask, Y, T, B):
        """mask (dim_y, T, B) bool or (T, B) unsigned integers -> (T, B) uint32 words, bit i = component i observed."""
        m = np.asarray(mask)
        if m.dtype == np.bool_ and m.shape == (Y, T, B):
            return (m.astype(np.uint32) << np.arange(Y, dtype=np.uint32)[:, None, None]).sum(axis=0, dtype=np.uint32)
        if m.dtype.kind == 'u' and m.shape == (T, B):
            return np.ascontiguousarray(m & np.asarray((1 << Y) - 1, dtype=m.dtype), dtype=np.uint32)
        raise ValueError('masked pass: mask must be a bool array of shape {} or an unsigned-integer array of shape {} (got {} {})'
                         .format((Y, T, B), (T, B), m.dtype, m.shape))

    def masked_kernel_name(self, batch=0, launch_loop=False):
        """Which kernel(s) `masked_pass*` run for this filter: k_masked_loop<..> (the whole pass in one launch) where the fused time
        loop has an instantiation, and for user models; else the launch loop apply dyn | apply obs | k_masked_update."""
        self._additive_gauss_only('the masked pass covers')
        self._check_user_points()
        return self._kernel_name('ssmq_masked_kernel_name', int(batch), _lib.MASKED_LAUNCH_LOOP if launch_loop else 0)

    def _launch_masked(self, lib, B, ld, T, flags, gate, d_y, d_mask, d_m0, d_P0, d_fm, d_fP, d_used, d_nis, d_ll, d_st):
        gqg, rr = self._noise()
        vp, dp = _lib.vp, _lib.dp
        _lib.check(lib.ssmq_filter_masked_dev(*self._pair(), B, ld, T, flags, vp(d_y), vp(d_mask), vp(d_m0), vp(d_P0), dp(gqg), dp(rr),
                                              dp(gate), vp(d_fm), vp(d_fP), vp(d_used), vp(d_nis), vp(d_ll), vp(d_st)),
                   'ssmq_filter_masked_dev')

    def masked_pass_dev(self, d_y, B, ld, T, d_mask=None, gate=None, launch_loop=False):
        """`forward_pass_dev` with missing and gated measurements: measurements on the device (planes [T][dim_y][ld]), d_mask a
        DeviceBuffer of uint32 words [T][ld] (bit i: component i observed; what `ssmod.detection_mask_dev` returns) or None: NaN =
        missing.  Results left on the device - DeviceBuffers (d_fm [T][D][ld], d_fP [T][D*D][ld], d_used [T][ld] uint32, d_nis [T][ld],
        d_loglik [T][ld], d_status [ld] int32); the caller frees them.  Every trajectory starts from the model's initial moments."""
        gate = self._masked_refusal(gate)
        self._check_user_points()
        lib = _lib.load()
        D = self.mod_dyn.dim_state
        with _lib.Staging() as stage:
            d_m0, d_P0 = self._initial_planes(stage, B, ld)
            d_fm, d_fP = stage.device(8 * T * D * ld), stage.device(8 * T * D * D * ld)
            d_used, d_nis, d_ll, d_st = stage.device(4 * T * ld), stage.device(8 * T * ld), stage.device(8 * T * ld), stage.device(4 * ld)
            self._launch_masked(lib, B, ld, T, _lib.MASKED_LAUNCH_LOOP if launch_loop else 0, gate, d_y, d_mask, d_m0, d_P0, d_fm, d_fP,
                                d_used, d_nis, d_ll, d_st)
            _lib.sync()
            return stage.release(d_fm, d_fP, d_used, d_nis, d_ll, d_st)

    def masked_pass_batch(self, data, mask=None, gate=None, x0_mean=None, x0_cov=None, raise_on_failure=True, return_scores=False,
                          launch_loop=False):
        """The forward pass when not every component of y_k arrived, data (dim_y, T, B).  mask (dim_y, T, B) bool, or (T, B) unsigned
        integers (bit i: component i of y_k was observed); None: a NaN in `data` means not observed.  With o the number of observed
        components of a step and the subscript o their rows and columns, after the time update of `forward_pass_batch` and one
        measurement transform at the prior (y^, P_h without noise, C):
            S = P_h + R;  e = y_k - y^;  d2 = e_o' S_oo^-1 e_o;  ll = -(o log 2 pi + log det S_oo + d2) / 2     (both 0 for o = 0)
            take = (o > 0) and not (d2 > gate[o])
            take: K = C_o' S_oo^-1, m = m- + K e_o, P = P- - K S_oo K';  else m = m-, P = P- (bit for bit the prior).
        The value under a cleared mask bit is never read.  gate: None, one threshold for every o, or dim_y thresholds for o = 1 ..
        dim_y (`gate_thresholds`).  Returns and sets fi_mean (D, T, B), fi_cov (D, D, T, B) and `status` as the forward pass does;
        with return_scores a dict: fm, fP, used (dim_y, T, B) bool - the components the update applied, none where nothing was offered
        or the gate rejected -, nis (T, B) = d2 and loglik (T, B) = ll of the OFFERED components (rejected or not), loglik_total (B,),
        n_used (B,): the number of components used over the pass, and status.  A trajectory with an observed NaN component, or whose
        factorisation fails, is NaN from that step on (status = 1 + step).  Neither the weights of the transforms nor the noise of
        the filter are touched.  launch_loop=True forces the launch-loop route."""
        gate = self._masked_refusal(gate)
        data = np.asarray(data, dtype=np.float64)
        Y, T, B = data.shape
        words = None if mask is None else self._mask_words(mask, Y, T, B)
        self._check_user_points()
        lib = _lib.load()
        D = self.mod_dyn.dim_state
        ld = _lib.padded(B)
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_mask = None
            if words is not None:
                planes = np.zeros((T, ld), dtype=np.uint32)
                planes[:, :B] = words
                d_mask = stage.scratch(4 * T * ld)
                d_mask.upload(planes)
            d_m0, d_P0 = self._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d_fm, d_fP = stage.scratch(8 * T * D * ld), stage.scratch(8 * T * D * D * ld)
            d_used, d_nis, d_ll, d_st = stage.scratch(4 * T * ld), stage.scratch(8 * T * ld), stage.scratch(8 * T * ld), stage.scratch(4 * ld)
            self._launch_masked(lib, B, ld, T, _lib.MASKED_LAUNCH_LOOP if launch_loop else 0, gate, d_y, d_mask, d_m0, d_P0, d_fm, d_fP,
                                d_used, d_nis, d_ll, d_st)
            fm = _lib.download_study(d_fm, (D,), T, B, ld)
            fP = _lib.download_study(d_fP, (D, D), T, B, ld)
            if return_scores:
                uw = d_used.download((T, ld), dtype=np.uint32)[:, :B]
                nis = _lib.download_study(d_nis, (), T, B, ld)
                ll = _lib.download_study(d_ll, (), T, B, ld)
            self.status = d_st.download((ld,), dtype=np.int32)[:B]
        if raise_on_failure:
            _raise_failed(self.status)
        self.fi_mean, self.fi_cov = fm, fP
        if not return_scores:
            return fm, fP
        used = ((uw[None, :, :] >> np.arange(Y, dtype=np.uint32)[:, None, None]) & 1).astype(bool)
        return {'fm': fm, 'fP': fP, 'used': used, 'nis': nis, 'loglik': ll, 'loglik_total': ll.sum(axis=0),
                'n_used': used.sum(axis=(0, 1)), 'status': self.status}

    def masked_pass(self, data, mask=None, gate=None):
        """`masked_pass_batch` for one trajectory, data (dim_y, T), mask (dim_y, T) bool or (T,) unsigned integers -> filtered means
        (D, T), covariances (D, D, T)."""
        fm, fP = self.masked_pass_batch(np.asarray(data)[..., None], None if mask is None else np.asarray(mask)[..., None], gate)
        return fm[..., 0], fP[..., 0]

    # ---- iterated posterior linearisation smoother (IPLS): forward and backward sweep, re-linearised around the smoothed moments ----
    _IPLS_RANGE = ('the iterated smoother covers the additive-noise Gaussian filters with unscented or spherical-radial point sets '
                   '(sigma-point, GP and t-process quadrature) on the built-in model pairs of the fused time loop, and user models '
                   '(device_code) with 2 .. 2 D + 1 points')

    def _ipls_refusal(self, iterations):
        """Raises what keeps a filter or an iteration count out of the iterated smoother - before the library is touched."""
        self._additive_gauss_only('the iterated smoother covers')
        from .mtran import TruncatedSigmaPointTransform
        from .bq.bqmtran import _MultiOutputTransform
        for tf in (self.tf_dyn, self.tf_obs):
            for cls, what in ((LinearizationTransform, 'linearisation (the iterated extended Kalman smoother)'), (TaylorGPQDTransform, 'Taylor-GPQD'),
                              (GaussianProcessDerTransform, 'GPQ+D'), (TruncatedSigmaPointTransform, 'truncated'),
                              (_MultiOutputTransform, 'multi-output'), (GaussHermiteTransform, 'Gauss-Hermite')):
                if isinstance(tf, cls):
                    raise NotImplementedError('{}; not implemented for {} transforms'.format(self._IPLS_RANGE, what))
        return _iteration_count(iterations)

    def iterated_smoother_kernel_name(self, iterations):
        """Which kernel `iterated_smoother*` launches once per iteration for this filter: k_ipls_pass<..>."""
        iterations = self._ipls_refusal(iterations)
        self._check_user_points()
        return self._kernel_name('ssmq_smoother_iterated_kernel_name', iterations, unsupported=True)

    def _launch_ipls(self, lib, B, ld, T, iterations, d_y, d_m0, d_P0, d_lin_m, d_lin_P, outs):
        gqg, rr = self._noise()
        vp, dp = _lib.vp, _lib.dp
        # unsupported: the pair has no kernel (another point count, ...)
        _lib.check(lib.ssmq_smoother_iterated_dev(*self._pair(), B, ld, T, vp(d_y), vp(d_m0), vp(d_P0), dp(gqg), dp(rr), iterations, 0,
                                                  vp(d_lin_m), vp(d_lin_P), *[vp(b) for b in outs]), 'ssmq_smoother_iterated_dev',
                   unsupported=True)

    @staticmethod
    def _ipls_outputs(alloc, D, T, ld):
        """The eight outputs of `ssmq_smoother_iterated_dev`: d_fm, d_fP, d_sm, d_sP, d_sm0, d_sP0, d_delta, d_status."""
        return [alloc(n) for n in (8 * T * D * ld, 8 * T * D * D * ld, 8 * T * D * ld, 8 * T * D * D * ld, 8 * D * ld, 8 * D * D * ld,
                                   8 * ld, 4 * ld)]

    def iterated_smoother_dev(self, d_y, B, ld, T, iterations):
        """The iterated smoother on measurements that are already on the device (planes [T][dim_y][ld]), results left there:
        DeviceBuffers (d_fm [T][D][ld], d_fP [T][D*D][ld], d_sm, d_sP likewise, d_sm0 [D][ld], d_sP0 [D*D][ld], d_delta [ld], d_status
        [ld] int32); the caller frees them.  Every trajectory starts from the model's initial moments."""
        iterations = self._ipls_refusal(iterations)
        self._check_user_points()
        lib = _lib.load()
        with _lib.Staging() as stage:
            d_m0, d_P0 = self._initial_planes(stage, B, ld)
            outs = self._ipls_outputs(stage.device, self.mod_dyn.dim_state, T, ld)
            self._launch_ipls(lib, B, ld, T, iterations, d_y, d_m0, d_P0, None, None, outs)
            return stage.release(*outs)

    def iterated_smoother_batch(self, data, iterations=3, x0_mean=None, x0_cov=None, raise_on_failure=True, return_delta=False,
                                lin_mean=None, lin_cov=None):
        """The iterated posterior linearisation smoother (IPLS, Garcia-Fernandez, Svensson, Sarkka 2017), data (dim_y, T, B).  With
        x_{-1} ~ N(x0_mean, x0_cov) and step k = 0 .. T-1 (both transforms of step k use time index k), every iteration linearises
        the dynamics at (ml_{k-1}, Pl_{k-1}) and the measurement at (ml_k, Pl_k) by statistical linear regression, runs the affine
        Kalman filter and an RTS pass on the linearised model down to the initial state; iteration i > 1 takes the smoothed moments
        of iteration i - 1, iteration 1 `lin_mean` (D, T + 1, B) / `lin_cov` (D, D, T + 1, B) (column 0: the initial state) or,
        without them, its own running moments - so iterations = 1 is the plain filter and a properly indexed RTS smoother (the last
        smoothed step IS the filtered one; `backward_pass` keeps the reference's index quirk instead).
        Returns sm (D, T, B), sP (D, D, T, B) and with return_delta also delta (B,) = max_{k,d} |ms_k - ms_k of the iteration
        before| / sqrt(Ps_k[d, d]) (there is no stopping rule); sets sm_mean, sm_cov, fi_mean, fi_cov (the last iteration's filtered
        moments), sm_x0_mean (D, B), sm_x0_cov (D, D, B) and status (0, or 1 + the failing step of the first failing iteration: every
        output of that trajectory is NaN)."""
        iterations = self._ipls_refusal(iterations)
        self._check_user_points()
        if (lin_mean is None) != (lin_cov is None):
            raise ValueError('lin_mean and lin_cov come together')
        lib = _lib.load()
        data = np.asarray(data, dtype=np.float64)
        Y, T, B = data.shape
        D = self.mod_dyn.dim_state
        ld = _lib.padded(B)
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_m0, d_P0 = self._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d_lm = d_lP = None
            if lin_mean is not None:
                lin_mean, lin_cov = np.asarray(lin_mean, dtype=np.float64), np.asarray(lin_cov, dtype=np.float64)
                if lin_mean.shape != (D, T + 1, B) or lin_cov.shape != (D, D, T + 1, B):
                    raise ValueError('lin_mean (D, T + 1, B) and lin_cov (D, D, T + 1, B) expected')
                d_lm, d_lP = stage.scratch(8 * (T + 1) * D * ld), stage.scratch(8 * (T + 1) * D * D * ld)
                _lib.upload_study(lin_mean, D, ld, d_lm)
                _lib.upload_study(lin_cov.reshape(D * D, T + 1, B), D * D, ld, d_lP)
            outs = self._ipls_outputs(stage.scratch, D, T, ld)
            self._launch_ipls(lib, B, ld, T, iterations, d_y, d_m0, d_P0, d_lm, d_lP, outs)
            fm, fP = _lib.download_study(outs[0], (D,), T, B, ld), _lib.download_study(outs[1], (D, D), T, B, ld)
            sm, sP = _lib.download_study(outs[2], (D,), T, B, ld), _lib.download_study(outs[3], (D, D), T, B, ld)
            sm0 = outs[4].download((D, ld))[:, :B].copy()
            sP0 = outs[5].download((D, D, ld))[..., :B].copy()
            delta = outs[6].download((ld,))[:B].copy()
            self.status = outs[7].download((ld,), dtype=np.int32)[:B].copy()
        if raise_on_failure:
            _raise_failed(self.status)
        self.fi_mean, self.fi_cov, self.sm_mean, self.sm_cov = fm, fP, sm, sP
        self.sm_x0_mean, self.sm_x0_cov = sm0, sP0
        return (sm, sP, delta) if return_delta else (sm, sP)

    def iterated_smoother(self, data, iterations=3):
        """`iterated_smoother_batch` for one trajectory, data (dim_y, T) -> smoothed means (D, T), covariances (D, D, T)."""
        sm, sP = self.iterated_smoother_batch(np.asarray(data)[..., None], iterations)
        return sm[..., 0], sP[..., 0]


def run_filters(algs, data, x0_mean=None, x0_cov=None, raise_on_failure=True):
    """Several filters over the SAME measurements as one device launch - the loop `for alg in algs: alg.forward_pass(y)` of the
    reference's studies (research/bsq/bsq_ungm.py:132-137, research/tpq/tpq_base.py:175-192), for data of shape (dim_y, T, B).
    Returns [(fi_mean (D, T, B), fi_cov (D, D, T, B)), ...] in the order of `algs` and leaves `fi_mean / fi_cov / status` on
    every filter, exactly what `alg.forward_pass_batch(data)` would have produced (the same kernels run, concurrently:
    `ssmq_filter_forward_multi_dev`).  The filters must be additive-noise Gaussian / Studentian filters; they may differ in
    models and state dimension, the measurements are uploaded once."""
    lib = _lib.load()
    data = np.asarray(data, dtype=np.float64)
    Y, T, B = data.shape
    ld = _lib.padded(B)
    for a in algs:
        if isinstance(a, BootstrapParticleFilter):
            a._refuse('run_filters')
        if not isinstance(a, GaussianInference) or not a._additive:
            raise NotImplementedError('run_filters: additive-noise Gaussian / Studentian filters only')
        if isinstance(a, MultiOutputGaussianProcessKalman):
            raise NotImplementedError('run_filters: not implemented for the multi-output filter (its forward pass is a launch loop)')
        if isinstance(a, TruncatedInference):
            raise NotImplementedError('run_filters: not implemented for the truncated filters (their forward pass is a launch loop that '
                                      'ssmq_filter_forward_multi_dev refuses by name)')
        if isinstance(a, ExtendedKalmanGPQD):
            raise NotImplementedError('run_filters: not implemented for ExtendedKalmanGPQD (its forward pass is a launch loop that '
                                      'ssmq_filter_forward_multi_dev refuses by name)')
        if isinstance(a, GaussianProcessDerKalman):
            raise NotImplementedError('run_filters: not implemented for GaussianProcessDerKalman (its forward pass is a launch loop that '
                                      'ssmq_filter_forward_multi_dev refuses by name)')
        if a.mod_obs.dim_out != Y:
            raise ValueError('run_filters: every filter must take the same measurements')
    with _lib.Staging() as stage:
        d_y = stage.scratch(8 * T * Y * ld)
        _lib.upload_study(data, Y, ld, d_y)
        jobs = (_lib.FilterJob * len(algs))()
        keep, bufs = [], []
        for j, a in zip(jobs, algs):
            a._data = data
            D = a.mod_dyn.dim_state
            d_m0, d_P0 = a._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d_fm, d_fP, d_st = stage.scratch(8 * T * D * ld), stage.scratch(8 * T * D * D * ld), stage.scratch(4 * ld)
            bufs.append((d_fm, d_fP, d_st))
            h_dyn, f_dyn, h_obs, f_obs = a._pair()
            gqg, rr = a._noise()
            keep += [f_dyn, f_obs, gqg, rr]
            j.h_dyn, j.f_dyn, j.h_obs, j.f_obs = h_dyn, ctypes.pointer(f_dyn), h_obs, ctypes.pointer(f_obs)
            j.B, j.ld, j.T = B, ld, T
            j.d_y, j.d_m0, j.d_P0 = d_y.ptr, d_m0.ptr, d_P0.ptr
            j.GQG, j.R = _lib.dp(gqg), _lib.dp(rr)
            j.d_fm, j.d_fP, j.d_status = d_fm.ptr, d_fP.ptr, d_st.ptr
            if a._recursion == 'student':
                sc = np.ascontiguousarray(a.scale_sequence(T), dtype=np.float64)
                keep.append(sc)
                j.scale, j.dof = _lib.dp(sc), float(a.dof)
        _lib.check(lib.ssmq_filter_forward_multi_dev(len(algs), jobs), 'ssmq_filter_forward_multi_dev')
        out, failed = [], None
        for a, (d_fm, d_fP, d_st) in zip(algs, bufs):
            D = a.mod_dyn.dim_state
            a.fi_mean = _lib.download_study(d_fm, (D,), T, B, ld)
            a.fi_cov = _lib.download_study(d_fP, (D, D), T, B, ld)
            a.status = d_st.download((ld,), dtype=np.int32)[:B]
            if a.status.any() and failed is None:
                failed = a
            out.append((a.fi_mean, a.fi_cov))
    if raise_on_failure and failed is not None:
        _raise_failed(failed.status, prefix=type(failed).__name__ + ': ')
    return out


class CubatureKalman(GaussianInference):
    """ssinf.py:360-371."""

    def __init__(self, dyn, obs):
        super().__init__(dyn, obs, SphericalRadialTransform(dyn.dim_in), SphericalRadialTransform(obs.dim_in))


def _need_device_jacobians(what, dyn, obs):
    """The extended Kalman filters take a user model (device_code) that states its Jacobian (device_jacobian), no other."""
    for m in (dyn, obs):
        if is_user_model(m) and not has_device_jacobian(m):
            raise user_unsupported('{} (model Jacobians: {} has no device_jacobian)'.format(what, type(m).__name__))


class ExtendedKalman(GaussianInference):
    """Extended Kalman filter and smoother (ssinf.py:347-357): both transforms are linearisations around the mean.  Runs for
    the models whose Jacobians the reference implements (its own test skips the others: tests/test_ssinf.py:96-101) and for
    models of your own that have a `device_jacobian` next to their `device_code` (forward pass; a user model may be paired with
    a built-in one).  On a pair of built-in additive-noise models the whole time loop is one kernel (k_ekf_loop: forward pass,
    smoother, and as a member of `run_filters`; SSMQ_NO_EKF_LOOP=1 or SSMQ_NO_FUSED=1 switch it off).  Everything else - a pair with a
    user member, models that take their noise as an argument - runs the launch loop k_linearize | k_linearize | k_kalman_update per
    step, a user member's transform being the kernel compiled for it at run time (k_linearize_fn)."""

    def __init__(self, dyn, obs):
        _need_device_jacobians('ExtendedKalman', dyn, obs)
        super().__init__(dyn, obs, LinearizationTransform(dyn.dim_in), LinearizationTransform(obs.dim_in))


class ExtendedKalmanGPQD(GaussianInference):
    """Extended Kalman filter and smoother whose linearisations are calibrated by single-point Gaussian-process quadrature with
    derivative observations and an RBF kernel (ssinf.py:1302-1319): rbf_par_dyn (1, 1 + dim_in), rbf_par_obs (1, 1 + dim_state) =
    [alpha, ell_1 ..].  Runs where `ExtendedKalman` runs (the models with a Jacobian), on the same launch loop (k_taylor_gpqd |
    k_taylor_gpqd | k_kalman_update per step); additive-noise models only, built-in ones and models of your own that have a
    `device_jacobian` (their transforms run k_taylor_gpqd_fn, compiled at run time).  With this package's (E, D) cross-covariance it
    also runs for dim_y != dim_state, where the reference's own filter stops."""

    def __init__(self, dyn, obs, rbf_par_dyn, rbf_par_obs):
        _need_device_jacobians('ExtendedKalmanGPQD', dyn, obs)
        if not (dyn.noise_additive and obs.noise_additive):
            raise NotImplementedError('ExtendedKalmanGPQD runs for additive-noise models only')
        super().__init__(dyn, obs, TaylorGPQDTransform(dyn.dim_in, rbf_par_dyn), TaylorGPQDTransform(obs.dim_state, rbf_par_obs))


class UnscentedKalman(GaussianInference):
    """ssinf.py:374-402."""

    def __init__(self, dyn, obs, kappa=None, alpha=1.0, beta=2.0):
        super().__init__(dyn, obs, UnscentedTransform(dyn.dim_in, kappa=kappa, alpha=alpha, beta=beta),
                         UnscentedTransform(obs.dim_in, kappa=kappa, alpha=alpha, beta=beta))


class TruncatedInference(GaussianInference):
    """Base of the filters whose measurement update is aware of the effective dimension of the measurement model (ssinf.py:836-901;
    the reference calls them experimental): the time update is the plain transform of the rule, the measurement update the
    truncated one (`mtran.TruncatedSigmaPointTransform`) - measurement mean and covariance from the rule of dimension `dim_eff`,
    the state-measurement covariance from the rule of the full state dimension.

    `dim_eff` is this package's one deliberate departure from the reference: None (the default) means `obs.dim_substate`, the
    number of leading state entries the measurement model reads, which is what these classes promise.  The reference passes
    `obs.dim_in`, which equals `dim_state` for every additive-noise model there, so its three filters coincide with the UKF / CKF /
    GHKF (ssinf.py:859, 878, 900); `dim_eff=obs.dim_state` gives that behaviour.

    forward_pass / forward_pass_batch / forward_pass_dev and backward_pass / backward_pass_batch run as the captured launch loop
    (apply dyn | k_apply_trunc | k_kalman_update per step; the smoother's variant keeps the predictive moments).  Built-in models
    with additive noise; `run_filters` raises NotImplementedError for these classes."""

    def __init__(self, dyn, obs, tf_dyn_cls, tf_obs_cls, dim_eff, *rule_args):
        if is_user_model(dyn) or is_user_model(obs):
            raise user_unsupported('the truncated filters (built-in models)')
        if not (dyn.noise_additive and obs.noise_additive):
            raise NotImplementedError('{} runs for additive-noise models only'.format(type(self).__name__))
        self.dim_eff = int(obs.dim_substate if dim_eff is None else dim_eff)
        tf_obs = tf_obs_cls(obs.dim_state, self.dim_eff, *rule_args)
        tf_obs._device_integrand(obs.meas_eval)          # range and what the model reads: refused here, before the library is touched
        super().__init__(dyn, obs, tf_dyn_cls(dyn.dim_in, *rule_args), tf_obs)


class TruncatedUnscentedKalman(TruncatedInference):
    """Truncated unscented Kalman filter and smoother (ssinf.py:844-860); dim_eff=None: obs.dim_substate, see `TruncatedInference`."""

    def __init__(self, dyn, obs, kappa=None, alpha=1.0, beta=2.0, dim_eff=None):
        super().__init__(dyn, obs, UnscentedTransform, TruncatedUnscentedTransform, dim_eff, kappa, alpha, beta)


class TruncatedCubatureKalman(TruncatedInference):
    """Truncated cubature Kalman filter and smoother (ssinf.py:863-879); dim_eff=None: obs.dim_substate, see `TruncatedInference`."""

    def __init__(self, dyn, obs, dim_eff=None):
        super().__init__(dyn, obs, SphericalRadialTransform, TruncatedSphericalRadialTransform, dim_eff)


class TruncatedGaussHermiteKalman(TruncatedInference):
    """Truncated Gauss-Hermite Kalman filter and smoother (ssinf.py:882-901); dim_eff=None: obs.dim_substate, see
    `TruncatedInference`."""

    def __init__(self, dyn, obs, degree, dim_eff=None):
        super().__init__(dyn, obs, GaussHermiteTransform, TruncatedGaussHermiteTransform, dim_eff, degree)


class GaussHermiteKalman(GaussianInference):
    """ssinf.py:405-420."""

    def __init__(self, dyn, obs, deg=3):
        super().__init__(dyn, obs, GaussHermiteTransform(dyn.dim_in, degree=deg),
                         GaussHermiteTransform(obs.dim_in, degree=deg))


def par_grid(alphas, *ells):
    """The Cartesian grid of kernel-parameter rows [alpha, ell_1 .. ell_D]: alphas and one sequence per input dimension ->
    (P, 1 + D), the first axis varying slowest."""
    axes = [np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (alphas,) + ells]
    if any(a.ndim != 1 or a.size == 0 for a in axes):
        raise ValueError('par_grid: every argument is a non-empty one-dimensional sequence')
    mesh = np.meshgrid(*axes, indexing='ij')
    return np.ascontiguousarray(np.stack([m.ravel() for m in mesh], axis=1))


def fit_table(loglik_total, status, theta_status):
    """The bookkeeping of `fit_kernel_parameters`: loglik_total, status (P, B), theta_status (P,) -> (index, table).  table[p] sums
    row p over the trajectories on which EVERY row with theta_status == 0 succeeded (so the rows are comparable; NaN for a row
    whose weights failed); index is the argmax over the rows with theta_status == 0.  ValueError if no row or no trajectory is
    left."""
    ll, st, ts = np.asarray(loglik_total, dtype=np.float64), np.asarray(status), np.asarray(theta_status)
    rows = ts == 0
    if not rows.any():
        raise ValueError('fit_kernel_parameters: the weights of every parameter row failed')
    keep = ~(st[rows] != 0).any(axis=0)
    if not keep.any():
        raise ValueError('fit_kernel_parameters: no trajectory is left on which every parameter row succeeded')
    table = np.full(ll.shape[0], np.nan)
    table[rows] = ll[rows][:, keep].sum(axis=1)
    return int(np.flatnonzero(rows)[np.argmax(table[rows])]), table


class _LikelihoodSweep:
    """Kernel-parameter sweeps by measurement likelihood (`ssmq_filter_sweep_dev`, k_filter_sweep<>): the filter's recursion for P
    rows of kernel parameters on B measurement sequences in one launch that keeps only the scores.  Row p pairs par_dyn[p] with
    par_obs[p].  Range: the 'rbf' kernel, built-in additive-noise models with Gaussian noise, D <= 6, Y <= 4, at most 2 D + 1
    points.  None of these methods touches fi_mean / fi_cov / status or the weights of the object."""

    _sweep_kind = 0          # SSMQ_SWEEP_GP; 1: SSMQ_SWEEP_BS

    def _sweep_setup(self, par_dyn, par_obs):
        """Every refusal, before the library is loaded; the arguments of the C entry points that do not depend on the data."""
        from .ssmod import GaussRV
        what = 'likelihood sweeps cover'
        if is_user_model(self.mod_dyn) or is_user_model(self.mod_obs):
            raise user_unsupported('the likelihood sweep (built-in models, D <= 6, Y <= 4, at most 2 D + 1 points)')
        self._additive_gauss_only(what)
        for rv in (self.mod_dyn.init_rv, self.mod_dyn.noise_rv, self.mod_obs.noise_rv):
            if not isinstance(rv, GaussRV):
                raise NotImplementedError(what + ' Gaussian initial state and noise; not implemented for {}'.format(type(rv).__name__))
        D, Y = self.mod_dyn.dim_state, self.mod_obs.dim_out
        for tf in (self.tf_dyn, self.tf_obs):
            if type(tf.model.kernel).__name__ != 'RBFGauss':
                raise NotImplementedError(what + " the 'rbf' kernel; not implemented for {}".format(type(tf.model.kernel).__name__))
            if tf.model.points.shape[0] != D or not 2 <= tf.model.points.shape[1] <= 2 * D + 1:
                raise NotImplementedError(what + ' 2 .. 2 D + 1 points in the state dimension D <= 6 (Y <= 4); got points {}'.format(
                    tf.model.points.shape))
        if D > 6 or Y > 4:
            raise NotImplementedError(what + ' D <= 6, Y <= 4; got D = {}, Y = {}'.format(D, Y))
        pd, po = (np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64) for p in (par_dyn, par_obs))
        if pd.ndim != 2 or po.ndim != 2 or pd.shape[0] != po.shape[0] or pd.shape[0] < 1 or pd.shape[1] != 1 + D or po.shape[1] != 1 + D:
            raise ValueError('likelihood sweep: par_dyn and par_obs are (P, 1 + D) with the same P >= 1 (row p pairs par_dyn[p] with '
                             'par_obs[p]); got {} and {}'.format(pd.shape, po.shape))
        f_dyn, _ = resolve_integrand(self.mod_dyn.dyn_eval)
        f_obs, _ = resolve_integrand(self.mod_obs.meas_eval)
        head, keep = [f_dyn, f_obs, self._sweep_kind, self._sweep_kind], [pd, po]
        mul = []
        for tf in (self.tf_dyn, self.tf_obs):
            xi = np.ascontiguousarray(tf.model.points, dtype=np.float64)
            keep.append(xi)
            head += [_lib.dp(xi), xi.shape[1]]
            mi = np.ascontiguousarray(tf.model.mulind, dtype=np.int32) if self._sweep_kind == 1 else None
            keep.append(mi)
            mul += [None if mi is None else mi.ctypes.data_as(_lib.c_int32_p), 0 if mi is None else mi.shape[1]]
        gqg, rr = self._noise()
        m0, P0 = np.ascontiguousarray(self.x0_mean, dtype=np.float64), np.ascontiguousarray(self._initial_cov(), dtype=np.float64)
        keep += [gqg, rr, m0, P0]
        return dict(head=head + mul + [_lib.dp(pd), _lib.dp(po), pd.shape[0], float(self.tf_dyn.model.kernel.jitter),
                                       float(self.tf_obs.model.kernel.jitter), D, Y],
                    noise=[_lib.dp(m0), _lib.dp(P0), _lib.dp(gqg), _lib.dp(rr)], P=pd.shape[0], D=D, Y=Y, keep=keep, par=(pd, po))

    def likelihood_sweep_kernel_name(self, P=1):
        """Which kernel `likelihood_sweep_*` run for this filter (the same for every number of rows P)."""
        D = self.mod_dyn.dim_state
        s = self._sweep_setup(np.ones((int(P), 1 + D)), np.ones((int(P), 1 + D)))
        h = s['head']
        buf = ctypes.create_string_buffer(512)
        _lib.check(_lib.load().ssmq_filter_sweep_kernel_name(h[0], h[1], h[2], h[3], h[5], h[7], s['D'], s['Y'], buf, 512),
                   'ssmq_filter_sweep_kernel_name', True)
        return buf.value.decode()

    def _sweep_launch(self, stage, s, d_y, B, ld, T, steps, device):
        alloc = stage.device if device else stage.scratch
        P = s['P']
        d_tot, d_nis, d_st = alloc(8 * P * ld), alloc(8 * P * ld), alloc(4 * P * ld)
        d_ll = alloc(8 * P * T * ld) if steps else None
        ts = np.zeros(P, dtype=np.int32)
        vp = _lib.vp
        _lib.check(_lib.load().ssmq_filter_sweep_dev(*s['head'], B, ld, T, vp(d_y), *s['noise'], vp(d_tot), vp(d_nis), vp(d_ll), vp(d_st),
                                                     ts.ctypes.data_as(_lib.c_int32_p)), 'ssmq_filter_sweep_dev', True)
        return d_tot, d_nis, d_ll, d_st, ts

    def likelihood_sweep_dev(self, d_y, B, ld, T, par_dyn, par_obs, steps=False):
        """The sweep on measurements that are already on the device (planes [T][dim_y][ld], ld a multiple of 64): DeviceBuffers
        d_loglik_total [P][ld], d_nis_mean [P][ld], d_loglik [P][T][ld] (None without `steps`), d_status [P][ld] int32 - the caller
        frees them - and theta_status (P,) int32 on the host.  Every trajectory starts from the model's initial moments."""
        return self._sweep_dev(self._sweep_setup(par_dyn, par_obs), d_y, B, ld, T, steps)

    def _sweep_dev(self, s, d_y, B, ld, T, steps):
        if ld % 64 or ld < B:
            raise ValueError('likelihood sweep: ld is a multiple of 64 and at least B')
        with _lib.Staging() as stage:
            d_tot, d_nis, d_ll, d_st, ts = self._sweep_launch(stage, s, d_y, B, ld, T, steps, True)
            stage.release(*[b for b in (d_tot, d_nis, d_ll, d_st) if b is not None])
        return d_tot, d_nis, d_ll, d_st, ts

    def likelihood_sweep_batch(self, data, par_dyn, par_obs, steps=False):
        """data (dim_y, T, B), par_dyn / par_obs (P, 1 + D) -> dict: loglik_total (P, B) = sum_k log p(y_k | y_1..k-1) under row p,
        nis_mean (P, B), status (P, B) int32 (0, 1 + the first step whose scores are not numbers, or -1 for a row whose weights
        failed; the totals of such an item are NaN), theta_status (P,) int32 (0, or what the weights call reported: dynamics + 4 x
        measurement), and with `steps` loglik (P, T, B).  Row p is `type(self)(dyn, obs, par_dyn[p:p+1], par_obs[p:p+1])`'s
        forward_pass_batch followed by innovations_batch, computed by the dense kernels without storing a filtered moment."""
        return self._sweep_batch(self._sweep_setup(par_dyn, par_obs), data, steps)

    def _sweep_batch(self, s, data, steps):
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 3 or data.shape[0] != s['Y']:
            raise ValueError('likelihood sweep: data is (dim_y, T, B)')
        Y, T, B = data.shape
        if B < 1 or T < 1:
            raise ValueError('likelihood sweep: data holds at least one step of at least one trajectory')
        ld, P = _lib.padded(B), s['P']
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_tot, d_nis, d_ll, d_st, ts = self._sweep_launch(stage, s, d_y, B, ld, T, steps, False)
            out = {'theta_status': ts}
            out['loglik_total'] = d_tot.download((P, ld))[:, :B].copy()
            out['nis_mean'] = d_nis.download((P, ld))[:, :B].copy()
            out['status'] = d_st.download((P, ld), dtype=np.int32)[:, :B].copy()
            if steps:
                out['loglik'] = d_ll.download((P, T, ld))[:, :, :B].copy()
        return out

    def fit_kernel_parameters(self, data, par_dyn, par_obs):
        """The row of the grid with the largest measurement likelihood: (index, par_dyn[index], par_obs[index], table) with
        table[p] the sum of loglik_total[p] over the trajectories on which every row succeeded (`fit_table`).  Construct the
        filter with the chosen row: `type(alg)(dyn, obs, par_dyn[index:index + 1], par_obs[index:index + 1])`."""
        return self._sweep_fit(self.likelihood_sweep_batch(data, par_dyn, par_obs), par_dyn, par_obs)

    @staticmethod
    def _sweep_fit(out, par_dyn, par_obs):
        index, table = fit_table(out['loglik_total'], out['status'], out['theta_status'])
        pd, po = np.atleast_2d(np.asarray(par_dyn, dtype=np.float64)), np.atleast_2d(np.asarray(par_obs, dtype=np.float64))
        return index, pd[index].copy(), po[index].copy(), table


class GaussianProcessKalman(_LikelihoodSweep, GaussianInference):
    """ssinf.py:423-463."""

    def __init__(self, dyn, obs, kern_par_dyn, kern_par_obs, kernel='rbf', points='ut', point_hyp=None):
        t_dyn = GaussianProcessTransform(dyn.dim_in, dyn.dim_state, kern_par_dyn, kernel, points, point_hyp)
        t_obs = GaussianProcessTransform(obs.dim_in, obs.dim_out, kern_par_obs, kernel, points, point_hyp)
        super().__init__(dyn, obs, t_dyn, t_obs)


class GaussianProcessDerKalman(GaussianInference):
    """GP quadrature Kalman filter and smoother with derivative observations at the sigma points (the filter of the reference's
    research/gpqd line of work): both transforms are `GaussianProcessDerTransform`s, kern_par_dyn (1, 1 + dim_in), kern_par_obs
    (1, 1 + dim_state), which_der_dyn / which_der_obs the points that carry a Jacobian (None: all).  Runs on the captured launch
    loop (k_apply_gpqd | k_apply_gpqd | k_kalman_update per step; the smoother's variant keeps the predictive moments), routed as
    ExtendedKalmanGPQD is; additive-noise models only, built-in ones with a Jacobian and models of your own that have a
    `device_jacobian` (forward pass).  `run_filters` raises NotImplementedError for this class."""

    def __init__(self, dyn, obs, kern_par_dyn, kern_par_obs, points='ut', point_hyp=None, which_der_dyn=None, which_der_obs=None):
        _need_device_jacobians('GaussianProcessDerKalman', dyn, obs)
        if not (dyn.noise_additive and obs.noise_additive):
            raise NotImplementedError('GaussianProcessDerKalman runs for additive-noise models only')
        t_dyn = GaussianProcessDerTransform(dyn.dim_in, dyn.dim_state, kern_par_dyn, points, point_hyp, which_der=which_der_dyn)
        t_obs = GaussianProcessDerTransform(obs.dim_state, obs.dim_out, kern_par_obs, points, point_hyp, which_der=which_der_obs)
        t_dyn._device_integrand(dyn.dyn_eval)          # refused here, before the library is touched
        t_obs._device_integrand(obs.meas_eval)
        super().__init__(dyn, obs, t_dyn, t_obs)


class MultiOutputGaussianProcessKalman(GaussianInference):
    """GP quadrature Kalman filter with one kernel-parameter row per output (ssinf.py:911-961): kern_par_dyn (dim_state, 1 +
    dim_in), kern_par_obs (dim_out, 1 + dim_in).  The forward pass runs as the launch loop (apply dyn | apply obs | update per
    step, both transforms k_apply_mo); additive noise and the built-in models only; the smoother and `run_filters` are not
    implemented for it."""

    def __init__(self, dyn, obs, kern_par_dyn, kern_par_obs, kernel='rbf', points='ut', point_hyp=None):
        if is_user_model(dyn) or is_user_model(obs):
            raise user_unsupported('the multi-output transforms (D <= 16, E <= 8, N <= 64, built-in models)')
        if not (dyn.noise_additive and obs.noise_additive):
            raise NotImplementedError('MultiOutputGaussianProcessKalman runs for additive-noise models only')
        t_dyn = MultiOutputGaussianProcessTransform(dyn.dim_in, dyn.dim_state, kern_par_dyn, kernel, points, point_hyp)
        t_obs = MultiOutputGaussianProcessTransform(obs.dim_in, obs.dim_out, kern_par_obs, kernel, points, point_hyp)
        super().__init__(dyn, obs, t_dyn, t_obs)

    def backward_pass(self):
        raise NotImplementedError('the RTS smoother is not implemented for the multi-output filter')

    def backward_pass_batch(self):
        raise NotImplementedError('the RTS smoother is not implemented for the multi-output filter')

    def forward_pass_batch(self, data, x0_mean=None, x0_cov=None, raise_on_failure=True, smooth=False):
        if smooth:
            raise NotImplementedError('the RTS smoother is not implemented for the multi-output filter')
        return super().forward_pass_batch(data, x0_mean=x0_mean, x0_cov=x0_cov, raise_on_failure=raise_on_failure)


class BayesSardKalman(_LikelihoodSweep, GaussianInference):
    """ssinf.py:466-502."""

    _sweep_kind = 1

    def __init__(self, dyn, obs, kern_par_dyn, kern_par_obs, mulind_dyn=2, mulind_obs=2, points='ut', point_hyp=None):
        t_dyn = BayesSardTransform(dyn.dim_in, dyn.dim_state, kern_par_dyn, mulind_dyn, points, point_hyp)
        t_obs = BayesSardTransform(obs.dim_in, obs.dim_out, kern_par_obs, mulind_obs, points, point_hyp)
        super().__init__(dyn, obs, t_dyn, t_obs)


def _per_row(value, P, name, low, low_ok, default):
    """A sweep argument that is a scalar or (P,): the (P,) float64 array, `default` for None; ValueError for another shape and for a
    row at or below `low` (below, with low_ok), naming the row."""
    v = np.asarray(default if value is None else value, dtype=np.float64)
    if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != P):
        raise ValueError('likelihood sweep: {} is a scalar or has one entry per parameter row, ({},); got shape {}'.format(name, P, v.shape))
    v = np.ascontiguousarray(np.broadcast_to(v, (P,)))
    bad = ~(v >= low) if low_ok else ~(v > low)
    bad |= ~np.isfinite(v)
    if bad.any():
        p = int(np.flatnonzero(bad)[0])
        raise ValueError('likelihood sweep: {} of row {} is {!r}; it must be a finite number {} {}'.format(
            name, p, float(v[p]), 'of at least' if low_ok else 'above', low))
    return v


class _TProcessLikelihoodSweep(_LikelihoodSweep):
    """Likelihood sweeps of the t-process filters (`ssmq_filter_sweep_t_dev`, k_filter_score<>): `_LikelihoodSweep` over rows of
    (par_dyn[p], par_obs[p], nu[p], dof[p]).  Row p is the filter constructed with par_dyn[p:p+1], par_obs[p:p+1] (and dof[p]) whose
    two t-process models have `nu` = nu[p] - `tf_dyn.model.nu` / `tf_obs.model.nu`: as in the reference the constructors' `nu` / `dof_tp`
    never reaches the model, so that is where a filter's nu is set.  Its score is the Gaussian `innovations`
    for `StudentProcessKalmanSweep` and `student_scores` for `StudentProcessStudent`.  nu and dof are scalars or (P,) and default to the
    object's values; nu >= 2, dof > 2 (ValueError naming the row - nothing is replaced silently inside a sweep); dof belongs to the
    Studentian class only.  Range: the 'rbf' kernel, built-in additive-noise models, D <= 4, Y <= 2, 2 .. 2 D + 1 points.  None of
    these methods touches fi_mean / fi_cov / status or the weights of the object."""

    def _sweep_setup(self, par_dyn, par_obs, nu=None, dof=None):
        """Every refusal, before the library is loaded; the arguments of the C entry points that do not depend on the data."""
        from .ssmod import GaussRV
        what = 'likelihood sweeps of the t-process filters cover'
        student = self._recursion == 'student'
        if is_user_model(self.mod_dyn) or is_user_model(self.mod_obs):
            raise user_unsupported('the likelihood sweep (built-in models, D <= 4, Y <= 2, at most 2 D + 1 points)')
        if not self._additive:
            raise NotImplementedError(what + ' additive-noise models; not implemented for models that take their noise as an argument '
                                      '(non-additive noise)')
        if not student:
            for rv in (self.mod_dyn.init_rv, self.mod_dyn.noise_rv, self.mod_obs.noise_rv):
                if not isinstance(rv, GaussRV):
                    raise NotImplementedError(what + ' Gaussian initial state and noise for the Gaussian recursion; not implemented for '
                                              '{}'.format(type(rv).__name__))
        D, Y = self.mod_dyn.dim_state, self.mod_obs.dim_out
        for tf in (self.tf_dyn, self.tf_obs):
            if not isinstance(tf, StudentTProcessTransform):
                raise NotImplementedError(what + ' t-process transforms; got {}'.format(type(tf).__name__))
            if type(tf.model.kernel).__name__ != 'RBFGauss':
                raise NotImplementedError(what + " the 'rbf' kernel; not implemented for {} (the Monte-Carlo weights of 'rbf-student' "
                                          'are not swept)'.format(type(tf.model.kernel).__name__))
            if tf.model.points.shape[0] != D or not 2 <= tf.model.points.shape[1] <= 2 * D + 1:
                raise NotImplementedError(what + ' 2 .. 2 D + 1 points in the state dimension D <= 4 (Y <= 2); got points {}'.format(
                    tf.model.points.shape))
        if D > 4 or Y > 2:
            raise NotImplementedError(what + ' D <= 4, Y <= 2; got D = {}, Y = {}'.format(D, Y))
        pd, po = (np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64) for p in (par_dyn, par_obs))
        if pd.ndim != 2 or po.ndim != 2 or pd.shape[0] != po.shape[0] or pd.shape[0] < 1 or pd.shape[1] != 1 + D or po.shape[1] != 1 + D:
            raise ValueError('likelihood sweep: par_dyn and par_obs are (P, 1 + D) with the same P >= 1 (row p pairs par_dyn[p] with '
                             'par_obs[p]); got {} and {}'.format(pd.shape, po.shape))
        P = pd.shape[0]
        if P > 65535:
            raise NotImplementedError(what + ' at most 65535 rows; got {}'.format(P))
        if dof is not None and not student:
            raise ValueError('likelihood sweep: dof is the Studentian filters\' (StudentProcessStudent); {} has the Gaussian recursion'.format(
                type(self).__name__))
        nu_dyn = _per_row(nu, P, 'nu', 2.0, True, self.tf_dyn.model.nu)
        nu_obs = _per_row(nu, P, 'nu', 2.0, True, self.tf_obs.model.nu)
        dofs = _per_row(dof, P, 'dof', 2.0, False, self.dof) if student else None
        # the additive terms and the initial matrix of every row: scale matrices in the Studentian recursion (StudentianInference.__init__)
        if student:
            sc = [(float(d) - 2) / float(d) for d in dofs]
            S0 = np.ascontiguousarray([c * self.x0_cov for c in sc], dtype=np.float64)
            gqg = np.ascontiguousarray([self.G.dot(c * self.q_cov).dot(self.G.T) for c in sc], dtype=np.float64)
            rr = np.ascontiguousarray([c * self.r_cov for c in sc], dtype=np.float64)
        else:
            g1, r1 = self._noise()
            S0, gqg, rr = (np.ascontiguousarray(np.broadcast_to(a, (P,) + np.shape(a)), dtype=np.float64) for a in (self.x0_cov, g1, r1))
        f_dyn, _ = resolve_integrand(self.mod_dyn.dyn_eval)
        f_obs, _ = resolve_integrand(self.mod_obs.meas_eval)
        xd, xo = (np.ascontiguousarray(tf.model.points, dtype=np.float64) for tf in (self.tf_dyn, self.tf_obs))
        m0 = np.ascontiguousarray(self.x0_mean, dtype=np.float64)
        dp = _lib.dp
        return dict(head=[f_dyn, f_obs, 1 if student else 0, dp(xd), xd.shape[1], dp(xo), xo.shape[1], dp(pd), dp(po), dp(nu_dyn), dp(nu_obs),
                          dp(dofs), P, float(self.tf_dyn.model.kernel.jitter), float(self.tf_obs.model.kernel.jitter), D, Y],
                    noise=[dp(m0), dp(S0), dp(gqg), dp(rr)], P=P, D=D, Y=Y, dof=dofs, par=(pd, po), nu=(nu_dyn, nu_obs),
                    keep=[pd, po, xd, xo, nu_dyn, nu_obs, dofs, m0, S0, gqg, rr])

    def likelihood_sweep_kernel_name(self, P=1):
        """Which kernel `likelihood_sweep_*` run for this filter (the same for every number of rows P)."""
        D = self.mod_dyn.dim_state
        s = self._sweep_setup(np.ones((int(P), 1 + D)), np.ones((int(P), 1 + D)))
        h = s['head']
        buf = ctypes.create_string_buffer(512)
        _lib.check(_lib.load().ssmq_filter_sweep_t_kernel_name(h[0], h[1], h[2], h[4], h[6], s['D'], s['Y'], buf, 512),
                   'ssmq_filter_sweep_t_kernel_name', True)
        return buf.value.decode()

    def _sweep_launch(self, stage, s, d_y, B, ld, T, steps, device):
        alloc = stage.device if device else stage.scratch
        P = s['P']
        d_tot, d_nis, d_st = alloc(8 * P * ld), alloc(8 * P * ld), alloc(4 * P * ld)
        d_ll = alloc(8 * P * T * ld) if steps else None
        ts = np.zeros(P, dtype=np.int32)
        scale = None if s['dof'] is None else np.ascontiguousarray([self._row_scale(float(d), T) for d in s['dof']], dtype=np.float64)
        vp = _lib.vp
        _lib.check(_lib.load().ssmq_filter_sweep_t_dev(*s['head'], B, ld, T, vp(d_y), *s['noise'], _lib.dp(scale), vp(d_tot), vp(d_nis), vp(d_ll),
                                                       vp(d_st), ts.ctypes.data_as(_lib.c_int32_p)), 'ssmq_filter_sweep_t_dev', True)
        return d_tot, d_nis, d_ll, d_st, ts

    def likelihood_sweep_dev(self, d_y, B, ld, T, par_dyn, par_obs, nu=None, dof=None, steps=False):
        """`_LikelihoodSweep.likelihood_sweep_dev` over rows of (par_dyn, par_obs, nu, dof)."""
        return self._sweep_dev(self._sweep_setup(par_dyn, par_obs, nu, dof), d_y, B, ld, T, steps)

    def likelihood_sweep_batch(self, data, par_dyn, par_obs, nu=None, dof=None, steps=False):
        """data (dim_y, T, B), par_dyn / par_obs (P, 1 + D), nu / dof scalars or (P,) -> the dict of
        `_LikelihoodSweep.likelihood_sweep_batch`: loglik_total, nis_mean, status (P, B), theta_status (P,), with `steps` loglik
        (P, T, B).  Row p: see the class."""
        return self._sweep_batch(self._sweep_setup(par_dyn, par_obs, nu, dof), data, steps)

    def fit_kernel_parameters(self, data, par_dyn, par_obs, nu=None, dof=None):
        """The row with the largest measurement likelihood: (index, par_dyn[index], par_obs[index], table) (`fit_table`); nu[index] and
        dof[index] are the caller's to read off."""
        return self._sweep_fit(self.likelihood_sweep_batch(data, par_dyn, par_obs, nu, dof), par_dyn, par_obs)


class StudentProcessKalman(GaussianInference):
    """ssinf.py:505-552.  As in the reference the transforms are built with dim_out = 1 (I_out = eye(1)), so the whole
    scaled (E, E) model-variance matrix is added for E > 1.  The class itself has no likelihood sweep (tests/test_sweep_host.py pins
    that); `StudentProcessKalmanSweep` is this filter with one."""

    def __init__(self, dyn, obs, kern_par_dyn, kern_par_obs, kernel='rbf', points='ut', point_hyp=None, nu=3.0):
        t_dyn = StudentTProcessTransform(dyn.dim_in, 1, kern_par_dyn, kernel, points, point_hyp, nu=nu)
        t_obs = StudentTProcessTransform(obs.dim_in, 1, kern_par_obs, kernel, points, point_hyp, nu=nu)
        super().__init__(dyn, obs, t_dyn, t_obs)


class StudentProcessKalmanSweep(_TProcessLikelihoodSweep, StudentProcessKalman):
    """`StudentProcessKalman` - the same constructor, the same filter, bit for bit - with `likelihood_sweep_batch` /
    `likelihood_sweep_dev` / `likelihood_sweep_kernel_name` / `fit_kernel_parameters` over rows of (par_dyn, par_obs, nu): row p is the
    `StudentProcessKalman` of that row, scored by `forward_pass_batch` then `innovations_batch`."""


class StudentianInference(GaussianInference):
    """Additive-noise Studentian filter (ssinf.py:555-736): the state and measurement are jointly Student-t; the moment
    transforms are fed scale matrices and the measurement update rescales the filtered scale matrix by
    (dof + delta'delta) / (dof + dim_y).  `forward_pass*` return the filtered mean and the reference's `x_cov_fi`."""

    def __init__(self, mod_dyn, mod_obs, tf_dyn, tf_obs, dof=4.0, fixed_dof=True):
        assert isinstance(mod_dyn, TransitionModel) and isinstance(mod_obs, MeasurementModel)
        assert isinstance(tf_dyn, MomentTransform) and isinstance(tf_obs, MomentTransform)
        if not (mod_dyn.noise_additive and mod_obs.noise_additive):
            raise NotImplementedError('the device filter loop covers additive-noise models')
        if dof <= 2.0:
            dof = 4.0
        self.mod_dyn, self.mod_obs, self.tf_dyn, self.tf_obs = mod_dyn, mod_obs, tf_dyn, tf_obs
        # NB: as in the reference, get_stats() hands back SCALE matrices that are then treated as covariances
        self.x0_mean, self.x0_cov, self.x0_dof = mod_dyn.init_rv.get_stats()
        self.q_mean, self.q_cov, self.q_dof = mod_dyn.noise_rv.get_stats()
        self.r_mean, self.r_cov, self.r_dof = mod_obs.noise_rv.get_stats()
        self.G = mod_dyn.noise_gain
        scale = (dof - 2) / dof
        self.x_smat_0 = scale * self.x0_cov
        self.q_smat = scale * self.q_cov
        self.r_smat = scale * self.r_cov
        self.dof, self.fixed_dof = dof, fixed_dof
        self.fi_mean = self.fi_cov = None
        self.status = None

    def _initial_cov(self):
        return self.x_smat_0

    def backward_pass_batch(self):
        raise NotImplementedError('the reference has no Student smoother either (ssinf.py:738-740)')

    def _innovations_refusal(self):
        return NotImplementedError('innovation scores cover the additive-noise Gaussian recursion; not implemented for the Studentian '
                                   'recursion (its predictive density is a Student t, not the Gaussian the scores assume): see '
                                   'student_scores')

    # ---- Student-t measurement likelihood: the Studentian filters' counterpart of the innovation scores ---------------------------
    def _row_scale(self, dof, steps):
        """`scale_sequence(steps)` of this filter had it been constructed with `dof`."""
        return self.scale_sequence(steps) if self.fixed_dof else np.full(steps, (dof - 2) / dof)

    def _student_scores_refusal(self):
        """Raises what keeps a filter out of `student_scores*` - before the library is touched."""
        what = 'student scores cover'
        rng = ('fully-symmetric (sigma-point) and t-process transforms with the \'rbf\' kernel on built-in additive-noise models, D <= 4, '
               'Y <= 2, 2 .. 2 D + 1 points (the same count for both transforms)')
        if is_user_model(self.mod_dyn) or is_user_model(self.mod_obs):
            raise user_unsupported('the student scores (' + rng + ')')
        if not self._additive:
            raise NotImplementedError(what + ' additive-noise models; not implemented for models that take their noise as an argument '
                                      '(non-additive noise)')
        kinds = set()
        for tf in (self.tf_dyn, self.tf_obs):
            if isinstance(tf, (TruncatedUnscentedTransform, TruncatedSphericalRadialTransform, TruncatedGaussHermiteTransform)):
                raise NotImplementedError(what + ' ' + rng + '; not implemented for truncated transforms ({})'.format(type(tf).__name__))
            if isinstance(tf, StudentTProcessTransform):
                if type(tf.model.kernel).__name__ != 'RBFGauss':
                    raise NotImplementedError(what + " the 'rbf' kernel; not implemented for {} (the Monte-Carlo weights of "
                                              "'rbf-student')".format(type(tf.model.kernel).__name__))
                kinds.add('tp')
            elif isinstance(tf, FullySymmetricStudentTransform):
                kinds.add('fs')
            else:
                raise NotImplementedError(what + ' ' + rng + '; got {}'.format(type(tf).__name__))
        D, Y = self.mod_dyn.dim_state, self.mod_obs.dim_out
        n = (self.tf_dyn._num_points(), self.tf_obs._num_points())
        if len(kinds) != 1 or D > 4 or Y > 2 or n[0] != n[1] or not 2 <= n[0] <= 2 * D + 1:
            raise NotImplementedError(what + ' ' + rng + '; got D = {}, Y = {}, points {}, transforms {} / {}'.format(
                D, Y, n, type(self.tf_dyn).__name__, type(self.tf_obs).__name__))

    def student_scores_kernel_name(self):
        """Which kernel `student_scores*` run for this filter: k_filter_score<..,STU=1>."""
        self._student_scores_refusal()
        return self._kernel_name('ssmq_student_scores_kernel_name', unsupported=True)

    def _launch_student_scores(self, lib, B, ld, T, d_y, d_nis, d_ll, d_tot, d_nm, d_st):
        gqg, rr = self._noise()
        sc = np.ascontiguousarray(self.scale_sequence(T), dtype=np.float64)
        m0, S0 = np.ascontiguousarray(self.x0_mean, dtype=np.float64), np.ascontiguousarray(self._initial_cov(), dtype=np.float64)
        vp, dp = _lib.vp, _lib.dp
        _lib.check(lib.ssmq_student_scores_dev(*self._pair(), B, ld, T, vp(d_y), dp(m0), dp(S0), dp(gqg), dp(rr), dp(sc),
                                               ctypes.c_double(self.dof), vp(d_nis), vp(d_ll), vp(d_tot), vp(d_nm), vp(d_st)),
                   'ssmq_student_scores_dev', True)

    def student_scores_dev(self, d_y, B, ld, T):
        """Student scores of measurements that are already on the device (planes [T][dim_y][ld], ld a multiple of 64, e.g. from
        `ssmod.simulate_dev`): DeviceBuffers (d_nis [T][ld], d_loglik [T][ld], d_loglik_total [ld], d_nis_mean [ld], d_status [ld]
        int32); the caller frees them.  Every trajectory starts from the model's initial moments."""
        self._student_scores_refusal()
        if ld % 64 or ld < B:
            raise ValueError('student scores: ld is a multiple of 64 and at least B')
        lib = _lib.load()
        with _lib.Staging() as stage:
            d_nis, d_ll = stage.device(8 * T * ld), stage.device(8 * T * ld)
            d_tot, d_nm, d_st = stage.device(8 * ld), stage.device(8 * ld), stage.device(4 * ld)
            self._launch_student_scores(lib, B, ld, T, d_y, d_nis, d_ll, d_tot, d_nm, d_st)
            return stage.release(d_nis, d_ll, d_tot, d_nm, d_st)

    def student_scores_batch(self, data):
        """One-step-ahead Student-t measurement likelihood of every step, data (dim_y, T, B), computed by one scoring pass that stores
        no filtered moment.  With (m, S) the running mean and scale matrix, y_mean, S_y = sc_k P_y + r_smat the predictive measurement
        mean and scale matrix of step k and e = y_k - y_mean,
            nis[k] = Delta^2 = e' S_y^-1 e                     (expected value under the density below: dim_y dof / (dof - 2))
            loglik[k] = log t_dof(y_k | y_mean, S_y) = lgamma((dof + Y) / 2) - lgamma(dof / 2) - Y / 2 log(dof pi) - log det S_y / 2
                        - (dof + Y) / 2 log1p(Delta^2 / dof).
        The filter's update, with its factor (dof + Delta^2) / (dof + dim_y), is the conditional of a joint Student t with `dof`
        degrees of freedom; this is the marginal of y_k under the same joint - so dof is the filter's `dof`, not the dof_pr of
        `scale_sequence`.  Returns a dict: nis (T, B), loglik (T, B), loglik_total (B,), nis_mean (B,), status (B,) - 1 + the first
        step whose scores are not numbers (the totals and the remaining steps are then NaN), 0 if none.  Touches neither fi_mean /
        fi_cov / status nor the weights."""
        self._student_scores_refusal()
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 3 or data.shape[0] != self.mod_obs.dim_out:
            raise ValueError('student scores: data is (dim_y, T, B)')
        Y, T, B = data.shape
        if B < 1 or T < 1:
            raise ValueError('student scores: data holds at least one step of at least one trajectory')
        lib = _lib.load()
        ld = _lib.padded(B)
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_nis, d_ll = stage.scratch(8 * T * ld), stage.scratch(8 * T * ld)
            d_tot, d_nm, d_st = stage.scratch(8 * ld), stage.scratch(8 * ld), stage.scratch(4 * ld)
            self._launch_student_scores(lib, B, ld, T, d_y, d_nis, d_ll, d_tot, d_nm, d_st)
            out = {'nis': _lib.download_study(d_nis, (), T, B, ld), 'loglik': _lib.download_study(d_ll, (), T, B, ld)}
            out['loglik_total'] = d_tot.download((ld,))[:B].copy()
            out['nis_mean'] = d_nm.download((ld,))[:B].copy()
            out['status'] = d_st.download((ld,), dtype=np.int32)[:B].copy()
        return out

    def student_scores(self, data):
        """`student_scores_batch` for one trajectory, data (dim_y, T): nis (T,), loglik (T,), loglik_total, nis_mean, status."""
        out = self.student_scores_batch(np.asarray(data)[..., None])
        return {k: (v[..., 0] if v.ndim else v) for k, v in out.items()}

    def scale_sequence(self, steps):
        """(dof_pr - 2) / dof_pr of every time update (ssinf.py:652-660; dof_fi grows by dim_out per update, :735)."""
        out = np.zeros(steps)
        dof_fi = self.x0_dof
        for k in range(steps):
            if self.fixed_dof:
                dof_pr = min(dof_fi, self.q_dof, self.r_dof)
                out[k] = (dof_pr - 2) / dof_pr
            else:
                out[k] = (self.dof - 2) / self.dof
            dof_fi += self.mod_obs.dim_out
        return out

    _recursion = 'student'

    def _noise(self):
        """The scale matrices that stand where the Gaussian recursion has G Q G' and R."""
        return (np.ascontiguousarray(self.G.dot(self.q_smat).dot(self.G.T), dtype=np.float64),
                np.ascontiguousarray(self.r_smat, dtype=np.float64))

    def _launch(self, lib, B, ld, T, d_y, d_m0, d_P0, d_fm, d_fP, d_st):
        gqg, rr = self._noise()
        sc = np.ascontiguousarray(self.scale_sequence(T), dtype=np.float64)
        vp, dp = _lib.vp, _lib.dp
        _lib.check(lib.ssmq_student_filter_forward_dev(*self._pair(), B, ld, T, vp(d_y), vp(d_m0), vp(d_P0), dp(gqg), dp(rr), dp(sc),
                                                       ctypes.c_double(self.dof), vp(d_fm), vp(d_fP), vp(d_st)),
                   'ssmq_student_filter_forward_dev')


class FullySymmetricStudent(StudentianInference):
    """Student filter with the fully-symmetric rule (ssinf.py:743-790)."""

    def __init__(self, dyn, obs, degree=3, kappa=None, dof=4.0, fixed_dof=True):
        dyn_dof = min(dyn.init_rv.dof, dyn.noise_rv.dof)
        obs_dof = min(dyn_dof, obs.noise_rv.dof)
        t_dyn = FullySymmetricStudentTransform(dyn.dim_in, degree, kappa, dyn_dof)
        t_obs = FullySymmetricStudentTransform(obs.dim_in, degree, kappa, obs_dof)
        super().__init__(dyn, obs, t_dyn, t_obs, dof, fixed_dof)


class StudentProcessStudent(_TProcessLikelihoodSweep, StudentianInference):
    """Student-t process quadrature Student filter, the TPQSF (ssinf.py:793-857).  kernel='rbf' (the default) builds both
    transforms with the Gaussian-expectation RBF kernel, as this class always has; kernel='rbf-student' builds the
    reference's filter: the weights of both transforms come from the 'rbf-student' kernel, the RBF kernel with Monte-Carlo
    Student-t expectations (bq/bqkern.py:457-536), computed on the device.  mc: a dict of kernel attributes (`num_samples`,
    `seed`, `dof`) set on both transforms' kernels before their weights are computed; without it the kernels have the
    constructor's defaults, as in the reference (dof 4.0, 2e6 samples; seed 0).  The same seed gives the same filter, bit
    for bit."""

    def __init__(self, dyn, obs, kern_par_dyn, kern_par_obs, point_par=None, dof=4.0, fixed_dof=True, dof_tp=4.0,
                 kernel='rbf', mc=None):
        assert kern_par_dyn.shape[1] == dyn.dim_in + 1 and kern_par_obs.shape[1] == obs.dim_in + 1
        if kernel not in ('rbf', 'rbf-student'):
            raise ValueError("kernel must be 'rbf' or 'rbf-student', got {!r}".format(kernel))
        if mc and kernel != 'rbf-student':
            raise ValueError("mc sets attributes of the 'rbf-student' kernel; the 'rbf' kernel has none")
        point_par = {} if point_par is None else point_par
        pp_dyn, pp_obs = dict(point_par), dict(point_par)
        pp_dyn.update({'dof': dyn.noise_rv.dof})
        pp_obs.update({'dof': obs.noise_rv.dof})
        mc = dict(mc) if mc else None
        t_dyn = StudentTProcessTransform(dyn.dim_in, 1, kern_par_dyn, kernel, 'fs', pp_dyn, nu=dof_tp, kern_attr=mc)
        t_obs = StudentTProcessTransform(obs.dim_in, 1, kern_par_obs, kernel, 'fs', pp_obs, nu=dof_tp, kern_attr=mc)
        super().__init__(dyn, obs, t_dyn, t_obs, dof, fixed_dof)


class MarginalInference(GaussianInference):
    """Gaussian filter with the moment-transform (kernel) parameters marginalised (ssinf.py:1034-1273; the reference
    calls it experimental).  Per measurement: Laplace approximation of the log-parameter posterior (BFGS on
    -log N(y | m_y(theta), P_y(theta)) - log N(theta | prior)), then a spherical-radial rule over that posterior mixing
    the theta-conditioned state posteriors.  Every evaluation "weights(theta) -> two transforms -> update" runs on the
    device through `ssmq_gp_theta_step`, batched over theta: one call per finite-difference gradient
    (param_dim + 1 items) and one per marginalisation (2 param_dim items).  The optimiser itself is SciPy on the host, as
    in the reference.  GP-quadrature transforms; dynamics with additive noise or with the noise as an argument (the
    augmented moments of ssinf.py:1174-1176); additive measurement models - the reference builds the measurement transform
    on `dim_state` inputs (ssinf.py:1288) and cannot run a non-additive one either.

    Reference quirks kept: the measurement update evaluates both transforms at time index k, not k - 1
    (ssinf.py:112 passes k); the mixture covariance is the weighted sum of the conditional covariances, without the
    spread-of-the-means term (ssinf.py:1114-1115); the predictive moments the smoother uses come from the generic time
    update at index k - 1 (ssinf.py:104-107) with whatever weights the dynamics transform was LAST given - the dummy unit
    parameters at the first step, afterwards those of the last parameter point of the previous step's marginalisation
    (BQTransform.apply keeps the weights of its last `kern_par`, bq/bqmtran.py:93-95)."""

    def __init__(self, dyn, obs, tf_dyn, tf_obs, par_mean=None, par_cov=None):
        super().__init__(dyn, obs, tf_dyn, tf_obs)
        if not self.mod_obs.noise_additive:
            raise NotImplementedError('marginalised filter: the measurement transform is built on dim_state inputs '
                                      '(ssinf.py:1288); a measurement model that takes its noise as an argument does not '
                                      'run in the reference either')
        self.param_dyn_dim = self.mod_dyn.dim_in + 1
        self.param_obs_dim = self.mod_obs.dim_state + 1
        self.param_dim = self.param_dyn_dim + self.param_obs_dim
        self.param_prior_mean = np.zeros(self.param_dim) if par_mean is None else np.asarray(par_mean, dtype=float)
        self.param_prior_cov = np.eye(self.param_dim) if par_cov is None else np.asarray(par_cov, dtype=float)
        self.param_mean, self.param_cov = self.param_prior_mean, self.param_prior_cov
        self.param_jitter = 1e-8 * np.eye(self.param_dim)
        self.param_upts = SphericalRadialTransform.unit_sigma_points(self.param_dim)
        self.param_wts = SphericalRadialTransform.weights(self.param_dim)
        self.param_pts_num = self.param_upts.shape[1]
        self.x_mean_fi, self.x_cov_fi = self.x0_mean, self.x0_cov
        self.fd_step = 1.4901161193847656e-08      # SciPy's default forward-difference step for BFGS
        self._last_theta = None                    # parameters the reference's transforms would hold by now
        self.pr_mean = self.pr_cov = self.pr_xx_cov = None

    def reset(self):
        super().reset()
        self.param_mean, self.param_cov = self.param_prior_mean, self.param_prior_cov
        self.x_mean_fi, self.x_cov_fi = self.x0_mean, self.x0_cov
        self.pr_mean = self.pr_cov = self.pr_xx_cov = None
        # _last_theta stays: the reference's reset() does not touch the weights its transforms were last given either

    def _augment(self, mean, cov):
        """ssinf.py:271-272 / 1174-1176: [mean; q_mean], blockdiag(cov, Q) for dynamics that take their noise as an argument;
        mean (D,) / cov (D, D) or per-item (P, D) / (P, D, D)."""
        if self.mod_dyn.noise_additive:
            return mean, cov
        mean, cov = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)
        qm, qc = np.atleast_1d(self.q_mean), np.atleast_2d(self.q_cov)
        D, dq = self.mod_dyn.dim_state, qm.shape[0]
        m = np.concatenate((mean, np.broadcast_to(qm, mean.shape[:-1] + (dq,))), axis=-1)
        c = np.zeros(cov.shape[:-2] + (D + dq, D + dq))
        c[..., :D, :D] = cov
        c[..., D:, D:] = qc
        return m, c

    def _theta_static(self):
        """What rarely changes between calls of `theta_step` (the marginalised filter makes hundreds per time step and the
        ctypes conversions were a third of a call): integrand descriptors, transform handles, the noise terms, and a
        prototype of the entry point that takes the array addresses as plain integers.  Rebuilt when a model constant, a
        state index or a noise covariance has been changed since (compared by value: research code assigns them after
        construction)."""
        state_index = getattr(self.mod_obs, 'state_index', None)
        key = (self.mod_dyn._par(), self.mod_obs._par(), None if state_index is None else tuple(state_index))
        st = getattr(self, '_theta_cache', None)
        if st is not None and st['key'] == key and np.array_equal(st['q_cov'], self.q_cov) and \
                np.array_equal(st['rr'], self.r_cov) and np.array_equal(st['G'], self.G):
            # The handles follow a transform object that was re-assigned and points / I_out that were replaced (research code
            # assigns alg.tf_dyn / tf_obs and their attributes after construction - a cached pointer would go stale or dangle).
            # What the theta step reads from a handle is its shape, its unit points and the model-variance mode - the weights are
            # made on the device per parameter item - so that is what is compared here (two tiny tobytes()); the full comparison
            # of _handle_for (six arrays per handle, 5 us per call of a 65 us step) runs only when one of them differs.
            sig = self._theta_signature()
            if sig != st.get('sig'):
                st['h_dyn'], st['h_obs'] = self.tf_dyn._handle_for(st['e_dyn']), self.tf_obs._handle_for(st['e_obs'])
                st['sig'] = sig
            return st
        lib = _lib.load()
        f_dyn, e_dyn = resolve_integrand(self.mod_dyn.dyn_eval)
        f_obs, e_obs = resolve_integrand(self.mod_obs.meas_eval)
        vp = ctypes.c_void_p
        proto = ctypes.CFUNCTYPE(ctypes.c_int, vp, vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_double, vp, vp, ctypes.c_int,
                                 vp, ctypes.c_int, ctypes.c_double, vp, vp, vp, vp, vp, vp)
        st = dict(key=key, fn=proto(('ssmq_gp_theta_step', lib)), f_dyn=f_dyn, f_obs=f_obs, e_dyn=e_dyn, e_obs=e_obs,
                  pf_dyn=ctypes.addressof(f_dyn), pf_obs=ctypes.addressof(f_obs),
                  h_dyn=self.tf_dyn._handle_for(e_dyn), h_obs=self.tf_obs._handle_for(e_obs),
                  q_cov=np.array(self.q_cov, dtype=np.float64), G=np.array(self.G, dtype=np.float64),
                  gqg=(np.ascontiguousarray(self.G.dot(self.q_cov).dot(self.G.T), dtype=np.float64)
                       if self.mod_dyn.noise_additive else None),
                  rr=np.array(self.r_cov, dtype=np.float64, order='C'))
        st['sig'] = self._theta_signature()
        self._theta_cache = st
        return st

    def _theta_signature(self):
        """Identity of the two transform objects plus the bytes of what `ssmq_gp_theta_step` takes from their handles."""
        td, to = self.tf_dyn, self.tf_obs
        return (id(td), id(to), td.model.points.tobytes(), to.model.points.tobytes(), td.I_out.shape, to.I_out.shape,
                td.model.points.shape, to.model.points.shape)

    def theta_step(self, theta, mean, cov, y, time):
        """theta (P, param_dim) log-parameters; mean (D,) / cov (D, D) shared by all items or (P, D) / (P, D, D);
        y (Y,) or (P, Y).  Returns conditional posterior means (P, D), covariances (P, D, D), log-likelihoods (P,) and
        the status flags (P,) of `ssmq_gp_theta_step`."""
        c = self._theta_static()
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim < 2:
            theta = theta.reshape(1, -1)
        P = theta.shape[0]
        D = self.mod_dyn.dim_state
        par = np.exp(theta)
        pd = np.ascontiguousarray(par[:, :self.param_dyn_dim])
        po = np.ascontiguousarray(par[:, self.param_dyn_dim:])
        mean, cov = self._augment(mean, cov)
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        cov = np.ascontiguousarray(cov, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        om, oc, ll = np.empty((P, D)), np.empty((P, D, D)), np.empty(P)
        st = np.zeros(P, dtype=np.int32)
        gqg = c['gqg']
        _lib.check(c['fn'](c['h_dyn'], c['pf_dyn'], c['h_obs'], c['pf_obs'], P, pd.ctypes.data, po.ctypes.data,
                           float(self.tf_dyn.model.kernel.jitter),
                           mean.ctypes.data, cov.ctypes.data, 1 if mean.ndim == 1 else 0, y.ctypes.data,
                           1 if y.ndim == 1 else 0, float(time), None if gqg is None else gqg.ctypes.data,
                           c['rr'].ctypes.data, om.ctypes.data, oc.ctypes.data, ll.ctypes.data, st.ctypes.data),
                   'ssmq_gp_theta_step')
        return om, oc, ll, st

    def _param_log_prior(self, theta):
        """log N(theta | param_mean, param_cov) (ssinf.py:1200-1218); host arithmetic on param_dim numbers."""
        d = np.atleast_2d(theta) - self.param_mean
        L = np.linalg.cholesky(self.param_cov)
        v = np.linalg.solve(L, d.T)
        return -0.5 * ((v ** 2).sum(axis=0) + 2 * np.log(np.diag(L)).sum() + self.param_dim * np.log(2 * np.pi))

    def _param_log_likelihood(self, theta, y, k):
        """ssinf.py:1153-1198 for one or many theta rows."""
        ll = self.theta_step(theta, self.x_mean_fi, self.x_cov_fi, y, k)[2]
        return ll if np.ndim(theta) == 2 else float(ll[0])

    def _param_neg_log_posterior(self, theta, y, k):
        """ssinf.py:1220-1241."""
        val = -self._param_log_likelihood(theta, y, k) - self._param_log_prior(theta)
        return val if np.ndim(theta) == 2 else float(val[0])

    def _param_objective_and_gradient(self, theta, y, k):
        """Objective and its forward-difference gradient from ONE theta-batched device call (param_dim + 1 items)."""
        pts = np.vstack((theta, theta + self.fd_step * np.eye(self.param_dim)))
        val = self._param_neg_log_posterior(pts, y, k)
        val = np.where(np.isfinite(val), val, np.inf)
        return float(val[0]), (val[1:] - val[0]) / ((theta + self.fd_step) - theta)

    def _param_posterior_moments(self, y, k):
        """Laplace approximation of the parameter posterior (ssinf.py:1243-1273)."""
        from scipy.optimize import minimize
        res = minimize(self._param_objective_and_gradient, self.param_mean, (y, k), method='BFGS', jac=True)
        self.param_mean, self.param_cov = res.x, res.hess_inv + self.param_jitter

    def _state_posterior_moments(self, theta, y, k):
        """ssinf.py:1117-1151."""
        m, c, _, st = self.theta_step(theta, self.x_mean_fi, self.x_cov_fi, y, k)
        if st.any():
            raise np.linalg.LinAlgError('Matrix is not positive definite (theta item {}, flags {})'.format(
                int(np.flatnonzero(st)[0]), int(st[np.flatnonzero(st)[0]])))
        return (m, c) if np.ndim(theta) == 2 else (m[0], c[0])

    def _measurement_update(self, y, time=None, laplace=None):
        """ssinf.py:1083-1115: all 2 param_dim theta points in one device call.  laplace = (mean, cov) of the parameter
        posterior replaces the optimiser run (a caller that has them already, e.g. to continue from another
        implementation's iterates)."""
        if laplace is None:
            self._param_posterior_moments(y, time)
        else:
            self.param_mean, self.param_cov = np.asarray(laplace[0], dtype=float), np.asarray(laplace[1], dtype=float)
        chol = np.linalg.cholesky(self.param_cov)
        param_pts = self.param_mean[:, None] + chol.dot(self.param_upts)
        mean, cov = self._state_posterior_moments(param_pts.T, y, time)
        self.x_mean_fi = np.einsum('ji,j->i', mean, self.param_wts)
        self.x_cov_fi = np.einsum('kij,k->ij', cov, self.param_wts)
        self._last_theta = param_pts[:, -1].copy()       # the parameters the reference's transforms are left with

    def _predictive_moments(self, time):
        """The generic time update of forward_pass (ssinf.py:104-107 -> :254-295), dynamics half: what the smoother later
        reads as pr_mean / pr_cov / pr_xx_cov.  One device transform with the weights the reference's dynamics transform
        holds at this point (see the class docstring)."""
        par = None if self._last_theta is None else np.exp(self._last_theta[:self.param_dyn_dim])[None, :]
        m_in, P_in = self._augment(np.asarray(self.x_mean_fi, dtype=float), np.asarray(self.x_cov_fi, dtype=float))
        m_pr, P_pr, C = self.tf_dyn.apply(self.mod_dyn.dyn_eval, m_in, P_in, np.atleast_1d(float(time)), par)
        if self.mod_dyn.noise_additive:
            P_pr = P_pr + self.G.dot(self.q_cov).dot(self.G.T)
        return m_pr, P_pr, C[:, :self.mod_dyn.dim_state]

    def _innovations_refusal(self):
        return NotImplementedError('innovation scores cover the additive-noise Gaussian recursion; not implemented for the marginalised '
                                   'filter (its predictive density is a mixture over the kernel parameters)')

    def forward_pass(self, data, keep_predictive=True):
        """data (dim_y, T) -> (D, T), (D, D, T).  ssinf.py:66-118.  The generic time update of step k only feeds the
        smoother (its moments are overwritten by the theta-conditioned ones inside the measurement update):
        keep_predictive=False skips it."""
        data = np.asarray(data, dtype=np.float64)
        T = data.shape[1]
        D = self.mod_dyn.dim_state
        fm, fP = np.zeros((D, T)), np.zeros((D, D, T))
        pm, pP, pC = np.zeros((D, T)), np.zeros((D, D, T)), np.zeros((D, D, T))
        for k in range(1, T + 1):
            if keep_predictive:
                pm[:, k - 1], pP[..., k - 1], pC[..., k - 1] = self._predictive_moments(k - 1)
            self._measurement_update(data[:, k - 1], k)
            fm[:, k - 1], fP[..., k - 1] = self.x_mean_fi, self.x_cov_fi
        self.fi_mean, self.fi_cov = fm, fP
        self.pr_mean, self.pr_cov, self.pr_xx_cov = (pm, pP, pC) if keep_predictive else (None, None, None)
        return fm, fP

    def backward_pass(self):
        """RTS smoothing of the last forward_pass (ssinf.py:120-147, inherited by the reference's MarginalInference): the
        recursion on the device (`ssmq_rts_backward_dev`) over the moments the forward pass kept."""
        assert self.fi_mean is not None and self.pr_mean is not None, 'run forward_pass (keep_predictive=True) first'
        lib = _lib.load()
        D, T = self.fi_mean.shape
        ld = 64

        def planes(a, n):             # (n..., T) -> [T][n][ld], trajectory 0
            buf = np.zeros((T, n, ld))
            buf[:, :, 0] = np.asarray(a, dtype=np.float64).reshape(n, T).T
            if n == D * D:
                buf[:, :, 1:] = np.eye(D).reshape(1, -1, 1)          # padding lanes are never read; keep them PD anyway
            d = _lib.DeviceBuffer(buf.nbytes)
            d.upload(buf)
            return d
        d_fm, d_fP = planes(self.fi_mean, D), planes(self.fi_cov, D * D)
        d_pm, d_pP, d_pC = planes(self.pr_mean, D), planes(self.pr_cov, D * D), planes(self.pr_xx_cov, D * D)
        d_sm, d_sP, d_st = _lib.DeviceBuffer(8 * T * D * ld), _lib.DeviceBuffer(8 * T * D * D * ld), _lib.DeviceBuffer(4 * ld)
        d_st.zero()
        _lib.check(lib.ssmq_rts_backward_dev(D, 1, ld, T, *(ctypes.c_void_p(b.ptr) for b in (d_fm, d_fP, d_pm, d_pP, d_pC, d_sm,
                                                                                             d_sP, d_st))), 'ssmq_rts_backward_dev')
        sm = d_sm.download((T, D, ld))[:, :, 0].T
        sP = d_sP.download((T, D, D, ld))[..., 0].transpose(1, 2, 0)
        st = int(d_st.download((ld,), dtype=np.int32)[0])
        for b in (d_fm, d_fP, d_pm, d_pP, d_pC, d_sm, d_sP, d_st):
            b.free()
        if st:
            raise np.linalg.LinAlgError('Matrix is not positive definite (a predictive covariance of the smoother)')
        self.sm_mean, self.sm_cov = np.ascontiguousarray(sm), np.ascontiguousarray(sP)
        return self.sm_mean, self.sm_cov

    def laplace_batch(self, mean, cov, y, time, prior_mean, prior_cov):
        """The Laplace step (ssinf.py:1243-1273) of B trajectories at once: B BFGS runs in lock step, every round one
        theta-batched device call (`ssmq_gp_marginal_laplace_batch`, csrc/ssmq_bfgs_lockstep.hip).  mean (B, D) / cov (B, D, D)
        filtered moments, y (B, Y), prior_mean (B, P) / prior_cov (B, P, P).  Returns the posterior modes (B, P), the BFGS
        inverse Hessians (B, P, P), status (B,), iterations (B,) and the number of device calls."""
        c = self._theta_static()
        lib = _lib.load()
        mean, cov = self._augment(np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64))
        mean, cov = np.ascontiguousarray(mean), np.ascontiguousarray(cov)
        y = np.ascontiguousarray(y, dtype=np.float64)
        B, P = mean.shape[0], self.param_dim
        pm, pc = np.ascontiguousarray(prior_mean, dtype=np.float64), np.ascontiguousarray(prior_cov, dtype=np.float64)
        theta = pm.copy()
        hinv = np.empty((B, P, P))
        st, it = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        rounds = ctypes.c_int64(0)
        dp = lambda a: None if a is None else a.ctypes.data_as(_lib.c_double_p)       # noqa: E731
        ip = lambda a: a.ctypes.data_as(_lib.c_int32_p)       # noqa: E731
        _lib.check(lib.ssmq_gp_marginal_laplace_batch(c['h_dyn'], ctypes.byref(c['f_dyn']), c['h_obs'], ctypes.byref(c['f_obs']), B,
                                                      float(self.tf_dyn.model.kernel.jitter), dp(mean), dp(cov), dp(y), float(time),
                                                      dp(c['gqg']), dp(c['rr']), dp(pm), dp(pc), float(self.fd_step), dp(theta),
                                                      dp(hinv), ip(st), ip(it), ctypes.byref(rounds)),
                   'ssmq_gp_marginal_laplace_batch')
        return theta, hinv, st, it, int(rounds.value)

    def forward_pass_batch(self, data, **kwargs):
        """data (dim_y, T, B) -> (D, T, B), (D, D, T, B): the Monte-Carlo loop around forward_pass (research/tpq/tpq_base.py:175-192;
        every trajectory from the prior, as `reset()` leaves the filter), ONE call of `ssmq_gp_marginal_filter_batch`
        (csrc/ssmq_marginal.hip): every trajectory walks its own Laplace steps (BFGS), mixtures over the parameter points and time
        steps, and each device round serves whatever the unfinished trajectories are waiting for - the number of rounds is the
        longest trajectory's, not the sum over the steps of the slowest one's (forward_pass_batch_stepwise).
        `batch_failed[b]` = the step at which trajectory b failed (where forward_pass raises LinAlgError), 0 otherwise; its
        moments are NaN from that step on.  `batch_stats`: device rounds, BFGS iterations, theta items."""
        c = self._theta_static()
        lib = _lib.load()
        data = np.asarray(data, dtype=np.float64)
        Y, T, B = data.shape
        D, P = self.mod_dyn.dim_state, self.param_dim
        self.reset()
        y = np.ascontiguousarray(data.transpose(2, 1, 0))                      # (B, T, Y)
        dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_lib.c_double_p)   # noqa: E731
        additive = self.mod_dyn.noise_additive
        qm = None if additive else np.ascontiguousarray(np.atleast_1d(self.q_mean), dtype=np.float64)
        qc = None if additive else np.ascontiguousarray(np.atleast_2d(self.q_cov), dtype=np.float64)
        x0m, x0c = np.ascontiguousarray(self.x0_mean, dtype=np.float64), np.ascontiguousarray(self.x0_cov, dtype=np.float64)
        pm0, pc0 = np.ascontiguousarray(self.param_prior_mean, dtype=np.float64), np.ascontiguousarray(self.param_prior_cov, dtype=np.float64)
        upts, uwts = np.ascontiguousarray(self.param_upts, dtype=np.float64), np.ascontiguousarray(self.param_wts, dtype=np.float64)
        fm, fP = np.empty((B, T, D)), np.empty((B, T, D, D))
        failed = np.zeros(B, dtype=np.int32)
        th, pcl = np.empty((B, P)), np.empty((B, P, P))
        stats = (ctypes.c_int64 * 3)()
        keep = (y, qm, qc, x0m, x0c, pm0, pc0, upts, uwts)                     # alive for the duration of the call
        _lib.check(lib.ssmq_gp_marginal_filter_batch(
            c['h_dyn'], ctypes.byref(c['f_dyn']), c['h_obs'], ctypes.byref(c['f_obs']), B, T, float(self.tf_dyn.model.kernel.jitter),
            dp(y), dp(x0m), dp(x0c), dp(qm), dp(qc), dp(c['gqg']), dp(c['rr']), dp(pm0), dp(pc0), dp(upts), dp(uwts),
            int(self.param_pts_num), float(self.fd_step), float(self.param_jitter[0, 0]), dp(fm), dp(fP),
            failed.ctypes.data_as(_lib.c_int32_p), dp(th), dp(pcl), stats), 'ssmq_gp_marginal_filter_batch')
        del keep
        self.batch_failed = (failed & 0xffff).astype(np.int64) if T < 65536 else failed.astype(np.int64)
        # why (include/ssmq.h): 1 prior not PD, 2 / 3 Laplace covariance not finite / not PD, 4 a mixture point's step failed, 5 mixture not finite
        self.batch_failed_reason = (failed >> 16).astype(np.int64) if T < 65536 else np.zeros(B, dtype=np.int64)
        self.batch_stats = dict(rounds=int(stats[0]), iterations=int(stats[1]), items=int(stats[2]), fallbacks=0)
        self.param_mean, self.param_cov = th[-1], pcl[-1]
        self.batch_param_mean, self.batch_param_cov = th, pcl      # every trajectory's last parameter posterior (B, P), (B, P, P)
        self.fi_mean = np.ascontiguousarray(fm.transpose(2, 1, 0))
        self.fi_cov = np.ascontiguousarray(fP.transpose(2, 3, 1, 0))
        if B and T and not failed[-1]:
            self.x_mean_fi, self.x_cov_fi = fm[-1, -1].copy(), fP[-1, -1].copy()
        return self.fi_mean, self.fi_cov

    def forward_pass_batch_stepwise(self, data, **kwargs):
        """The same with the trajectories in lock step PER TIME STEP (round 4's first version, kept as a second route to the same
        numbers): the Laplace step of every trajectory (`laplace_batch`: B x (param_dim + 1) theta items per device call), then the
        marginalisation over the 2 param_dim parameter sigma points of every trajectory in ONE call (B x 2 param_dim items).
        `batch_failed[b]` = the step at which trajectory b failed (where forward_pass raises LinAlgError), 0 otherwise; its
        moments are NaN from that step on.  `batch_stats`: device rounds, BFGS iterations."""
        data = np.asarray(data, dtype=np.float64)
        Y, T, B = data.shape
        D, P = self.mod_dyn.dim_state, self.param_dim
        self.reset()
        xm = np.tile(np.asarray(self.x0_mean, dtype=float), (B, 1))
        xP = np.tile(np.asarray(self.x0_cov, dtype=float), (B, 1, 1))
        pm = np.tile(self.param_prior_mean, (B, 1))
        pc = np.tile(self.param_prior_cov, (B, 1, 1))
        fm, fP = np.zeros((D, T, B)), np.zeros((D, D, T, B))
        npts = self.param_pts_num
        self.batch_stats = dict(rounds=0, fallbacks=0, iterations=0)
        # failed[b] = step at which trajectory b left the batch (0: still in it).  Where the serial loop raises LinAlgError for a
        # trajectory (a kernel matrix / covariance that is not positive definite at one of its parameter points), the batch keeps
        # going: NaN moments from that step on, the trajectory parked on the prior so that it costs nothing further.
        failed = np.zeros(B, dtype=np.int64)
        pts = None
        for k in range(1, T + 1):
            y = np.ascontiguousarray(data[:, k - 1, :].T)
            theta, hinv, st, it, rounds = self.laplace_batch(xm, xP, y, k, pm, pc)
            self.batch_stats['rounds'] += rounds
            self.batch_stats['iterations'] += int(it.sum())
            pm_new, pc_new = theta, hinv + self.param_jitter
            bad = (st == _lib.BFGS_PRIOR_NOT_PD) | ~np.all(np.isfinite(pm_new), axis=1) | ~np.all(np.isfinite(pc_new), axis=(1, 2))
            # a Laplace covariance that is not positive definite: numpy.linalg.cholesky would raise in _measurement_update
            ok_c = np.all(np.linalg.eigvalsh(np.where(bad[:, None, None], np.eye(P), 0.5 * (pc_new + pc_new.transpose(0, 2, 1)))) > 0, axis=1)
            bad |= ~ok_c
            pm_new[bad], pc_new[bad] = self.param_prior_mean, self.param_prior_cov
            pm, pc = pm_new, pc_new
            chol = np.linalg.cholesky(pc)
            pts = pm[:, :, None] + chol @ self.param_upts                      # (B, P, 2 P)
            items = np.ascontiguousarray(pts.transpose(0, 2, 1)).reshape(B * npts, P)
            m, c, _, sts = self.theta_step(items, np.repeat(xm, npts, axis=0), np.repeat(xP, npts, axis=0),
                                           np.repeat(y, npts, axis=0), k)
            bad |= sts.reshape(B, npts).any(axis=1)
            xm = np.einsum('bjd,j->bd', m.reshape(B, npts, D), self.param_wts)
            xP = np.einsum('bjde,j->bde', c.reshape(B, npts, D, D), self.param_wts)
            bad |= ~np.all(np.isfinite(xm), axis=1) | ~np.all(np.isfinite(xP), axis=(1, 2))
            newly = bad & (failed == 0)
            failed[newly] = k
            out = failed > 0
            xm[out], xP[out] = self.x0_mean, self.x0_cov
            pm[out], pc[out] = self.param_prior_mean, self.param_prior_cov
            fm[:, k - 1, :], fP[:, :, k - 1, :] = xm.T, xP.transpose(1, 2, 0)
            fm[:, k - 1, out], fP[:, :, k - 1, out] = np.nan, np.nan
        self.batch_failed = failed
        self.x_mean_fi, self.x_cov_fi, self.param_mean, self.param_cov = xm[-1], xP[-1], pm[-1], pc[-1]
        self._last_theta = pts[-1, :, -1].copy() if pts is not None else None
        self.fi_mean, self.fi_cov = fm, fP
        return fm, fP

    def forward_pass_serial(self, data, **kwargs):
        """One trajectory after another, one SciPy BFGS run per trajectory and step: the reference's own loop
        (research/tpq/tpq_base.py:175-192 around ssinf.py:66-118); kept as the yardstick of forward_pass_batch."""
        data = np.asarray(data, dtype=np.float64)
        out = []
        for b in range(data.shape[2]):
            self.reset()
            out.append(self.forward_pass(data[..., b], keep_predictive=False))
        self.fi_mean = np.stack([o[0] for o in out], axis=-1)
        self.fi_cov = np.stack([o[1] for o in out], axis=-1)
        return self.fi_mean, self.fi_cov

    def backward_pass_batch(self):
        raise NotImplementedError('the marginalised filter smooths one trajectory at a time: forward_pass + backward_pass')

    def kernel_name(self):
        return 'per theta batch: k_weights x2 | k_pack_wide_consts x2 | k_apply_wave x2 | k_kalman_update | k_gauss_logpdf'


class MarginalizedGaussianProcessKalman(MarginalInference):
    """ssinf.py:1276-1292.  The transforms are built with dim_out = 1 as in the reference, so model_var * I_out is
    broadcast over the whole covariance."""

    def __init__(self, dyn, obs, kernel='rbf', points='ut', point_hyp=None, par_mean=None, par_cov=None):
        kpar_dyn = np.ones((1, dyn.dim_in + 1))
        kpar_obs = np.ones((1, obs.dim_state + 1))
        t_dyn = GaussianProcessTransform(dyn.dim_in, 1, kpar_dyn, kernel, points, point_hyp)
        t_obs = GaussianProcessTransform(obs.dim_state, 1, kpar_obs, kernel, points, point_hyp)
        super().__init__(dyn, obs, t_dyn, t_obs, par_mean, par_cov)


class BootstrapParticleFilter:
    """Bootstrap particle filter (sequential Monte Carlo) on the device - the ground truth the moment-matching filters are measured
    against (`ssmq_particle_filter_dev`, one launch of k_particle_filter<D>: one trajectory per workgroup, the cloud in LDS).  In the
    time convention of the Gaussian filters: x_{-1} ~ init_rv, step j = 0 .. T-1: x_j = f(x_{j-1}, j) + G q, y_j = h(x_j, j) + r; the
    particles are weighted by the measurement density (GaussRV or StudentRV noise) and resampled systematically when the effective
    sample size falls below ess_threshold * num_particles (>= 1: every step, <= 0: never).  A class of its own, not a
    GaussianInference: it has no moment transforms.  A trajectory's results depend on `seed`, its global index, num_particles,
    ess_threshold and its own data alone.

    The initial state and the process noise may each be a GaussRV or a StudentRV (dof >= 2), in any combination: a Student-t draw is
    mean + L z / sqrt(u), u ~ Gamma(dof / 2, scale 2 / dof), as `ssmod.simulate_dev` draws it (`ssmq_particle_filter_rv_dev`,
    k_particle_filter<D, QK=1>) - the ground truth of a heavy-tailed study.  For a StudentRV initial state `x0_cov` is the SCALE
    matrix (default: the random variable's `scale`), not a covariance.  All-Gaussian models run the Gaussian kernels as before.

    It also answers the smoothing question, E[x_k | y_0..T-1], from the same cloud (`ssmq_particle_smoother_dev`): `smoother`,
    `smoother_batch`, `smoother_dev` with method='marginal' - the marginal forward-filter backward-smoother (FFBSm), one launch of
    k_particle_smooth<D>, O(N^2) transition densities per step and trajectory, deterministic given the forward pass; it needs process
    noise of full rank (G Q G' positive definite; for StudentRV process noise G Q G' is the scale and the transition density the
    Student-t's, k_particle_smooth<D, QK=1>) - or method='genealogy' - ancestor tracing (k_particle_lineage<D>), for every model
    the filter covers, with `unique`, the number of distinct ancestors left at each step, as the diagnostic of its collapse.  The
    smoothed initial state x_{-1} is not computed: the filter does not keep its initial cloud."""

    RANGE = ('BootstrapParticleFilter covers forward passes (forward_pass, forward_pass_batch, forward_pass_dev) and particle '
             "smoothers (smoother, smoother_batch, smoother_dev; method='marginal' needs G Q G' positive definite) of built-in "
             'additive-noise models with a GaussRV or StudentRV (dof >= 2) initial state and process noise and GaussRV or StudentRV '
             'measurement noise, '
             'dim_state <= 6, dim_out <= 4, dim_noise <= 6, num_particles a multiple of 64 in 64 .. 4096 with '
             '(2 dim_state + 1) num_particles <= 13312')

    def __init__(self, dyn, obs, num_particles=1024, ess_threshold=0.5, seed=0):
        assert isinstance(dyn, TransitionModel) and isinstance(obs, MeasurementModel)
        from .ssmod import GaussRV, StudentRV
        self.mod_dyn, self.mod_obs = dyn, obs
        self.num_particles, self.ess_threshold, self.seed = int(num_particles), float(ess_threshold), int(seed)
        if is_user_model(dyn) or is_user_model(obs):
            raise NotImplementedError('{}; not implemented for user models (device_code)'.format(self.RANGE))
        if not (dyn.noise_additive and obs.noise_additive):
            raise NotImplementedError('{}; not implemented for models that take their noise as an argument (non-additive noise)'.format(self.RANGE))
        for rv, what in ((dyn.init_rv, 'initial state'), (dyn.noise_rv, 'process noise')):
            if not isinstance(rv, (GaussRV, StudentRV)):
                raise NotImplementedError('{}; not implemented for a {} {}'.format(self.RANGE, type(rv).__name__, what))
        # Student-t on either side: the *_rv entry points; all-Gaussian models keep the entry points they always called
        self._heavy = isinstance(dyn.init_rv, StudentRV) or isinstance(dyn.noise_rv, StudentRV)
        if not isinstance(obs.noise_rv, (GaussRV, StudentRV)):
            raise NotImplementedError('{}; not implemented for {} measurement noise'.format(self.RANGE, type(obs.noise_rv).__name__))
        if np.isnan(self.ess_threshold):
            raise ValueError('ess_threshold must not be NaN')
        self.x0_mean, self.x0_cov = dyn.init_rv.get_stats()[:2]          # StudentRV: the scale matrix, as the kernel reads the plane
        self.G = np.ascontiguousarray(dyn.noise_gain, dtype=np.float64)
        self._check_range()
        self.reset()

    def reset(self):
        self.fi_mean = self.fi_cov = self.status = None
        self.loglik = self.loglik_total = self.ess = None
        self.particles = self.log_weights = self.ancestors = None
        self.sm_mean = self.sm_cov = self.ess_smooth = self.smoothed_log_weights = self.lineage = self.unique = None
        if any(getattr(self, n, None) is not None for n in ('d_loglik', 'd_ess', 'd_ess_smooth')):
            self.free_dev()
        self.d_loglik = self.d_ess = self.d_ess_smooth = None
        self._data = None

    def _initial_planes(self, stage, B, ld, x0_mean=None, x0_cov=None):
        return initial_planes(stage, self.mod_dyn.dim_state, self.x0_mean, self.x0_cov, B, ld, x0_mean, x0_cov)

    def _c_args(self):
        """The model part of the C call (and the arrays it points to, to be kept alive)."""
        from .ssmod import _rv_desc, _lower_factor
        f_dyn, _ = self.mod_dyn.device_integrand()
        f_obs, _ = self.mod_obs.device_integrand()
        r, keep = _rv_desc(self.mod_obs.noise_rv, 'the measurement noise')
        qm = np.ascontiguousarray(self.mod_dyn.noise_rv.mean, dtype=np.float64)
        qL = _lower_factor(self.mod_dyn.noise_rv.get_stats()[1])          # StudentRV: of the scale matrix
        return f_dyn, f_obs, r, qm, qL, keep

    def _rv_args(self):
        """The descriptors of the initial state and the process noise for the *_rv entry points (and what they point to)."""
        from .ssmod import _rv_desc
        x0, keep0 = _rv_desc(self.mod_dyn.init_rv, 'the initial state')
        q, keepq = _rv_desc(self.mod_dyn.noise_rv, 'the process noise')
        return x0, q, (keep0, keepq)

    def _check_range(self):
        """The library's range check, without a device: NotImplementedError (the range named) or ValueError before anything runs."""
        f_dyn, f_obs, r, qm, qL, keep = self._c_args()
        buf = ctypes.create_string_buffer(256)
        if self._heavy:
            x0, q, keep_rv = self._rv_args()
            rc = _lib.load().ssmq_particle_kernel_name_rv(ctypes.byref(f_dyn), ctypes.byref(f_obs), self.mod_dyn.dim_state,
                                                          self.mod_obs.dim_out, qm.size, self.num_particles, ctypes.byref(x0),
                                                          ctypes.byref(q), ctypes.byref(r), buf, 256)
        else:
            rc = _lib.load().ssmq_particle_kernel_name(ctypes.byref(f_dyn), ctypes.byref(f_obs), self.mod_dyn.dim_state, self.mod_obs.dim_out,
                                                       qm.size, self.num_particles, ctypes.byref(r), buf, 256)
        if rc == -1:             # SSMQ_E_ARG
            raise ValueError(_lib.last_error())
        _lib.check(rc, 'ssmq_particle_kernel_name_rv' if self._heavy else 'ssmq_particle_kernel_name', unsupported=True)
        return buf.value.decode()

    def kernel_name(self):
        """The kernel a forward pass launches, with the LDS it requests per trajectory."""
        return self._check_range()

    def _launch(self, lib, B, ld, T, traj_offset, d_y, d_m0, d_P0, d_fm, d_fP, d_ll, d_ess, d_st, d_part=None, d_logw=None, d_anc=None):
        if T < 1:
            raise ValueError('BootstrapParticleFilter: at least one time step is needed (T = {})'.format(T))
        f_dyn, f_obs, r, qm, qL, keep = self._c_args()
        vp, dp = _lib.vp, _lib.dp
        if self._heavy:
            x0, q, keep_rv = self._rv_args()
            _lib.check(lib.ssmq_particle_filter_rv_dev(ctypes.byref(f_dyn), ctypes.byref(f_obs), self.mod_dyn.dim_state, self.mod_obs.dim_out,
                                                       qm.size, self.num_particles, B, ld, T, vp(d_y), vp(d_m0), vp(d_P0), ctypes.byref(x0),
                                                       ctypes.byref(q), dp(self.G), ctypes.byref(r), self.ess_threshold,
                                                       ctypes.c_uint64(self.seed), ctypes.c_uint64(int(traj_offset)), vp(d_fm), vp(d_fP),
                                                       vp(d_ll), vp(d_ess), vp(d_st), vp(d_part), vp(d_logw), vp(d_anc)),
                       'ssmq_particle_filter_rv_dev', unsupported=True)
            return
        _lib.check(lib.ssmq_particle_filter_dev(ctypes.byref(f_dyn), ctypes.byref(f_obs), self.mod_dyn.dim_state, self.mod_obs.dim_out,
                                                qm.size, self.num_particles, B, ld, T, vp(d_y), vp(d_m0), vp(d_P0), dp(qm), dp(qL),
                                                dp(self.G), ctypes.byref(r), self.ess_threshold, ctypes.c_uint64(self.seed),
                                                ctypes.c_uint64(int(traj_offset)), vp(d_fm), vp(d_fP), vp(d_ll), vp(d_ess), vp(d_st),
                                                vp(d_part), vp(d_logw), vp(d_anc)), 'ssmq_particle_filter_dev', unsupported=True)

    def forward_pass_dev(self, d_y, B, ld, T, traj_offset=0):
        """Filter measurements that are already on the device (planes [T][dim_y][ld], e.g. from `ssmod.simulate_dev`) and leave the
        results there: returns the triple of the Gaussian filters, DeviceBuffers (d_fm [T][D][ld], d_fP [T][D*D][ld], d_status [ld]) for
        `mcshard.device_error_sums` / `device_traj_scores` / `device_score_bars`; the caller frees them.  The log-likelihood increments
        [T + 1][ld] (row T: the total) and the effective sample sizes [T][ld] stay on the device as `d_loglik` / `d_ess`: the filter owns
        these two - the next forward_pass_dev, `reset()` or `free_dev()` frees them.  Every trajectory starts from the model's initial
        moments; trajectory b draws from the stream of global index traj_offset + b."""
        lib = _lib.load()
        D = self.mod_dyn.dim_state
        self.free_dev()
        with _lib.Staging() as stage:
            d_m0, d_P0 = self._initial_planes(stage, B, ld)
            d_fm, d_fP, d_st = stage.device(8 * T * D * ld), stage.device(8 * T * D * D * ld), stage.device(4 * ld)
            d_ll, d_ess = stage.device(8 * (T + 1) * ld), stage.device(8 * T * ld)
            d_st.zero()
            self._launch(lib, B, ld, T, traj_offset, d_y, d_m0, d_P0, d_fm, d_fP, d_ll, d_ess, d_st)
            stage.release(d_fm, d_fP, d_st, d_ll, d_ess)
        self.d_loglik, self.d_ess = d_ll, d_ess
        return d_fm, d_fP, d_st

    def free_dev(self):
        """Frees the device planes the last forward_pass_dev or smoother_dev left with the filter (`d_loglik`, `d_ess`,
        `d_ess_smooth`)."""
        if self.d_loglik is not None:        # (the two are set together)
            self.d_loglik.free()
            self.d_ess.free()
        if getattr(self, 'd_ess_smooth', None) is not None:
            self.d_ess_smooth.free()
        self.d_loglik = self.d_ess = self.d_ess_smooth = None

    def forward_pass_batch(self, data, x0_mean=None, x0_cov=None, raise_on_failure=True, return_particles=False):
        """data (dim_y, T, B) -> filtered means (D, T, B) and covariances (D, D, T, B): the weighted mean and covariance of the cloud
        after each measurement.  Optional per-trajectory initial moments x0_mean (B, D), x0_cov (B, D, D).  Sets fi_mean, fi_cov,
        status (B,) (0, or 1 + the step whose largest log-weight was not finite: NaN from there on), loglik (T, B) - the increments
        log p(y_j | y_0..j-1) -, loglik_total (B,) and ess (T, B); with return_particles also particles (D, N, T, B) after the
        propagation of each step, log_weights (N, T, B) after its measurement (normalised, before resampling) and ancestors
        (N, T, B) chosen after it (the identity where the step did not resample)."""
        lib = _lib.load()
        data = np.asarray(data, dtype=np.float64)
        Y, T, B = data.shape
        if Y != self.mod_obs.dim_out:
            raise ValueError('data must have shape (dim_y = {}, T, B)'.format(self.mod_obs.dim_out))
        if T < 1:
            raise ValueError('BootstrapParticleFilter: at least one time step is needed (T = {})'.format(T))
        self._data = data
        D, N = self.mod_dyn.dim_state, self.num_particles
        ld = _lib.padded(B)
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_m0, d_P0 = self._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d_fm, d_fP, d_st = stage.scratch(8 * T * D * ld), stage.scratch(8 * T * D * D * ld), stage.scratch(4 * ld)
            d_ll, d_ess = stage.scratch(8 * (T + 1) * ld), stage.scratch(8 * T * ld)
            d_part = d_logw = d_anc = None
            if return_particles:
                d_part, d_logw, d_anc = stage.scratch(8 * T * D * B * N), stage.scratch(8 * T * B * N), stage.scratch(4 * T * B * N)
            d_st.zero()
            self._launch(lib, B, ld, T, 0, d_y, d_m0, d_P0, d_fm, d_fP, d_ll, d_ess, d_st, d_part, d_logw, d_anc)
            fm = _lib.download_study(d_fm, (D,), T, B, ld)
            fP = _lib.download_study(d_fP, (D, D), T, B, ld)
            self.status = d_st.download((ld,), dtype=np.int32)[:B]
            ll = d_ll.download((T + 1, ld))
            self.loglik, self.loglik_total = np.ascontiguousarray(ll[:T, :B]), ll[T, :B].copy()
            self.ess = np.ascontiguousarray(d_ess.download((T, ld))[:, :B])
            if return_particles:
                self.particles = np.ascontiguousarray(d_part.download((T, D, B, N)).transpose(1, 3, 0, 2))
                self.log_weights = np.ascontiguousarray(d_logw.download((T, B, N)).transpose(2, 0, 1))
                self.ancestors = np.ascontiguousarray(d_anc.download((T, B, N), dtype=np.int32).transpose(2, 0, 1))
            else:
                self.particles = self.log_weights = self.ancestors = None
        self.fi_mean, self.fi_cov = fm, fP
        if raise_on_failure:
            _raise_failed(self.status, message='Particle filter degenerate: no finite log-weight (trajectory {}, step {})')
        return self.fi_mean, self.fi_cov

    def forward_pass(self, data):
        """data (dim_y, T) -> filtered means (D, T), covariances (D, D, T): trajectory 0 of a batch of one."""
        fm, fP = self.forward_pass_batch(np.asarray(data)[..., None])
        return fm[..., 0], fP[..., 0]

    # ---- particle smoothers over the cloud of a forward pass -------------------------------------------------------------------------
    SMOOTHER_METHODS = {'marginal': 0, 'genealogy': 1}        # SSMQ_PS_MARGINAL, SSMQ_PS_GENEALOGY

    def _smoother_check(self, method):
        """The library's range check of a smoother, without a device: ValueError for an unknown method (or a condition number of
        G Q G' above 1e12), NotImplementedError where method='marginal' has no transition density to work with."""
        if method not in self.SMOOTHER_METHODS:
            raise ValueError("BootstrapParticleFilter: unknown smoother method {!r} ('marginal' or 'genealogy')".format(method))
        f_dyn, f_obs, r, qm, qL, keep = self._c_args()
        buf = ctypes.create_string_buffer(256)
        if self._heavy:
            x0, q, keep_rv = self._rv_args()
            rc = _lib.load().ssmq_particle_smoother_kernel_name_rv(ctypes.byref(f_dyn), self.mod_dyn.dim_state, qm.size, self.num_particles,
                                                                   ctypes.byref(q), _lib.dp(self.G), self.SMOOTHER_METHODS[method], buf, 256)
        else:
            rc = _lib.load().ssmq_particle_smoother_kernel_name(ctypes.byref(f_dyn), self.mod_dyn.dim_state, qm.size, self.num_particles,
                                                                _lib.dp(qm), _lib.dp(qL), _lib.dp(self.G), self.SMOOTHER_METHODS[method], buf, 256)
        if rc == -1:             # SSMQ_E_ARG
            raise ValueError(_lib.last_error())
        _lib.check(rc, 'ssmq_particle_smoother_kernel_name_rv' if self._heavy else 'ssmq_particle_smoother_kernel_name', unsupported=True)
        return buf.value.decode()

    def smoother_kernel_name(self, method='marginal'):
        """The kernel a smoother of this method launches after the forward pass, with the LDS it requests per trajectory."""
        return self._smoother_check(method)

    def cloud_block(self, T, B, cloud_bytes=2 ** 30):
        """Trajectories per block of a smoother pass: the weighted cloud of a block, (8 (D + 1) + 4) T N bytes per trajectory, fits
        cloud_bytes (at least one trajectory)."""
        per = (8 * (self.mod_dyn.dim_state + 1) + 4) * int(T) * self.num_particles
        return int(max(1, min(int(B), int(cloud_bytes) // per)))

    def _smooth_blocks(self, lib, stage, method, B, ld, T, traj_offset, cloud_bytes, d_y, d_m0, d_P0, d, host=None):
        """Forward pass with the cloud kept, then the smoother, in consecutive blocks of `cloud_block` trajectories: block b0 works on
        the planes of `d` (fm, fP, ll, ess, st, sm, sP, ess_s, unique - pitch ld) from column b0 on and draws from the streams
        traj_offset + b0 .., so that nothing depends on the block size.  host: dict of host arrays in the device's layout
        (particles (T, D, B, N), log_weights, smoothed_log_weights (T, B, N), ancestors, lineage (T, B, N) int32) the clouds are
        downloaded into, block by block."""
        D, N, code = self.mod_dyn.dim_state, self.num_particles, self.SMOOTHER_METHODS[method]
        f_dyn, f_obs, r, qm, qL, keep = self._c_args()
        vp, dp = _lib.vp, _lib.dp
        if self._heavy:
            x0, q, keep_rv = self._rv_args()
        nb = self.cloud_block(T, B, cloud_bytes)
        d_part, d_logw, d_anc = stage.scratch(8 * T * D * nb * N), stage.scratch(8 * T * nb * N), stage.scratch(4 * T * nb * N)
        d_lws = stage.scratch(8 * T * nb * N) if host is not None else None
        d_lin = stage.scratch(4 * T * nb * N) if host is not None and code == 1 else None
        for b0 in range(0, B, nb):
            n = min(nb, B - b0)
            at = lambda name: d[name].view((4 if name in ('st', 'unique') else 8) * b0)          # noqa: E731
            self._launch(lib, n, ld, T, traj_offset + b0, d_y.view(8 * b0), d_m0.view(8 * b0), d_P0.view(8 * b0), at('fm'), at('fP'),
                         at('ll'), at('ess'), at('st'), d_part, d_logw, d_anc)
            clouds = (vp(d_part), vp(d_logw), vp(d_anc), vp(at('fm')), vp(at('fP')), vp(at('ess')), vp(at('st')), vp(at('sm')), vp(at('sP')),
                      vp(at('ess_s')), vp(d_lws), vp(d_lin), vp(at('unique')) if code == 1 else None)
            if self._heavy:
                _lib.check(lib.ssmq_particle_smoother_rv_dev(ctypes.byref(f_dyn), D, qm.size, N, n, ld, T, ctypes.byref(q), dp(self.G), code,
                                                             *clouds), 'ssmq_particle_smoother_rv_dev', unsupported=True)
            else:
                _lib.check(lib.ssmq_particle_smoother_dev(ctypes.byref(f_dyn), D, qm.size, N, n, ld, T, dp(qm), dp(qL), dp(self.G), code,
                                                          *clouds), 'ssmq_particle_smoother_dev', unsupported=True)
            if host is not None:
                host['particles'][:, :, b0:b0 + n] = d_part.download((T, D, n, N))
                host['log_weights'][:, b0:b0 + n] = d_logw.download((T, n, N))
                host['ancestors'][:, b0:b0 + n] = d_anc.download((T, n, N), dtype=np.int32)
                host['smoothed_log_weights'][:, b0:b0 + n] = d_lws.download((T, n, N))
                if code == 1:
                    host['lineage'][:, b0:b0 + n] = d_lin.download((T, n, N), dtype=np.int32)

    def smoother_dev(self, d_y, B, ld, T, method='marginal', traj_offset=0, cloud_bytes=2 ** 30):
        """Smooth measurements that are already on the device (planes [T][dim_y][ld]) and leave the results there: returns the triple
        of the Gaussian smoothers, DeviceBuffers (d_sm [T][D][ld], d_sP [T][D*D][ld], d_status [ld]) for `mcshard.device_error_sums` /
        `device_traj_scores` / `device_score_bars`; the caller frees them.  The forward pass runs first, with the cloud kept on the
        device: (8 (D + 1) + 4) T B N bytes, processed in consecutive blocks of trajectories whose cloud fits cloud_bytes - the results
        do not depend on the block size, bit for bit.  `d_ess_smooth` [T][ld], like `d_loglik` and `d_ess` of the forward pass, stays
        with the filter: the next forward_pass_dev or smoother_dev, `reset()` or `free_dev()` frees them.  Trajectory b draws from the
        stream of global index traj_offset + b.  The smoothed initial state is not computed."""
        self._smoother_check(method)
        if T < 1:
            raise ValueError('BootstrapParticleFilter: at least one time step is needed (T = {})'.format(T))
        lib = _lib.load()
        D = self.mod_dyn.dim_state
        self.free_dev()
        with _lib.Staging() as stage:
            d_m0, d_P0 = self._initial_planes(stage, B, ld)
            d = dict(fm=stage.scratch(8 * T * D * ld), fP=stage.scratch(8 * T * D * D * ld), ll=stage.device(8 * (T + 1) * ld),
                     ess=stage.device(8 * T * ld), st=stage.device(4 * ld), sm=stage.device(8 * T * D * ld),
                     sP=stage.device(8 * T * D * D * ld), ess_s=stage.device(8 * T * ld), unique=stage.scratch(4 * T * ld))
            d['st'].zero()
            self._smooth_blocks(lib, stage, method, B, ld, T, traj_offset, cloud_bytes, d_y, d_m0, d_P0, d)
            stage.release(d['sm'], d['sP'], d['st'], d['ll'], d['ess'], d['ess_s'])
        self.d_loglik, self.d_ess, self.d_ess_smooth = d['ll'], d['ess'], d['ess_s']
        return d['sm'], d['sP'], d['st']

    def smoother_batch(self, data, method='marginal', x0_mean=None, x0_cov=None, raise_on_failure=True, return_particles=False,
                       cloud_bytes=2 ** 30):
        """data (dim_y, T, B) -> smoothed means (D, T, B) and covariances (D, D, T, B): the moments of the smoothing posterior
        p(x_k | y_0..T-1) from the particle filter's cloud.  method='marginal': the marginal forward-filter backward-smoother, the
        cloud of step k re-weighted by exp(ls_k) (needs G Q G' positive definite: NotImplementedError otherwise); method='genealogy':
        the ancestors of the final particles under the final weights (every model; `unique` (T, B), the number of distinct
        ancestors, tells where it has collapsed).  Step T-1 is the filter's.  Runs `forward_pass_batch` with the cloud kept on the
        device, then the smoother, in consecutive blocks of trajectories whose cloud - (8 (D + 1) + 4) T N bytes per trajectory - fits
        cloud_bytes; the results do not depend on the block size, bit for bit.  Sets sm_mean, sm_cov, ess_smooth (T, B) and
        everything forward_pass_batch sets; with return_particles also smoothed_log_weights (N, T, B) (genealogy: the final weights,
        repeated) and for 'genealogy' lineage (N, T, B).  A trajectory the filter failed on is NaN at every step, its status kept.
        The smoothed initial state x_{-1} is not computed: the filter does not keep its initial cloud."""
        self._smoother_check(method)
        lib = _lib.load()
        data = np.asarray(data, dtype=np.float64)
        Y, T, B = data.shape
        if Y != self.mod_obs.dim_out:
            raise ValueError('data must have shape (dim_y = {}, T, B)'.format(self.mod_obs.dim_out))
        if T < 1:
            raise ValueError('BootstrapParticleFilter: at least one time step is needed (T = {})'.format(T))
        self._data = data
        D, N = self.mod_dyn.dim_state, self.num_particles
        ld = _lib.padded(B)
        host = None
        if return_particles:
            host = dict(particles=np.empty((T, D, B, N)), log_weights=np.empty((T, B, N)), smoothed_log_weights=np.empty((T, B, N)),
                        ancestors=np.empty((T, B, N), dtype=np.int32), lineage=np.empty((T, B, N), dtype=np.int32))
        with _lib.Staging() as stage:
            d_y = stage.scratch(8 * T * Y * ld)
            _lib.upload_study(data, Y, ld, d_y)
            d_m0, d_P0 = self._initial_planes(stage, B, ld, x0_mean, x0_cov)
            d = dict(fm=stage.scratch(8 * T * D * ld), fP=stage.scratch(8 * T * D * D * ld), ll=stage.scratch(8 * (T + 1) * ld),
                     ess=stage.scratch(8 * T * ld), st=stage.scratch(4 * ld), sm=stage.scratch(8 * T * D * ld),
                     sP=stage.scratch(8 * T * D * D * ld), ess_s=stage.scratch(8 * T * ld), unique=stage.scratch(4 * T * ld))
            d['st'].zero()
            self._smooth_blocks(lib, stage, method, B, ld, T, 0, cloud_bytes, d_y, d_m0, d_P0, d, host)
            self.fi_mean, self.fi_cov = _lib.download_study(d['fm'], (D,), T, B, ld), _lib.download_study(d['fP'], (D, D), T, B, ld)
            self.sm_mean, self.sm_cov = _lib.download_study(d['sm'], (D,), T, B, ld), _lib.download_study(d['sP'], (D, D), T, B, ld)
            self.status = d['st'].download((ld,), dtype=np.int32)[:B]
            ll = d['ll'].download((T + 1, ld))
            self.loglik, self.loglik_total = np.ascontiguousarray(ll[:T, :B]), ll[T, :B].copy()
            self.ess = np.ascontiguousarray(d['ess'].download((T, ld))[:, :B])
            self.ess_smooth = np.ascontiguousarray(d['ess_s'].download((T, ld))[:, :B])
            self.unique = np.ascontiguousarray(d['unique'].download((T, ld), dtype=np.int32)[:, :B]) if method == 'genealogy' else None
        self.particles = self.log_weights = self.ancestors = self.smoothed_log_weights = self.lineage = None
        if return_particles:
            self.particles = np.ascontiguousarray(host['particles'].transpose(1, 3, 0, 2))
            for name in ('log_weights', 'ancestors', 'smoothed_log_weights') + (('lineage',) if method == 'genealogy' else ()):
                setattr(self, name, np.ascontiguousarray(host[name].transpose(2, 0, 1)))
        if raise_on_failure:
            _raise_failed(self.status, message='Particle filter degenerate: no finite log-weight (trajectory {}, step {})')
        return self.sm_mean, self.sm_cov

    def smoother(self, data, method='marginal'):
        """data (dim_y, T) -> smoothed means (D, T), covariances (D, D, T): trajectory 0 of a batch of one."""
        sm, sP = self.smoother_batch(np.asarray(data)[..., None], method=method)
        return sm[..., 0], sP[..., 0]

    def _refuse(self, what):
        raise NotImplementedError('{}; {} is not implemented for it'.format(self.RANGE, what))


def _refusing(name, what):
    def method(self, *args, **kwargs):
        self._refuse(what)
    method.__name__ = name
    return method


# what a GaussianInference has and the particle filter refuses: (method, its wording in the NotImplementedError)
for _name, _what in (('backward_pass', 'the RTS smoother (backward_pass)'), ('backward_pass_batch', 'the RTS smoother (backward_pass_batch)')) + \
        tuple((n, n) for n in ('innovations', 'innovations_batch', 'innovations_dev', 'innovations_kernel_name', 'iterated_pass',
                               'iterated_pass_batch', 'iterated_pass_dev', 'iterated_kernel_name', 'iterated_smoother',
                               'iterated_smoother_batch', 'iterated_smoother_dev', 'iterated_smoother_kernel_name', 'robust_pass',
                               'robust_pass_batch', 'robust_pass_dev', 'robust_kernel_name', 'masked_pass', 'masked_pass_batch',
                               'masked_pass_dev', 'masked_kernel_name')):
    setattr(BootstrapParticleFilter, _name, _refusing(_name, _what))


# ---------------------------------------------------------------------------------------------------------------
# The floor of a filter study: the posterior Cramer-Rao lower bound (Tichavsky, Muravchik, Nehorai 1998) from the true states
# ---------------------------------------------------------------------------------------------------------------
def posterior_crlb_dev(dyn, obs, d_x, B, ld, T):
    """The bound from true states that are already on the device: d_x planes [T + 1][dim_state][ld], the raw output of
    `ssmod.simulate_dev(dyn, obs, T + 1, B)` (plane 0 the initial state, plane j + 1 the state the filters call x_j).  One process:
    `mcshard.device_crlb_sums` then `mcshard.finalize_crlb`, whose dict it returns - info (D, D, T), bound (D, D, T) with
    E[(x_j - m_j)(x_j - m_j)'] >= bound[:, :, j] for every estimator m_j of x_j from y_0 .. y_j, rmse_bound (T,) = sqrt(trace bound),
    status.  Additive Gaussian noise, models with a Jacobian on the device (the built-in ones that have one, user models with
    `device_jacobian`), dim_state <= 6, dim_out <= 4, process noise of full rank; NotImplementedError names the range otherwise."""
    from . import mcshard
    return mcshard.finalize_crlb(mcshard.device_crlb_sums(dyn, obs, d_x, B, ld, T), dyn, B)


def posterior_crlb(dyn, obs, x):
    """`posterior_crlb_dev` for true states on the host: x (dim_state, T + 1, B), x[:, 0] the initial states."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3 or x.shape[0] != dyn.dim_state or x.shape[1] < 2:
        raise ValueError('posterior_crlb: x must have shape (dim_state = {}, T + 1 >= 2, B), got {}'.format(dyn.dim_state, x.shape))
    D, T1, B = x.shape
    ld = _lib.padded(B)
    with _lib.Staging() as stage:
        d_x = stage.device(8 * T1 * D * ld)
        _lib.upload_study(x, D, ld, d_x)
        return posterior_crlb_dev(dyn, obs, d_x, B, ld, T1 - 1)
