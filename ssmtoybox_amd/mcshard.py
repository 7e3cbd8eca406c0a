"""
Sharding of independent Monte-Carlo trajectories across ranks (one process per GPU) and the final aggregation of the
error sums - the only collective of the path.

Trajectories never interact inside the moment-transform / filter path (the reference loops `for imc in range(mc)`,
research/tpq/tpq_base.py:187-189), so each rank owns a contiguous slice of the MC index and no data-path collective
exists.  Phase 1 all-reduces per-time-step sums (squared error, RMSE, NLL, MSE matrix, counts) that a reduction kernel
produced from the filter's own output buffers; phase 2 - only if the log-credibility ratio is wanted, because it needs
the GLOBAL MSE matrix per step (utils.py:113-120 via research/tpq/tpq_base.py:167-169) - all-reduces the LCR sums.
Messages are a few KB: latency-bound, one fused all-reduce per phase.

The collective itself is `ssmq_allreduce_sum` of the C ABI: RCCL over xGMI, opened by libssmq at run time, no PyTorch
(`RcclComm`).  Rendezvous needs only the launcher's environment (RANK, WORLD_SIZE, MASTER_PORT): rank 0 creates the
128-byte RCCL id and leaves it in a file that the other ranks of the node pick up.  `TorchComm` wraps a
`torch.distributed` process group instead - used by the CPU tests (gloo, no GPU, no RCCL) and for rehearsals with several
ranks on one GPU.
"""
import ctypes
import os
import time

import numpy as np

from . import _lib


def shard_bounds(total, rank, world):
    """Contiguous slice [lo, hi) of `total` trajectories owned by `rank`; sizes differ by at most one."""
    base, rem = divmod(int(total), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


# ---------------------------------------------------------------------------------------------------------------
# communicators
# ---------------------------------------------------------------------------------------------------------------
class SingleComm:
    """One process: every reduction is the identity."""
    rank, world = 0, 1

    def allreduce_sum(self, flat):
        return flat

    def allreduce_max(self, flat):
        return flat

    def barrier(self):
        if _lib.device_count() > 0:
            _lib.sync()

    def close(self):
        pass


def _id_file(rank_env=None):
    """Where rank 0 leaves the RCCL id for the other ranks of this launch.  All ranks of one node are children of one
    launcher process, so (parent pid, MASTER_PORT) names the launch; SSMQ_RCCL_ID_FILE overrides."""
    explicit = os.environ.get('SSMQ_RCCL_ID_FILE')
    if explicit:
        return explicit
    tmp = os.environ.get('TMPDIR', '/tmp')
    # an elastic restart keeps (ppid, port, run id): the restart count tells the attempts apart
    return os.path.join(tmp, 'ssmq_rccl_{}_{}_{}_{}.id'.format(
        os.getppid(), os.environ.get('MASTER_PORT', '0'), os.environ.get('TORCHELASTIC_RUN_ID', 'none'),
        os.environ.get('TORCHELASTIC_RESTART_COUNT', '0')))


class RcclComm:
    """RCCL communicator behind the C ABI (ssmq_comm_*).  One per process; the device must be selected first."""

    def __init__(self, rank, world, id_file=None, timeout_s=300.0, force=False, init_timeout_s=240.0):
        """force: create an RCCL communicator even for world = 1 (rehearsal of the RCCL path on one GPU)."""
        lib = _lib.load()
        self.rank, self.world = int(rank), int(world)
        self._file = id_file or _id_file()
        self._rccl = self.world > 1 or force
        buf = ctypes.create_string_buffer(128)
        if self._rccl:
            if self.rank == 0:
                # nothing of an earlier attempt under the same name may be taken for this one's
                import glob
                for stale in [self._file] + glob.glob(self._file + '.st*'):
                    try:
                        os.unlink(stale)
                    except OSError:
                        pass
                _lib.check(lib.ssmq_comm_unique_id(buf, 128), 'ssmq_comm_unique_id')
                tmp = self._file + '.tmp{}'.format(os.getpid())
                with open(tmp, 'wb') as f:
                    f.write(buf.raw)
                os.replace(tmp, self._file)          # atomic: readers see all 128 bytes or no file
            else:
                t0 = time.time()
                while True:
                    try:
                        # a file left behind by an earlier launch that happened to share (ppid, port) is older than this
                        # process: ignore it
                        if os.path.getmtime(self._file) >= _process_start_time() - 1.0:
                            with open(self._file, 'rb') as f:
                                raw = f.read()
                            if len(raw) == 128:
                                break
                    except OSError:
                        pass
                    if _fresh_content(self._file + '.st0') == b'0':
                        raise _lib.SsmqError('RCCL rendezvous: rank 0 could not create the id')
                    if time.time() - t0 > timeout_s:
                        raise _lib.SsmqError('RCCL rendezvous: no id file {} after {} s'.format(self._file, timeout_s))
                    time.sleep(0.01)
                buf = ctypes.create_string_buffer(raw, 128)
        # ncclCommInitRank is collective: if a peer never arrives it blocks for good.  It runs on a helper thread (ctypes
        # releases the GIL) so that this rank can give up after init_timeout_s and report the failure (open_comm then
        # moves every rank to the gloo fallback); a thread left behind in RCCL is abandoned (hung_init).
        self.hung_init = False
        if self._rccl and (self.world > 1 or os.environ.get('SSMQ_RCCL_INIT_THREAD') == '1'):   # (env: one-rank rehearsal)
            import threading
            box = {}
            dev = lib.ssmq_current_device()              # HIP's current device is per thread: select it over there too

            def _init():
                try:
                    if dev >= 0:
                        _lib.check(lib.ssmq_set_device(dev), 'ssmq_set_device')
                    box['rc'] = lib.ssmq_comm_init(self.rank, self.world, buf, 128)
                    box['err'] = _lib.last_error() if box['rc'] else ''
                except Exception as e:                   # noqa: BLE001
                    box['rc'], box['err'] = -1, str(e)
            th = threading.Thread(target=_init, daemon=True)
            th.start()
            th.join(init_timeout_s)
            if th.is_alive():
                self.hung_init = True
                lib.ssmq_comm_abandon_init()             # the thread still holds stdout on stderr: take it back
                raise _lib.SsmqError('RCCL communicator: ncclCommInitRank did not return within {} s'.format(init_timeout_s))
            if box.get('rc'):
                raise _lib.SsmqError('ssmq_comm_init failed (code {}): {}'.format(box['rc'], box.get('err', '')))
        else:
            _lib.check(lib.ssmq_comm_init(self.rank, self.world, buf if self._rccl else None, 128), 'ssmq_comm_init')

    def _reduce(self, fn, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float64).copy()
        if self._rccl and flat.size:
            _lib.check(fn(flat.ctypes.data_as(_lib.c_double_p), flat.size), 'ssmq_allreduce')
        return flat

    def allreduce_sum(self, flat):
        return self._reduce(_lib.load().ssmq_allreduce_sum, flat)

    def allreduce_max(self, flat):
        return self._reduce(_lib.load().ssmq_allreduce_max, flat)

    def barrier(self):
        _lib.check(_lib.load().ssmq_comm_barrier(), 'ssmq_comm_barrier')

    def close(self):
        self.barrier()                                # nobody is still looking for the id file
        _lib.check(_lib.load().ssmq_comm_destroy(), 'ssmq_comm_destroy')
        for path in ([self._file] if self.rank == 0 and self._rccl else []) + [getattr(self, 'status_file', None)]:
            try:
                if path:
                    os.unlink(path)
            except OSError:
                pass


def _fresh_content(path):
    """Content of a rendezvous file written by this launch (not older than the launcher), else None."""
    try:
        if os.path.getmtime(path) >= _process_start_time() - 1.0:
            with open(path, 'rb') as f:
                return f.read()
    except OSError:
        pass
    return None


def _process_start_time():
    try:
        return os.stat('/proc/{}'.format(os.getppid())).st_ctime
    except OSError:
        return 0.0


class TorchComm:
    """A torch.distributed process group as the communicator (CPU tests over gloo; rehearsals)."""

    def __init__(self, dist, device=None):
        self.dist = dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.device = device or ('cuda' if dist.get_backend() == 'nccl' else 'cpu')

    def _reduce(self, flat, op):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float64).copy()).to(self.device)
        if self.world > 1:
            self.dist.all_reduce(t, op=op)
        return t.cpu().numpy()

    def allreduce_sum(self, flat):
        return self._reduce(flat, self.dist.ReduceOp.SUM)

    def allreduce_max(self, flat):
        return self._reduce(flat, self.dist.ReduceOp.MAX)

    def barrier(self):
        if _lib.device_count() > 0:
            _lib.sync()
        self.dist.barrier()

    def close(self):
        self.dist.barrier()


def open_comm(rank, world, force_rccl=False, consensus_timeout_s=120.0, log=None):
    """Communicator of a launched job: RCCL behind the C ABI; if creating it fails on ANY rank, every rank falls back to
    a torch.distributed gloo group (the collective is a few KB at the end of the run, never the data path) and says so.
    The ranks agree through one status file each next to the id file, so no rank is left waiting inside a collective
    that others never entered."""
    if world <= 1 and not force_rccl:
        return SingleComm()
    comm, err = None, ''
    try:
        comm = RcclComm(rank, world, force=force_rccl)
    except Exception as e:                                   # noqa: BLE001 - any failure means "no RCCL on this rank"
        err = '{}: {}'.format(type(e).__name__, e)
    hung = 'did not return' in err
    if world <= 1:
        if comm is None:
            raise _lib.SsmqError('RCCL communicator: ' + err)
        return comm
    base = _id_file()
    with open('{}.st{}.tmp'.format(base, rank), 'wb') as f:
        f.write(b'1' if comm is not None else b'0')
    os.replace('{}.st{}.tmp'.format(base, rank), '{}.st{}'.format(base, rank))
    t0, states = time.time(), {}
    while len(states) < world and time.time() - t0 < consensus_timeout_s:
        for r in range(world):
            if r not in states:
                v = _fresh_content('{}.st{}'.format(base, r))
                if v in (b'0', b'1'):
                    states[r] = v == b'1'
        if len(states) < world:
            time.sleep(0.01)
    if len(states) == world and all(states.values()):
        comm.status_file = '{}.st{}'.format(base, rank)
        return comm
    why = err or 'rank(s) {} reported no RCCL communicator'.format(
        sorted(set(range(world)) - {r for r, ok in states.items() if ok}))
    (log or (lambda m: None))('rank {}: RCCL unavailable ({}); all-reduce falls back to gloo'.format(rank, why))
    import torch.distributed as dist
    dist.init_process_group('gloo')                          # every rank is past the status files once this returns
    try:
        os.unlink('{}.st{}'.format(base, rank))
    except OSError:
        pass
    fb = TorchComm(dist)
    fb.fallback_reason = why
    fb.abandoned_rccl_thread = hung      # the caller should leave with os._exit once its output is written
    return fb


def _as_comm(comm):
    """None -> single process; an object with is_initialized() (torch.distributed) -> TorchComm; else as given."""
    if comm is None:
        return SingleComm()
    if hasattr(comm, 'is_initialized'):
        return TorchComm(comm) if comm.is_initialized() else SingleComm()
    return comm


# ---------------------------------------------------------------------------------------------------------------
# device-side sums of this rank's trajectories
# ---------------------------------------------------------------------------------------------------------------
def device_error_sums(D, B, ld, T, d_x, d_fm, d_fP, d_status=None):
    """Phase-1 sums of this rank's trajectories, reduced on the device (`ssmq_error_sums_dev`).
    d_x, d_fm: DeviceBuffer planes [T][D][ld]; d_fP [T][D*D][ld] (the buffers the filter wrote); d_status [ld] or None.
    Returns a dict of arrays: se (T, D) squared error (utils.py:18-38), rmse (T,) sum of ||x - m|| (the quantity
    research/tpq/tpq_base.py:158-159 averages), nll (T,) negative log-likelihood (utils.py:123-148), mse (T, D, D) outer
    products (utils.py:41-64), n_ok (T,) trajectories counted, n_pd (T,) of them in the nll sum (all whose P is
    nonsingular: the reference's formula does not need a positive-definite P), n_all (T,) trajectories this rank ran
    (so that what was left out is known after the reduction)."""
    lib = _lib.load()
    W = lib.ssmq_error_sums_width(D)
    if W < 0:
        raise _lib.SsmqError('ssmq_error_sums_width: dimension {} out of range'.format(D))
    sums, ps = _lib.out_c((T, W))
    _lib.check(lib.ssmq_error_sums_dev(D, B, ld, T, ctypes.c_void_p(d_x.ptr), ctypes.c_void_p(d_fm.ptr),
                                       ctypes.c_void_p(d_fP.ptr), ctypes.c_void_p(d_status.ptr if d_status else None),
                                       ps), 'ssmq_error_sums_dev')
    return dict(se=sums[:, :D].copy(), rmse=sums[:, D].copy(), nll=sums[:, D + 1].copy(),
                mse=sums[:, D + 2:D + 2 + D * D].reshape(T, D, D).copy(), n_ok=sums[:, D + 2 + D * D].copy(),
                n_pd=sums[:, D + 3 + D * D].copy(), n_all=np.full(T, float(B)))


def device_lcr_sums(D, B, ld, T, d_x, d_fm, d_fP, mse_global, d_status=None, reg=1e-6):
    """Phase 2 (`ssmq_lcr_sums_dev`): sums over this rank's trajectories of the log credibility ratio (utils.py:66-120)
    per time step, given the GLOBAL MSE matrices (T, D, D) (+ reg I as research/tpq/tpq_base.py:161-167 does).
    Returns dict lcr (T,), n (T,)."""
    lib = _lib.load()
    M, pM = _lib.as_c(np.asarray(mse_global, dtype=np.float64) + reg * np.eye(D))
    sums, ps = _lib.out_c((T, 2))
    _lib.check(lib.ssmq_lcr_sums_dev(D, B, ld, T, ctypes.c_void_p(d_x.ptr), ctypes.c_void_p(d_fm.ptr),
                                     ctypes.c_void_p(d_fP.ptr), ctypes.c_void_p(d_status.ptr if d_status else None),
                                     pM, ps), 'ssmq_lcr_sums_dev')
    return dict(lcr=sums[:, 0].copy(), n=sums[:, 1].copy())


# ---------------------------------------------------------------------------------------------------------------
# per-trajectory scores and their bootstrap error bars (single process)
# ---------------------------------------------------------------------------------------------------------------
BOOT_MAX_N, BOOT_MAX_SAMPLES, BOOT_MAX_ROWS = 2 ** 31 - 1, 2 ** 20, 19      # include/ssmq.h ssmq_bootstrap_var_dev


def score_names(D):
    """Names of the D + 3 rows of `device_traj_scores`."""
    return ['rmse_{}'.format(d) for d in range(D)] + ['rmse', 'nll', 'lcr']


def _check_bootstrap_range(n, samples, rows):
    """The range of ssmq_bootstrap_var_dev, checked before the library is touched."""
    if not 1 <= n <= BOOT_MAX_N:
        raise ValueError('bootstrap: the number of included entries n = {} is outside 1 <= n < 2^31'.format(n))
    if not 1 <= samples <= BOOT_MAX_SAMPLES:
        raise ValueError('bootstrap: samples = {} is outside 1 <= S <= 2^20'.format(samples))
    if not 1 <= rows <= BOOT_MAX_ROWS:
        raise ValueError('bootstrap: rows = {} is outside 1 <= R <= 19'.format(rows))


def device_traj_scores(D, B, ld, T, d_x, d_fm, d_fP, mse_global=None, d_status=None, k0=0, reg=1e-6):
    """Time-averaged scores of every trajectory over the steps k0 .. T-1 (`ssmq_traj_scores_dev`) - what the reference's
    studies resample for their error bars (research/bsq/bsq_ungm.py:64-76).  Inputs as for `device_error_sums`;
    mse_global (T, D, D) and reg as for `device_lcr_sums` (None: the lcr row is NaN).
    Returns (d_scores, names): a DeviceBuffer [D + 3][ld] - rmse_0 .. rmse_{D-1} per-dimension RMSE, rmse mean ||x - m||,
    nll, lcr - that the caller frees, and the row names.  Excluded trajectories and the lanes B .. ld-1 hold NaN."""
    if not 0 <= k0 < T:
        raise ValueError('device_traj_scores: k0 = {} is outside 0 <= k0 < T = {}'.format(k0, T))
    lib = _lib.load()
    R = lib.ssmq_traj_scores_rows(D)
    if R < 0:
        raise _lib.SsmqError('ssmq_traj_scores_rows: dimension {} out of range'.format(D))
    pM = None
    if mse_global is not None:
        M, pM = _lib.as_c(np.asarray(mse_global, dtype=np.float64).reshape(T, D, D) + reg * np.eye(D))
    d_scores = _lib.DeviceBuffer(8 * R * ld)
    try:
        _lib.check(lib.ssmq_traj_scores_dev(D, B, ld, T, k0, ctypes.c_void_p(d_x.ptr), ctypes.c_void_p(d_fm.ptr),
                                            ctypes.c_void_p(d_fP.ptr), ctypes.c_void_p(d_status.ptr if d_status else None),
                                            pM, ctypes.c_void_p(d_scores.ptr)), 'ssmq_traj_scores_dev')
    except Exception:
        d_scores.free()
        raise
    return d_scores, score_names(D)


def bootstrap_var_dev(d_scores, ld, rows, B, status=None, samples=1000, seed=0, return_means=False):
    """Bootstrap variance of the mean (utils.py:223-244) of each of the `rows` rows of the device block d_scores [rows][ld],
    resampling the included trajectories among the first B: those with status == 0 (status: host array (B,) or None = all).
    The draws are a counter-based function of (seed, resample, position, number of included entries) and are shared by the
    rows (`ssmq_bootstrap_var_dev`).  Returns var (rows,), and the resample means (rows, samples) with return_means.
    Single process: with several ranks the score rows have to be gathered first."""
    if status is None:
        n, idx = int(B), None
    else:
        idx = np.flatnonzero(np.asarray(status).reshape(-1)[:B] == 0).astype(np.int32)
        n = int(idx.size)
    _check_bootstrap_range(n, int(samples), int(rows))
    if n > ld:
        raise ValueError('bootstrap: {} entries in rows of {}'.format(n, ld))
    lib = _lib.load()
    d_idx = d_means = None
    try:
        if idx is not None:
            d_idx = _lib.DeviceBuffer(idx.nbytes)
            d_idx.upload(idx)
        if return_means:
            d_means = _lib.DeviceBuffer(8 * rows * samples)
        var, pv = _lib.out_c((rows,))
        _lib.check(lib.ssmq_bootstrap_var_dev(ctypes.c_void_p(d_scores.ptr), ld, rows, ctypes.c_void_p(d_idx.ptr if d_idx else None),
                                              n, samples, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), pv,
                                              ctypes.c_void_p(d_means.ptr if d_means else None)), 'ssmq_bootstrap_var_dev')
        return (var, d_means.download((rows, samples))) if return_means else var
    finally:
        for b in (d_idx, d_means):
            if b is not None:
                b.free()


def device_score_bars(D, B, ld, T, d_x, d_fm, d_fP, d_status=None, samples=10000, seed=0, k0=0):
    """The tail of a study on the device: phase-1 sums -> global MSE matrices -> per-trajectory scores -> bootstrap.
    Returns {name: {'mean', 'var', 'bar'}} for the rows of `device_traj_scores`: mean over the included trajectories, the
    bootstrap variance of that mean and bar = 2 sqrt(var), as the reference's tables print them.  Single process."""
    _check_bootstrap_range(max(int(B), 1), int(samples), D + 3)
    mse = finalize(device_error_sums(D, B, ld, T, d_x, d_fm, d_fP, d_status))['mse']
    status = d_status.download((B,), dtype=np.int32) if d_status else None
    d_scores, names = device_traj_scores(D, B, ld, T, d_x, d_fm, d_fP, mse, d_status, k0)
    try:
        var = bootstrap_var_dev(d_scores, ld, len(names), B, status, samples, seed)
        sc = d_scores.download((len(names), ld))[:, :B]
    finally:
        d_scores.free()
    if status is not None:
        sc = sc[:, status == 0]
    return {nm: dict(mean=float(np.mean(sc[r])), var=float(var[r]), bar=float(2.0 * np.sqrt(var[r])))
            for r, nm in enumerate(names)}


# ---------------------------------------------------------------------------------------------------------------
# posterior Cramer-Rao lower bound: the floor of a filter study (include/ssmq.h ssmq_pcrlb_sums_dev / ssmq_pcrlb_finalize)
# ---------------------------------------------------------------------------------------------------------------
def _crlb_check(rc, what):
    """SSMQ_E_ARG is a ValueError, SSMQ_E_UNSUPPORTED a NotImplementedError that names the range, anything else as `_lib.check`."""
    if rc == -1:
        raise ValueError(_lib.last_error())
    return _lib.check(rc, what, unsupported=True)


def _crlb_noise(dyn):
    """(q, G, keep): the process noise as struct ssmq_rv, the noise gain, and the arrays both point to."""
    from .ssmod import _rv_desc
    q, keep = _rv_desc(dyn.noise_rv, 'the process noise')
    G = np.ascontiguousarray(dyn.noise_gain, dtype=np.float64)
    return q, G, (keep, G)


def _crlb_model_args(dyn, obs):
    """The model part of the C calls: (f_dyn, f_obs, D, Y, dq, q, G, r) and what has to stay alive."""
    from .ssmod import _rv_desc
    f_dyn, _ = dyn.device_integrand()
    f_obs, _ = obs.device_integrand()
    q, G, keep_q = _crlb_noise(dyn)
    r, keep_r = _rv_desc(obs.noise_rv, 'the measurement noise')
    args = (ctypes.byref(f_dyn), ctypes.byref(f_obs), dyn.dim_state, obs.dim_out, int(q.dim), ctypes.byref(q), _lib.dp(G), ctypes.byref(r))
    return args, (f_dyn, f_obs, q, r, keep_q, keep_r)


def crlb_kernel_name(dyn, obs):
    """The kernels `device_crlb_sums` would run for this pair: the library's range check without a device (NotImplementedError
    naming the range, or ValueError)."""
    args, keep = _crlb_model_args(dyn, obs)
    buf = ctypes.create_string_buffer(512)
    _crlb_check(_lib.load().ssmq_pcrlb_kernel_name(*args, buf, 512), 'ssmq_pcrlb_kernel_name')
    return buf.value.decode()


def device_crlb_sums(dyn, obs, d_x, B, ld, T):
    """Phase-1 sums of the posterior Cramer-Rao recursion over this rank's B true trajectories (`ssmq_pcrlb_sums_dev`).
    d_x: DeviceBuffer planes [T + 1][D][ld], the raw output of `ssmod.simulate_dev(dyn, obs, T + 1, B)` - plane 0 the initial state,
    plane j + 1 the state the filters call x_j.  Returns an ndarray (T, S), S = D (D + 1) / 2 + D D + D (D + 1) / 2: per step the sums
    over the trajectories of F' Qi F (lower triangle, packed), F and H' Ri H (lower triangle, packed).  Sums, not means: add the arrays
    of all ranks (`allreduce_sums` takes the array unchanged), then `finalize_crlb`.  The bits depend on B and the states alone."""
    lib = _lib.load()
    args, keep = _crlb_model_args(dyn, obs)
    D = dyn.dim_state
    S = lib.ssmq_pcrlb_sums_width(D)
    sums, ps = _lib.out_c((max(int(T), 0), max(S, 0)))
    _crlb_check(lib.ssmq_pcrlb_sums_dev(*args[:5], B, ld, T, _lib.vp(d_x), *args[5:], ps), 'ssmq_pcrlb_sums_dev')
    return sums


def finalize_crlb(sums, dyn, B_total):
    """The recursion J_j = D22_j - D12_j' (J_{j-1} + D11_j)^-1 D12_j, J_{-1} = P0^-1, from the all-reduced sums of B_total trajectories
    (`ssmq_pcrlb_finalize`; host, no device).  Returns a dict: info (D, D, T) the information matrices J_j, bound (D, D, T) their
    inverses - the lower bound of every filter's error covariance at step j -, rmse_bound (T,) = sqrt(trace bound), and status: 0, or
    1 + the first step with a non-finite sum or a matrix that is not positive definite (NaN from that step on)."""
    from .ssmod import GaussRV
    if not isinstance(dyn.init_rv, GaussRV):
        raise NotImplementedError('finalize_crlb: not implemented for a {} initial state; range: additive Gaussian noise, a GaussRV initial '
                                  'state, dim_state <= 6'.format(type(dyn.init_rv).__name__))
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    D = dyn.dim_state
    if sums.ndim != 2 or sums.shape[0] < 1 or sums.shape[1] != D * (D + 1) + D * D:
        raise ValueError('finalize_crlb: sums must have shape (T >= 1, {}), got {}'.format(D * (D + 1) + D * D, sums.shape))
    T = sums.shape[0]
    P0, pP0 = _lib.as_c(np.atleast_2d(dyn.init_rv.cov))
    q, G, keep = _crlb_noise(dyn)
    info, pi = _lib.out_c((T, D, D))
    bound, pb = _lib.out_c((T, D, D))
    rmse, pr = _lib.out_c((T,))
    status = ctypes.c_int32(0)
    _crlb_check(_lib.load().ssmq_pcrlb_finalize(D, T, int(B_total), _lib.dp(sums), pP0, ctypes.byref(q), _lib.dp(G), pi, pb, pr,
                                                ctypes.byref(status)), 'ssmq_pcrlb_finalize')
    return dict(info=np.ascontiguousarray(info.transpose(1, 2, 0)), bound=np.ascontiguousarray(bound.transpose(1, 2, 0)), rmse_bound=rmse,
                status=int(status.value))


def _pack(sums, keys):
    return np.concatenate([np.asarray(sums[k], dtype=np.float64).reshape(-1) for k in keys])


def _unpack(flat, sums, keys):
    out, pos = {}, 0
    for k in keys:
        n = int(np.asarray(sums[k]).size)
        out[k] = flat[pos:pos + n].reshape(np.asarray(sums[k]).shape)
        pos += n
    return out


def allreduce_sums(sums, comm=None):
    """Sum a dict of arrays over all ranks with ONE all-reduce of the packed buffer.  comm: RcclComm / TorchComm /
    an initialised torch.distributed module / None (single process).  A bare ndarray (`device_crlb_sums`) is summed as it is."""
    comm = _as_comm(comm)
    if isinstance(sums, np.ndarray):
        return np.asarray(comm.allreduce_sum(sums.reshape(-1))).reshape(sums.shape)
    keys = sorted(sums)
    return _unpack(comm.allreduce_sum(_pack(sums, keys)), sums, keys)


def finalize(total, strict=False):
    """Global averages from all-reduced phase-1 sums: rmse_avg (T,), nll_avg (T,), mse (T, D, D), rmse_total (), count ()
    trajectories aggregated, and what was LEFT OUT of them: excluded_failed (T,) trajectories whose filter had failed
    (lost positive definiteness: the reference raises LinAlgError there and has no result for the run at all),
    excluded_not_pd (T,) finished trajectories whose filtered covariance at that step is singular (no NLL term:
    numpy.linalg.inv raises there).  The reference averages over all runs (utils.py:123-148 via research/tpq/tpq_base.py:154-172), so an average
    taken over fewer runs is not the same statistic: with strict=True the averages of a step with exclusions are NaN."""
    n = np.maximum(total['n_ok'], 1.0)
    T = total['rmse'].shape[0]
    n_all = total.get('n_all', total['n_ok'])
    out = dict(rmse_avg=total['rmse'] / n, nll_avg=total['nll'] / np.maximum(total['n_pd'], 1.0),
               mse=total['mse'] / n[:, None, None],
               rmse_total=float(np.sqrt(total['se'].sum() / max(total['n_ok'].sum(), 1.0))),
               count=float(total['n_ok'].max()) if T else 0.0,
               excluded_failed=n_all - total['n_ok'], excluded_not_pd=total['n_ok'] - total['n_pd'])
    if strict:
        bad = out['excluded_failed'] > 0
        out['rmse_avg'] = np.where(bad, np.nan, out['rmse_avg'])
        out['mse'] = np.where(bad[:, None, None], np.nan, out['mse'])
        out['nll_avg'] = np.where(bad | (out['excluded_not_pd'] > 0), np.nan, out['nll_avg'])
        if bad.any():
            out['rmse_total'] = float('nan')
    return out


def finalize_lcr(total):
    """Average log credibility ratio per time step (the inclination indicator's summand) from all-reduced phase-2 sums."""
    return total['lcr'] / np.maximum(total['n'], 1.0)
