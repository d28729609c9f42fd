"""The running normalisers of a learner, on the device: ObsNorm (gaq.h gaq_obs_norm) and RetNorm (gaq.h gaq_ret_norm), the two halves of
SB3's VecNormalize.  Both keep fp64 running statistics that change only when update_dev / load_state_dict are called and publish an fp32
table that normalize_dev applies; what they share is _RunningNorm.  AdvNorm (gaq.h gaq_adv_norm) standardises a batch of advantages with
that batch's own statistics and carries nothing between calls.  gym_art_amd.policy re-exports the three and attaches an ObsNorm to
policies and critics."""
import ctypes as C

import numpy as np

from . import _lib


class _RunningNorm:
    """What the two normalisers share: the handle and its life, the stream, the tensor check, count / mean / var on a class's _stats()
    and the refusal of a state saved with other hyper-parameters.  A class names its hyper-parameters in _HYPER and its gaq_*_destroy."""
    _HYPER = ()
    _DESTROY = None

    def _open(self):
        if getattr(self, "handle", None) is None:
            raise ValueError("the %s is closed" % type(self).__name__)
        return self.handle

    def _check(self, name, t, dtype, shape, shape_ok):
        """ValueError unless t is a contiguous tensor of `dtype` (a torch dtype, or its name) on the env's device whose shape passes
        shape_ok; `shape` puts that test into words"""
        import torch
        want = getattr(torch, dtype) if isinstance(dtype, str) else dtype
        if not isinstance(t, torch.Tensor) or t.dtype != want or not t.is_contiguous() or not shape_ok(t):
            raise ValueError("%s must be a contiguous %s tensor%s, got %s %s"
                             % (name, dtype, shape, getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ()))))
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError("%s must be on the normaliser's device cuda:%d, is on %s" % (name, self.device, t.device))

    def _stream(self, stream):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)

    @property
    def count(self):
        return self._stats()[0]

    @property
    def mean(self):
        return self._stats()[1]

    @property
    def var(self):
        """the population variance M2 / count as float64 (ones before any update)"""
        count, _, m2 = self._stats()
        return m2 / count if count > 0 else m2 * 0.0 + 1.0

    def _check_hyper(self, state):
        for key in self._HYPER:
            if key in state and float(np.float32(state[key])) != getattr(self, key):
                raise ValueError("the state was saved with %s=%r, this normaliser has %r" % (key, state[key], getattr(self, key)))

    def close(self):
        """Destroy the handle.  (An ObsNorm: detach it from, or close, every policy and critic it is attached to first: they keep its
        address.)"""
        if getattr(self, "handle", None) is not None:
            getattr(self._lib, self._DESTROY)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObsNorm(_RunningNorm):
    """Running observation statistics and the normaliser built on them, on the device (gaq.h gaq_obs_norm): one element is
    min(max((x - mean[k]) * inv_std[k], -clip), clip) in fp32 with inv_std = 1 / sqrt(var + eps).  Attach it to the env's policies and
    critics (set_obs_norm): their kernels normalise inside the rollout; the observations a rollout returns stay raw, update_dev feeds them
    to the statistics and normalize_dev gives the learner's torch net exactly what the device policy saw.  Statistics change only when
    update_dev / load_state_dict are called, never inside a rollout.  Before any update the mean is 0 and the variance 1."""
    _HYPER = ("eps", "clip")
    _DESTROY = "gaq_obs_norm_destroy"

    def __init__(self, env, eps=1e-5, clip=5.0):
        self._lib = _lib.load()
        self.env_handle = _lib.handle_value(env._handle)
        self.device, self.dim = int(env.device), int(env.obs_dim)
        self.eps, self.clip = float(np.float32(eps)), float(np.float32(clip))       # as the library holds them (fp32)
        h = C.c_void_p()
        _lib.check(self._lib.gaq_obs_norm_create(env._handle, self.eps, self.clip, C.byref(h)))
        self.handle = h

    @classmethod
    def from_stats(cls, env, mean, var, count=1.0, eps=1e-5, clip=5.0):
        """A normaliser with given statistics -- an rl_games RunningMeanStd (running_mean, running_var, count) or an SB3 VecNormalize
        obs_rms (mean, var, count): mean and var [obs_dim] (population variance), count the number of samples behind them."""
        norm = cls(env, eps, clip)
        norm.load_state_dict({"count": count, "mean": mean, "m2": np.asarray(var, dtype=np.float64) * float(count)})
        return norm

    def _rows(self, obs, what):
        self._check(what, obs, "float32", " of shape [rows, %d] or [T, N, %d]" % (self.dim, self.dim),
                    lambda t: t.dim() in (2, 3) and t.shape[-1] == self.dim)
        return int(obs.numel() // self.dim)

    def update_dev(self, obs, stream=None):
        """Merge the rows of obs ([rows, D] or [T, N, D], contiguous float32 on the env's device) into the running statistics and
        publish the new table: one streaming pass on the current torch stream (or `stream`), no host synchronisation, deterministic."""
        handle, rows = self._open(), self._rows(obs, "obs")
        _lib.check(self._lib.gaq_obs_norm_update_dev(handle, rows, _lib.ptr(obs), self._stream(stream)))

    def normalize_dev(self, obs, out=None, stream=None):
        """The normalised rows of obs -> `out` (allocated if None; out=obs normalises in place): bit for bit what an attached policy
        or critic stages.  Returns out."""
        import torch
        handle, rows = self._open(), self._rows(obs, "obs")
        if out is None:
            out = torch.empty_like(obs)
        elif self._rows(out, "out") != rows or out.shape != obs.shape:
            raise ValueError("out must have obs's shape %s, got %s" % (tuple(obs.shape), tuple(out.shape)))
        _lib.check(self._lib.gaq_obs_norm_apply_dev(handle, rows, _lib.ptr(obs), _lib.ptr(out), self._stream(stream)))
        return out

    def _stats(self):
        count = C.c_double()
        mean, m2 = np.empty(self.dim, np.float64), np.empty(self.dim, np.float64)
        _lib.check(self._lib.gaq_obs_norm_get_stats(self._open(), C.byref(count), _lib.ptr(mean), _lib.ptr(m2)))
        return float(count.value), mean, m2

    def state_dict(self):
        """{"count", "mean", "m2", "eps", "clip"}: the fp64 state as numpy (synchronous)"""
        count, mean, m2 = self._stats()
        return {"count": count, "mean": mean, "m2": m2, "eps": self.eps, "clip": self.clip}

    def load_state_dict(self, state):
        """Replace the statistics (count, mean [D], m2 [D]) and republish the table (synchronous).  eps and clip are the object's:
        a state saved with others is refused."""
        handle = self._open()
        mean = np.ascontiguousarray(np.asarray(state["mean"], dtype=np.float64).reshape(-1))
        m2 = np.ascontiguousarray(np.asarray(state["m2"], dtype=np.float64).reshape(-1))
        if mean.shape != (self.dim,) or m2.shape != (self.dim,):
            raise ValueError("mean and m2 must have %d entries (the env's obs_dim), got %s and %s" % (self.dim, mean.shape, m2.shape))
        self._check_hyper(state)
        _lib.check(self._lib.gaq_obs_norm_set_stats(handle, float(state["count"]), _lib.ptr(mean), _lib.ptr(m2)))


class RetNorm(_RunningNorm):
    """Return normalisation on the device (gaq.h gaq_ret_norm), the reward half of SB3's VecNormalize: every env carries a running
    discounted return R = gamma R + r (fp64, cleared after a done), update_dev feeds the T N returns of a rollout to running fp64
    statistics, and normalize_dev computes min(max(r * inv_std, -clip), clip) in fp32 with inv_std = 1 / sqrt(var + eps) -- the mean is
    not subtracted.  Statistics change only when update_dev / load_state_dict are called, so a whole rollout is normalised with one
    table (SB3 updates at every step).  Before any update the variance is 1."""
    _HYPER = ("gamma", "eps", "clip")
    _DESTROY = "gaq_ret_norm_destroy"

    def __init__(self, env, gamma=0.99, eps=1e-8, clip=10.0):
        self._lib = _lib.load()
        self.device, self.num_envs = int(env.device), int(env.num_envs)
        self.gamma, self.eps, self.clip = (float(np.float32(v)) for v in (gamma, eps, clip))     # as the library holds them (fp32)
        h = C.c_void_p()
        _lib.check(self._lib.gaq_ret_norm_create(env._handle, self.gamma, self.eps, self.clip, C.byref(h)))
        self.handle = h

    @classmethod
    def from_stats(cls, env, var, count=1.0, mean=0.0, gamma=0.99, eps=1e-8, clip=10.0):
        """A normaliser with given statistics -- an SB3 VecNormalize ret_rms (var, count, mean; population variance).  The per-env
        returns start at zero."""
        norm = cls(env, gamma, eps, clip)
        norm.load_state_dict({"count": count, "mean": mean, "m2": float(var) * float(count)})
        return norm

    def _shaped(self, name, t, shape=None, dtype=None):
        """_check: a contiguous float32 (or `dtype`) tensor (of `shape`, if given) on the env's device"""
        import torch
        self._check(name, t, torch.float32 if dtype is None else dtype, "" if shape is None else " of shape %s" % (shape,),
                    lambda t: shape is None or tuple(t.shape) == shape)

    def update_dev(self, rew, done, stream=None):
        """Advance the per-env returns over rew [T, N] (float32) and done [T, N] (uint8) as a rollout wrote them (contiguous, on the
        env's device), merge the T N returns into the running statistics and publish the new table: one streaming pass on the current
        torch stream (or `stream`), no host synchronisation, deterministic."""
        import torch
        handle = self._open()
        if not isinstance(rew, torch.Tensor) or rew.dim() != 2 or rew.shape[0] < 1 or rew.shape[1] != self.num_envs:
            raise ValueError("rew must have shape [T, %d] with T >= 1, got %s" % (self.num_envs, tuple(getattr(rew, "shape", ()))))
        shape = tuple(rew.shape)
        self._shaped("rew", rew, shape)
        self._shaped("done", done, shape, torch.uint8)
        _lib.check(self._lib.gaq_ret_norm_update_dev(handle, shape[0], _lib.ptr(rew), _lib.ptr(done), self._stream(stream)))

    def normalize_dev(self, rew, out=None, stream=None):
        """The normalised rewards of rew (any contiguous float32 tensor on the env's device) -> `out` (allocated if None; out=rew
        normalises in place, any other overlap is not allowed).  Returns out."""
        import torch
        handle = self._open()
        self._shaped("rew", rew)
        if out is None:
            out = torch.empty_like(rew)
        else:
            self._shaped("out", out, tuple(rew.shape))
        _lib.check(self._lib.gaq_ret_norm_apply_dev(handle, rew.numel(), _lib.ptr(rew), _lib.ptr(out), self._stream(stream)))
        return out

    def reset_returns(self, mask=None):
        """Zero the running return of the envs whose mask entry is true ([N] bool / uint8, host or device), or of every env for None:
        for envs the caller resets outside a rollout (a done inside one clears its env's return by itself).  Enqueued on the current
        stream."""
        import torch
        handle = self._open()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device="cuda:%d" % self.device, dtype=torch.uint8).contiguous()
            if m.shape != (self.num_envs,):
                raise ValueError("mask must have one entry per env (%d), got shape %s" % (self.num_envs, tuple(m.shape)))
        _lib.check(self._lib.gaq_ret_norm_reset_returns_dev(handle, _lib.ptr(m), self._stream(None)))

    def _stats(self):
        count, mean, m2 = C.c_double(), C.c_double(), C.c_double()
        _lib.check(self._lib.gaq_ret_norm_get_stats(self._open(), C.byref(count), C.byref(mean), C.byref(m2)))
        return float(count.value), float(mean.value), float(m2.value)

    @property
    def returns(self):
        """the running discounted return of each env, [N] float64 numpy (synchronous)"""
        r = np.empty(self.num_envs, np.float64)
        _lib.check(self._lib.gaq_ret_norm_get_returns(self._open(), _lib.ptr(r)))
        return r

    def state_dict(self):
        """{"count", "mean", "m2", "returns", "gamma", "eps", "clip"}: the fp64 state, returns as numpy (synchronous)"""
        count, mean, m2 = self._stats()
        return {"count": count, "mean": mean, "m2": m2, "returns": self.returns, "gamma": self.gamma, "eps": self.eps, "clip": self.clip}

    def load_state_dict(self, state):
        """Replace the statistics (count, mean, m2) and, where the state has them, the per-env returns ([N]), and republish the table
        (synchronous).  gamma, eps and clip are the object's: a state saved with others, or for another N, is refused."""
        handle = self._open()
        self._check_hyper(state)
        returns = None
        if state.get("returns") is not None:
            returns = np.ascontiguousarray(np.asarray(state["returns"], dtype=np.float64))
            if returns.shape != (self.num_envs,):
                raise ValueError("returns must have %d entries (the env's num_envs), got shape %s" % (self.num_envs, returns.shape))
        _lib.check(self._lib.gaq_ret_norm_set_stats(handle, float(state["count"]), float(state["mean"]), float(state["m2"])))
        if returns is not None:
            _lib.check(self._lib.gaq_ret_norm_set_returns(handle, _lib.ptr(returns)))


class AdvNorm(_RunningNorm):
    """Advantage standardisation on the device (gaq.h gaq_adv_norm): normalize_dev computes (A - mean) / (std + eps) in fp32 with the
    fp64 mean and standard deviation of the batch it is given -- what rl_games and SB3 do before the PPO loss -- in a fixed order, so
    the same input gives the same bits.  eps is added to the standard deviation; ddof=1 is torch.std's default, ddof=0 the population
    value.  Nothing is carried from one batch to the next; of _RunningNorm it takes the handle's life, the stream and the tensor check."""
    _DESTROY = "gaq_adv_norm_destroy"

    def __init__(self, env, eps=1e-8, ddof=1):
        self._lib = _lib.load()
        self.device = int(env.device)
        self.eps, self.ddof = float(np.float32(eps)), int(ddof)                     # eps as the library holds it (fp32)
        if self.ddof != ddof:
            raise ValueError("ddof must be 0 or 1, got %r" % (ddof,))
        h = C.c_void_p()
        _lib.check(self._lib.gaq_adv_norm_create(env._handle, self.eps, self.ddof, C.byref(h)))
        self.handle = h

    def normalize_dev(self, adv, out=None, stream=None):
        """The standardised advantages of adv (any contiguous float32 tensor on the env's device with at least 1 + ddof elements) ->
        `out` (allocated if None; out=adv standardises in place, any other overlap is not allowed).  Three launches on the current
        torch stream (or `stream`), no host synchronisation.  Returns out."""
        import torch
        handle = self._open()
        self._check("adv", adv, "float32", "", lambda t: True)
        if out is None:
            out = torch.empty_like(adv)
        else:
            self._check("out", out, "float32", " of shape %s" % (tuple(adv.shape),), lambda t: t.shape == adv.shape)
        _lib.check(self._lib.gaq_adv_norm_apply_dev(handle, adv.numel(), _lib.ptr(adv), _lib.ptr(out), self._stream(stream)))
        return out

    def _stats(self):
        count, mean, m2 = C.c_double(), C.c_double(), C.c_double()
        _lib.check(self._lib.gaq_adv_norm_get_stats(self._open(), C.byref(count), C.byref(mean), C.byref(m2)))
        return float(count.value), float(mean.value), float(m2.value)

    def stats(self):
        """(count, mean, std) of the last batch as float64 (synchronous): std = sqrt(M2 / (count - ddof)); zeros before the first"""
        count, mean, m2 = self._stats()
        return count, mean, float(np.sqrt(m2 / (count - self.ddof))) if count > self.ddof else 0.0

    @property
    def var(self):
        """the variance M2 / (count - ddof) of the last batch as float64"""
        count, _, m2 = self._stats()
        return m2 / (count - self.ddof) if count > self.ddof else 0.0
