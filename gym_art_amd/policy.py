"""Device MLP policies for closed-loop rollouts (include/gaq.h gaq_policy, QuadrotorEnv.rollout_policy_dev).

The policy is obs (obs_dim) -> [Linear -> act] x n_hidden -> Linear -> 4 (-> tanh), fp32, with act tanh or relu for every hidden
layer, 1 to 3 hidden layers of widths that are multiples of 16, and optional Gaussian exploration a = mean + exp(log_std) * z.
Observation normalisation belongs in the first layer (fold it in before packing).

Three engines evaluate it (gaq.h GAQ_POLICY_ENGINE_*): "valu" (widths up to 128, the fused closed-loop launch where the layout has one),
"mfma" (the hidden layers on the fp32 matrix cores, widths up to 256, one policy launch + one step launch per step) and "bf16" (every
layer on the bf16 matrix cores, widths up to 256, launched like "mfma").  "valu" and "mfma" compute the same bits on every net both accept.
"bf16" computes in reduced precision (MLPPolicy); engine="auto" never picks it: it picks "valu" whenever it can run the net and "mfma"
otherwise."""
import ctypes as C

import numpy as np

from . import _lib

_ACTS = {"tanh": 0, "relu": 1}
ENGINES = {"valu": 0, "mfma": 1, "bf16": 3}      # 2 stays unassigned (gaq.h)
_MAX_WIDTH = {"valu": 128, "mfma": 256, "bf16": 256}
_ENGINE_NOTE = {"valu": "", "mfma": " (MFMA engine)", "bf16": " (bf16 engine)"}


class _Desc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("in_dim", C.c_int32), ("n_hidden", C.c_int32), ("width", C.c_int32 * 3),
                ("hidden_act", C.c_int32), ("out_tanh", C.c_int32)]


class _DescEx(C.Structure):
    """gaq_policy_desc_ex: the fields of gaq_policy_desc, then the engine"""
    _fields_ = _Desc._fields_ + [("engine", C.c_int32)]


def pack_weights(layers):
    """[(W [out, in], b [out]), ...] (hidden layers, then the 4-output layer) -> the flat fp32 layout of gaq.h: per hidden layer
    W'[out/16][in][16] (W'[c][k][j] = W[16c + j][k]) then bias; output layer W'[in][4] = W.T then bias[4]."""
    out = []
    for W, b in layers[:-1]:
        W = np.asarray(W, dtype=np.float32)
        o, i = W.shape
        out.append(W.reshape(o // 16, 16, i).transpose(0, 2, 1).reshape(-1))
        out.append(np.asarray(b, dtype=np.float32).reshape(-1))
    W, b = layers[-1]
    out.append(np.asarray(W, dtype=np.float32).T.reshape(-1))
    out.append(np.asarray(b, dtype=np.float32).reshape(-1))
    return np.ascontiguousarray(np.concatenate(out))


def check_layers(layers, in_dim, hidden_act, engine="valu"):
    """ValueError unless `layers` is an MLP the device engine can run (obs_dim inputs, 1-3 hidden layers, widths 16k <= 128 for "valu" and
    <= 256 for "mfma" and "bf16", 4 outputs)."""
    if engine not in ENGINES:
        raise ValueError("engine must be 'valu', 'mfma' or 'bf16', got %r" % (engine,))
    maxw = _MAX_WIDTH[engine]
    if hidden_act not in _ACTS:
        raise ValueError("hidden activation must be 'tanh' or 'relu', got %r" % (hidden_act,))
    if not 2 <= len(layers) <= 4:
        raise ValueError("the policy needs 1 to 3 hidden layers and an output layer, got %d Linear layers" % len(layers))
    prev = int(in_dim)
    for k, (W, b) in enumerate(layers):
        W, b = np.asarray(W), np.asarray(b)
        if W.ndim != 2 or b.shape != (W.shape[0],):
            raise ValueError("layer %d: W must be [out, in] and b [out]" % k)
        if W.shape[1] != prev:
            raise ValueError("layer %d takes %d inputs, expected %d (the env's obs_dim for the first layer)" % (k, W.shape[1], prev))
        last = k == len(layers) - 1
        if last and W.shape[0] != 4:
            raise ValueError("the output layer must have 4 outputs, has %d" % W.shape[0])
        if not last and (W.shape[0] % 16 != 0 or not 16 <= W.shape[0] <= maxw):
            raise ValueError("hidden layer %d has width %d: widths must be multiples of 16 in [16, %d]%s"
                             % (k, W.shape[0], maxw, _ENGINE_NOTE[engine]))
        prev = W.shape[0]


def resolve_engine(layers, in_dim, hidden_act, engine="auto"):
    """The engine a policy of these layers runs on: "valu" / "mfma" / "bf16" as asked (ValueError if that engine cannot run them);
    "auto" = "valu" for every net the VALU engine accepts (so existing callers keep their results and the fused launch), "mfma" for the
    rest.  "auto" never returns "bf16": reduced precision is the caller's choice."""
    if engine == "auto":
        try:
            check_layers(layers, in_dim, hidden_act, "valu")
            return "valu"
        except ValueError:
            engine = "mfma"
    check_layers(layers, in_dim, hidden_act, engine)
    return engine


def torch_layers(module):
    """nn.Sequential [Linear, act, Linear, act, ..., Linear (, Tanh)] -> ([(W, b), ...], 'tanh' | 'relu', out_tanh); ValueError otherwise."""
    import torch.nn as nn
    mods = list(module.children()) if isinstance(module, nn.Sequential) else [module]
    out_tanh = False
    if mods and isinstance(mods[-1], nn.Tanh):
        out_tanh, mods = True, mods[:-1]
    if not mods or not isinstance(mods[-1], nn.Linear):
        raise ValueError("the policy must end with a Linear layer (optionally followed by Tanh)")
    layers, acts = [], set()
    for k, m in enumerate(mods):
        if k % 2 == 0:
            if not isinstance(m, nn.Linear):
                raise ValueError("module %d: expected Linear, got %s" % (k, type(m).__name__))
            W = m.weight.detach().float().cpu().numpy()
            b = np.zeros(W.shape[0], np.float32) if m.bias is None else m.bias.detach().float().cpu().numpy()
            layers.append((W, b))
        elif isinstance(m, nn.Tanh):
            acts.add("tanh")
        elif isinstance(m, nn.ReLU):
            acts.add("relu")
        else:
            raise ValueError("module %d: only Tanh and ReLU activations are supported, got %s" % (k, type(m).__name__))
    if len(acts) != 1:
        raise ValueError("every hidden layer must use the same activation (tanh or relu), got %s" % sorted(acts))
    return layers, acts.pop(), out_tanh


class MLPPolicy:
    """An MLP evaluated on the device inside QuadrotorEnv.rollout_policy_dev.  Build with from_torch / from_arrays.

    engine="bf16" runs every layer on the bf16 matrix cores under this contract (gaq.h GAQ_POLICY_ENGINE_MFMA_BF16):
    - weights: the fp32 weights are rounded to bf16 (round to nearest even) once, when they are set; biases stay fp32.  A bf16 torch
      module loses nothing (from_torch widens it with .float(), which is exact, and re-rounding a bf16 value is the identity);
    - activations: the input of every layer (the observation and each hidden activation) is rounded once to bf16; the activation
      function runs in fp32 on the fp32 sum and only its result is rounded;
    - accumulation: each unit starts at its fp32 bias and sums bf16 x bf16 products in fp32, the 4 outputs likewise; the order of those
      fp32 sums is the matrix core's, so the results are deterministic but not bit-equal to the fp32 engines or to torch;
    - the output tanh and the exploration term are those of the other engines (the same draws for the same seed, env and step)."""

    def __init__(self, env, layers, hidden_act="tanh", out_tanh=False, log_std=None, engine="auto"):
        self.engine = resolve_engine(layers, env.obs_dim, hidden_act, engine)
        self._lib = _lib.load()
        self.env_handle = _lib.handle_value(env._handle)
        self.hidden_act, self.out_tanh = hidden_act, bool(out_tanh)
        self.widths = [int(np.asarray(W).shape[0]) for W, _ in layers[:-1]]
        if self.engine == "valu":       # the original entry points: exactly what every caller before the MFMA engine got
            d, create, count = _Desc(), self._lib.gaq_policy_create, self._lib.gaq_policy_weight_count
        else:
            d, create, count = _DescEx(), self._lib.gaq_policy_create_ex, self._lib.gaq_policy_weight_count_ex
            d.engine = ENGINES[self.engine]
        d.struct_size = C.sizeof(d)
        d.in_dim, d.n_hidden = int(env.obs_dim), len(self.widths)
        for k, w in enumerate(self.widths):
            d.width[k] = w
        d.hidden_act, d.out_tanh = _ACTS[hidden_act], int(self.out_tanh)
        h = C.c_void_p()
        _lib.check(create(env._handle, C.byref(d), C.byref(h)))
        self.handle = h
        assert self._lib.gaq_policy_engine(h) == ENGINES[self.engine]
        self.packed = pack_weights(layers)
        assert self.packed.size == count(C.byref(d))
        _lib.check(self._lib.gaq_policy_set_weights(h, _lib.ptr(self.packed)))
        self.set_log_std(log_std)

    def set_log_std(self, log_std=None):
        """Exploration: a = mean + exp(log_std[k]) * z_k (4 floats), or None for the deterministic policy."""
        self.log_std = None if log_std is None else np.ascontiguousarray(np.asarray(log_std, dtype=np.float32).reshape(4))
        _lib.check(self._lib.gaq_policy_set_explore(self.handle, _lib.ptr(self.log_std)))

    @classmethod
    def from_arrays(cls, env, layers, hidden_act="tanh", out_tanh=False, log_std=None, engine="auto"):
        """layers = [(W, b), ...]: the hidden layers then the 4-output layer, W [out, in] as in torch.nn.Linear."""
        return cls(env, [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in layers],
                   hidden_act, out_tanh, log_std, engine)

    @classmethod
    def from_torch(cls, module, env, log_std=None, engine="auto"):
        """An nn.Sequential of Linear / Tanh / ReLU: Linear and activation alternate, the last Linear has 4 outputs and may be
        followed by a Tanh.  Every hidden activation must be the same."""
        layers, act, out_tanh = torch_layers(module)
        return cls(env, layers, act, out_tanh, log_std, engine)

    def close(self):
        if getattr(self, "handle", None) is not None:
            self._lib.gaq_policy_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
