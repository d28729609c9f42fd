"""Device MLP policies for closed-loop rollouts (include/gaq.h gaq_policy, QuadrotorEnv.rollout_policy_dev).

The policy is obs (obs_dim) -> [Linear -> act] x n_hidden -> Linear -> 4 (-> tanh), fp32, with act tanh or relu for every hidden
layer, 1 to 3 hidden layers of widths that are multiples of 16, and optional Gaussian exploration a = mean + exp(log_std) * z.
Observation normalisation is an ObsNorm (norm.py), or is folded into the first layer before packing.

Three engines evaluate it (gaq.h GAQ_POLICY_ENGINE_*): "valu" (widths up to 128, the fused closed-loop launch where the layout has one),
"mfma" (the hidden layers on the fp32 matrix cores, widths up to 256, one policy launch + one step launch per step) and "bf16" (every
layer on the bf16 matrix cores, widths up to 256, launched like "mfma").  "valu" and "mfma" compute the same bits on every net both accept.
"bf16" computes in reduced precision (MLPPolicy); engine="auto" never picks it: it picks "valu" whenever it can run the net and "mfma"
otherwise.

GRUPolicy puts a GRU cell in front of such a head (obs -> GRU(H) -> [Linear -> act] x 0..2 -> Linear -> 4 (-> tanh)) and runs it on the fp32
matrix cores, with a per-env hidden state that lives in a torch tensor across steps and calls (gaq.h gaq_policy_desc_rnn).

LSTMPolicy is the same with an LSTM cell (torch nn.LSTMCell, gate rows i, f, g, o) and two per-env states, .hidden and .cell
(gaq.h GAQ_POLICY_CELL_LSTM).  Everything said of a GRUPolicy below -- value head, log-probabilities, terminal values, a separate
critic -- holds for an LSTMPolicy too.

An encoder in front of the cell: GRUPolicy.with_encoder and LSTMPolicy.with_encoder take encoder = [(W, b), ...], 1 or 2 Linear ->
hidden_act layers on the observation (widths multiples of 16 up to 256) whose last width the cell takes in the observation's place -- obs -> encoder -> core ->
heads, the recurrent actor-critic of sample-factory and rl_games (gaq.h gaq_policy_desc_rnn_enc; from_torch_encoder(nn.Sequential, cell, head, env)).
Its weights are a block of their own (set_encoder_weights, set_encoder_weights_dev, get_encoder_weights, pack_encoder_weights /
unpack_encoder_weights); an attached ObsNorm normalises what the encoder reads.  Every rollout form works; the learner's sequence
passes and AdamDev refuse such a policy for now.

Actor-critic rollouts: an "mfma" MLPPolicy or a GRUPolicy can carry a value head, a linear critic V = w . y + b on the activations the
4-output layer reads (value=(w, b), set_value_head); rollout_policy_dev(..., values=, logp=) then also returns V per step and the
log-probability of each applied action, and QuadrotorEnv.gae_dev turns them into advantages (gaq.h gaq_step_policy_ac_many_dev).
engine="auto" with a value head resolves to "mfma" (the "valu" and "bf16" engines have none); without one it keeps the choice above.

Separate critic: MLPCritic is a value network of its own, obs -> [Linear -> act] x n_hidden -> Linear -> 1 on the fp32 matrix cores
(gaq.h gaq_critic).  rollout_policy_dev(..., critic=) takes values and term_values from it instead of a value head -- for an "mfma"
MLPPolicy or a GRUPolicy without one -- and values_dev evaluates it on any stored observations.

Observation normalisation: ObsNorm keeps running mean / variance of the observations on the device and, attached to a policy or a
critic (obs_norm=, set_obs_norm), makes their kernels compute clamp((x - mean) / sqrt(var + eps), +-clip) where they stage each
observation -- what rl_games' normalize_input and SB3's VecNormalize put in front of a net (gaq.h gaq_obs_norm).  Every engine but "valu"
takes one; engine="auto" with obs_norm= resolves to "mfma".

Return normalisation: RetNorm is VecNormalize's other half -- a per-env running discounted return, running statistics of it, and rewards
divided by its standard deviation and clamped (gaq.h gaq_ret_norm).  It attaches to nothing: update_dev and normalize_dev run on a
rollout's rew / done tensors between rollout_policy_dev and gae_dev.

Gradients on the device: an "mfma" MLPPolicy and an MLPCritic with hidden widths up to 128 also run the learner's passes over stored
rows (gaq.h "gradients on the device"): logp_dev (log-probabilities and means of stored observations), ppo_grad_dev / mse_grad_dev (the
clipped PPO surrogate's and the squared value error's gradients, with their statistics) and backward_dev (a caller-given output
gradient), each deterministic and in the packed weight layout.  unpack_weights turns a packed gradient into nn.Linear shapes, and
set_weights_dev takes a packed device tensor back, so an optimiser can step the weights without a host copy.

Gradients of a recurrent policy: a GRUPolicy of H <= 64 (head widths <= 64) runs the same two halves over stored SEQUENCES
(gaq.h "gradients of a recurrent policy"): evaluate_seq_dev recomputes logp, V, the means and the final state of T steps from h0 with
the rollout's own bits, ppo_seq_grad_dev returns the truncated-BPTT gradient of the combined PPO loss; unpack_gru_weights is the
inverse of pack_gru_weights, and GRUPolicy.set_weights / set_weights_dev take new weights.  An LSTMPolicy of H <= 64 has the same
halves with its second state (gaq.h "gradients of an LSTM policy"): evaluate_seq_dev(obs, actions, done, h0, c0, ...), and
ppo_bptt_grad_dev / ppo_bptt_grad_idx_dev, whose gradient unpack_lstm_weights turns into nn.LSTMCell's shapes.

The optimiser on the device: AdamDev steps a policy's or a critic's weights in place from those gradient tensors (gaq.h "the optimiser
on the device") -- global-norm clipping, Adam / AdamW, no host synchronisation, capturable in a graph -- and get_weights /
get_value_head read the weights back from the handle."""
import ctypes as C

import numpy as np

from . import _lib
from .norm import AdvNorm, ObsNorm, RetNorm          # (their home is norm.py; they are part of this module's interface)

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


class _DescRnn(C.Structure):
    """gaq_policy_desc_rnn: the fields of gaq_policy_desc_ex, then the recurrent cell"""
    _fields_ = _DescEx._fields_ + [("cell", C.c_int32)]


class _DescRnnEnc(C.Structure):
    """gaq_policy_desc_rnn_enc: the fields of gaq_policy_desc_rnn (in_dim = the encoder's last width), then the encoder"""
    _fields_ = _DescRnn._fields_ + [("enc_in_dim", C.c_int32), ("enc_layers", C.c_int32), ("enc_width", C.c_int32 * 2)]


CELL_GRU = 1          # gaq.h GAQ_POLICY_CELL_GRU
CELL_LSTM = 3         # gaq.h GAQ_POLICY_CELL_LSTM (2 stays unassigned)


class _Cell:
    """What differs between the recurrent cells: the gaq.h id, the gates per unit (rows of W_ih / W_hh: GRU r, z, n; LSTM i, f, g, o),
    the name in messages and of the torch modules (nn.<name>Cell, nn.<name>), and the per-env state tensors a policy keeps."""

    def __init__(self, cell_id, gates, name, states):
        self.id, self.gates, self.name, self.states = cell_id, gates, name, states


_GRU = _Cell(CELL_GRU, 3, "GRU", ("hidden",))
_LSTM = _Cell(CELL_LSTM, 4, "LSTM", ("hidden", "cell"))


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


def unpack_weights(packed, in_dim, widths, n_out):
    """The inverse of pack_weights / pack_critic_weights: a flat array or tensor in the packed layout of a net with `in_dim` inputs,
    hidden `widths` and `n_out` outputs (4: a policy, 1: a critic) -> [(W [out, in], b [out]), ...] in nn.Linear shapes, NumPy for a
    NumPy input and torch (same device and dtype) for a tensor.  A packed gradient (MLPPolicy.ppo_grad_dev ...) unpacks into what
    param.grad takes.  ValueError for a wrong size."""
    widths = [int(w) for w in widths]
    in_dim, n_out = int(in_dim), int(n_out)
    flat = packed.reshape(-1)
    offs, want = weight_layout(in_dim, widths, n_out)
    if int(flat.shape[0]) != want:
        raise ValueError("packed has %d floats, a %s net packs into %d" % (int(flat.shape[0]), [in_dim] + widths + [n_out], want))
    perm = (lambda a: a.transpose(0, 2, 1)) if isinstance(flat, np.ndarray) else (lambda a: a.permute(0, 2, 1))
    out, prev = [], in_dim
    for w, off in zip(widths, offs):
        W = perm(flat[off:off + w * prev].reshape(w // 16, prev, 16)).reshape(w, prev)
        out.append((W, flat[off + w * prev:off + w * prev + w]))
        prev = w
    off = offs[-1]
    W = flat[off:off + n_out * prev].reshape(prev, n_out).T
    out.append((W, flat[off + n_out * prev:want]))
    return out


def weight_layout(in_dim, widths, n_out):
    """The packed layout of a net with `in_dim` inputs, hidden `widths` and `n_out` outputs: (the float offset of every layer's section,
    the output layer's last; the total floats).  A section is the layer's weights, then its bias.  (csrc/gaq_policy.hip net_layout
    describes the same layout.)  ValueError for a width that is no positive multiple of 16."""
    offs, n, prev = [], 0, int(in_dim)
    for w in widths:
        if w % 16 != 0 or w < 16:
            raise ValueError("hidden widths must be positive multiples of 16, got %s" % (list(widths),))
        offs.append(n)
        n += w * prev + w
        prev = w
    offs.append(n)
    return offs, n + n_out * prev + n_out


class _DeviceGrad:
    """What MLPPolicy and MLPCritic share of the gradients on the device (gaq.h): the checks of the row tensors, the outputs, the
    stream, and weights set from a packed device tensor.  N_OUT: 4 or 1; the classes keep .device, .in_dim, .widths, ._count."""

    N_OUT = None

    def _rows(self, obs):
        """obs [..., in_dim] -> (its leading shape, the number of rows)"""
        import torch
        if not isinstance(obs, torch.Tensor) or obs.dim() < 1 or obs.shape[-1] != self.in_dim:
            raise ValueError("obs must be a tensor of shape [..., %d], got %s" % (self.in_dim, tuple(getattr(obs, "shape", ()))))
        _lib.check_dev_f32("obs", obs, obs.shape, self.device)
        lead = tuple(obs.shape[:-1])
        return lead, int(np.prod(lead, dtype=np.int64))

    def _out(self, name, t, shape, like, dtype=None, zero=False):
        """`t` checked, or a new tensor of `shape` on the device of `like`"""
        import torch
        if t is None:
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype or torch.float32, device=like.device)
        _lib.check_dev_f32(name, t, shape, self.device, dtype)
        return t

    @staticmethod
    def _stream(like, stream):
        import torch
        return C.c_void_p(torch.cuda.current_stream(like.device).cuda_stream if stream is None else stream)

    def _idx(self, idx):
        """idx of an index-gathered call, checked: a contiguous int32 [rows] tensor on the handle's device -> rows"""
        import torch
        if not isinstance(idx, torch.Tensor) or idx.dim() != 1:
            raise ValueError("idx must be a contiguous torch.int32 tensor of shape [rows], got %s %s"
                             % (getattr(idx, "dtype", type(idx).__name__), tuple(getattr(idx, "shape", ()))))
        _lib.check_dev_f32("idx", idx, idx.shape, self.device, torch.int32)
        return int(idx.shape[0])

    def _rows_idx(self, idx, obs):
        """_rows for a call that may gather: -> (obs's leading shape, the call's rows, the source rows).  idx None: the call's rows are
        obs's; else idx is checked (before obs) and names them."""
        rows = None if idx is None else self._idx(idx)
        lead, src = self._rows(obs)
        return lead, src if idx is None else rows, src

    def unpack(self, packed):
        """unpack_weights for this net: a packed tensor or array (weights, a gradient) -> [(W, b), ...] in nn.Linear shapes"""
        return unpack_weights(packed, self.in_dim, self.widths, self.N_OUT)

    def _set_weights_dev(self, setter, packed):
        _lib.check_dev_f32("packed", packed, (self._count,), self.device)
        _lib.check(setter(self.handle, _lib.ptr(packed)))
        self.packed = None                                   # the host copy is stale: the weights live in the caller's tensor


def encoder_weight_count(in_dim, widths):
    """The floats of an encoder's block (gaq.h gaq_policy_encoder_weight_count): per layer W * in + W.  ValueError for a width that is
    no positive multiple of 16."""
    return weight_layout(in_dim, widths, 0)[1]


def pack_encoder_weights(layers):
    """[(W [out, in], b [out]), ...] (the encoder's 1 or 2 layers) -> the flat fp32 block gaq_policy_set_encoder_weights takes: per
    layer W'[out/16][in][16] (W'[c][k][j] = W[16c + j][k]) then bias -- pack_weights' hidden-layer rule, and no output layer."""
    out = []
    for W, b in layers:
        W = np.asarray(W, dtype=np.float32)
        o, i = W.shape
        out.append(W.reshape(o // 16, 16, i).transpose(0, 2, 1).reshape(-1))
        out.append(np.asarray(b, dtype=np.float32).reshape(-1))
    return np.ascontiguousarray(np.concatenate(out))


def unpack_encoder_weights(packed, in_dim, widths):
    """The inverse of pack_encoder_weights: a flat array or tensor of an encoder with `in_dim` inputs and layer `widths` ->
    [(W [out, in], b [out]), ...] in nn.Linear shapes (NumPy for NumPy, torch for a tensor).  ValueError for a wrong size."""
    widths = [int(w) for w in widths]
    flat = packed.reshape(-1)
    offs, want = weight_layout(int(in_dim), widths, 0)
    if int(flat.shape[0]) != want:
        raise ValueError("packed has %d floats, an encoder %s packs into %d" % (int(flat.shape[0]), [int(in_dim)] + widths, want))
    perm = (lambda a: a.transpose(0, 2, 1)) if isinstance(flat, np.ndarray) else (lambda a: a.permute(0, 2, 1))
    out, prev = [], int(in_dim)
    for w, off in zip(widths, offs):
        out.append((perm(flat[off:off + w * prev].reshape(w // 16, prev, 16)).reshape(w, prev), flat[off + w * prev:off + w * prev + w]))
        prev = w
    return out


def check_encoder_layers(layers, in_dim):
    """ValueError (the text says "encoder") unless `layers` is 1 or 2 (W [out, in], b [out]) layers on `in_dim` inputs whose widths
    are multiples of 16 in [16, 256]; returns the widths."""
    if not 1 <= len(layers) <= 2:
        raise ValueError("the encoder needs 1 or 2 Linear layers, got %d" % len(layers))
    prev, widths = int(in_dim), []
    for k, (W, b) in enumerate(layers):
        W, b = np.asarray(W), np.asarray(b)
        if W.ndim != 2 or b.shape != (W.shape[0],):
            raise ValueError("encoder layer %d: W must be [out, in] and b [out], got %s and %s" % (k, W.shape, b.shape))
        if W.shape[1] != prev:
            raise ValueError("encoder layer %d takes %d inputs, expected %d (the env's obs_dim for the first layer)" % (k, W.shape[1], prev))
        if W.shape[0] % 16 != 0 or not 16 <= W.shape[0] <= 256:
            raise ValueError("encoder layer %d has width %d: widths must be multiples of 16 in [16, 256]" % (k, W.shape[0]))
        prev = int(W.shape[0])
        widths.append(prev)
    return widths


def torch_encoder(module):
    """nn.Sequential [Linear, act (, Linear, act)] with act Tanh or ReLU for every layer (a trailing activation is required: the cell
    takes activations) -> ([(W, b), ...], 'tanh' | 'relu'); ValueError (the text says "encoder") otherwise."""
    import torch.nn as nn
    mods = list(module.children()) if isinstance(module, nn.Sequential) else [module]
    if len(mods) not in (2, 4):
        raise ValueError("the encoder must be nn.Sequential(Linear, act) or (Linear, act, Linear, act), got %d modules" % len(mods))
    layers, acts = [], set()
    for k, m in enumerate(mods):
        if k % 2 == 0:
            if not isinstance(m, nn.Linear):
                raise ValueError("encoder module %d: expected Linear, got %s" % (k, type(m).__name__))
            W = m.weight.detach().float().cpu().numpy()
            layers.append((W, np.zeros(W.shape[0], np.float32) if m.bias is None else m.bias.detach().float().cpu().numpy()))
        elif isinstance(m, (nn.Tanh, nn.ReLU)):
            acts.add("tanh" if isinstance(m, nn.Tanh) else "relu")
        else:
            raise ValueError("encoder module %d: only Tanh and ReLU activations are supported, got %s" % (k, type(m).__name__))
    if len(acts) != 1:
        raise ValueError("every encoder layer must use the same activation (tanh or relu), got %s" % sorted(acts))
    return layers, acts.pop()


def pack_gru_weights(gru, head_layers):
    """(W_ih [3H, I], W_hh [3H, H], b_ih [3H], b_hh [3H]) (torch GRUCell, gate rows r, z, n) and the head's layers -> the flat fp32
    layout of gaq.h gaq_policy_desc_rnn: W_ih' [3H/16][I][16], b_ih, W_hh' [3H/16][H][16], b_hh, then pack_weights(head_layers)."""
    W_ih, W_hh, b_ih, b_hh = (np.asarray(x, dtype=np.float32) for x in gru)
    out = []
    for W, b in ((W_ih, b_ih), (W_hh, b_hh)):
        o, i = W.shape
        out.append(W.reshape(o // 16, 16, i).transpose(0, 2, 1).reshape(-1))
        out.append(b.reshape(-1))
    out.append(pack_weights(head_layers))
    return np.ascontiguousarray(np.concatenate(out))


def unpack_gru_weights(packed, in_dim, hidden_size, head_widths=()):
    """The inverse of pack_gru_weights: a flat array or tensor in the packed layout of a GRU of `hidden_size` units on `in_dim` inputs
    with a head of hidden `head_widths` -> ((weight_ih [3H, I], weight_hh [3H, H], bias_ih [3H], bias_hh [3H]) in nn.GRUCell's shapes
    and gate order, [(W, b), ...] the head's layers in nn.Linear shapes), NumPy for a NumPy input and torch (same device and dtype)
    for a tensor.  A packed gradient (GRUPolicy.ppo_seq_grad_dev) unpacks into what param.grad takes.  ValueError for a wrong size."""
    return _unpack_cell_weights(_GRU, packed, in_dim, hidden_size, head_widths)


def unpack_lstm_weights(packed, in_dim, hidden_size, head_widths=()):
    """unpack_gru_weights for pack_lstm_weights' layout: ((weight_ih [4H, I], weight_hh [4H, H], bias_ih [4H], bias_hh [4H]) in
    nn.LSTMCell's shapes and gate order, the head's layers)."""
    return _unpack_cell_weights(_LSTM, packed, in_dim, hidden_size, head_widths)


def _unpack_cell_weights(cell, packed, in_dim, hidden_size, head_widths):
    I, H, G = int(in_dim), int(hidden_size), cell.gates
    head_widths = [int(w) for w in head_widths]
    if H % 16 != 0 or H < 16:
        raise ValueError("hidden_size must be a positive multiple of 16, got %d" % H)
    flat = packed.reshape(-1)
    floats = G * H * (I + H) + 2 * G * H
    want = floats + weight_layout(H, head_widths, 4)[1]
    if int(flat.shape[0]) != want:
        raise ValueError("packed has %d floats, a %s(%d, %d) with head %s packs into %d"
                         % (int(flat.shape[0]), cell.name, I, H, head_widths + [4], want))
    perm = (lambda a: a.transpose(0, 2, 1)) if isinstance(flat, np.ndarray) else (lambda a: a.permute(0, 2, 1))
    o = 0
    W_ih = perm(flat[o:o + G * H * I].reshape(G * H // 16, I, 16)).reshape(G * H, I)
    o += G * H * I
    b_ih = flat[o:o + G * H]
    o += G * H
    W_hh = perm(flat[o:o + G * H * H].reshape(G * H // 16, H, 16)).reshape(G * H, H)
    o += G * H * H
    b_hh = flat[o:o + G * H]
    return (W_ih, W_hh, b_ih, b_hh), unpack_weights(flat[floats:], H, head_widths, 4)


def check_cell_layers(cell, weights, head_layers, in_dim, hidden_act):
    """ValueError unless weights = (W_ih, W_hh, b_ih, b_hh) is a cell (_Cell) of H units (a multiple of 16 in [16, 256]) on obs_dim
    inputs and head_layers are 0 to 2 hidden layers on H (widths multiples of 16 in [16, 256]) then a 4-output layer."""
    G = cell.gates
    if len(weights) != 4:
        raise ValueError("%s must be (W_ih, W_hh, b_ih, b_hh)" % cell.name.lower())
    W_ih, W_hh, b_ih, b_hh = (np.asarray(x) for x in weights)
    if W_ih.ndim != 2 or W_ih.shape[0] % G != 0:
        raise ValueError("W_ih must be [%dH, obs_dim], got shape %s" % (G, W_ih.shape))
    H = W_ih.shape[0] // G
    if H % 16 != 0 or not 16 <= H <= 256:
        raise ValueError("the %s has %d units: H must be a multiple of 16 in [16, 256]" % (cell.name, H))
    if W_ih.shape[1] != int(in_dim):
        raise ValueError("W_ih takes %d inputs, expected the env's obs_dim %d" % (W_ih.shape[1], int(in_dim)))
    if W_hh.shape != (G * H, H):
        raise ValueError("W_hh must be [%dH, H] = [%d, %d], got %s" % (G, G * H, H, W_hh.shape))
    if b_ih.shape != (G * H,) or b_hh.shape != (G * H,):
        raise ValueError("b_ih and b_hh must be [%dH] = [%d]" % (G, G * H))
    if not 1 <= len(head_layers) <= 3:
        raise ValueError("the head needs 0 to 2 hidden layers and an output layer, got %d Linear layers" % len(head_layers))
    check_layers([(np.zeros((H, int(in_dim)), np.float32), np.zeros(H, np.float32))] + list(head_layers), in_dim, hidden_act, "mfma")


def torch_cell(cell, module):
    """nn.<name>Cell, or nn.<name> with one unidirectional layer and no proj_size, of the cell (_Cell) -> (W_ih, W_hh, b_ih, b_hh) as
    fp32 arrays (a missing bias becomes zeros); ValueError otherwise (the other cell's modules by name)."""
    import torch.nn as nn
    name = "nn." + cell.name
    if isinstance(module, getattr(nn, cell.name + "Cell")):
        ws = (module.weight_ih, module.weight_hh, module.bias_ih, module.bias_hh)
    elif isinstance(module, getattr(nn, cell.name)):
        if module.num_layers != 1:
            raise ValueError("%s must have num_layers=1, has %d" % (name, module.num_layers))
        if module.bidirectional:
            raise ValueError("a bidirectional %s cannot run step by step in a rollout" % name)
        if getattr(module, "proj_size", 0):
            raise ValueError("%s with proj_size is not supported" % name)
        ws = (module.weight_ih_l0, module.weight_hh_l0, getattr(module, "bias_ih_l0", None), getattr(module, "bias_hh_l0", None))
    else:
        raise ValueError("the cell must be %sCell or %s, got %s" % (name, name, type(module).__name__))
    W_ih, W_hh = (w.detach().float().cpu().numpy() for w in ws[:2])
    b_ih, b_hh = (np.zeros(W_ih.shape[0], np.float32) if b is None else b.detach().float().cpu().numpy() for b in ws[2:])
    return W_ih, W_hh, b_ih, b_hh


def check_gru_layers(gru, head_layers, in_dim, hidden_act):
    """check_cell_layers for a GRU cell (W_ih [3H, obs_dim], gate rows r, z, n)"""
    check_cell_layers(_GRU, gru, head_layers, in_dim, hidden_act)


def check_lstm_layers(lstm, head_layers, in_dim, hidden_act):
    """check_cell_layers for an LSTM cell (W_ih [4H, obs_dim], gate rows i, f, g, o)"""
    check_cell_layers(_LSTM, lstm, head_layers, in_dim, hidden_act)


def torch_gru(cell):
    """nn.GRUCell, or nn.GRU with one unidirectional layer -> (W_ih, W_hh, b_ih, b_hh) as fp32 arrays; ValueError otherwise."""
    return torch_cell(_GRU, cell)


def torch_lstm(cell):
    """nn.LSTMCell, or nn.LSTM with one unidirectional layer and no proj_size -> (W_ih, W_hh, b_ih, b_hh) as fp32 arrays; ValueError
    otherwise (GRU modules by name: GRUPolicy takes those)."""
    return torch_cell(_LSTM, cell)


def pack_lstm_weights(lstm, head_layers):
    """(W_ih [4H, I], W_hh [4H, H], b_ih [4H], b_hh [4H]) (torch LSTMCell, gate rows i, f, g, o) and the head's layers -> the flat fp32
    layout of gaq.h GAQ_POLICY_CELL_LSTM: W_ih' [4H/16][I][16], b_ih, W_hh' [4H/16][H][16], b_hh, then pack_weights(head_layers).  The
    rule is pack_gru_weights' (it never looks at the number of gates)."""
    return pack_gru_weights(lstm, head_layers)


def torch_head(module):
    """A bare nn.Linear(H, 4) (alone or in a Sequential, optionally followed by Tanh), or an MLP Sequential in the form torch_layers
    takes -> ([(W, b), ...], 'tanh' | 'relu', out_tanh).  A head without hidden layers reports 'tanh', which it never uses."""
    import torch.nn as nn
    mods = list(module.children()) if isinstance(module, nn.Sequential) else [module]
    out_tanh = bool(mods) and isinstance(mods[-1], nn.Tanh)
    if out_tanh:
        mods = mods[:-1]
    if len(mods) == 1 and isinstance(mods[0], nn.Linear):
        m = mods[0]
        W = m.weight.detach().float().cpu().numpy()
        b = np.zeros(W.shape[0], np.float32) if m.bias is None else m.bias.detach().float().cpu().numpy()
        return [(W, b)], "tanh", out_tanh
    return torch_layers(module)


def _check_mlp_layers(layers, in_dim, hidden_act, noun, output, n_out, maxw, note=""):
    """ValueError unless `layers` is obs_dim inputs, 1-3 hidden layers of widths 16k <= maxw and n_out outputs: check_layers and
    check_critic_layers.  noun: "policy" / "critic"; output: how the message calls the last layer; note: behind the width message."""
    if hidden_act not in _ACTS:
        raise ValueError("hidden activation must be 'tanh' or 'relu', got %r" % (hidden_act,))
    if not 2 <= len(layers) <= 4:
        raise ValueError("the %s needs 1 to 3 hidden layers and an output layer, got %d Linear layers" % (noun, len(layers)))
    prev = int(in_dim)
    for k, (W, b) in enumerate(layers):
        W, b = np.asarray(W), np.asarray(b)
        if W.ndim != 2 or b.shape != (W.shape[0],):
            raise ValueError("layer %d: W must be [out, in] and b [out], got %s and %s" % (k, W.shape, b.shape))
        if W.shape[1] != prev:
            raise ValueError("layer %d takes %d inputs, expected %d (the env's obs_dim for the first layer)" % (k, W.shape[1], prev))
        last = k == len(layers) - 1
        if last and W.shape[0] != n_out:
            raise ValueError("%s must have %d output%s, has %d" % (output, n_out, "s" if n_out > 1 else "", W.shape[0]))
        if not last and (W.shape[0] % 16 != 0 or not 16 <= W.shape[0] <= maxw):
            raise ValueError("hidden layer %d has width %d: widths must be multiples of 16 in [16, %d]%s" % (k, W.shape[0], maxw, note))
        prev = W.shape[0]


def check_layers(layers, in_dim, hidden_act, engine="valu"):
    """ValueError unless `layers` is an MLP the device engine can run (obs_dim inputs, 1-3 hidden layers, widths 16k <= 128 for "valu" and
    <= 256 for "mfma" and "bf16", 4 outputs)."""
    if engine not in ENGINES:
        raise ValueError("engine must be 'valu', 'mfma' or 'bf16', got %r" % (engine,))
    _check_mlp_layers(layers, in_dim, hidden_act, "policy", "the output layer", 4, _MAX_WIDTH[engine], _ENGINE_NOTE[engine])


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


def check_value_head(last_width, engine, w, b):
    """The value head V = w . y + b of a policy whose last hidden layer has `last_width` units, as the last_width + 1 floats
    gaq_policy_set_value_head takes (weights, then bias).  w is [last_width] or [1, last_width] (torch Linear(W, 1).weight), b a scalar
    (or [1]).  ValueError for another shape, or for an engine without a value head ("valu", "bf16")."""
    if engine not in ENGINES:
        raise ValueError("engine must be 'valu', 'mfma' or 'bf16', got %r" % (engine,))
    if engine != "mfma":
        raise ValueError("the %r engine has no value head: use engine='mfma' (or a GRUPolicy)" % (engine,))
    w, b = np.asarray(w, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if w.shape not in ((int(last_width),), (1, int(last_width))):
        raise ValueError("the value head's weights must be [%d] or [1, %d] (the last hidden layer's width), got shape %s"
                         % (last_width, last_width, w.shape))
    if b.shape not in ((), (1,)):
        raise ValueError("the value head's bias must be a scalar, got shape %s" % (b.shape,))
    return np.ascontiguousarray(np.concatenate([w.reshape(-1), b.reshape(-1)]))


def torch_value(module):
    """nn.Linear(W, 1) -> (w [W], b scalar) as fp32 arrays; ValueError for anything else."""
    import torch.nn as nn
    if not isinstance(module, nn.Linear) or module.out_features != 1:
        raise ValueError("value must be an nn.Linear(W, 1) on the last hidden layer, got %s"
                         % (module if isinstance(module, nn.Linear) else type(module).__name__,))
    w = module.weight.detach().float().cpu().numpy().reshape(-1)
    b = np.float32(0.0) if module.bias is None else module.bias.detach().float().cpu().numpy().reshape(())
    return w, b


def _fill_desc(d, in_dim, widths, hidden_act, **own):
    """The fields every description has (_Desc, _DescEx, _DescRnn, _CriticDesc), then its `own` (out_tanh, engine, cell); returns d"""
    d.struct_size = C.sizeof(d)
    d.in_dim, d.n_hidden, d.hidden_act = int(in_dim), len(widths), _ACTS[hidden_act]
    for k, w in enumerate(widths):
        d.width[k] = w
    for name, v in own.items():
        setattr(d, name, v)
    return d


class _Handle:
    """The lifetime of a library handle: what every policy, MLPCritic and AdamDev share.  The classes name the library's destroy
    function; the instances keep ._lib and .handle."""

    _DESTROY = None

    def _unregister(self):
        """before the handle goes: take back what was registered with it"""

    def close(self):
        if getattr(self, "handle", None) is not None:
            self._unregister()
            getattr(self._lib, self._DESTROY)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceNet(_Handle):
    """What every policy and MLPCritic share: the handle's lifetime, the attached normaliser and the weights read back.  The classes
    name the library's destroy, set-normaliser and get-weights functions; the instances keep ._lib and .handle."""

    _SET_OBS_NORM = _GET_WEIGHTS = None
    obs_norm = None

    def get_packed(self):
        """The weights as they stand on the device, in the packed layout set_weights_dev takes: a float32 array [weight_count]
        (synchronous: after everything enqueued on the device -- an AdamDev step included)."""
        out = np.empty(self._count, dtype=np.float32)
        _lib.check(getattr(self._lib, self._GET_WEIGHTS)(self.handle, _lib.ptr(out)))
        return out

    def get_weights(self):
        """The weights as they stand on the device, in the shapes .unpack gives: what to export to torch or to a file once an AdamDev
        steps them in the handle (synchronous)."""
        return self.unpack(self.get_packed())

    def set_obs_norm(self, norm):
        """Attach an ObsNorm of the same env (None: detach): every launch that evaluates this net -- a policy's in a rollout, terminal
        observations included; a critic's values_dev and every value a rollout takes from it -- then normalises the observation it
        stages.  The net keeps a reference.  ValueError for a policy on the "valu" engine."""
        if norm is not None and not isinstance(norm, ObsNorm):
            raise ValueError("obs_norm must be an ObsNorm or None, got %s" % type(norm).__name__)
        if norm is not None and norm.handle is None:
            raise ValueError("the ObsNorm is closed")
        _lib.check(getattr(self._lib, self._SET_OBS_NORM)(self.handle, None if norm is None else norm.handle))
        self.obs_norm = norm

    def _unregister(self):
        """before the handle goes: take back the buffers registered with it (a recurrent policy's states)"""

    def close(self):
        super().close()
        self.obs_norm = None


class _DevicePolicy(_DeviceNet):
    """What MLPPolicy, GRUPolicy and LSTMPolicy share: the value head and exploration"""

    _DESTROY, _SET_OBS_NORM, _GET_WEIGHTS = "gaq_policy_destroy", "gaq_policy_set_obs_norm", "gaq_policy_get_weights"

    def get_value_head(self):
        """The value head as it stands on the device: (w [W], b) float32 (synchronous); GaqError without one."""
        out = np.empty(self.widths[-1] + 1, dtype=np.float32)
        _lib.check(self._lib.gaq_policy_get_value_head(self.handle, _lib.ptr(out)))
        return out[:-1].copy(), out[-1]

    def set_value_head(self, w=None, b=None):
        """The critic V = w . y + b on the activations the 4-output layer reads (w [W] or [1, W], b a scalar; W = the last hidden
        layer's width, for a GRU without head layers H), or set_value_head(None) to remove it.  rollout_policy_dev(values=...) needs it."""
        if w is None:
            self.value_head = None
            _lib.check(self._lib.gaq_policy_set_value_head(self.handle, None))
            return
        self.value_head = check_value_head(self.widths[-1], self.engine, w, 0.0 if b is None else b)
        assert self._lib.gaq_policy_value_width(self.handle) == self.widths[-1]
        _lib.check(self._lib.gaq_policy_set_value_head(self.handle, _lib.ptr(self.value_head)))

    def set_value_head_dev(self, packed):
        """The value head from a float32 tensor [W + 1] on the policy's device: the weights, then the bias -- grad_value's layout
        (gaq_policy_set_value_head_dev; synchronous, no host copy): what an optimiser that steps the head's tensor calls after each
        step.  .value_head becomes True: the head lives in the caller's tensor."""
        _lib.check_dev_f32("packed", packed, (self.widths[-1] + 1,), self.device)
        if self.engine != "mfma":
            raise ValueError("the %r engine has no value head: use engine='mfma' (or a GRUPolicy)" % (self.engine,))
        _lib.check(self._lib.gaq_policy_set_value_head_dev(self.handle, _lib.ptr(packed)))
        self.value_head = True

    def set_log_std(self, log_std=None):
        """Exploration: a = mean + exp(log_std[k]) * z_k (4 floats), or None for the deterministic policy."""
        self.log_std = None if log_std is None else np.ascontiguousarray(np.asarray(log_std, dtype=np.float32).reshape(4))
        _lib.check(self._lib.gaq_policy_set_explore(self.handle, _lib.ptr(self.log_std)))

    log_std_dev = None                                        # device mode: the [4] view of the table the kernels read

    def log_std_to_device(self):
        """Keep log_std on the device (gaq_policy_set_explore_dev): the policy allocates a float32 tensor of 12 words, log_std[4] |
        std[4] | inv_std[4], registers it, and every rollout, log-prob and gradient launch reads log_std there -- what an AdamDev
        with learn_log_std steps in place, so that a captured gradient call + step learns log_std and the next rollout flies with
        the new scale, no synchronisation anywhere.  At the switch the kernels see the bits they saw before.  An "mfma" MLPPolicy, a
        GRUPolicy or an LSTMPolicy with log_std set.  Returns .log_std_dev, a [4] view of the table: read it with torch ops on the
        stream; .log_std is only what the host last set (get_log_std() reads the device).  Create the AdamDev after the switch."""
        import torch
        if self.log_std_dev is None:
            dev = torch.device("cuda", self.device)
            table = torch.empty(12, dtype=torch.float32, device=dev)
            _lib.check(self._lib.gaq_policy_set_explore_dev(self.handle, _lib.ptr(table),
                                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            self._explore_table, self.log_std_dev = table, table[:4]
        return self.log_std_dev

    def log_std_to_host(self):
        """Leave device mode (synchronous): log_std becomes the values the table holds, on the host, as set_log_std would set them."""
        if self.log_std_dev is not None:
            _lib.check(self._lib.gaq_policy_set_explore_dev(self.handle, None, None))
            self._explore_table = self.log_std_dev = None
            self.log_std = self.get_log_std()

    def get_log_std(self):
        """The current log_std, a float32 array [4], in either mode (device mode: synchronous, after everything enqueued on the
        device); .log_std follows.  GaqError for a deterministic policy."""
        out = np.empty(4, dtype=np.float32)
        _lib.check(self._lib.gaq_policy_get_log_std(self.handle, _lib.ptr(out)))
        self.log_std = out
        return out.copy()


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


class MLPPolicy(_DevicePolicy, _DeviceGrad):
    """An MLP evaluated on the device inside QuadrotorEnv.rollout_policy_dev.  Build with from_torch / from_arrays.

    engine="bf16" runs every layer on the bf16 matrix cores under this contract (gaq.h GAQ_POLICY_ENGINE_MFMA_BF16):
    - weights: the fp32 weights are rounded to bf16 (round to nearest even) once, when they are set; biases stay fp32.  A bf16 torch
      module loses nothing (from_torch widens it with .float(), which is exact, and re-rounding a bf16 value is the identity);
    - activations: the input of every layer (the observation and each hidden activation) is rounded once to bf16; the activation
      function runs in fp32 on the fp32 sum and only its result is rounded;
    - accumulation: each unit starts at its fp32 bias and sums bf16 x bf16 products in fp32, the 4 outputs likewise; the order of those
      fp32 sums is the matrix core's, so the results are deterministic but not bit-equal to the fp32 engines or to torch;
    - the output tanh and the exploration term are those of the other engines (the same draws for the same seed, env and step)."""

    def __init__(self, env, layers, hidden_act="tanh", out_tanh=False, log_std=None, engine="auto", value=None, obs_norm=None):
        # (a value head and a normaliser live on the "mfma" engine: "auto" with either means "mfma"; without it is what it always was)
        needs_mfma = value is not None or obs_norm is not None
        self.engine = resolve_engine(layers, env.obs_dim, hidden_act, "mfma" if engine == "auto" and needs_mfma else engine)
        if value is not None:
            check_value_head(int(np.asarray(layers[-2][0]).shape[0]), self.engine, *value)
        self._lib = _lib.load()
        self.env_handle = _lib.handle_value(env._handle)
        self.hidden_act, self.out_tanh = hidden_act, bool(out_tanh)
        self.device, self.in_dim = int(env.device), int(env.obs_dim)
        self.widths = [int(np.asarray(W).shape[0]) for W, _ in layers[:-1]]
        if self.engine == "valu":       # the original entry points: exactly what every caller before the MFMA engine got
            d, own, create, count = _Desc(), {}, self._lib.gaq_policy_create, self._lib.gaq_policy_weight_count
        else:
            d, own, create, count = _DescEx(), {"engine": ENGINES[self.engine]}, self._lib.gaq_policy_create_ex, self._lib.gaq_policy_weight_count_ex
        _fill_desc(d, env.obs_dim, self.widths, hidden_act, out_tanh=int(self.out_tanh), **own)
        h = C.c_void_p()
        _lib.check(create(env._handle, C.byref(d), C.byref(h)))
        self.handle = h
        assert self._lib.gaq_policy_engine(h) == ENGINES[self.engine]
        self.packed = pack_weights(layers)
        self._count = int(count(C.byref(d)))
        assert self.packed.size == self._count
        _lib.check(self._lib.gaq_policy_set_weights(h, _lib.ptr(self.packed)))
        self.set_log_std(log_std)
        self.value_head = None
        if value is not None:
            self.set_value_head(*value)
        if obs_norm is not None:
            self.set_obs_norm(obs_norm)

    N_OUT = 4

    def set_weights(self, layers):
        """New weights for the same architecture: layers = [(W, b), ...] as from_arrays takes them (synchronous)."""
        layers = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in layers]
        check_layers(layers, self.in_dim, self.hidden_act, self.engine)
        widths = [int(W.shape[0]) for W, _ in layers[:-1]]
        if widths != self.widths:
            raise ValueError("set_weights: hidden widths %s, the policy was built with %s" % (widths, self.widths))
        packed = pack_weights(layers)
        assert packed.size == self._count
        _lib.check(self._lib.gaq_policy_set_weights(self.handle, _lib.ptr(packed)))
        self.packed = packed

    def set_weights_dev(self, packed):
        """New weights from a packed float32 tensor [weight_count] on the policy's device (gaq_policy_set_weights_dev; synchronous, no
        host copy): what an optimiser that steps the packed tensor calls after each step.  .packed becomes None."""
        self._set_weights_dev(self._lib.gaq_policy_set_weights_dev, packed)

    def logp_dev(self, obs, actions, out=None, mean=None, stream=None):
        """Log-probabilities of stored actions under the current weights and log_std (gaq_policy_logp_dev): obs [..., obs_dim],
        actions [..., 4] -> out [...] (allocated if None); mean [..., 4], if given, receives the policy's mean, bit for bit the
        deterministic rollout's action.  An "mfma" policy of widths <= 128 with log_std set; one launch, no host synchronisation."""
        lead, rows = self._rows(obs)
        _lib.check_dev_f32("actions", actions, lead + (4,), self.device)
        out = self._out("out", out, lead, obs)
        if mean is not None:
            _lib.check_dev_f32("mean", mean, lead + (4,), self.device)
        _lib.check(self._lib.gaq_policy_logp_dev(self.handle, rows, _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(out), _lib.ptr(mean),
                                                 self._stream(obs, stream)))
        return out

    def backward_dev(self, obs, dout, scale=1.0, grad=None, stream=None):
        """grad [weight_count] (packed layout; allocated if None) = sum over rows of scale * dout . d mean / d theta for a caller-given
        dout [..., 4], the gradient with respect to the mean (gaq_policy_backward_dev).  Returns grad."""
        lead, rows = self._rows(obs)
        _lib.check_dev_f32("dout", dout, lead + (4,), self.device)
        grad = self._out("grad", grad, (self._count,), obs)
        _lib.check(self._lib.gaq_policy_backward_dev(self.handle, rows, _lib.ptr(obs), _lib.ptr(dout), float(scale), _lib.ptr(grad),
                                                     self._stream(obs, stream)))
        return grad

    def ppo_grad_dev(self, obs, actions, logp_old, adv, clip=0.2, scale=None, grad=None, grad_log_std=None, stats=None, stream=None):
        """The gradient of the clipped PPO surrogate L = -min(r A, clamp(r, 1 - clip, 1 + clip) A), r = exp(logp - logp_old), summed
        over the rows and times `scale` (default 1 / rows: the mean), with respect to the packed weights -> grad [weight_count] and to
        log_std -> grad_log_std [4]; stats [4] float64 = sum of L (unscaled), rows clipped, sum of r - 1 - log r (the k3 KL estimate),
        rows (gaq_policy_grad_ppo_dev).  obs [..., obs_dim], actions [..., 4], logp_old and adv [...].  Two launches, no host
        synchronisation, deterministic.  Returns (grad, grad_log_std, stats)."""
        return self._ppo_grad(None, obs, actions, logp_old, adv, clip, scale, grad, grad_log_std, stats, stream)

    def ppo_grad_idx_dev(self, idx, obs, actions, logp_old, adv, clip=0.2, scale=None, grad=None, grad_log_std=None, stats=None,
                         stream=None):
        """ppo_grad_dev on the minibatch idx names, without a gathered copy (gaq_policy_grad_ppo_idx_dev): idx is a contiguous int32
        [rows] tensor on the policy's device, and row j of the minibatch is row idx[j] of the source tensors -- obs [..., obs_dim],
        actions [..., 4], logp_old and adv [...], the rollout's own buffers; a leading [T, N] shape is flattened, so idx indexes
        t * N + n.  With every index in range each output is bit for bit ppo_grad_dev's on obs.flatten(0, -2)[idx] etc.; an index out
        of range contributes nothing and is counted.  scale defaults to 1 / rows.  Returns (grad, grad_log_std, stats [5] float64:
        ppo_grad_dev's four, then the number of indices skipped).  Two launches, no host synchronisation, deterministic."""
        return self._ppo_grad(idx, obs, actions, logp_old, adv, clip, scale, grad, grad_log_std, stats, stream)

    def _ppo_grad(self, idx, obs, actions, logp_old, adv, clip, scale, grad, grad_log_std, stats, stream):
        """ppo_grad_dev (idx None) and ppo_grad_idx_dev"""
        import torch
        lead, rows, src = self._rows_idx(idx, obs)
        _lib.check_dev_f32("actions", actions, lead + (4,), self.device)
        _lib.check_dev_f32("logp_old", logp_old, lead, self.device)
        _lib.check_dev_f32("adv", adv, lead, self.device)
        grad = self._out("grad", grad, (self._count,), obs)
        grad_log_std = self._out("grad_log_std", grad_log_std, (4,), obs)
        stats = self._out("stats", stats, (4 if idx is None else 5,), obs, torch.float64)
        scale = 1.0 / max(rows, 1) if scale is None else float(scale)
        call, first = (self._lib.gaq_policy_grad_ppo_dev, ()) if idx is None else (self._lib.gaq_policy_grad_ppo_idx_dev, (_lib.ptr(idx), src))
        _lib.check(call(self.handle, rows, *first, _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(logp_old), _lib.ptr(adv), float(clip), scale,
                        _lib.ptr(grad), _lib.ptr(grad_log_std), _lib.ptr(stats), self._stream(obs, stream)))
        return grad, grad_log_std, stats

    def evaluate_dev(self, obs, actions, logp=None, value=None, mean=None, stream=None):
        """The learner's forward pass of a policy with a value head on stored rows (gaq_policy_eval_ac_dev): obs [..., obs_dim],
        actions [..., 4] -> logp [...] and value [...] (allocated if None); mean [..., 4], if given, receives the policy's mean.  logp
        and mean are logp_dev's bits, value the bits rollout_policy_dev(values=) records on the same observation.  An "mfma" policy of
        widths <= 128 with log_std and a value head set; one launch, no host synchronisation.  Returns (logp, value)."""
        lead, rows = self._rows(obs)
        _lib.check_dev_f32("actions", actions, lead + (4,), self.device)
        logp = self._out("logp", logp, lead, obs)
        value = self._out("value", value, lead, obs)
        if mean is not None:
            _lib.check_dev_f32("mean", mean, lead + (4,), self.device)
        _lib.check(self._lib.gaq_policy_eval_ac_dev(self.handle, rows, _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(logp), _lib.ptr(value),
                                                    _lib.ptr(mean), self._stream(obs, stream)))
        return logp, value

    def ppo_ac_grad_dev(self, obs, actions, logp_old, adv, ret, v_old=None, clip=0.2, vclip=None, vf_coef=0.5, ent_coef=0.0, scale=None,
                        grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None):
        """The gradient of the combined PPO loss of a policy with a value head on its trunk, L = L_clip + vf_coef L_V - ent_coef H per
        row, summed over the rows and times `scale` (default 1 / rows), in one forward and one backward pass
        (gaq_policy_grad_ppo_ac_dev).  L_clip is ppo_grad_dev's surrogate; L_V = (V - ret)^2 / 2, or with vclip > 0 (then v_old [...] is
        needed) max((V - ret)^2, (v_old + clamp(V - v_old, +-vclip) - ret)^2) / 2, the PPO2 clipped value loss; H the Gaussian's entropy
        (it adds -ent_coef * scale * rows to each component of grad_log_std).  Returns (grad [weight_count]: the packed trunk and
        4-output layer, grad_value [W + 1]: the value head's weights then bias, grad_log_std [4], stats [6] float64 = sum of L_clip,
        rows with the ratio clipped, sum of r - 1 - log r, sum of L_V (unweighted, unscaled), rows whose value gradient the clip cut,
        rows).  Two launches, no host synchronisation, deterministic."""
        return self._ppo_ac_grad("ppo_ac_grad_dev", None, obs, actions, logp_old, adv, ret, v_old, clip, vclip, vf_coef, ent_coef, scale, grad,
                                 grad_value, grad_log_std, stats, stream)

    def ppo_ac_grad_idx_dev(self, idx, obs, actions, logp_old, adv, ret, v_old=None, clip=0.2, vclip=None, vf_coef=0.5, ent_coef=0.0,
                            scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None):
        """ppo_ac_grad_dev on the minibatch idx names, without a gathered copy (gaq_policy_grad_ppo_ac_idx_dev): idx, the source
        tensors and the bit equality as ppo_grad_idx_dev states them, ret and v_old [...] included.  scale defaults to 1 / rows.
        Returns (grad, grad_value, grad_log_std, stats [7] float64: ppo_ac_grad_dev's six, then the number of indices skipped).  With a
        permutation from perm_dev(epoch_dev=) and AdamDev.step(sync_log_std=False) an epoch of shuffled minibatches is capturable in a
        graph."""
        return self._ppo_ac_grad("ppo_ac_grad_idx_dev", idx, obs, actions, logp_old, adv, ret, v_old, clip, vclip, vf_coef, ent_coef, scale,
                                 grad, grad_value, grad_log_std, stats, stream)

    def _ppo_ac_grad(self, who, idx, obs, actions, logp_old, adv, ret, v_old, clip, vclip, vf_coef, ent_coef, scale, grad, grad_value,
                     grad_log_std, stats, stream):
        """ppo_ac_grad_dev (idx None) and ppo_ac_grad_idx_dev; who: the public method's name, for its messages"""
        import torch
        lead, rows, src = self._rows_idx(idx, obs)
        _lib.check_dev_f32("actions", actions, lead + (4,), self.device)
        for name, t in (("logp_old", logp_old), ("adv", adv), ("ret", ret)):
            _lib.check_dev_f32(name, t, lead, self.device)
        vclip = 0.0 if vclip is None else float(vclip)
        if v_old is not None:
            _lib.check_dev_f32("v_old", v_old, lead, self.device)
        elif vclip > 0.0:
            raise ValueError("%s: vclip > 0 needs v_old" % who)
        grad = self._out("grad", grad, (self._count,), obs)
        grad_value = self._out("grad_value", grad_value, (self.widths[-1] + 1,), obs)
        grad_log_std = self._out("grad_log_std", grad_log_std, (4,), obs)
        stats = self._out("stats", stats, (6 if idx is None else 7,), obs, torch.float64)
        scale = 1.0 / max(rows, 1) if scale is None else float(scale)
        call, first = ((self._lib.gaq_policy_grad_ppo_ac_dev, ()) if idx is None
                       else (self._lib.gaq_policy_grad_ppo_ac_idx_dev, (_lib.ptr(idx), src)))
        _lib.check(call(self.handle, rows, *first, _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(logp_old), _lib.ptr(adv), _lib.ptr(ret),
                        _lib.ptr(v_old), float(clip), vclip, float(vf_coef), float(ent_coef), scale, _lib.ptr(grad), _lib.ptr(grad_value),
                        _lib.ptr(grad_log_std), _lib.ptr(stats), self._stream(obs, stream)))
        return grad, grad_value, grad_log_std, stats

    def evaluate_wide_dev(self, obs, actions, logp=None, value=None, mean=None, stream=None):
        """evaluate_dev for hidden widths up to 256 (gaq_policy_eval_wide_dev; gaq.h "the wide learner"): an "mfma" policy with log_std
        set, with or without a value head, whose in_dim rounded up to 16 + hidden widths sum to at most 560 (18-256-256 passes, three
        layers of 256 do not).  obs [..., obs_dim], actions [..., 4] -> logp [...] (allocated if None); mean [..., 4], if given,
        receives the policy's mean.  With a value head value [...] is written (allocated if None); without one it must be None and
        None is returned in its place.  On widths <= 128 every output is evaluate_dev's bits.  Returns (logp, value)."""
        lead, rows = self._rows(obs)
        _lib.check_dev_f32("actions", actions, lead + (4,), self.device)
        logp = self._out("logp", logp, lead, obs)
        if self.value_head is None and value is not None:
            raise ValueError("evaluate_wide_dev: the policy has no value head: value must be None")
        if self.value_head is not None:
            value = self._out("value", value, lead, obs)
        if mean is not None:
            _lib.check_dev_f32("mean", mean, lead + (4,), self.device)
        _lib.check(self._lib.gaq_policy_eval_wide_dev(self.handle, rows, _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(logp), _lib.ptr(value),
                                                      _lib.ptr(mean), self._stream(obs, stream)))
        return logp, value

    def ppo_wide_grad_dev(self, obs, actions, logp_old, adv, ret=None, v_old=None, *, idx=None, clip=0.2, vclip=None, vf_coef=0.5,
                          ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None):
        """The PPO gradient for hidden widths up to 256 (gaq_policy_grad_ppo_wide_dev; evaluate_wide_dev states the family and its one
        limit).  With a value head it is ppo_ac_grad_dev -- with idx (a contiguous int32 [rows] tensor: the minibatch's source rows)
        ppo_ac_grad_idx_dev -- in loss, outputs and stats ([6] float64, [7] with idx), and ret [...] is needed.  Without one ret, v_old
        and grad_value must be None, the loss is L_clip - ent_coef H, grad_value is returned as None and stats keeps its layout (the
        value loss and the rows its clip cut: 0).  On widths <= 128 every output is the narrow call's bits.  The packed gradients go to
        unpack_weights, set_weights_dev, set_value_head_dev and AdamDev.step as they are.  scale defaults to 1 / rows.  Returns
        (grad, grad_value, grad_log_std, stats).  Two launches, no host synchronisation, deterministic."""
        import torch
        who = "ppo_wide_grad_dev"
        lead, rows, src = self._rows_idx(idx, obs)
        _lib.check_dev_f32("actions", actions, lead + (4,), self.device)
        for name, t in (("logp_old", logp_old), ("adv", adv)):
            _lib.check_dev_f32(name, t, lead, self.device)
        vclip = 0.0 if vclip is None else float(vclip)
        if self.value_head is None:
            if ret is not None or v_old is not None or grad_value is not None:
                raise ValueError("%s: the policy has no value head: ret, v_old and grad_value must be None" % who)
        else:
            if ret is None:
                raise ValueError("%s: the policy has a value head: its loss needs ret" % who)
            _lib.check_dev_f32("ret", ret, lead, self.device)
            if v_old is not None:
                _lib.check_dev_f32("v_old", v_old, lead, self.device)
            elif vclip > 0.0:
                raise ValueError("%s: vclip > 0 needs v_old" % who)
            grad_value = self._out("grad_value", grad_value, (self.widths[-1] + 1,), obs)
        grad = self._out("grad", grad, (self._count,), obs)
        grad_log_std = self._out("grad_log_std", grad_log_std, (4,), obs)
        stats = self._out("stats", stats, (6 if idx is None else 7,), obs, torch.float64)
        scale = 1.0 / max(rows, 1) if scale is None else float(scale)
        _lib.check(self._lib.gaq_policy_grad_ppo_wide_dev(
            self.handle, rows, _lib.ptr(idx), src, _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(logp_old), _lib.ptr(adv), _lib.ptr(ret),
            _lib.ptr(v_old), float(clip), vclip, float(vf_coef), float(ent_coef), scale, _lib.ptr(grad), _lib.ptr(grad_value),
            _lib.ptr(grad_log_std), _lib.ptr(stats), self._stream(obs, stream)))
        return grad, grad_value, grad_log_std, stats

    @classmethod
    def from_arrays(cls, env, layers, hidden_act="tanh", out_tanh=False, log_std=None, engine="auto", value=None, obs_norm=None):
        """layers = [(W, b), ...]: the hidden layers then the 4-output layer, W [out, in] as in torch.nn.Linear; value = (w, b): the
        value head (set_value_head); obs_norm: an ObsNorm (set_obs_norm)."""
        return cls(env, [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in layers],
                   hidden_act, out_tanh, log_std, engine, value, obs_norm)

    @classmethod
    def from_torch(cls, module, env, log_std=None, engine="auto", value=None, obs_norm=None):
        """An nn.Sequential of Linear / Tanh / ReLU: Linear and activation alternate, the last Linear has 4 outputs and may be
        followed by a Tanh.  Every hidden activation must be the same.  value: an nn.Linear(W, 1) on the last hidden layer; obs_norm:
        an ObsNorm (set_obs_norm)."""
        layers, act, out_tanh = torch_layers(module)
        return cls(env, layers, act, out_tanh, log_std, engine, None if value is None else torch_value(value), obs_norm)


class _RecurrentPolicy(_DevicePolicy):
    """What GRUPolicy and LSTMPolicy share; CELL (_Cell) is what differs.  The states are [N, H] float32 tensors on the env's device,
    zero at first, registered with the library: .hidden and, for a cell with two, .cell."""

    engine = "mfma"
    CELL = None
    _REGISTER = {"hidden": "gaq_policy_set_hidden_dev", "cell": "gaq_policy_set_cell_dev"}

    encoder_widths = ()                                       # with an encoder: its layer widths; the cell then takes the last one

    def __init__(self, env, weights, head_layers, hidden_act="tanh", out_tanh=False, log_std=None, value=None, encoder=None, obs_norm=None):
        import torch
        weights = tuple(np.asarray(x, dtype=np.float32) for x in weights)
        head_layers = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in head_layers]
        if encoder is not None:
            encoder = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in encoder]
            self.encoder_widths = tuple(check_encoder_layers(encoder, env.obs_dim))
        self.cell_in = self._check_cell_in(weights, int(env.obs_dim))
        check_cell_layers(self.CELL, weights, head_layers, self.cell_in, hidden_act)
        if value is not None:
            check_value_head(int(head_layers[-1][0].shape[1]), self.engine, *value)
        self._lib = _lib.load()
        self.env_handle = _lib.handle_value(env._handle)
        self.hidden_act, self.out_tanh = hidden_act, bool(out_tanh)
        self.hidden_size = int(weights[1].shape[1])
        self.device, self.in_dim = int(env.device), int(env.obs_dim)
        self.widths = [self.hidden_size] + [int(W.shape[0]) for W, _ in head_layers[:-1]]
        d = _fill_desc(_DescRnn(), self.cell_in, self.widths, hidden_act, out_tanh=int(self.out_tanh), engine=ENGINES["mfma"],
                       cell=self.CELL.id)
        h = C.c_void_p()
        if encoder is None:
            _lib.check(self._lib.gaq_policy_create_rnn(env._handle, C.byref(d), C.byref(h)))
        else:
            de = _fill_desc(_DescRnnEnc(), self.cell_in, self.widths, hidden_act, out_tanh=int(self.out_tanh), engine=ENGINES["mfma"],
                            cell=self.CELL.id, enc_in_dim=int(env.obs_dim), enc_layers=len(encoder))
            for k, w in enumerate(self.encoder_widths):
                de.enc_width[k] = w
            _lib.check(self._lib.gaq_policy_create_rnn_enc(env._handle, C.byref(de), C.byref(h)))
            self._enc_count = int(self._lib.gaq_policy_encoder_weight_count(C.byref(de)))
        self.handle = h
        assert self._lib.gaq_policy_encoder_width(h) == (self.encoder_widths[-1] if encoder is not None else 0)
        assert self._lib.gaq_policy_engine(h) == ENGINES["mfma"] and self._lib.gaq_policy_cell(h) == self.CELL.id
        self.packed = pack_gru_weights(weights, head_layers)          # (the rule never looks at the number of gates)
        self._count = int(self._lib.gaq_policy_weight_count_rnn(C.byref(d)))
        assert self.packed.size == self._count
        _lib.check(self._lib.gaq_policy_set_weights(h, _lib.ptr(self.packed)))
        if encoder is not None:
            self.set_encoder_weights(encoder)
        dev = torch.device("cuda", env.device)
        for name in self.CELL.states:
            setattr(self, name, torch.zeros((env.num_envs, self.hidden_size), dtype=torch.float32, device=dev))
        for name in self.CELL.states:
            _lib.check(getattr(self._lib, self._REGISTER[name])(h, _lib.ptr(getattr(self, name))))
        self.set_log_std(log_std)
        self.value_head = None
        if value is not None:
            self.set_value_head(*value)
        if obs_norm is not None:
            self.set_obs_norm(obs_norm)

    def _check_cell_in(self, weights, obs_dim):
        """the inputs of the cell: the env's obs_dim, or with an encoder its last width, which W_ih must then take"""
        if not self.encoder_widths:
            return obs_dim
        E = int(self.encoder_widths[-1])
        if len(weights) == 4 and weights[0].ndim == 2 and weights[0].shape[1] != E:
            raise ValueError("W_ih takes %d inputs, the encoder's last width is %d" % (weights[0].shape[1], E))
        return E

    def _need_encoder(self):
        if not self.encoder_widths:
            raise ValueError("the policy has no encoder (with_encoder / from_torch_encoder build one)")

    def set_encoder_weights(self, layers):
        """New weights for the encoder, [(W, b), ...] as with_encoder takes them, of the same widths (synchronous)."""
        self._need_encoder()
        layers = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in layers]
        widths = tuple(check_encoder_layers(layers, self.in_dim))
        if widths != self.encoder_widths:
            raise ValueError("set_encoder_weights: encoder widths %s, the policy was built with %s" % (list(widths), list(self.encoder_widths)))
        packed = pack_encoder_weights(layers)
        assert packed.size == self._enc_count
        _lib.check(self._lib.gaq_policy_set_encoder_weights(self.handle, _lib.ptr(packed)))
        self.encoder_packed = packed

    def set_encoder_weights_dev(self, packed):
        """The encoder's weights from a packed float32 tensor [encoder_weight_count] on the policy's device, pack_encoder_weights'
        layout (gaq_policy_set_encoder_weights_dev; synchronous, no host copy).  .encoder_packed becomes None."""
        self._need_encoder()
        _lib.check_dev_f32("packed", packed, (self._enc_count,), self.device)
        _lib.check(self._lib.gaq_policy_set_encoder_weights_dev(self.handle, _lib.ptr(packed)))
        self.encoder_packed = None

    def get_encoder_weights(self):
        """The encoder's weights as they stand on the device, [(W, b), ...] in nn.Linear shapes (synchronous)."""
        self._need_encoder()
        out = np.empty(self._enc_count, dtype=np.float32)
        _lib.check(self._lib.gaq_policy_get_encoder_weights(self.handle, _lib.ptr(out)))
        return unpack_encoder_weights(out, self.in_dim, self.encoder_widths)

    def reset_hidden(self, mask=None):
        """Zero the rows of the states (.hidden; an LSTM's .cell too) whose mask entry is true ([N] bool / uint8, host or device), or
        every row for None; enqueued on the current stream."""
        import torch
        dev = self.hidden.device
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=dev, dtype=torch.uint8).contiguous()
            if m.shape != (self.hidden.shape[0],):
                raise ValueError("mask must have one entry per env (%d), got shape %s" % (self.hidden.shape[0], tuple(m.shape)))
        _lib.check(self._lib.gaq_policy_reset_hidden_dev(self.handle, _lib.ptr(m), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    def _set_states(self, *values):
        import torch
        for name, v in zip(self.CELL.states, values):
            state = getattr(self, name)
            state.copy_(torch.as_tensor(v, dtype=torch.float32).reshape(state.shape))

    @classmethod
    def from_torch(cls, cell, head, env, log_std=None, value=None):
        """cell: nn.GRUCell / nn.LSTMCell, or nn.GRU / nn.LSTM with num_layers=1 (unidirectional, no proj_size; a missing bias becomes
        zeros); head: nn.Linear(H, 4), or an MLP nn.Sequential of Linear / Tanh / ReLU as MLPPolicy.from_torch takes it (its first
        Linear takes H inputs); value: an nn.Linear(W, 1) on what the head's last Linear reads (W = H for a bare Linear(H, 4))."""
        weights = torch_cell(cls.CELL, cell)
        layers, act, out_tanh = torch_head(head)
        return cls(env, weights, layers, act, out_tanh, log_std, None if value is None else torch_value(value))

    @classmethod
    def with_encoder(cls, env, encoder, weights, head_layers, hidden_act="tanh", out_tanh=False, log_std=None, value=None, obs_norm=None):
        """The policy obs -> encoder -> cell -> head: encoder = [(W, b), ...], 1 or 2 Linear -> hidden_act layers on the observation
        (widths multiples of 16 in [16, 256]); weights = (W_ih, W_hh, b_ih, b_hh) of a cell whose W_ih takes the encoder's last width;
        the rest as the constructor takes it; obs_norm: an ObsNorm of the env, applied to what the encoder reads.  (A constructor of
        its own: the parameter lists of GRUPolicy(...), LSTMPolicy(...) and from_torch are what they always were.)"""
        self = cls.__new__(cls)
        _RecurrentPolicy.__init__(self, env, weights, head_layers, hidden_act, out_tanh, log_std, value, encoder, obs_norm)
        return self

    @classmethod
    def from_torch_encoder(cls, encoder, cell, head, env, log_std=None, value=None, obs_norm=None):
        """from_torch for the sample-factory / rl_games layout obs -> encoder -> core -> heads: encoder is nn.Sequential(Linear, act) or
        (Linear, act, Linear, act) on the observation, whose last width the cell takes; cell, head and value as from_torch takes them.
        The encoder's activation must be the head's hidden activation (a head without hidden layers takes the encoder's)."""
        weights = torch_cell(cls.CELL, cell)
        layers, act, out_tanh = torch_head(head)
        enc_layers, enc_act = torch_encoder(encoder)
        if len(layers) == 1:
            act = enc_act                                    # a bare Linear(H, 4) head reports 'tanh', which it never uses
        elif enc_act != act:
            raise ValueError("the encoder's activation (%s) must be the head's hidden activation (%s)" % (enc_act, act))
        return cls.with_encoder(env, enc_layers, weights, layers, act, out_tanh, log_std, None if value is None else torch_value(value),
                                obs_norm)

    N_OUT = 4

    def _unpack(self, packed):
        return _unpack_cell_weights(self.CELL, packed, self.cell_in, self.hidden_size, self.widths[1:])

    def _set_weights(self, weights, head_layers):
        weights = tuple(np.asarray(x, dtype=np.float32) for x in weights)
        head_layers = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in head_layers]
        check_cell_layers(self.CELL, weights, head_layers, self._check_cell_in(weights, self.in_dim), self.hidden_act)
        widths = [int(weights[1].shape[1])] + [int(W.shape[0]) for W, _ in head_layers[:-1]]
        if widths != self.widths:
            raise ValueError("set_weights: widths %s, the policy was built with %s" % (widths, self.widths))
        packed = pack_gru_weights(weights, head_layers)               # (the rule never looks at the number of gates)
        assert packed.size == self._count
        _lib.check(self._lib.gaq_policy_set_weights(self.handle, _lib.ptr(packed)))
        self.packed = packed

    # The learner's calls over stored sequences, written once over the cell's states: `states0` holds one initial state per entry of
    # CELL.states (h0; an LSTM's c0 too), `states_out` the tensors for the final ones or None.  (_out, _idx and _stream are _DeviceGrad's.)
    _STATE0 = {"hidden": "h0", "cell": "c0"}
    _STATE_OUT = {"hidden": "h_out", "cell": "c_out"}

    def _seq(self, obs, actions, done, states0):
        """the shapes of a call over stored sequences, checked -> (T, S)"""
        import torch
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[-1] != self.in_dim or obs.shape[0] < 1:
            raise ValueError("obs must be a tensor of shape [T, S, %d] with T >= 1, got %s" % (self.in_dim, tuple(getattr(obs, "shape", ()))))
        T, S = int(obs.shape[0]), int(obs.shape[1])
        _lib.check_dev_f32("obs", obs, (T, S, self.in_dim), self.device)
        if actions is not None:
            _lib.check_dev_f32("actions", actions, (T, S, 4), self.device)
        _lib.check_dev_f32("done", done, (T, S), self.device, torch.uint8)
        for name, t in zip(self.CELL.states, states0):
            _lib.check_dev_f32(self._STATE0[name], t, (S, self.hidden_size), self.device)
        return T, S

    def _evaluate_seq(self, call, obs, actions, done, states0, logp, value, mean, states_out, stream, who="evaluate_seq_dev", pad=0):
        """evaluate_seq_dev of either cell; call: its entry point; who: the public method's name, for its messages; pad: NULL pointers
        behind the initial and behind the final states (an entry point that takes an LSTM's c0 and c_out, called for a GRU)"""
        T, S = self._seq(obs, actions, done, states0)
        if self.log_std is not None and actions is not None:
            logp = self._out("logp", logp, (T, S), obs)
        elif logp is not None:
            raise ValueError("%s: logp needs log_std (set_log_std) and actions" % who)
        if self.value_head is not None:
            value = self._out("value", value, (T, S), obs)
        elif value is not None:
            raise ValueError("%s: value needs a value head (set_value_head)" % who)
        if mean is not None:
            _lib.check_dev_f32("mean", mean, (T, S, 4), self.device)
        for name, t in zip(self.CELL.states, states_out):
            if t is not None:
                _lib.check_dev_f32(self._STATE_OUT[name], t, (S, self.hidden_size), self.device)
        nulls = [None] * pad
        _lib.check(call(self.handle, T, S, _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(done), *[_lib.ptr(t) for t in states0], *nulls,
                        _lib.ptr(logp), _lib.ptr(value), _lib.ptr(mean), *[_lib.ptr(t) for t in states_out], *nulls,
                        self._stream(obs, stream)))
        return logp, value

    def _evaluate_enc_seq(self, obs, actions, done, states0, logp, value, mean, states_out, stream):
        """evaluate_enc_seq_dev of either cell: one entry point, which takes an LSTM's c0 and c_out and NULL in their place for a GRU"""
        self._need_encoder()
        return self._evaluate_seq(self._lib.gaq_policy_eval_enc_seq_dev, obs, actions, done, states0, logp, value, mean, states_out, stream,
                                  "evaluate_enc_seq_dev", 2 - len(self.CELL.states))

    def _ppo_grad(self, calls, who, idx, obs, actions, done, states0, logp_old, adv, ret, v_old, clip, vclip, vf_coef, ent_coef, scale,
                  grad, grad_value, grad_log_std, stats, stream, pad=0, grad_encoder=False):
        """the PPO gradient over sequences of either cell; calls: its contiguous (idx None) and index-gathered entry points; who: the
        public method's name, for its messages.  The encoder forms' entry points take an LSTM's c0 (pad: NULL pointers behind the
        states, for a GRU) and the encoder's gradient behind grad (grad_encoder: a tensor, or None to allocate one; False: the entry
        point has no such argument); the result then has it behind grad."""
        import torch
        S = None if idx is None else self._idx(idx)                         # (idx is checked before obs)
        T, S_src = self._seq(obs, actions, done, states0)
        S = S_src if idx is None else S
        if actions is None:
            raise ValueError("%s: actions are required" % who)
        for name, t in (("logp_old", logp_old), ("adv", adv)):
            _lib.check_dev_f32(name, t, (T, S_src), self.device)
        vclip = 0.0 if vclip is None else float(vclip)
        head = self.value_head is not None
        if head:
            _lib.check_dev_f32("ret", ret, (T, S_src), self.device)
            if v_old is not None:
                _lib.check_dev_f32("v_old", v_old, (T, S_src), self.device)
            elif vclip > 0.0:
                raise ValueError("%s: vclip > 0 needs v_old" % who)
            grad_value = self._out("grad_value", grad_value, (self.widths[-1] + 1,), obs)
        elif ret is not None or v_old is not None or grad_value is not None:
            raise ValueError("%s: ret, v_old and grad_value need a value head (set_value_head)" % who)
        grad = self._out("grad", grad, (self._count,), obs)
        enc_out = () if grad_encoder is False else (self._out("grad_encoder", grad_encoder, (self._enc_count,), obs),)
        grad_log_std = self._out("grad_log_std", grad_log_std, (4,), obs)
        stats = self._out("stats", stats, (6 if idx is None else 7,), obs, torch.float64)
        scale = 1.0 / max(T * S, 1) if scale is None else float(scale)
        call, first = (calls[0], ()) if idx is None else (calls[1], (_lib.ptr(idx), S_src))
        _lib.check(call(self.handle, T, S, *first, _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(done), *[_lib.ptr(t) for t in states0],
                        *[None] * pad, _lib.ptr(logp_old), _lib.ptr(adv), _lib.ptr(ret), _lib.ptr(v_old), float(clip), vclip, float(vf_coef),
                        float(ent_coef), scale, _lib.ptr(grad), *[_lib.ptr(t) for t in enc_out], _lib.ptr(grad_value), _lib.ptr(grad_log_std),
                        _lib.ptr(stats), self._stream(obs, stream)))
        return (grad,) + enc_out + (grad_value, grad_log_std, stats)

    def _ppo_enc_grad(self, who, idx, obs, actions, done, states0, logp_old, adv, ret, v_old, clip, vclip, vf_coef, ent_coef, scale,
                      grad, grad_encoder, grad_value, grad_log_std, stats, stream):
        """the PPO gradient over sequences of a policy with an encoder, either cell: _ppo_grad over the one pair of entry points that
        takes both cells"""
        self._need_encoder()
        calls = (self._lib.gaq_policy_grad_ppo_enc_seq_dev, self._lib.gaq_policy_grad_ppo_enc_seq_idx_dev)
        return self._ppo_grad(calls, who, idx, obs, actions, done, states0, logp_old, adv, ret, v_old, clip, vclip, vf_coef, ent_coef, scale,
                              grad, grad_value, grad_log_std, stats, stream, 2 - len(self.CELL.states), grad_encoder)

    def _unregister(self):
        for name in self.CELL.states:
            getattr(self._lib, self._REGISTER[name])(self.handle, None)


class GRUPolicy(_RecurrentPolicy, _DeviceGrad):
    """A recurrent actor evaluated on the device inside QuadrotorEnv.rollout_policy_dev: a GRU cell of H units (torch nn.GRUCell,
    gate order r, z, n) on the observation, then a head of 0 to 2 Linear -> hidden_act layers and a 4-output Linear (-> tanh), all
    fp32 on the matrix cores (gaq.h gaq_policy_desc_rnn).  Build with from_torch, or from gru = (W_ih, W_hh, b_ih, b_hh) and
    head_layers = [(W, b), ...].

    .hidden is the state: a [N, H] float32 tensor on the env's device, zero at first, registered with the library.  Each step of a
    rollout computes h <- GRU(obs, h), acts on h, steps the env, then zeroes the rows of envs that reported done; so after a call
    .hidden is the state the next action will use, and a rollout split into calls gives the same results.  Steps and resets made
    outside rollout_policy_dev (step_dev, reset_dev ...) do not touch it: call reset_hidden for the envs you reset yourself.
    Exploration is that of MLPPolicy (the same draws for the same seed, env and step)."""

    CELL = _GRU

    def __init__(self, env, gru, head_layers, hidden_act="tanh", out_tanh=False, log_std=None, value=None):
        super().__init__(env, gru, head_layers, hidden_act, out_tanh, log_std, value)

    def set_hidden(self, h):
        """Copy h ([N, H]) into .hidden."""
        self._set_states(h)

    def unpack(self, packed):
        """unpack_gru_weights for this net: a packed tensor or array (weights, a gradient) -> ((W_ih, W_hh, b_ih, b_hh), [(W, b), ...])"""
        return self._unpack(packed)

    def set_weights(self, gru, head_layers):
        """New weights for the same architecture: gru = (W_ih, W_hh, b_ih, b_hh) and head_layers as the constructor takes them
        (synchronous).  The hidden state stays as it is."""
        self._set_weights(gru, head_layers)

    def set_weights_dev(self, packed):
        """New weights from a packed float32 tensor [weight_count] on the policy's device, pack_gru_weights' layout
        (gaq_policy_set_weights_dev; synchronous, no host copy): what an optimiser that steps the packed tensor calls after each step.
        .packed becomes None."""
        self._set_weights_dev(self._lib.gaq_policy_set_weights_dev, packed)

    def evaluate_seq_dev(self, obs, actions, done, h0, logp=None, value=None, mean=None, h_out=None, stream=None):
        """The learner's forward pass over stored sequences (gaq_policy_eval_seq_dev): obs [T, S, obs_dim] (row t is the observation
        action t was computed from: of a rollout, cat(obs0[None], obs_out[:-1])), actions [T, S, 4], done [T, S] uint8 and h0 [S, H]
        (a copy of .hidden taken before the rollout call) -> logp [T, S] and value [T, S], each allocated if None where the policy has
        log_std / a value head (else left out: None is returned in its place); mean [T, S, 4] and h_out [S, H], if given, receive the
        policy's mean and the state after the last step with the rows of done[T-1] zeroed.  mean, value and h_out are bit for bit what
        rollout_policy_dev computed on the same data.  actions may be None when no logp is wanted (a deterministic policy).  One launch,
        no host synchronisation.  Returns (logp, value)."""
        return self._evaluate_seq(self._lib.gaq_policy_eval_seq_dev, obs, actions, done, (h0,), logp, value, mean, (h_out,), stream)

    def ppo_seq_grad_dev(self, obs, actions, done, h0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5,
                         ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None):
        """The truncated-BPTT gradient of the combined PPO loss over stored sequences (gaq_policy_grad_ppo_seq_dev): the loss of
        MLPPolicy.ppo_ac_grad_dev per (t, sequence), summed and times `scale` (default 1 / (T S)), with the hidden state carried from
        h0 through the T steps and restarted from 0 after every done, as the rollout does.  Nothing flows into h0.  obs, actions, done
        and h0 as evaluate_seq_dev takes them; logp_old, adv [T, S]; with a value head ret [T, S] (and v_old [T, S] for vclip > 0),
        without one ret and v_old must be None.  Returns (grad [weight_count] in pack_gru_weights' layout, grad_value [W + 1] or None
        without a value head, grad_log_std [4], stats [6] float64 as ppo_ac_grad_dev's).  Two launches, no host synchronisation,
        deterministic."""
        return self._ppo_seq_grad("ppo_seq_grad_dev", None, obs, actions, done, h0, logp_old, adv, ret, v_old, clip, vclip, vf_coef, ent_coef,
                                  scale, grad, grad_value, grad_log_std, stats, stream)

    def ppo_seq_grad_idx_dev(self, idx, obs, actions, done, h0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5,
                             ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None):
        """ppo_seq_grad_dev on the minibatch of sequences idx names, without a gathered copy (gaq_policy_grad_ppo_seq_idx_dev): idx is a
        contiguous int32 [S] tensor on the policy's device, and sequence s of the minibatch is column idx[s] of the source tensors --
        obs [T, S_src, obs_dim], actions [T, S_src, 4], done, logp_old, adv (ret, v_old) [T, S_src] and h0 [S_src, H], the rollout's own
        buffers.  With every index in range each output is bit for bit ppo_seq_grad_dev's on obs[:, idx], h0[idx] etc.; an index out of
        range contributes nothing and is counted.  scale defaults to 1 / (T S).  Returns (grad, grad_value or None, grad_log_std,
        stats [7] float64: ppo_seq_grad_dev's six, then the number of indices skipped)."""
        return self._ppo_seq_grad("ppo_seq_grad_idx_dev", idx, obs, actions, done, h0, logp_old, adv, ret, v_old, clip, vclip, vf_coef,
                                  ent_coef, scale, grad, grad_value, grad_log_std, stats, stream)

    def evaluate_seq_wide_dev(self, obs, actions, done, h0, logp=None, value=None, mean=None, h_out=None, stream=None):
        """evaluate_seq_dev for a GRU of up to 128 units (gaq_policy_eval_seq_wide_dev; gaq.h "the wide recurrent learner"): H a multiple
        of 16 up to 128, 0 to 2 head layers of width up to 64, no encoder.  The same parameters, results and contract: mean, value and
        h_out are bit for bit what rollout_policy_dev computed on the same data.  At H <= 64 every output is evaluate_seq_dev's bits.
        Returns (logp, value)."""
        return self._evaluate_seq(self._lib.gaq_policy_eval_seq_wide_dev, obs, actions, done, (h0,), logp, value, mean, (h_out,), stream,
                                  "evaluate_seq_wide_dev")

    def ppo_seq_wide_grad_dev(self, obs, actions, done, h0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5,
                              ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None, idx=None):
        """ppo_seq_grad_dev for a GRU of up to 128 units (gaq_policy_grad_ppo_seq_wide_dev; evaluate_seq_wide_dev states the family):
        the same loss, parameters and results.  With idx (a contiguous int32 [S] tensor on the policy's device) it is
        ppo_seq_grad_idx_dev: sequence s of the minibatch is column idx[s] of the [T, S_src, ...] source tensors, every output bit for
        bit the contiguous call's on the gathered inputs, an index out of range contributes nothing and is counted (stats [7] in place of
        [6]).  At H <= 64 every output is the narrow call's bits, and the narrow calls are the faster ones there.  The packed gradient
        goes to unpack, set_weights_dev and AdamDev.step as it is.  Returns (grad, grad_value or None, grad_log_std, stats).  Two
        launches, no host synchronisation, deterministic."""
        call = self._lib.gaq_policy_grad_ppo_seq_wide_dev
        calls = (lambda h, T, S, *rest: call(h, T, S, None, S, *rest), call)
        return self._ppo_grad(calls, "ppo_seq_wide_grad_dev", idx, obs, actions, done, (h0,), logp_old, adv, ret, v_old, clip, vclip,
                              vf_coef, ent_coef, scale, grad, grad_value, grad_log_std, stats, stream)

    def evaluate_enc_seq_dev(self, obs, actions, done, h0, logp=None, value=None, mean=None, h_out=None, stream=None):
        """evaluate_seq_dev for a policy with an encoder (with_encoder / from_torch_encoder; gaq_policy_eval_enc_seq_dev): the same
        parameters and results, with obs [T, S, obs_dim] the observations the ENCODER read.  Two launches: the rollout's encoder kernel
        over the T S stored rows (through the attached ObsNorm), then the cell's forward sequence kernel on the features; mean, value
        and h_out are bit for bit what rollout_policy_dev computed on the same data.  The features live in a scratch of the handle's
        that grows only when a call needs more than every call before it.  A policy without an encoder is refused (ValueError)."""
        return self._evaluate_enc_seq(obs, actions, done, (h0,), logp, value, mean, (h_out,), stream)

    def ppo_enc_seq_grad_dev(self, obs, actions, done, h0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5,
                             ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None,
                             grad_encoder=None):
        """ppo_seq_grad_dev for a policy with an encoder (gaq_policy_grad_ppo_enc_seq_dev): the same loss and parameters, with obs
        [T, S, obs_dim] the observations the ENCODER read, and the gradient flowing through the cell's input into the encoder's
        layers (an attached ObsNorm is frozen).  Split passes, not one fused kernel: the rollout's encoder kernel over the T S stored
        rows, the GRU's sequence kernel on the features, which also writes dfeat_t = W_ih^T [gate deltas], then the encoder's
        backward as a batch over the T S rows; every partial is summed in ascending order in fp64, no atomics.  Returns (grad
        [weight_count] of the cell and the head, grad_encoder [encoder weight count] in pack_encoder_weights' layout --
        unpack_encoder_weights gives nn.Linear shapes -- grad_value or None, grad_log_std [4], stats [6] float64)."""
        return self._ppo_enc_grad("ppo_enc_seq_grad_dev", None, obs, actions, done, (h0,), logp_old, adv, ret, v_old, clip, vclip, vf_coef,
                                  ent_coef, scale, grad, grad_encoder, grad_value, grad_log_std, stats, stream)

    def ppo_enc_seq_grad_idx_dev(self, idx, obs, actions, done, h0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None,
                                 vf_coef=0.5, ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None,
                                 stream=None, grad_encoder=None):
        """ppo_enc_seq_grad_dev on the minibatch of sequences idx names, without a gathered copy (gaq_policy_grad_ppo_enc_seq_idx_dev):
        ppo_seq_grad_idx_dev's contract -- sequence s is column idx[s] of the [T, S_src, ...] source tensors, every output bit for bit the
        contiguous call's on the gathered inputs, an index out of range contributes nothing and is counted in stats[6].  Only the rows
        the indices name are encoded and read.  T x S_src must not exceed 2^31 - 1.  Returns (grad, grad_encoder, grad_value or None,
        grad_log_std, stats [7] float64)."""
        return self._ppo_enc_grad("ppo_enc_seq_grad_idx_dev", idx, obs, actions, done, (h0,), logp_old, adv, ret, v_old, clip, vclip,
                                  vf_coef, ent_coef, scale, grad, grad_encoder, grad_value, grad_log_std, stats, stream)

    def _ppo_seq_grad(self, who, idx, obs, actions, done, h0, *rest):
        """ppo_seq_grad_dev (idx None) and ppo_seq_grad_idx_dev; who: the public method's name, for its messages"""
        calls = (self._lib.gaq_policy_grad_ppo_seq_dev, self._lib.gaq_policy_grad_ppo_seq_idx_dev)
        return self._ppo_grad(calls, who, idx, obs, actions, done, (h0,), *rest)


class LSTMPolicy(_RecurrentPolicy, _DeviceGrad):
    """A recurrent actor evaluated on the device inside QuadrotorEnv.rollout_policy_dev: an LSTM cell of H units (torch nn.LSTMCell,
    gate order i, f, g, o) on the observation, then the head a GRUPolicy has -- 0 to 2 Linear -> hidden_act layers and a 4-output
    Linear (-> tanh) on h' -- all fp32 on the matrix cores (gaq.h GAQ_POLICY_CELL_LSTM).  Build with from_torch, or from
    lstm = (W_ih, W_hh, b_ih, b_hh) and head_layers = [(W, b), ...].

    .hidden and .cell are the state: two [N, H] float32 tensors on the env's device, zero at first, registered with the library.
    Each step of a rollout computes (h, c) <- LSTM(obs, h, c), acts on h, steps the env, then zeroes the rows of both for envs that
    reported done; so after a call they hold the state the next action will use, a rollout split into calls gives the same bits, and
    a checkpoint is the env's state plus copies of both.  Steps and resets made outside rollout_policy_dev do not touch them: call
    reset_hidden for the envs you reset yourself.  Value head, log-probabilities, terminal values and a separate critic work as for a
    GRUPolicy; exploration is that of MLPPolicy (the same draws for the same seed, env and step)."""

    CELL = _LSTM

    def __init__(self, env, lstm, head_layers, hidden_act="tanh", out_tanh=False, log_std=None, value=None):
        super().__init__(env, lstm, head_layers, hidden_act, out_tanh, log_std, value)

    def set_hidden(self, h, c):
        """Copy h and c ([N, H] each) into .hidden and .cell."""
        self._set_states(h, c)

    def unpack(self, packed):
        """unpack_lstm_weights for this net: a packed tensor or array -> ((W_ih, W_hh, b_ih, b_hh), [(W, b), ...])"""
        return self._unpack(packed)

    def set_weights(self, lstm, head_layers):
        """New weights for the same architecture: lstm = (W_ih, W_hh, b_ih, b_hh) and head_layers as the constructor takes them
        (synchronous).  The hidden and cell states stay as they are."""
        self._set_weights(lstm, head_layers)

    def set_weights_dev(self, packed):
        """New weights from a packed float32 tensor [weight_count] on the policy's device, pack_lstm_weights' layout
        (gaq_policy_set_weights_dev; synchronous, no host copy): what an optimiser that steps the packed tensor calls after each step.
        .packed becomes None."""
        self._set_weights_dev(self._lib.gaq_policy_set_weights_dev, packed)

    def evaluate_seq_dev(self, obs, actions, done, h0, c0, logp=None, value=None, mean=None, h_out=None, c_out=None, stream=None):
        """The learner's forward pass over stored sequences (gaq_policy_eval_lstm_seq_dev): obs [T, S, obs_dim] (row t is the
        observation action t was computed from: of a rollout, cat(obs0[None], obs_out[:-1])), actions [T, S, 4], done [T, S] uint8,
        h0 and c0 [S, H] (copies of .hidden and .cell taken before the rollout call) -> logp [T, S] and value [T, S], each allocated if
        None where the policy has log_std / a value head (else left out: None is returned in its place); mean [T, S, 4], h_out and
        c_out [S, H], if given, receive the policy's mean and the two states after the last step with the rows of done[T-1] zeroed.
        mean, value, h_out and c_out are bit for bit what rollout_policy_dev computed on the same data.  actions may be None when no
        logp is wanted (a deterministic policy).  One launch, no host synchronisation.  Returns (logp, value)."""
        return self._evaluate_seq(self._lib.gaq_policy_eval_lstm_seq_dev, obs, actions, done, (h0, c0), logp, value, mean, (h_out, c_out),
                                  stream)

    def ppo_bptt_grad_dev(self, obs, actions, done, h0, c0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5,
                          ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None):
        """The truncated-BPTT gradient of the combined PPO loss over stored sequences (gaq_policy_grad_ppo_lstm_seq_dev): the loss of
        MLPPolicy.ppo_ac_grad_dev per (t, sequence), summed and times `scale` (default 1 / (T S)), with the hidden and cell states
        carried from h0 and c0 through the T steps and restarted from 0 after every done, as the rollout does.  Nothing flows into h0
        or c0.  obs, actions, done, h0 and c0 as evaluate_seq_dev takes them; logp_old, adv [T, S]; with a value head ret [T, S] (and
        v_old [T, S] for vclip > 0), without one ret and v_old must be None.  Returns (grad [weight_count] in pack_lstm_weights'
        layout -- unpack() gives nn.LSTMCell's shapes -- grad_value [W + 1] or None without a value head, grad_log_std [4], stats [6]
        float64 as ppo_ac_grad_dev's).  Two launches, no host synchronisation, deterministic."""
        return self._ppo_bptt_grad("ppo_bptt_grad_dev", None, obs, actions, done, h0, c0, logp_old, adv, ret, v_old, clip, vclip, vf_coef,
                                   ent_coef, scale, grad, grad_value, grad_log_std, stats, stream)

    def ppo_bptt_grad_idx_dev(self, idx, obs, actions, done, h0, c0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None,
                              vf_coef=0.5, ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None,
                              stream=None):
        """ppo_bptt_grad_dev on the minibatch of sequences idx names, without a gathered copy (gaq_policy_grad_ppo_lstm_seq_idx_dev): idx
        is a contiguous int32 [S] tensor on the policy's device, and sequence s of the minibatch is column idx[s] of the source tensors
        -- obs [T, S_src, obs_dim], actions [T, S_src, 4], done, logp_old, adv (ret, v_old) [T, S_src], h0 and c0 [S_src, H], the
        rollout's own buffers.  With every index in range each output is bit for bit ppo_bptt_grad_dev's on obs[:, idx], h0[idx],
        c0[idx] etc.; an index out of range contributes nothing and is counted.  scale defaults to 1 / (T S).  Returns (grad,
        grad_value or None, grad_log_std, stats [7] float64: ppo_bptt_grad_dev's six, then the number of indices skipped)."""
        return self._ppo_bptt_grad("ppo_bptt_grad_idx_dev", idx, obs, actions, done, h0, c0, logp_old, adv, ret, v_old, clip, vclip, vf_coef,
                                   ent_coef, scale, grad, grad_value, grad_log_std, stats, stream)

    def evaluate_enc_seq_dev(self, obs, actions, done, h0, c0, logp=None, value=None, mean=None, h_out=None, c_out=None, stream=None):
        """evaluate_seq_dev for a policy with an encoder (with_encoder / from_torch_encoder; gaq_policy_eval_enc_seq_dev): the same
        parameters and results, with obs [T, S, obs_dim] the observations the ENCODER read.  Two launches: the rollout's encoder kernel
        over the T S stored rows (through the attached ObsNorm), then the cell's forward sequence kernel on the features; mean, value,
        h_out and c_out are bit for bit what rollout_policy_dev computed on the same data.  The features live in a scratch of the
        handle's that grows only when a call needs more than every call before it.  A policy without an encoder is refused
        (ValueError)."""
        return self._evaluate_enc_seq(obs, actions, done, (h0, c0), logp, value, mean, (h_out, c_out), stream)

    def ppo_enc_seq_grad_dev(self, obs, actions, done, h0, c0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5,
                             ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None,
                             grad_encoder=None):
        """ppo_bptt_grad_dev for a policy with an encoder (gaq_policy_grad_ppo_enc_seq_dev): the same loss and parameters, with obs
        [T, S, obs_dim] the observations the ENCODER read, and the gradient flowing through the cell's input into the encoder's
        layers (an attached ObsNorm is frozen).  Split passes, not one fused kernel: the rollout's encoder kernel over the T S stored
        rows, the LSTM's sequence kernel on the features, which also writes dfeat_t = W_ih^T [gate deltas], then the encoder's
        backward as a batch over the T S rows; every partial is summed in ascending order in fp64, no atomics.  Returns (grad
        [weight_count] of the cell and the head, grad_encoder [encoder weight count] in pack_encoder_weights' layout --
        unpack_encoder_weights gives nn.Linear shapes -- grad_value or None, grad_log_std [4], stats [6] float64)."""
        return self._ppo_enc_grad("ppo_enc_seq_grad_dev", None, obs, actions, done, (h0, c0), logp_old, adv, ret, v_old, clip, vclip, vf_coef,
                                  ent_coef, scale, grad, grad_encoder, grad_value, grad_log_std, stats, stream)

    def ppo_enc_seq_grad_idx_dev(self, idx, obs, actions, done, h0, c0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None,
                                 vf_coef=0.5, ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None,
                                 stream=None, grad_encoder=None):
        """ppo_enc_seq_grad_dev on the minibatch of sequences idx names, without a gathered copy (gaq_policy_grad_ppo_enc_seq_idx_dev):
        ppo_bptt_grad_idx_dev's contract -- sequence s is column idx[s] of the [T, S_src, ...] source tensors, every output bit for bit the
        contiguous call's on the gathered inputs, an index out of range contributes nothing and is counted in stats[6].  Only the rows
        the indices name are encoded and read.  T x S_src must not exceed 2^31 - 1.  Returns (grad, grad_encoder, grad_value or None,
        grad_log_std, stats [7] float64)."""
        return self._ppo_enc_grad("ppo_enc_seq_grad_idx_dev", idx, obs, actions, done, (h0, c0), logp_old, adv, ret, v_old, clip, vclip,
                                  vf_coef, ent_coef, scale, grad, grad_encoder, grad_value, grad_log_std, stats, stream)

    def _ppo_bptt_grad(self, who, idx, obs, actions, done, h0, c0, *rest):
        """ppo_bptt_grad_dev (idx None) and ppo_bptt_grad_idx_dev; who: the public method's name, for its messages"""
        calls = (self._lib.gaq_policy_grad_ppo_lstm_seq_dev, self._lib.gaq_policy_grad_ppo_lstm_seq_idx_dev)
        return self._ppo_grad(calls, who, idx, obs, actions, done, (h0, c0), *rest)


class _CriticDesc(C.Structure):
    """gaq_critic_desc"""
    _fields_ = [("struct_size", C.c_uint32), ("in_dim", C.c_int32), ("n_hidden", C.c_int32), ("width", C.c_int32 * 3),
                ("hidden_act", C.c_int32)]


def check_critic_layers(layers, in_dim, hidden_act):
    """ValueError unless `layers` is a critic the device can run: obs_dim inputs, 1-3 hidden layers of widths 16k <= 256, 1 output."""
    _check_mlp_layers(layers, in_dim, hidden_act, "critic", "the critic's output layer", 1, _MAX_WIDTH["mfma"])


def pack_critic_weights(layers):
    """[(W [out, in], b [out]), ..., (w [1, in], b [1])] -> the flat fp32 layout of gaq.h gaq_critic: the hidden layers as pack_weights
    packs them, then the 1-output layer as a value head is laid out: w[in], then the bias.  (pack_weights' output-layer rule W.T gives
    exactly that for one output.)"""
    return pack_weights(layers)


class MLPCritic(_DeviceNet, _DeviceGrad):
    """A value network of its own, evaluated on the device: obs (obs_dim) -> [Linear -> act] x n_hidden -> Linear -> 1, fp32 on the
    matrix cores, act tanh or relu for every hidden layer, 1 to 3 hidden layers of widths that are multiples of 16 in [16, 256]
    (gaq.h gaq_critic).  Build with from_torch / from_arrays.  QuadrotorEnv.rollout_policy_dev(..., critic=) takes `values` and
    `term_values` from it; values_dev evaluates it on any observations.  It is feed-forward: with a GRUPolicy too it sees the
    observation only.  V of a row is bit for bit what an "mfma" MLPPolicy with the same hidden layers and the output layer as its value
    head computes."""

    def __init__(self, env, layers, hidden_act="tanh"):
        layers = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in layers]
        check_critic_layers(layers, env.obs_dim, hidden_act)
        self._lib = _lib.load()
        self.env_handle = _lib.handle_value(env._handle)
        self.device, self.in_dim = int(env.device), int(env.obs_dim)
        self.hidden_act = hidden_act
        self.widths = [int(W.shape[0]) for W, _ in layers[:-1]]
        d = _fill_desc(_CriticDesc(), self.in_dim, self.widths, hidden_act)
        h = C.c_void_p()
        _lib.check(self._lib.gaq_critic_create(env._handle, C.byref(d), C.byref(h)))
        self.handle = h
        self._count = int(self._lib.gaq_critic_weight_count(C.byref(d)))
        self.packed = None
        self.set_weights(layers)

    def set_weights(self, layers):
        """New weights for the same architecture: layers = [(W, b), ...] as from_arrays takes them (synchronous)."""
        layers = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in layers]
        check_critic_layers(layers, self.in_dim, self.hidden_act)
        widths = [int(W.shape[0]) for W, _ in layers[:-1]]
        if widths != self.widths:
            raise ValueError("set_weights: hidden widths %s, the critic was built with %s" % (widths, self.widths))
        packed = pack_critic_weights(layers)
        assert packed.size == self._count
        _lib.check(self._lib.gaq_critic_set_weights(self.handle, _lib.ptr(packed)))
        self.packed = packed

    N_OUT = 1
    _DESTROY, _SET_OBS_NORM, _GET_WEIGHTS = "gaq_critic_destroy", "gaq_critic_set_obs_norm", "gaq_critic_get_weights"

    def set_weights_dev(self, packed):
        """New weights from a packed float32 tensor [weight_count] on the critic's device (gaq_critic_set_weights_dev; synchronous, no
        host copy).  .packed becomes None."""
        self._set_weights_dev(self._lib.gaq_critic_set_weights_dev, packed)

    def backward_dev(self, obs, dout, scale=1.0, grad=None, stream=None):
        """grad [weight_count] (packed layout; allocated if None) = sum over rows of scale * dout * dV / d theta for a caller-given
        dout [...] (gaq_critic_backward_dev; widths <= 128).  Returns grad."""
        lead, rows = self._rows(obs)
        _lib.check_dev_f32("dout", dout, lead, self.device)
        grad = self._out("grad", grad, (self._count,), obs)
        _lib.check(self._lib.gaq_critic_backward_dev(self.handle, rows, _lib.ptr(obs), _lib.ptr(dout), float(scale), _lib.ptr(grad),
                                                     self._stream(obs, stream)))
        return grad

    def mse_grad_dev(self, obs, target, scale=None, grad=None, stats=None, stream=None):
        """The gradient of L = (V - target)^2 / 2 summed over the rows and times `scale` (default 1 / rows) -> grad [weight_count];
        stats [2] float64 = sum of L (unscaled), rows (gaq_critic_grad_mse_dev).  Returns (grad, stats)."""
        return self._mse_grad(None, obs, target, scale, grad, stats, stream)

    def mse_grad_idx_dev(self, idx, obs, target, scale=None, grad=None, stats=None, stream=None):
        """mse_grad_dev on the minibatch idx names, without a gathered copy (gaq_critic_grad_mse_idx_dev): idx is a contiguous int32
        [rows] tensor on the critic's device, row j of the minibatch is row idx[j] of obs [..., obs_dim] and target [...] (a leading
        [T, N] shape is flattened: idx indexes t * N + n).  With every index in range each output is bit for bit mse_grad_dev's on the
        gathered rows; an index out of range contributes nothing and is counted.  scale defaults to 1 / rows.  Returns (grad,
        stats [3] float64: mse_grad_dev's two, then the number of indices skipped)."""
        return self._mse_grad(idx, obs, target, scale, grad, stats, stream)

    def _mse_grad(self, idx, obs, target, scale, grad, stats, stream):
        """mse_grad_dev (idx None) and mse_grad_idx_dev"""
        import torch
        lead, rows, src = self._rows_idx(idx, obs)
        _lib.check_dev_f32("target", target, lead, self.device)
        grad = self._out("grad", grad, (self._count,), obs)
        stats = self._out("stats", stats, (2 if idx is None else 3,), obs, torch.float64)
        scale = 1.0 / max(rows, 1) if scale is None else float(scale)
        call, first = (self._lib.gaq_critic_grad_mse_dev, ()) if idx is None else (self._lib.gaq_critic_grad_mse_idx_dev, (_lib.ptr(idx), src))
        _lib.check(call(self.handle, rows, *first, _lib.ptr(obs), _lib.ptr(target), scale, _lib.ptr(grad), _lib.ptr(stats),
                        self._stream(obs, stream)))
        return grad, stats

    def mse_wide_grad_dev(self, obs, target, *, idx=None, scale=None, grad=None, stats=None, stream=None):
        """mse_grad_dev -- with idx (a contiguous int32 [rows] tensor: the minibatch's source rows) mse_grad_idx_dev -- for hidden widths
        up to 256 (gaq_critic_grad_mse_wide_dev; gaq.h "the wide learner"): a critic whose in_dim rounded up to 16 + hidden widths sum
        to at most 560 (18-256-256 passes, three layers of 256 do not).  On widths <= 128 every output is the narrow call's bits, and
        the narrow call is the one to use there (it was measured 5 to 11 % faster on 18-128-128).
        Returns (grad, stats [2] float64, [3] with idx)."""
        import torch
        lead, rows, src = self._rows_idx(idx, obs)
        _lib.check_dev_f32("target", target, lead, self.device)
        grad = self._out("grad", grad, (self._count,), obs)
        stats = self._out("stats", stats, (2 if idx is None else 3,), obs, torch.float64)
        scale = 1.0 / max(rows, 1) if scale is None else float(scale)
        _lib.check(self._lib.gaq_critic_grad_mse_wide_dev(self.handle, rows, _lib.ptr(idx), src, _lib.ptr(obs), _lib.ptr(target), scale,
                                                          _lib.ptr(grad), _lib.ptr(stats), self._stream(obs, stream)))
        return grad, stats

    @classmethod
    def from_arrays(cls, env, layers, hidden_act="tanh"):
        """layers = [(W, b), ...]: the hidden layers then the 1-output layer, W [out, in] as in torch.nn.Linear."""
        return cls(env, layers, hidden_act)

    @classmethod
    def from_torch(cls, module, env):
        """An nn.Sequential of Linear / Tanh / ReLU: Linear and activation alternate, the last Linear has 1 output and nothing follows
        it.  Every hidden activation must be the same."""
        layers, act, out_tanh = torch_layers(module)
        if out_tanh:
            raise ValueError("a critic's output is not squashed: the module must end with Linear(W, 1), not Tanh")
        return cls(env, layers, act)

    def values_dev(self, obs, out=None, stream=None):
        """V of obs [..., obs_dim] (contiguous float32 on the env's device) -> `out` [...] (allocated if None), one launch on the
        current torch stream (or `stream`), no host synchronisation (gaq_critic_eval_dev).  Returns out."""
        import torch
        if not isinstance(obs, torch.Tensor) or obs.dim() < 1 or obs.shape[-1] != self.in_dim or obs.dtype != torch.float32 \
                or not obs.is_contiguous():
            raise ValueError("obs must be a contiguous float32 tensor of shape [..., %d], got %s %s"
                             % (self.in_dim, getattr(obs, "dtype", type(obs).__name__), tuple(getattr(obs, "shape", ()))))
        _lib.check_dev_f32("obs", obs, obs.shape, self.device, whose="the critic's")     # (the device: the rest is checked above)
        out = self._out("out", out, tuple(obs.shape[:-1]), obs)
        _lib.check(self._lib.gaq_critic_eval_dev(self.handle, int(out.numel()), _lib.ptr(obs), _lib.ptr(out), self._stream(obs, stream)))
        return out


def perm_dev(n, seed, epoch=0, epoch_dev=None, out=None, device=None, stream=None):
    """A pseudo-random permutation of 0 .. n-1 as an int32 [n] tensor on the device, a pure function of (n, seed, epoch), in one launch
    with no host synchronisation (gaq_perm_dev; gaq.h states the formula).  perm[k * mb:(k + 1) * mb] are an epoch's minibatches for
    the *_idx_dev gradient calls.  epoch_dev: a one-element torch.int64 tensor on the device whose value the kernel reads when it runs,
    instead of `epoch` -- inside a captured graph, epoch_dev.add_(1) after the minibatches makes every replay draw a new permutation.
    out: an int32 [n] tensor to fill (allocated if None); device: an index or torch.device, by default that of out, of epoch_dev, or
    the current one."""
    import torch
    n = int(n)
    if n < 1 or n > 2 ** 31 - 1:
        raise ValueError("perm_dev: n must be in [1, 2^31 - 1], got %d" % n)
    if device is None:
        like = out if out is not None else epoch_dev
        device = like.device if isinstance(like, torch.Tensor) and like.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    index = torch.cuda.current_device() if device.index is None else device.index
    if epoch_dev is not None:
        _lib.check_dev_f32("epoch_dev", epoch_dev, (1,), index, torch.int64, whose="perm_dev's")
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=torch.device("cuda", index))
    else:
        _lib.check_dev_f32("out", out, (n,), index, torch.int32, whose="perm_dev's")
    st = C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream if stream is None else stream)
    mask = 2 ** 64 - 1
    _lib.check(_lib.load().gaq_perm_dev(n, int(seed) & mask, int(epoch) & mask, _lib.ptr(epoch_dev), _lib.ptr(out), st))
    return out


class _OptimDesc(C.Structure):
    """gaq_optim_desc"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("weight_decay", C.c_double), ("max_grad_norm", C.c_double)]


OPTIM_STEP_LOG_STD = 1          # gaq.h GAQ_OPTIM_STEP_LOG_STD


def optim_groups(weight_count, value_width=None, log_std=False):
    """The parameter groups of an AdamDev and their place in its state: ([(name, offset, floats), ...], total floats) for a handle of
    `weight_count` packed floats, a value head on a last layer of `value_width` units (None: no head) and, with log_std, the 4
    exploration parameters -- "weights", then "value_head", then "log_std", concatenated (gaq.h gaq_optim_state_count)."""
    groups, n = [("weights", 0, int(weight_count))], int(weight_count)
    if value_width is not None:
        groups.append(("value_head", n, int(value_width) + 1))
        n += int(value_width) + 1
    if log_std:
        groups.append(("log_std", n, 4))
        n += 4
    return groups, n


def optim_desc(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, learn_log_std=True):
    """AdamDev's hyper-parameters as the gaq_optim_desc the library takes (max_grad_norm None: 0, no clipping)"""
    d = _OptimDesc()
    d.struct_size, d.flags = C.sizeof(d), OPTIM_STEP_LOG_STD if learn_log_std else 0
    d.lr, d.beta1, d.beta2, d.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
    d.weight_decay, d.max_grad_norm = float(weight_decay), 0.0 if max_grad_norm is None else float(max_grad_norm)
    return d


class AdamDev(_Handle):
    """Adam / AdamW on the device for one policy or critic (gaq.h "the optimiser on the device"): step() takes the gradient tensors as
    ppo_grad_dev / ppo_ac_grad_dev / ppo_seq_grad_dev / mse_grad_dev write them, clips them by their global norm (max_grad_norm;
    torch's clip_grad_norm_ rule) and steps the handle's own weights in place, where its rollout and gradient kernels read them: two
    launches, no host synchronisation, capturable in a graph (the step count and lr live on the device: a replay advances them).
    weight_decay is decoupled (AdamW's) and never applies to log_std.  Any MLPPolicy but a "bf16" one, a GRUPolicy, an LSTMPolicy or
    an MLPCritic, with weights set.

    The groups are fixed here: the packed weights, the value head if the policy has one now, and log_std if learn_log_std and the
    policy explores (.groups names them; adding or removing the value head later makes step() fail).  A gradient norm that is not
    finite skips the step: weights, moments and step count keep their bits and .skipped goes up.

    log_std: the handle's kernels take log_std from the host, so the optimiser steps a copy of its own on the device and
    sync_log_std() hands it to the policy (policy.log_std included).  Until then the policy's kernels use the OLD log_std.  It is the
    one synchronous call of a minibatch, step() makes it unless sync_log_std=False, and it cannot be captured in a graph.
    A CAPTURED gradient call or rollout keeps the log_std it was captured with (it is a kernel argument): capture gradient call +
    step with learn_log_std=False, or capture again after every sync_log_std().  The optimiser owns the log_std it steps: after a
    policy.set_log_std(...) with other values, or None, step() and sync_log_std() raise GaqError until the policy's log_std is the
    optimiser's again.
    All of that paragraph is HOST mode.  After policy.log_std_to_device() (before the AdamDev is created) log_std is device state
    like the weights: the optimiser steps the policy's table in place and publishes exp(log_std) and exp(-log_std) beside it, the
    next launch -- captured or not -- reads them, sync_log_std() is a no-op and step() never waits.  A graph of gradient call + step
    then learns log_std; policy.set_log_std(...) between steps is simply what the next step steps.  Switching the policy's mode
    under a living optimiser makes step() raise.

    The optimiser keeps a reference to the policy or critic, as a net keeps its ObsNorm; close the optimiser before the handle it
    steps (a step on a closed handle raises).  After a step .packed of the handle is None: get_weights() reads the weights back."""

    _DESTROY = "gaq_optim_destroy"

    def __init__(self, handle, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, learn_log_std=True):
        if not isinstance(handle, _DeviceNet) or getattr(handle, "handle", None) is None:
            raise ValueError("AdamDev steps an open MLPPolicy, GRUPolicy, LSTMPolicy or MLPCritic, got %s" % type(handle).__name__)
        self._lib = _lib.load()
        self.net = handle
        self.device = handle.device
        d = optim_desc(lr, betas, eps, weight_decay, max_grad_norm, learn_log_std)
        create = self._lib.gaq_optim_create_policy if isinstance(handle, _DevicePolicy) else self._lib.gaq_optim_create_critic
        h = C.c_void_p()
        _lib.check(create(handle.handle, C.byref(d), C.byref(h)))
        self.handle = h
        self.lr = float(lr)
        is_policy = isinstance(handle, _DevicePolicy)
        self.steps_value_head = is_policy and handle.value_head is not None
        self.steps_log_std = bool(learn_log_std) and is_policy and handle.log_std is not None
        self.groups, self._count = optim_groups(handle._count, handle.widths[-1] if self.steps_value_head else None, self.steps_log_std)
        assert int(self._lib.gaq_optim_state_count(h)) == self._count

    def _open(self):
        if getattr(self, "handle", None) is None:
            raise ValueError("the AdamDev is closed")
        if self.net.handle is None:
            raise ValueError("the %s this AdamDev steps is closed" % type(self.net).__name__)
        return self.handle

    def _stream(self, stream):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)

    def step(self, grad, grad_value=None, grad_log_std=None, stats=None, stream=None, sync_log_std=True):
        """One step on grad [weight_count], grad_value [W + 1] (needed exactly when the optimiser steps a value head) and
        grad_log_std [4] (needed when it steps log_std, ignored otherwise): float32 tensors on the handle's device, as the gradient
        calls return them.  stats, if given, is a float64 tensor [4] that receives the norm before clipping, the coef applied, the
        step count after the call and 1 for a skipped step.  Enqueued on the current torch stream (or `stream`); with sync_log_std
        (and a stepped log_std) it then waits for that stream and hands the new log_std to the policy.  Returns stats."""
        import torch
        h = self._open()
        _lib.check_dev_f32("grad", grad, (self.net._count,), self.device)
        if grad_value is not None:
            _lib.check_dev_f32("grad_value", grad_value, (self.net.widths[-1] + 1,), self.device)
        if self.steps_log_std:
            _lib.check_dev_f32("grad_log_std", grad_log_std, (4,), self.device)
        if stats is not None:
            _lib.check_dev_f32("stats", stats, (4,), self.device, torch.float64)
        st = self._stream(stream)
        _lib.check(self._lib.gaq_optim_step_dev(h, _lib.ptr(grad), _lib.ptr(grad_value),
                                                _lib.ptr(grad_log_std) if self.steps_log_std else None, _lib.ptr(stats), st))
        self.net.packed = None                                # the weights live in the handle now
        if self.steps_value_head:
            self.net.value_head = True
        if sync_log_std and self.steps_log_std:
            self.sync_log_std(st)
        return stats

    def set_lr(self, lr, stream=None):
        """A new learning rate for the steps enqueued after it (an enqueued write: no synchronisation, and a captured step sees it
        at its next replay)."""
        _lib.check(self._lib.gaq_optim_set_lr_dev(self._open(), float(lr), self._stream(stream)))
        self.lr = float(lr)

    def sync_log_std(self, stream=None):
        """Wait for the stream, read the stepped log_std and hand it to the policy (set_explore; policy.log_std follows).  Nothing
        to do when the optimiser steps no log_std."""
        h = self._open()
        if not self.steps_log_std or self.net.log_std_dev is not None:   # (device mode: the kernels read what the step wrote)
            return
        _lib.check(self._lib.gaq_optim_sync_log_std(h, stream if isinstance(stream, C.c_void_p) else self._stream(stream)))
        ls = np.empty(4, dtype=np.float32)
        _lib.check(self._lib.gaq_optim_get_log_std(h, _lib.ptr(ls)))
        self.net.log_std = ls

    def _state(self):
        step, skipped = C.c_uint64(), C.c_uint64()
        m, v = np.empty(self._count, np.float32), np.empty(self._count, np.float32)
        _lib.check(self._lib.gaq_optim_get_state(self._open(), C.byref(step), C.byref(skipped), _lib.ptr(m), _lib.ptr(v)))
        return int(step.value), int(skipped.value), m, v

    @property
    def step_count(self):
        return self._state()[0]

    @property
    def skipped(self):
        return self._state()[1]

    def state_dict(self):
        """{"step", "skipped", "lr", "m", "v"}: the counters, the learning rate and the two moments as float32 arrays
        [state count], the groups concatenated as .groups says (synchronous).  The weights are the handle's (get_weights), log_std the
        policy's (after sync_log_std)."""
        step, skipped, m, v = self._state()
        return {"step": step, "skipped": skipped, "lr": self.lr, "m": m, "v": v}

    def load_state_dict(self, state):
        """Restore a state_dict (synchronous).  ValueError for moments of another size: a state saved for other groups."""
        m = np.ascontiguousarray(np.asarray(state["m"], dtype=np.float32).reshape(-1))
        v = np.ascontiguousarray(np.asarray(state["v"], dtype=np.float32).reshape(-1))
        if m.size != self._count or v.size != self._count:
            raise ValueError("the state holds %d and %d floats, this optimiser's groups %s hold %d"
                             % (m.size, v.size, [g[0] for g in self.groups], self._count))
        step, skipped = C.c_uint64(int(state["step"])), C.c_uint64(int(state.get("skipped", 0)))
        _lib.check(self._lib.gaq_optim_set_state(self._open(), C.byref(step), C.byref(skipped), _lib.ptr(m), _lib.ptr(v)))
        if "lr" in state:
            self.set_lr(state["lr"])

    def close(self):
        super().close()
        self.net = None


class AdamEncDev(AdamDev):
    """AdamDev for a GRUPolicy or LSTMPolicy WITH an encoder (with_encoder / from_torch_encoder; gaq_optim_create_policy_enc), which
    AdamDev refuses: the encoder's block is a fourth group, "encoder", placed after log_std -- .groups names all of them, and the
    moments of state_dict / load_state_dict are the groups concatenated in that order.  The gradient norm and the clip are joint over
    all groups, weight_decay applies to the encoder as to the weights, and the block is stepped in place where the rollout's encoder
    kernel and the gradient calls read it: rollout_policy_dev -> ... -> ppo_enc_seq_grad[_idx]_dev -> step() closes on the device
    and can be captured in a graph (with policy.log_std_to_device() before the optimiser is made, log_std is learnt inside it).
    Everything else -- hyper-parameters, host and device mode of log_std, skipped steps, set_lr -- is AdamDev's.  After a step
    .encoder_packed of the policy is None: get_encoder_weights() reads the block back."""

    def __init__(self, handle, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, learn_log_std=True):
        if not isinstance(handle, _RecurrentPolicy) or getattr(handle, "handle", None) is None or not handle.encoder_widths:
            raise ValueError("AdamEncDev steps an open GRUPolicy or LSTMPolicy with an encoder (AdamDev takes the others), got %s"
                             % type(handle).__name__)
        self._lib = _lib.load()
        self.net = handle
        self.device = handle.device
        d = optim_desc(lr, betas, eps, weight_decay, max_grad_norm, learn_log_std)
        h = C.c_void_p()
        _lib.check(self._lib.gaq_optim_create_policy_enc(handle.handle, C.byref(d), C.byref(h)))
        self.handle = h
        self.lr = float(lr)
        self.steps_value_head = handle.value_head is not None
        self.steps_log_std = bool(learn_log_std) and handle.log_std is not None
        groups, n = optim_groups(handle._count, handle.widths[-1] if self.steps_value_head else None, self.steps_log_std)
        self.groups, self._count = groups + [("encoder", n, handle._enc_count)], n + handle._enc_count
        assert int(self._lib.gaq_optim_state_count(h)) == self._count

    def step(self, grad, grad_encoder, grad_value=None, grad_log_std=None, stats=None, stream=None, sync_log_std=True):
        """AdamDev.step with grad_encoder [encoder weight count], the second result of ppo_enc_seq_grad_dev /
        ppo_enc_seq_grad_idx_dev, behind grad.  Returns stats."""
        import torch
        h = self._open()
        _lib.check_dev_f32("grad", grad, (self.net._count,), self.device)
        _lib.check_dev_f32("grad_encoder", grad_encoder, (self.net._enc_count,), self.device)
        if grad_value is not None:
            _lib.check_dev_f32("grad_value", grad_value, (self.net.widths[-1] + 1,), self.device)
        if self.steps_log_std:
            _lib.check_dev_f32("grad_log_std", grad_log_std, (4,), self.device)
        if stats is not None:
            _lib.check_dev_f32("stats", stats, (4,), self.device, torch.float64)
        st = self._stream(stream)
        _lib.check(self._lib.gaq_optim_step_enc_dev(h, _lib.ptr(grad), _lib.ptr(grad_encoder), _lib.ptr(grad_value),
                                                    _lib.ptr(grad_log_std) if self.steps_log_std else None, _lib.ptr(stats), st))
        self.net.packed = None                                # the weights and the encoder's block live in the handle now
        self.net.encoder_packed = None
        if self.steps_value_head:
            self.net.value_head = True
        if sync_log_std and self.steps_log_std:
            self.sync_log_std(st)
        return stats
