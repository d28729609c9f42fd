"""Helpers of the encoder tests (gaq.h gaq_policy_desc_rnn_enc: obs -> MLP encoder -> GRU / LSTM cell -> head): random encoders, the
description, and an fp64 NumPy reference of a closed-loop rollout fed the device's recorded observations, dones and terminal rows --
the encoder in front of the cell and head of tests/gru_util.py and tests/lstm_util.py, whose helpers it reuses, with their rollout
semantics (a done after step t -> zero state at step t + 1).  The encoder, the cell and the head are parameters, so the yardstick of the
GPU tests runs the same rollout with torch fp32 on the CPU in their place (yardstick_parts)."""
import ctypes as C

import numpy as np

from tests.gru_util import gru_step64, head64
from tests.lstm_util import lstm_step64, torch_head32, value64

CELLS = {"gru": 1, "lstm": 3}                    # gaq.h GAQ_POLICY_CELL_*
GATES = {"gru": 3, "lstm": 4}


def _encoder(D, widths, seed=0, scale=None):
    """1 or 2 layers on D inputs, weights ~ 1 / sqrt(fan_in) so that no unit saturates; `scale` [D] is folded into the first layer"""
    rng = np.random.RandomState(seed)
    dims = [D] + list(widths)
    layers = [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
              for k in range(len(widths))]
    if scale is not None:
        W, b = layers[0]
        layers[0] = ((W / np.asarray(scale)[None, :]).astype(np.float32), b)
    return layers


def _cell(cell, H, I, seed=0, scale=None):
    """(W_ih [GH, I], W_hh [GH, H], b_ih, b_hh) of a GRU / LSTM cell, weights ~ 1 / sqrt(I + H) by default"""
    rng = np.random.RandomState(seed)
    G = GATES[cell]
    s = 1.0 / np.sqrt(I + H) if scale is None else scale
    return tuple((s * rng.randn(*shape)).astype(np.float32) for shape in ((G * H, I), (G * H, H), (G * H,), (G * H,)))


def _desc_enc(widths, enc_widths, enc_in=18, cell=1, engine=1, in_dim=None, act=0):
    """gaq_policy_desc_rnn_enc of a cell of widths[0] units (+ head widths) behind an encoder; in_dim defaults to the last encoder width"""
    from gym_art_amd.policy import _DescRnnEnc
    d = _DescRnnEnc()
    d.struct_size = C.sizeof(_DescRnnEnc)
    d.in_dim = enc_widths[-1] if in_dim is None else in_dim
    d.n_hidden, d.hidden_act = len(widths), act
    for k, w in enumerate(widths[:3]):
        d.width[k] = w
    d.engine, d.cell = engine, cell
    d.enc_in_dim, d.enc_layers = enc_in, len(enc_widths)
    for k, w in enumerate(enc_widths[:2]):
        d.enc_width[k] = w
    return d


def norm64(norm, x):
    """clamp((x - mean) * inv_std, +-clip) in float64; norm = (mean [D], inv_std [D], clip) or None"""
    if norm is None:
        return x
    mean, inv_std, clip = norm
    return np.clip((x - np.asarray(mean, np.float64)) * np.asarray(inv_std, np.float64), -clip, clip)


def encoder64(enc, act, x, norm=None):
    """the features [N, E] of observations x [N, D] in float64"""
    y = norm64(norm, np.asarray(x, np.float64))
    for W, b in enc:
        y = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        y = np.tanh(y) if act == "tanh" else np.maximum(y, 0.0)
    return y


def cell_step64(cell, weights, x, state):
    """one step of the cell in float64: state = (h,) or (h, c) -> the new state, h' first"""
    if cell == "gru":
        return (gru_step64(weights, x, state[0]),)
    return lstm_step64(weights, x, *state)


def yardstick_parts(cell, enc, weights, layers, act, out_tanh, value=None, norm=None):
    """(encoder, step, head) as torch fp32 computes them on the CPU -- nn.functional.linear, nn.GRUCell / nn.LSTMCell, the head of
    tests/lstm_util.py torch_head32 -- on float64 arrays, the state rounded to fp32 each step as a torch fp32 rollout keeps it"""
    import torch
    F = torch.nn.functional
    tenc = [(torch.from_numpy(np.asarray(W, np.float32)), torch.from_numpy(np.asarray(b, np.float32))) for W, b in enc]
    W_ih, W_hh = weights[0], weights[1]
    mod = (torch.nn.GRUCell if cell == "gru" else torch.nn.LSTMCell)(W_ih.shape[1], W_hh.shape[1])
    with torch.no_grad():
        for p, a in zip((mod.weight_ih, mod.weight_hh, mod.bias_ih, mod.bias_hh), weights):
            p.copy_(torch.from_numpy(np.asarray(a, np.float32)))

    def encoder(x):
        y = torch.from_numpy(np.asarray(x, np.float32))
        if norm is not None:
            mean, inv_std, clip = norm
            y = torch.clamp((y - torch.from_numpy(np.asarray(mean, np.float32))) * torch.from_numpy(np.asarray(inv_std, np.float32)),
                            -float(clip), float(clip))
        for W, b in tenc:
            y = F.linear(y, W, b)
            y = torch.tanh(y) if act == "tanh" else torch.relu(y)
        return y.numpy().astype(np.float64)

    def step(x, state):
        with torch.no_grad():
            ts = tuple(torch.from_numpy(np.asarray(s, np.float32)) for s in state)
            out = mod(torch.from_numpy(np.asarray(x, np.float32)), ts[0] if cell == "gru" else ts)
        out = (out,) if cell == "gru" else out
        return tuple(o.numpy().astype(np.float64) for o in out)
    return encoder, step, torch_head32(layers, act, out_tanh, value)


def reference_rollout(cell, enc, weights, layers, act, out_tanh, obs0, obs, done, state0, value=None, term_rows=None, norm=None, parts=None):
    """A closed-loop rollout of obs -> encoder -> cell -> head from state0 = (h0,) or (h0, c0), with obs_{t-1} = obs0 for t = 0 and
    obs[t - 1] after, and the state zeroed in the rows of done[t] after step t.  Returns a dict: "a" the deterministic actions
    [T, N, 4], "h" (and "c") the final states [N, H]; with `value` "v" [T + 1, N] (row T: V from cell(enc(obs[T - 1]), the masked
    state), which is not kept) and, with `term_rows` [T, N, D] (read where done is set), "tv" [T, N]: V from cell(enc(terminal row),
    the state action t used) where done[t], 0 elsewhere.  `norm` = (mean, inv_std, clip) normalises what the ENCODER reads.
    `parts` = (encoder, step, head) replaces the fp64 pieces (yardstick_parts)."""
    obs0, obs, done = (np.asarray(a) for a in (obs0, obs, done))
    state = tuple(np.asarray(s, np.float64) for s in state0)
    if parts is None:
        enc_fn = lambda x: encoder64(enc, act, x, norm)
        step = lambda x, s: cell_step64(cell, weights, x, s)
        act_fn, v_fn = (lambda y: head64(layers, act, out_tanh, y)), (lambda y: value64(layers, act, value, y))
    else:
        enc_fn, step, (act_fn, v_fn) = parts
    T = obs.shape[0]
    acts, vals, tvs = [], [], []
    for t in range(T + 1):
        new = step(enc_fn(obs0 if t == 0 else obs[t - 1]), state)
        if value is not None:
            vals.append(v_fn(new[0]))
        if t == T:
            break
        acts.append(act_fn(new[0]))
        d = done[t] != 0
        if value is not None and term_rows is not None:
            tv = np.zeros(d.shape[0])
            if d.any():
                tv[d] = v_fn(step(enc_fn(np.asarray(term_rows[t])[d]), tuple(s[d] for s in new))[0])
            tvs.append(tv)
        state = tuple(np.where(d[:, None], 0.0, s) for s in new)
    out = dict(a=np.stack(acts), h=state[0])
    if cell == "lstm":
        out["c"] = state[1]
    if value is not None:
        out["v"] = np.stack(vals)
        if term_rows is not None:
            out["tv"] = np.stack(tvs)
    return out
