"""Helpers of the GRU policy tests: random GRU cells and heads, gaq_policy_desc_rnn descriptions, and an fp64 reference of a closed-loop
GRU rollout (gaq.h gaq_step_policy_many_dev with a GRU policy) fed the device's recorded observations and dones."""
import ctypes as C

import numpy as np


def _gru(H, D=18, seed=0, scale=0.3):
    rng = np.random.RandomState(seed)
    return tuple((scale * rng.randn(*s)).astype(np.float32) for s in ((3 * H, D), (3 * H, H), (3 * H,), (3 * H,)))


def _head(H, widths=(), seed=1):
    rng = np.random.RandomState(seed)
    dims = [H] + list(widths) + [4]
    return [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
            for k in range(len(dims) - 1)]


def _desc_rnn(widths, engine=1, cell=1, in_dim=18):
    from gym_art_amd.policy import _DescRnn
    d = _DescRnn()
    d.struct_size = C.sizeof(_DescRnn)
    d.in_dim, d.n_hidden = in_dim, len(widths)
    for k, w in enumerate(widths[:3]):
        d.width[k] = w
    d.engine, d.cell = engine, cell
    return d


def gru_step64(gru, x, h):
    """torch nn.GRUCell in float64 on numpy arrays: x [N, I], h [N, H] -> h'"""
    W_ih, W_hh, b_ih, b_hh = (np.asarray(a, np.float64) for a in gru)
    H = W_hh.shape[1]
    gi = x @ W_ih.T + b_ih
    gh = h @ W_hh.T + b_hh
    r = 1.0 / (1.0 + np.exp(-(gi[:, :H] + gh[:, :H])))
    z = 1.0 / (1.0 + np.exp(-(gi[:, H:2 * H] + gh[:, H:2 * H])))
    n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1.0 - z) * n + z * h


def head64(layers, act, out_tanh, h):
    y = h
    for W, b in layers[:-1]:
        y = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        y = np.tanh(y) if act == "tanh" else np.maximum(y, 0.0)
    W, b = layers[-1]
    y = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
    return np.tanh(y) if out_tanh else y


def reference_rollout(gru, layers, act, out_tanh, obs0, obs, done, h0):
    """The deterministic actions [T, N, 4] and the final state [N, H] of a closed-loop GRU rollout from h0, with obs_{t-1} = obs0 for
    t = 0 and obs[t - 1] after, and h zeroed in the rows of done[t] after step t."""
    obs0, obs, done = (np.asarray(a) for a in (obs0, obs, done))
    h = np.asarray(h0, np.float64)
    acts = []
    for t in range(obs.shape[0]):
        x = np.asarray(obs0 if t == 0 else obs[t - 1], np.float64)
        h = gru_step64(gru, x, h)
        acts.append(head64(layers, act, out_tanh, h))
        h = np.where(done[t][:, None] != 0, 0.0, h)
    return np.stack(acts), h
