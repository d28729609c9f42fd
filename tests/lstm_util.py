"""Helpers of the LSTM policy tests: random LSTM cells, gaq_policy_desc_rnn descriptions with cell = GAQ_POLICY_CELL_LSTM, and an fp64
reference of a closed-loop LSTM rollout (gaq.h gaq_step_policy_many_dev with an LSTM policy) fed the device's recorded observations and
dones -- actions, both final states, the value head's V per step and the terminal values -- written so that the cell step is a
parameter: the yardstick of the GPU tests runs the same rollout with torch's fp32 nn.LSTMCell (and an fp32 torch head) on the CPU in
its place."""
import numpy as np

from tests.gru_util import _desc_rnn, head64

CELL_LSTM = 3


def _lstm(H, D=18, seed=0, scale=0.3):
    rng = np.random.RandomState(seed)
    return tuple((scale * rng.randn(*s)).astype(np.float32) for s in ((4 * H, D), (4 * H, H), (4 * H,), (4 * H,)))


def _desc_lstm(widths, engine=1, cell=CELL_LSTM, in_dim=18):
    return _desc_rnn(widths, engine, cell, in_dim)


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_step64(lstm, x, h, c):
    """torch nn.LSTMCell in float64 on numpy arrays (gate rows i, f, g, o): x [N, I], h [N, H], c [N, H] -> (h', c')"""
    W_ih, W_hh, b_ih, b_hh = (np.asarray(a, np.float64) for a in lstm)
    H = W_hh.shape[1]
    z = x @ W_ih.T + b_ih + h @ W_hh.T + b_hh
    i, f, g, o = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sigmoid(z[:, 3 * H:])
    cn = f * c + i * g
    return o * np.tanh(cn), cn


def torch_step32(lstm):
    """the yardstick's cell: torch's fp32 nn.LSTMCell on the CPU with these weights, as a step function on float64 arrays (the state
    is rounded to fp32 each step, as a torch fp32 rollout keeps it)"""
    import torch
    W_ih, W_hh, b_ih, b_hh = lstm
    cell = torch.nn.LSTMCell(W_ih.shape[1], W_hh.shape[1])
    with torch.no_grad():
        for p, a in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), lstm):
            p.copy_(torch.from_numpy(np.asarray(a, np.float32)))

    def step(_, x, h, c):
        with torch.no_grad():
            hn, cn = cell(torch.from_numpy(np.asarray(x, np.float32)),
                          (torch.from_numpy(np.asarray(h, np.float32)), torch.from_numpy(np.asarray(c, np.float32))))
        return hn.numpy().astype(np.float64), cn.numpy().astype(np.float64)
    return step


def torch_head32(layers, act, out_tanh, value=None):
    """the yardstick's head: (actions(h'), V(h')) as torch fp32 computes them on the CPU (Linear, tanh / relu), on float64 arrays"""
    import torch
    F = torch.nn.functional
    tl = [(torch.from_numpy(np.asarray(W, np.float32)), torch.from_numpy(np.asarray(b, np.float32))) for W, b in layers]

    def trunk(h):
        y = torch.from_numpy(np.asarray(h, np.float32))
        for W, b in tl[:-1]:
            y = F.linear(y, W, b)
            y = torch.tanh(y) if act == "tanh" else torch.relu(y)
        return y

    def actions(h):
        z = F.linear(trunk(h), *tl[-1])
        return (torch.tanh(z) if out_tanh else z).numpy().astype(np.float64)

    def v(h):
        w = torch.from_numpy(np.asarray(value[0], np.float32).reshape(1, -1))
        return F.linear(trunk(h), w, torch.from_numpy(np.asarray(value[1], np.float32).reshape(1))).numpy().astype(np.float64)[:, 0]
    return actions, v


def hidden64(layers, act, h):
    """the head's hidden layers on h' in float64: the activations the 4-output layer and the value head read"""
    y = h
    for W, b in layers[:-1]:
        y = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        y = np.tanh(y) if act == "tanh" else np.maximum(y, 0.0)
    return y


def value64(layers, act, value, h):
    return hidden64(layers, act, h) @ np.asarray(value[0], np.float64).reshape(-1) + np.float64(value[1])


def reference_rollout(lstm, layers, act, out_tanh, obs0, obs, done, h0, c0, value=None, term_rows=None, step=lstm_step64, head=None):
    """A closed-loop LSTM rollout from (h0, c0) with obs_{t-1} = obs0 for t = 0 and obs[t - 1] after, h and c zeroed in the rows of
    done[t] after step t.  Returns a dict: "a" the deterministic actions [T, N, 4], "h" / "c" the final states [N, H], and with `value`
    "v" [T + 1, N] (row T: V of LSTM(obs[T - 1], the masked state), which is not kept) and, with `term_rows` [T, N, D] (read where done
    is set), "tv" [T, N]: V of LSTM(term row, the h' and c' action t used) where done[t], 0 elsewhere.  `step` is the cell and `head` =
    (actions(h'), V(h')) the head (fp64 by default; the yardstick passes torch_step32 and torch_head32)."""
    obs0, obs, done = (np.asarray(a) for a in (obs0, obs, done))
    h, c = np.asarray(h0, np.float64), np.asarray(c0, np.float64)
    T = obs.shape[0]
    acts, vals, tvs = [], [], []
    act_fn, v_fn = head if head is not None else (lambda y: head64(layers, act, out_tanh, y), lambda y: value64(layers, act, value, y))
    for t in range(T + 1):
        x = np.asarray(obs0 if t == 0 else obs[t - 1], np.float64)
        hn, cn = step(lstm, x, h, c)
        if value is not None:
            vals.append(v_fn(hn))
        if t == T:
            break
        acts.append(act_fn(hn))
        d = done[t] != 0
        if value is not None and term_rows is not None:
            tv = np.zeros(d.shape[0])
            if d.any():
                ht, _ = step(lstm, np.asarray(term_rows[t], np.float64)[d], hn[d], cn[d])
                tv[d] = v_fn(ht)
            tvs.append(tv)
        h, c = np.where(d[:, None], 0.0, hn), np.where(d[:, None], 0.0, cn)
    out = dict(a=np.stack(acts), h=h, c=c)
    if value is not None:
        out["v"] = np.stack(vals)
        if term_rows is not None:
            out["tv"] = np.stack(tvs)
    return out
