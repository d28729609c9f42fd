"""An fp64 restatement of the learner's passes for a recurrent policy with an encoder (gaq.h "sequences through an encoder":
gaq_policy_eval_enc_seq_dev, gaq_policy_grad_ppo_enc_seq_dev and its idx form) on fp32 inputs.  It composes what the tree has:
tests/enc_util.py's encoder (encoder64) in front of tests/policy_grad_seq_ref.py (the GRU) or tests/policy_grad_lstm_ref.py (the LSTM),
whose forward, loss and manual BPTT with the rollout's done selects run on the features as their `x`; what is new here is the gradient of
the loss in the features (dfeat_t = [the cell's gate deltas]_t W_ih, restated from those modules' backward sweeps: they do not return it)
and the encoder's backpropagation over the T S rows.  An attached normaliser (G's exact-table one) is frozen.

Cases: the encoders (16,) the smallest, (48,) three chunks, (80,) a wave owns two chunks of the dfeat product, (32, 64) two layers, and
(128,) the width limit on a GRU of H = 16; D = 18 and 19 (the partial k-step); one case behind the normaliser; tanh + output tanh and
relu; H in {16, 64}, both cells; with and without a value head; vclip 0 and 0.2.  Every case has TMAX = 6 steps of SMAX = 130 sequences
(two whole tiles and one of 2); CONFIGS and done_mask are the parents'.

Inputs, from RandomState(seed + 7000): enc_util._encoder weights (seed + 2), the parents' cell (on E inputs) and head, Gaussian
observations, then everything the parents draw, with their formulas, on the features.  The seed of each case (SEEDS)
was searched on the CPU (`python -m tests.policy_grad_enc_ref`) so that conditions() holds in the fp64 reference: the parent's conditions
on the features, and no relu pre-activation of the ENCODER within 2e-5 of 0.

Bounds: BASELINE holds, per case and (T, S), torch fp32 autograd's error on the CPU against this reference on the same inputs (Linear
layers, a GRUCell / LSTMCell loop with torch.where resets, a Linear head, a value Linear): (gradient of the cell and head, gradient of
the ENCODER, logp, V, sum L_clip, sum k3, sum L_V), each max|v - v64| / max|v64|, a gradient's the largest over its parameter tensors
(the encoder's W and b of every layer separately; the other: the cell's four, the head's, grad_value, grad_log_std).  The device's
bound is G.FACTOR = 8 x that, by the parents' rule (bounds())."""
import numpy as np

from tests import policy_grad_lstm_ref as L
from tests import policy_grad_seq_ref as S
from tests.enc_util import _encoder
from tests.gru_util import _gru, _head
from tests.lstm_util import _lstm

G, A = S.G, S.A
TMAX, SMAX, CONFIGS = S.TMAX, S.SMAX, S.CONFIGS
CLIP, LOG_STD, FACTOR = S.CLIP, S.LOG_STD, S.FACTOR
VF_COEF, ENT_COEF, VCLIP = S.VF_COEF, S.ENT_COEF, S.VCLIP
REF = {"gru": S, "lstm": L}


class EncCase:
    def __init__(self, cell, enc, H, head, act, out_tanh, D=18, norm=False, vclip=0.0, value=True):
        self.cell, self.enc, self.D, self.norm = cell, tuple(enc), D, norm
        mk = S.SeqCase if cell == "gru" else L.LstmCase
        self.inner = mk(H, head, act, out_tanh, D=self.enc[-1], norm=False, vclip=vclip, value=value)   # the cell on the features
        self.H, self.head, self.act, self.out_tanh, self.vclip, self.value = H, tuple(head), act, bool(out_tanh), float(vclip), value
        self.name = "enc%s-%s%s%s" % ("x".join(map(str, enc)), self.inner.name.replace("-d%d" % self.enc[-1], "", 1), "-d%d" % D if D != 18 else "",
                                      "-norm" if norm else "")

    def __repr__(self):
        return self.name


ENC_CASES = [EncCase("gru", (16,), 16, (), "tanh", True),
             EncCase("lstm", (48,), 64, (64, 64), "tanh", True, D=19, vclip=VCLIP),
             EncCase("gru", (80,), 64, (64,), "tanh", True, vclip=VCLIP),
             EncCase("lstm", (32, 64), 16, (), "relu", False, norm=True),
             EncCase("gru", (128,), 16, (), "relu", False, D=19, value=False),
             EncCase("lstm", (80,), 64, (16, 48), "tanh", True, value=False),
             EncCase("gru", (32, 64), 64, (16,), "relu", False, D=19),
             EncCase("lstm", (16,), 16, (), "tanh", True)]
CASES = {c.name: c for c in ENC_CASES}


def encoder_forward(case, inp, obs):
    """fp64: (the layers' inputs [z, a_0, ...] with z the normalised observation, the pre-activations)"""
    y = np.asarray(G.normalised(obs, case.D) if case.norm else obs, np.float64)
    acts, pre = [y], []
    for W, b in inp["enc"]:
        v = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        pre.append(v)
        y = np.tanh(v) if case.act == "tanh" else np.maximum(v, 0.0)
        acts.append(y)
    return acts, pre


def inputs(case, seed):
    """the parents' inputs, by their formulas, for the cell on the features of Gaussian observations"""
    R, inner = REF[case.cell], case.inner
    rng = np.random.RandomState(seed + 7000)
    E = case.enc[-1]
    inp = {case.cell: (_gru if case.cell == "gru" else _lstm)(case.H, E, seed), "head": _head(case.H, case.head, seed + 1),
           "enc": _encoder(case.D, case.enc, seed + 2)}
    obs = rng.randn(TMAX, SMAX, case.D).astype(np.float32)
    if case.norm:
        obs = (2.0 * obs + 0.25).astype(np.float32)
    acts, _ = encoder_forward(case, inp, obs.reshape(-1, case.D))
    inp["obs"], inp["x"] = obs, acts[-1].reshape(TMAX, SMAX, E)      # the cell reads the features in fp64, unrounded
    inp["h0"] = (0.5 * rng.randn(SMAX, case.H)).astype(np.float32)
    if case.cell == "lstm":
        inp["c0"] = (0.5 * rng.randn(SMAX, case.H)).astype(np.float32)
    inp["done"] = S.done_mask(rng)
    W = (case.head[-1] if case.head else case.H)
    inp["wv"] = (rng.randn(W) / np.sqrt(W)).astype(np.float32)
    inp["bv"] = np.float32(0.1 * rng.randn())
    steps, _ = R.forward_seq(inner, inp, TMAX, SMAX)
    mean = np.stack([s[-1][2] for s in steps])
    v = np.stack([s[-1][0][-1] for s in steps]) @ inp["wv"].astype(np.float64) + float(inp["bv"])
    std = np.exp(LOG_STD.astype(np.float64))
    mean_b = mean + 0.15 * std * rng.randn(TMAX, SMAX, 4)
    z = rng.randn(TMAX, SMAX, 4)
    inp["actions"] = (mean_b + std * z).astype(np.float32)
    inp["logp_old"] = ((-0.5 * z * z - LOG_STD).sum(axis=2) - G.TWO_LN_2PI).astype(np.float32)
    inp["adv"] = rng.randn(TMAX, SMAX).astype(np.float32)
    inp["ret"] = (v + 0.5 * rng.randn(TMAX, SMAX)).astype(np.float32)
    inp["v_old"] = (v + 0.25 * rng.randn(TMAX, SMAX)).astype(np.float32)
    return inp


def _gate_deltas(case, inp, ref, T, S, scale, s_lo=0, t_lo=0, done=None):
    """[T, S, gates H]: the deltas of the cell's input-side gate sums per step (da_r, da_z, da_n / da_i, da_f, da_g, da_o), by the
    parents' backward sweeps restated; their sum over (t, s) against x is the parents' own g_W_ih, which the CPU test compares"""
    R, inner = REF[case.cell], case.inner
    done = inp["done"] if done is None else done
    out = R.forward_seq(inner, inp, T, S, s_lo, t_lo, done=done)
    steps = out[0]
    sl = (slice(t_lo, t_lo + T), slice(s_lo, s_lo + S))
    f64 = lambda k: np.asarray(inp[k][sl], np.float64)
    inv = np.exp(-LOG_STD.astype(np.float64))
    z = (f64("actions") - ref["mean"]) * inv
    dl = np.where(ref["active"], -f64("adv") * ref["ratio"], 0.0)
    dmean = scale * dl[..., None] * z * inv
    dv, wv, head = ref["dv"], inp["wv"].astype(np.float64), inp["head"]
    actd = (lambda h: 1.0 - h * h) if case.act == "tanh" else (lambda h: (h > 0.0).astype(np.float64))
    cellw = [np.asarray(a, np.float64) for a in inp[case.cell]]
    W_hh, H = cellw[1], case.H
    carry_h, carry_c = np.zeros((S, H)), np.zeros((S, H))
    das = [None] * T
    for k in range(T - 1, -1, -1):
        hs, pre, m, zsum = steps[k][-1]
        d = dmean[k] * ((1.0 - m * m) if case.out_tanh else 1.0)
        d = d @ np.asarray(head[-1][0], np.float64) + dv[k][:, None] * wv[None, :]
        for l in range(len(head) - 2, -1, -1):
            d = (d * actd(hs[l + 1])) @ np.asarray(head[l][0], np.float64)
        dh = d + carry_h
        if case.cell == "gru":
            x, hin = steps[k][0], steps[k][1]
            rg, zg, n, n_h = REF["gru"].gates64(inp["gru"], x, hin)
            da_n = dh * (1.0 - zg) * (1.0 - n * n)
            da_z = dh * (hin - n) * zg * (1.0 - zg)
            da_r = da_n * n_h * rg * (1.0 - rg)
            das[k] = np.concatenate([da_r, da_z, da_n], axis=1)
            prev_h = dh * zg + np.concatenate([da_r, da_z, da_n * rg], axis=1) @ W_hh
            prev_c = carry_c
        else:
            x, hin, cin, h, c = steps[k][:5]
            ig, fg, gg, og = REF["lstm"].gates64(inp["lstm"], x, hin)
            tc = np.tanh(c)
            dc = carry_c + dh * og * (1.0 - tc * tc)
            das[k] = np.concatenate([dc * gg * ig * (1.0 - ig), dc * cin * fg * (1.0 - fg), dc * ig * (1.0 - gg * gg),
                                     dh * tc * og * (1.0 - og)], axis=1)
            prev_h, prev_c = das[k] @ W_hh, dc * fg
        if k > 0:
            keep = done[t_lo + k - 1, s_lo:s_lo + S, None] == 0
            carry_h, carry_c = np.where(keep, prev_h, 0.0), np.where(keep, prev_c, 0.0)
    return np.stack(das)


def ppo_enc_seq(case, inp, T, S, scale=None, s_lo=0, t_lo=0, done=None, **kw):
    """the fp64 reference of gaq_policy_grad_ppo_enc_seq_dev on the steps [t_lo, t_lo + T) of the sequences [s_lo, s_lo + S): the
    parent's dict (gradients of the cell and the head, logp, value, stats ...) plus "dfeat" [T, S, E], "g_enc" [(dW, db), ...] and
    "enc_pre" (the encoder's pre-activations)"""
    R = REF[case.cell]
    scale = 1.0 / (T * S) if scale is None else scale
    ref = R.ppo_seq(case.inner, inp, T, S, scale=scale, s_lo=s_lo, t_lo=t_lo, done=done, **kw)
    da = _gate_deltas(case, inp, ref, T, S, scale, s_lo, t_lo, done)
    W_ih = np.asarray(inp[case.cell][0], np.float64)
    dfeat = da @ W_ih
    obs = inp["obs"][t_lo:t_lo + T, s_lo:s_lo + S].reshape(T * S, case.D)
    acts, pre = encoder_forward(case, inp, obs)
    d = dfeat.reshape(T * S, -1)
    g_enc = [None] * len(inp["enc"])
    for l in range(len(inp["enc"]) - 1, -1, -1):
        d = d * ((1.0 - acts[l + 1] ** 2) if case.act == "tanh" else (pre[l] > 0.0))
        g_enc[l] = (d.T @ acts[l], d.sum(axis=0))
        d = d @ np.asarray(inp["enc"][l][0], np.float64)
    ref = dict(ref, dfeat=dfeat, g_enc=g_enc, enc_pre=pre, g_wih_check=np.einsum("tsg,tse->ge", da, np.asarray(
        inp["x"][t_lo:t_lo + T, s_lo:s_lo + S], np.float64)))
    return ref


def conditions(case, inp):
    """None if the inputs meet the conditions in the fp64 reference, else what fails: the parent's on the features, and no relu
    pre-activation of the encoder within 2e-5 of 0"""
    bad = REF[case.cell].conditions(case.inner, inp)
    if bad:
        return bad
    if case.act == "relu":
        _, pre = encoder_forward(case, inp, inp["obs"].reshape(-1, case.D))
        if min(float(np.abs(v).min()) for v in pre) < 2e-5:
            return "a relu pre-activation of the encoder within 2e-5 of 0"
    return None


def enc_errors(got_enc, ref):
    """G.rel of every tensor of the encoder's gradient: got_enc = [(dW, db), ...] as unpack_encoder_weights returns them"""
    return [G.rel(a, b) for gwb, rwb in zip(got_enc, ref["g_enc"]) for a, b in zip(gwb, rwb)]


def torch_errors(case, inp, T, S, dtype, each=False):
    """torch autograd of `dtype` on the CPU against the reference: (gradient of the cell and head, gradient of the encoder, logp, V,
    sum L_clip, sum k3, sum L_V); each: the two gradients' entries are the lists of every tensor's error"""
    import torch
    import torch.nn as nn
    R, inner = REF[case.cell], case.inner
    ref = ppo_enc_seq(case, inp, T, S)
    model = R.torch_model(inner, inp, dtype)
    lins = []
    for W, b in inp["enc"]:
        lin = nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data, lin.bias.data = torch.tensor(W), torch.tensor(b)
        lins.append(lin.to(dtype))
    tens = R.torch_tensors(dict(inp, x=np.zeros((T, S, 1), np.float32)), T, S, dtype)
    y = torch.tensor(np.asarray(G.normalised(inp["obs"][:T, :S], case.D) if case.norm else inp["obs"][:T, :S]), dtype=dtype)
    for lin in lins:
        y = lin(y)
        y = torch.tanh(y) if case.act == "tanh" else torch.relu(y)
    tens["x"] = y
    loss, lp, v, lsum, kl, lvsum = R.torch_loss(inner, tens, T, S, model)
    loss.backward()
    errs = R.grad_errors(*R.torch_grads(inner, model), ref)
    eerrs = enc_errors([(l.weight.grad.numpy(), l.bias.grad.numpy()) for l in lins], ref)
    f = lambda a: float(a.detach())
    return (errs if each else max(errs), eerrs if each else max(eerrs), G.rel(lp.detach().numpy(), ref["logp"]),
            G.rel(v.detach().numpy(), ref["value"]), G.rel(f(lsum), ref["stats"][0]), G.rel(f(kl), ref["stats"][2]),
            G.rel(f(lvsum), ref["stats"][3]) if case.value else 0.0)


def find_seed(case, limit=20000):
    for seed in range(limit):
        if conditions(case, inputs(case, seed)) is None:
            return seed
    raise RuntimeError("no seed below %d meets the conditions of %s" % (limit, case.name))


# the seed of each case: the first that meets conditions() (python -m tests.policy_grad_enc_ref)
SEEDS = {
    'enc16-gru16-tanh': 9,
    'enc48-lstm64x64x64-tanh-vclip-d19': 5,
    'enc80-gru64x64-tanh-vclip': 13,
    'enc32x64-lstm16-relu-norm': 3,
    'enc128-gru16-relu-nohead-d19': 4,
    'enc80-lstm64x16x48-tanh-nohead': 10,
    'enc32x64-gru64x16-relu-d19': 15,
    'enc16-lstm16-tanh': 0,
}

# per case and (T, S): torch fp32 autograd's (gradient, encoder gradient, logp, V, sum L_clip, sum k3, sum L_V) errors against the
# reference (python -m tests.policy_grad_enc_ref; torch on the CPU)
BASELINE = {
    'enc16-gru16-tanh': {(1, 1): (3.15e-07, 3.01e-07, 1.08e-07, 1.24e-07, 3.63e-07, 7.11e-06, 3.3e-07), (1, 65): (1.33e-06, 4.7e-07, 9.46e-08, 1.49e-07, 4.37e-08, 1.13e-07, 1.49e-09), (2, 63): (6.87e-07, 3.9e-07, 6.94e-08, 8.42e-08, 1.58e-06, 1.36e-07, 4.84e-08), (5, 64): (7.19e-07, 4.77e-07, 1.14e-07, 1.45e-07, 6.52e-06, 1.12e-07, 1.63e-10), (5, 65): (6.67e-07, 4.22e-07, 1.14e-07, 1.45e-07, 2.17e-06, 1.78e-07, 2.29e-08), (6, 130): (1.03e-06, 6.26e-07, 1.5e-07, 1.34e-07, 1.8e-07, 1.83e-08, 8.89e-09)},
    'enc48-lstm64x64x64-tanh-vclip-d19': {(1, 1): (5.25e-07, 5.31e-07, 8.2e-08, 5.11e-08, 3.83e-07, 1.79e-05, 2.25e-08), (1, 65): (5.38e-07, 1.2e-06, 9.67e-08, 2.37e-07, 3.91e-07, 6.3e-07, 4.8e-10), (2, 63): (8.12e-07, 7.99e-07, 9.35e-08, 2.19e-07, 5.51e-07, 1.61e-07, 6.63e-09), (5, 64): (7.71e-07, 9.22e-07, 1.6e-07, 2.37e-07, 2.77e-07, 8.8e-08, 1.2e-07), (5, 65): (6.71e-07, 8.7e-07, 1.6e-07, 2.37e-07, 6.91e-08, 3.27e-08, 8.36e-08), (6, 130): (9.59e-07, 9.27e-07, 1.61e-07, 2.37e-07, 4.16e-08, 8.6e-09, 5.75e-08)},
    'enc80-gru64x64-tanh-vclip': {(1, 1): (5.27e-07, 6.37e-07, 1.27e-07, 1.04e-07, 3.85e-07, 4.84e-05, 3.17e-07), (1, 65): (1.16e-06, 7.8e-07, 9.59e-08, 1.68e-07, 1.94e-06, 4.67e-07, 7.37e-08), (2, 63): (1.19e-06, 9.16e-07, 1.43e-07, 1.88e-07, 2.05e-06, 5.84e-08, 7.39e-08), (5, 64): (7.72e-07, 1.08e-06, 1.69e-07, 2.24e-07, 8.44e-07, 6.56e-08, 9.65e-08), (5, 65): (1.01e-06, 7.01e-07, 1.69e-07, 2.24e-07, 7.06e-07, 1.23e-07, 9.14e-08), (6, 130): (9.59e-07, 7.06e-07, 1.69e-07, 2.77e-07, 5.01e-07, 2.27e-08, 9.69e-08)},
    'enc32x64-lstm16-relu-norm': {(1, 1): (6.48e-07, 5.21e-07, 6.26e-08, 7.47e-08, 2.79e-07, 2.02e-06, 2.78e-07), (1, 65): (3.84e-07, 4.33e-07, 1.3e-07, 1.85e-07, 2.96e-07, 4.59e-08, 5.29e-08), (2, 63): (9.93e-07, 4.7e-07, 1.25e-07, 1.85e-07, 1.55e-07, 7.18e-08, 1.59e-08), (5, 64): (4.49e-07, 8.43e-07, 1.6e-07, 2.23e-07, 6.27e-08, 2.23e-07, 3.4e-09), (5, 65): (3.94e-07, 8.07e-07, 1.6e-07, 2.23e-07, 1.26e-07, 1.3e-07, 7.01e-08), (6, 130): (1.1e-06, 5.05e-07, 1.3e-07, 3e-07, 5.22e-08, 6.52e-08, 3.83e-08)},
    'enc128-gru16-relu-nohead-d19': {(1, 1): (4.56e-07, 2.75e-07, 4.17e-08, 3.27e-08, 1.3e-07, 1.52e-06, 0), (1, 65): (6.73e-07, 5.47e-07, 1.77e-07, 1.85e-07, 4.05e-07, 1.54e-07, 0), (2, 63): (6.74e-07, 5.49e-07, 1.58e-07, 1.79e-07, 5.34e-07, 1.91e-07, 0), (5, 64): (9.37e-07, 6.15e-07, 1.53e-07, 2.36e-07, 1.69e-05, 2.29e-07, 0), (5, 65): (9.4e-07, 6.65e-07, 1.65e-07, 2.36e-07, 0.000124, 1.97e-07, 0), (6, 130): (8.53e-07, 7.36e-07, 2.27e-07, 2.92e-07, 4.14e-07, 9.23e-09, 0)},
    'enc80-lstm64x16x48-tanh-nohead': {(1, 1): (6.65e-07, 5.53e-07, 4.17e-08, 2.38e-05, 2.62e-07, 2.19e-06, 0), (1, 65): (9.84e-07, 7.35e-07, 1.52e-07, 3.28e-07, 1.98e-08, 5.42e-07, 0), (2, 63): (7.75e-07, 1.15e-06, 1.58e-07, 3.38e-07, 1.96e-07, 1.54e-07, 0), (5, 64): (7.44e-07, 8.99e-07, 1.51e-07, 2.51e-07, 6.85e-08, 4.81e-08, 0), (5, 65): (9.37e-07, 9.22e-07, 1.51e-07, 2.51e-07, 4.2e-08, 1.98e-08, 0), (6, 130): (7.23e-07, 7.76e-07, 1.45e-07, 2.75e-07, 7.42e-08, 4.05e-08, 0)},
    'enc32x64-gru64x16-relu-d19': {(1, 1): (3.02e-07, 1.96e-07, 8.58e-08, 6.06e-08, 2.24e-07, 2.15e-06, 5.58e-08), (1, 65): (5.03e-07, 6.39e-07, 1.35e-07, 2.34e-07, 3.49e-07, 3.24e-07, 9.37e-08), (2, 63): (4.39e-07, 5.76e-07, 1.23e-07, 3.28e-07, 1.2e-07, 5.66e-08, 3.79e-08), (5, 64): (5.53e-07, 5.13e-07, 1.46e-07, 2.87e-07, 3.58e-06, 1.02e-07, 1.05e-07), (5, 65): (6.42e-07, 6.03e-07, 1.46e-07, 2.87e-07, 2.1e-06, 1.4e-07, 2.03e-08), (6, 130): (8.01e-07, 6.09e-07, 1.54e-07, 3.14e-07, 9.83e-08, 7.35e-08, 1.99e-08)},
    'enc16-lstm16-tanh': {(1, 1): (2.95e-07, 1.67e-07, 8.97e-08, 3.01e-07, 2.39e-07, 5.95e-06, 8.92e-08), (1, 65): (9.84e-07, 3.27e-07, 1.15e-07, 1.02e-07, 2.29e-07, 2.34e-07, 3.14e-08), (2, 63): (7.86e-07, 5.3e-07, 1.15e-07, 1.13e-07, 4.72e-07, 2.19e-07, 5.3e-08), (5, 64): (6.72e-07, 7.24e-07, 1.07e-07, 1.46e-07, 7.21e-08, 1.47e-07, 4.52e-08), (5, 65): (6.86e-07, 6.64e-07, 1.07e-07, 1.46e-07, 1.87e-07, 9.14e-08, 2.52e-08), (6, 130): (5.52e-07, 5.09e-07, 1.18e-07, 1.81e-07, 2.72e-07, 9.96e-08, 9.34e-09)},
}

_INPUTS, _REFS = {}, {}


def case_inputs(name):
    """the case and its inputs at its seed, computed once and shared: treat them as read-only"""
    if name not in _INPUTS:
        _INPUTS[name] = inputs(CASES[name], SEEDS[name])
    return CASES[name], _INPUTS[name]


def case_ref(name, T, S):
    """ppo_enc_seq of the case at its defaults on the prefix (T, S), computed once and shared: read-only"""
    if (name, T, S) not in _REFS:
        case, inp = case_inputs(name)
        _REFS[name, T, S] = ppo_enc_seq(case, inp, T, S)
    return _REFS[name, T, S]


def bounds(name, T, S):
    """The device's bounds for the case at (T, S), FACTOR x torch fp32's errors: (gradient, encoder gradient, logp, V, sum L_clip,
    sum k3, sum L_V).  The parents' rule: the two gradients' are the case's own at that size, and so are logp's and V's at more than
    one row; the true scalars -- the three sums at every size, logp and V at (1, 1) -- take the largest torch error over the cases at
    that size."""
    pooled = [max(BASELINE[c.name][T, S][k] for c in ENC_CASES) for k in range(2, 7)]
    own = BASELINE[name][T, S]
    one = T * S == 1
    return (FACTOR * own[0], FACTOR * own[1], FACTOR * (pooled[0] if one else own[2]), FACTOR * (pooled[1] if one else own[3]),
            FACTOR * pooled[2], FACTOR * pooled[3], FACTOR * pooled[4])


if __name__ == "__main__":
    import sys
    import torch
    seeds = {c.name: find_seed(c) for c in ENC_CASES}
    out = ["SEEDS = {"] + ["    %r: %d," % kv for kv in seeds.items()] + ["}", "", "BASELINE = {"]
    for c in ENC_CASES:
        inp = inputs(c, seeds[c.name])
        out.append("    %r: {%s}," % (c.name, ", ".join("(%d, %d): (%s)" % (T, S, ", ".join("%.3g" % e for e in torch_errors(c, inp, T, S, torch.float32)))
                                                        for T, S in CONFIGS)))
    out.append("}")
    print("\n".join(out))
    sys.stdout.flush()
