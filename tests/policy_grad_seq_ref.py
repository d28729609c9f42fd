"""An fp64 restatement of the recurrent learner's passes (gaq.h gaq_policy_eval_seq_dev, gaq_policy_grad_ppo_seq_dev) on fp32 inputs:
the forward pass over stored sequences from gru_util.gru_step64 and G.forward (head64's arithmetic with the layers' inputs kept), the
loss of tests/policy_grad_ac_ref.py (A below) per (t, sequence), and manual backpropagation through time with the rollout's done
selects -- with the cases, the inputs and the bounds the CPU and GPU tests share.

Semantics: hin_t = 0 where t > 0 and done[t-1] else h_{t-1} (h_{-1} = h0), h_t = GRU(x_t, hin_t), mean_t, V_t from the head on h_t; the
gradient is truncated at step 0 (nothing flows into h0) and flows from step t to t - 1 exactly where done[t-1] is clear.

Cases: four (H, head) shapes x (tanh + output tanh, relu without), one on a 19-wide observation and one behind G's exact-table
normaliser, each with a value head at vclip 0 and 0.2; two of them also without a value head.  Every case has TMAX = 6 steps of
SMAX = 130 sequences; the smaller (T, S) of CONFIGS are prefixes in both directions.

Inputs, from RandomState(seed + 3000): gru_util._gru / _head weights, Gaussian observations and h0, a done mask with a fixed pattern in
the first rows of each tile (done_mask) over 12 % random dones elsewhere, behaviour means 0.15 sigma off the net's, Gaussian advantages,
ret = V + 0.5 n and v_old = V + 0.25 n.  The seed of each case (SEEDS) was searched on the CPU (`python -m tests.policy_grad_seq_ref`)
so that conditions() holds in the fp64 reference.

Bounds: BASELINE holds, per case and (T, S), torch fp32 autograd's error on the CPU against this reference on the same inputs (a GRUCell
loop with torch.where resets, a Linear head, a value Linear): (gradient, logp, V, sum L_clip, sum k3, sum L_V), each
max|v - v64| / max|v64|, the gradient's the largest over the parameter tensors (weight_ih, bias_ih, weight_hh, bias_hh and the head's
separately), grad_value and grad_log_std.  The device's bound is G.FACTOR = 8 x that, for the reason G states (bounds())."""
import numpy as np

from tests import policy_grad_ac_ref as A
from tests import policy_grad_ref as G
from tests.gru_util import _gru, _head, gru_step64

TMAX, SMAX = 6, 130
CONFIGS = [(1, 1), (1, 65), (2, 63), (5, 64), (5, 65), (6, 130)]
CLIP, LOG_STD, FACTOR = G.CLIP, G.LOG_STD, G.FACTOR
VF_COEF, ENT_COEF, VCLIP = A.VF_COEF, A.ENT_COEF, A.VCLIP
SHAPES = [(16, ()), (48, (32,)), (64, (16, 48)), (64, (64, 64))]


class SeqCase:
    def __init__(self, H, head, act, out_tanh, D=18, norm=False, vclip=0.0, value=True):
        self.H, self.head, self.act, self.out_tanh, self.D, self.norm = H, tuple(head), act, bool(out_tanh), D, norm
        self.vclip, self.value = float(vclip), value
        self.name = "gru%d%s-%s%s%s%s" % (H, "".join("x%d" % w for w in head), act, "-d%d" % D if D != 18 else "", "-norm" if norm else "",
                                         "-vclip" if vclip > 0 else "" if value else "-nohead")

    def __repr__(self):
        return self.name


_NETS = [(H, hd, a, t, 18, False) for H, hd in SHAPES for a, t in G.STYLES] + [(64, (16, 48), "tanh", True, 19, False),
                                                                              (48, (32,), "relu", False, 18, True)]
SEQ_CASES = [SeqCase(H, hd, a, t, D=D, norm=nm, vclip=vc) for H, hd, a, t, D, nm in _NETS for vc in (0.0, VCLIP)] + \
            [SeqCase(16, (), "tanh", True, value=False), SeqCase(64, (64, 64), "relu", False, value=False)]
CASES = {c.name: c for c in SEQ_CASES}


def done_mask(rng):
    """done [TMAX, SMAX] uint8: 12 % random, then in each tile (rows 0 .. and 64 ..) row +0 none, +1 a reset after t = 0, +2 resets at
    t = 3 and 4 (one before the last step of T = 5, and done[T-1] of it), +3 two in a row at t = 1, 2, +4 none, +5 done at t = 4 and 5"""
    d = (rng.rand(TMAX, SMAX) < 0.12).astype(np.uint8)
    for b in (0, 64):
        d[:, b:b + 6] = 0
        d[0, b + 1] = 1
        d[3, b + 2] = d[4, b + 2] = 1
        d[1, b + 3] = d[2, b + 3] = 1
        d[4, b + 5] = d[5, b + 5] = 1
    return d


def done_conditions(done, T, S):
    """None if done[:T, :S] (T >= 5) has what the tests need, else what is missing"""
    d = np.asarray(done[:T, :S]) != 0
    if not d[0].any():
        return "no reset after t = 0"
    if not d[T - 2].any():
        return "no reset before the last step"
    if not (d[:-1] & d[1:]).any():
        return "no two dones in a row"
    if not d[T - 1].any():
        return "done[T-1] set nowhere"
    if d[:, 0].any() or (S > 64 and d[:, 64].any()):
        return "row 0 or row 64 has a done"
    return None


def gates64(gru, x, h):
    """(r, z, n, n_h) of torch's GRUCell in fp64"""
    W_ih, W_hh, b_ih, b_hh = (np.asarray(a, np.float64) for a in gru)
    H = W_hh.shape[1]
    gi, gh = x @ W_ih.T + b_ih, h @ W_hh.T + b_hh
    r = 1.0 / (1.0 + np.exp(-(gi[:, :H] + gh[:, :H])))
    z = 1.0 / (1.0 + np.exp(-(gi[:, H:2 * H] + gh[:, H:2 * H])))
    return r, z, np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:]), gh[:, 2 * H:]


def forward_seq(case, inp, T, S, s_lo=0, t_lo=0, h0=None, done=None):
    """fp64 forward of steps t_lo .. t_lo + T - 1 of the sequences s_lo .. s_lo + S - 1 from h0 (default: the case's): per step
    (x, hin, h, the head's G.forward tuple); and h_out"""
    done = inp["done"] if done is None else done
    h = np.asarray(inp["h0"][s_lo:s_lo + S] if h0 is None else h0, np.float64)
    steps = []
    for t in range(t_lo, t_lo + T):
        x = np.asarray(inp["x"][t, s_lo:s_lo + S], np.float64)
        hin = h if t == t_lo else np.where(done[t - 1, s_lo:s_lo + S, None] != 0, 0.0, h)
        h = gru_step64(inp["gru"], x, hin)
        steps.append((x, hin, h, G.forward(inp["head"], case.act, case.out_tanh, h)))
    return steps, np.where(done[t_lo + T - 1, s_lo:s_lo + S, None] != 0, 0.0, h)


def inputs(case, seed):
    rng = np.random.RandomState(seed + 3000)
    inp = dict(gru=_gru(case.H, case.D, seed), head=_head(case.H, case.head, seed + 1))
    obs = rng.randn(TMAX, SMAX, case.D).astype(np.float32)
    if case.norm:
        obs = (2.0 * obs + 0.25).astype(np.float32)
    inp["obs"], inp["x"] = obs, (G.normalised(obs, case.D) if case.norm else obs)
    inp["h0"] = (0.5 * rng.randn(SMAX, case.H)).astype(np.float32)
    inp["done"] = done_mask(rng)
    W = (case.head[-1] if case.head else case.H)
    inp["wv"] = (rng.randn(W) / np.sqrt(W)).astype(np.float32)
    inp["bv"] = np.float32(0.1 * rng.randn())
    steps, _ = forward_seq(case, inp, TMAX, SMAX)
    mean = np.stack([s[3][2] for s in steps])
    v = np.stack([s[3][0][-1] for s in steps]) @ inp["wv"].astype(np.float64) + float(inp["bv"])
    std = np.exp(LOG_STD.astype(np.float64))
    mean_b = mean + 0.15 * std * rng.randn(TMAX, SMAX, 4)
    z = rng.randn(TMAX, SMAX, 4)
    inp["actions"] = (mean_b + std * z).astype(np.float32)
    inp["logp_old"] = ((-0.5 * z * z - LOG_STD).sum(axis=2) - G.TWO_LN_2PI).astype(np.float32)
    inp["adv"] = rng.randn(TMAX, SMAX).astype(np.float32)
    inp["ret"] = (v + 0.5 * rng.randn(TMAX, SMAX)).astype(np.float32)
    inp["v_old"] = (v + 0.25 * rng.randn(TMAX, SMAX)).astype(np.float32)
    return inp


def ppo_seq(case, inp, T, S, scale=None, clip=CLIP, vclip=None, vf_coef=VF_COEF, ent_coef=ENT_COEF, s_lo=0, t_lo=0, h0=None, done=None,
            value=None):
    """the fp64 reference of gaq_policy_grad_ppo_seq_dev on the steps [t_lo, t_lo + T) of the sequences [s_lo, s_lo + S)"""
    done = inp["done"] if done is None else done
    value = case.value if value is None else value
    scale = 1.0 / (T * S) if scale is None else scale
    vclip = case.vclip if vclip is None else vclip
    steps, h_out = forward_seq(case, inp, T, S, s_lo, t_lo, h0, done)
    sl = (slice(t_lo, t_lo + T), slice(s_lo, s_lo + S))
    f64 = lambda k: np.asarray(inp[k][sl], np.float64)
    mean = np.stack([s[3][2] for s in steps])
    y = np.stack([s[3][0][-1] for s in steps])
    inv = np.exp(-LOG_STD.astype(np.float64))
    z = (f64("actions") - mean) * inv
    logp = (-0.5 * z * z - LOG_STD).sum(axis=2) - G.TWO_LN_2PI
    xr = logp - f64("logp_old")
    r, adv = np.exp(xr), f64("adv")
    s1, s2 = r * adv, np.clip(r, 1.0 - clip, 1.0 + clip) * adv
    dl = np.where(s1 <= s2, -adv * r, 0.0)
    dmean = scale * dl[..., None] * z * inv
    wv = inp["wv"].astype(np.float64)
    v = y @ wv + float(inp["bv"])
    if value:
        lv, dlv, cut, bound, e1, e2 = (a.reshape(T, S) for a in A.value_loss(v.reshape(-1), f64("ret").reshape(-1), f64("v_old").reshape(-1), vclip))
        dv = scale * vf_coef * dlv
    else:
        lv = dv = e1 = e2 = np.zeros((T, S))
        cut = bound = np.zeros((T, S), bool)
    # backward
    gru = [np.asarray(a, np.float64) for a in inp["gru"]]
    W_hh, H = gru[1], case.H
    head = inp["head"]
    actd = (lambda h: 1.0 - h * h) if case.act == "tanh" else (lambda h: (h > 0.0).astype(np.float64))
    g_head = [[np.zeros(np.shape(W), np.float64), np.zeros(np.shape(b), np.float64)] for W, b in head]
    g_gru = [np.zeros_like(a) for a in gru]
    g_value = np.zeros(len(wv) + 1)
    carry = np.zeros((S, H))
    dh0 = None
    for k in range(T - 1, -1, -1):
        x, hin, h, (hs, pre, m, zsum) = steps[k]
        d = dmean[k] * ((1.0 - m * m) if case.out_tanh else 1.0)
        g_head[-1][0] += d.T @ hs[-1]
        g_head[-1][1] += d.sum(axis=0)
        g_value[:-1] += dv[k] @ hs[-1]
        g_value[-1] += dv[k].sum()
        d = d @ np.asarray(head[-1][0], np.float64) + dv[k][:, None] * wv[None, :]
        for l in range(len(head) - 2, -1, -1):
            d = d * actd(hs[l + 1])
            g_head[l][0] += d.T @ hs[l]
            g_head[l][1] += d.sum(axis=0)
            d = d @ np.asarray(head[l][0], np.float64)
        dh = d + carry
        rg, zg, n, n_h = gates64(inp["gru"], x, hin)
        da_n = dh * (1.0 - zg) * (1.0 - n * n)
        da_z = dh * (hin - n) * zg * (1.0 - zg)
        da_r = da_n * n_h * rg * (1.0 - rg)
        di, dhh = np.concatenate([da_r, da_z, da_n], axis=1), np.concatenate([da_r, da_z, da_n * rg], axis=1)
        g_gru[0] += di.T @ x
        g_gru[1] += dhh.T @ hin
        g_gru[2] += di.sum(axis=0)
        g_gru[3] += dhh.sum(axis=0)
        prev = dh * zg + dhh @ W_hh
        if k > 0:
            carry = np.where(done[t_lo + k - 1, s_lo:s_lo + S, None] != 0, 0.0, prev)
        else:
            dh0 = prev
    rows = T * S
    return dict(logp=logp, mean=mean, value=v, h_out=h_out, ratio=r, active=s1 <= s2, dv=dv, cut=cut, bound=bound, e1=e1, e2=e2,
                pre=[p for s in steps for p in s[3][1]], dh0=dh0,
                g_gru=g_gru, g_head=[tuple(g) for g in g_head], gvalue=g_value,
                glogstd=(scale * dl[..., None] * (z * z - 1.0)).sum(axis=(0, 1)) - ent_coef * scale * rows,
                stats=np.array([(-np.minimum(s1, s2)).sum(), float((s2 < s1).sum()), (r - 1.0 - xr).sum(), lv.sum(), float(cut.sum()),
                                float(rows)]))


def conditions(case, inp):
    """None if the inputs meet the conditions in the fp64 reference, else what fails: G's and A's (no relu pre-activation within 2e-5
    of 0; no ratio within 1e-4 of 1 +- CLIP; 10 % to 70 % of the ratios outside the clip range; both signs of advantage; no
    |V - v_old| within 1e-4 of vclip; where the clamp binds |e1^2 - e2^2| >= 1e-6 max; 10 % to 70 % of the rows cut when vclip > 0);
    the done pattern of every T >= 5 config; rows 0 and 64 carry a gradient at t = 0 and through at least one later step (active ratio
    at t = 0 and at some t >= 1 below every T >= 2 config's end, and a value delta where there is a head)"""
    ref = ppo_seq(case, inp, TMAX, SMAX)
    if case.act == "relu" and ref["pre"] and min(float(np.abs(v).min()) for v in ref["pre"]) < 2e-5:
        return "a relu pre-activation within 2e-5 of 0"
    r = ref["ratio"]
    if float(np.minimum(np.abs(r - (1.0 - CLIP)), np.abs(r - (1.0 + CLIP))).min()) < 1e-4:
        return "a ratio within 1e-4 of the clip range's edge"
    out = float(((r < 1.0 - CLIP) | (r > 1.0 + CLIP)).mean())
    if not 0.1 <= out <= 0.7:
        return "%.3f of the ratios outside the clip range" % out
    if not ((inp["adv"] > 0).any() and (inp["adv"] < 0).any()):
        return "one sign of advantage only"
    if case.value and case.vclip > 0.0:
        dvo = np.abs(ref["value"] - np.asarray(inp["v_old"], np.float64))
        if float(np.abs(dvo - case.vclip).min()) < 1e-4:
            return "a |V - v_old| within 1e-4 of vclip"
        a, b = ref["e1"][ref["bound"]] ** 2, ref["e2"][ref["bound"]] ** 2
        if a.size and float((np.abs(a - b) / np.maximum(a, b)).min()) < 1e-6:
            return "e1^2 and e2^2 within 1e-6 relative"
        frac = float(ref["cut"].mean())
        if not 0.1 <= frac <= 0.7:
            return "%.3f of the rows' value gradients cut" % frac
    for T, S in CONFIGS:
        if T >= 5:
            bad = done_conditions(inp["done"], T, S)
            if bad:
                return bad
    for s in (0, 64):
        if not (ref["active"][0, s] and ref["active"][1, s]):
            return "row %d has no policy gradient at t = 0 or t = 1" % s
        if case.value and (ref["dv"][0, s] == 0.0 or ref["dv"][1, s] == 0.0):
            return "row %d has no value delta at t = 0 or t = 1" % s
    return None


def tensors(ref):
    """the reference's gradient tensors in the order the bounds name them: W_ih, b_ih, W_hh, b_hh, then (W, b) of every head layer"""
    g = ref["g_gru"]
    return [g[0], g[2], g[1], g[3]] + [a for Wb in ref["g_head"] for a in Wb]


def grad_errors(got_gru, got_head, got_value, got_logstd, ref):
    """G.rel of every parameter tensor (W_ih, b_ih, W_hh, b_hh, the head's W and b), then grad_value (if any) and grad_log_std.
    got_gru = (W_ih, W_hh, b_ih, b_hh) as unpack_gru_weights returns them.  A tensor whose reference is exactly 0 must be exactly 0."""
    got = [got_gru[0], got_gru[2], got_gru[1], got_gru[3]] + [a for Wb in got_head for a in Wb]
    errs = []
    for a, b in zip(got, tensors(ref)):
        errs.append(G.rel(a, b) if np.abs(b).max() > 0 else float(np.abs(np.asarray(a)).max()))
    if got_value is not None:
        errs.append(G.rel(got_value, ref["gvalue"]))
    errs.append(G.rel(got_logstd, ref["glogstd"]))
    return errs


def torch_model(case, inp, dtype):
    """the twin module: (GRUCell, [Linear ...] of the head, value Linear, log_std)"""
    import torch
    import torch.nn as nn
    cell = nn.GRUCell(case.D, case.H)
    W_ih, W_hh, b_ih, b_hh = inp["gru"]
    cell.weight_ih.data, cell.weight_hh.data = torch.tensor(W_ih), torch.tensor(W_hh)
    cell.bias_ih.data, cell.bias_hh.data = torch.tensor(b_ih), torch.tensor(b_hh)
    lins = []
    for W, b in inp["head"]:
        lin = nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data, lin.bias.data = torch.tensor(W), torch.tensor(b)
        lins.append(lin)
    critic = nn.Linear(len(inp["wv"]), 1)
    critic.weight.data, critic.bias.data = torch.tensor(inp["wv"][None, :]), torch.tensor(np.asarray(inp["bv"]).reshape(1))
    for m in [cell, critic] + lins:
        m.to(dtype)
    return cell, lins, critic, torch.tensor(LOG_STD, dtype=dtype, requires_grad=True)


def torch_loss(case, tens, T, S, model, scale=None, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF):
    """the combined loss through torch ops: tens = dict of tensors x, actions, done, h0, logp_old, adv, ret, v_old cut to [T, S];
    returns (scale * sum L, logp, V, sum L_clip, sum k3, sum L_V)"""
    import torch
    cell, lins, critic, log_std = model
    scale = 1.0 / (T * S) if scale is None else scale
    h = tens["h0"]
    means, vs = [], []
    for t in range(T):
        if t > 0:
            h = torch.where(tens["done"][t - 1][:, None] != 0, torch.zeros_like(h), h)
        h = cell(tens["x"][t], h)
        y = h
        for lin in lins[:-1]:
            y = lin(y)
            y = torch.tanh(y) if case.act == "tanh" else torch.relu(y)
        m = lins[-1](y)
        means.append(torch.tanh(m) if case.out_tanh else m)
        vs.append(critic(y)[:, 0])
    mean, v = torch.stack(means), torch.stack(vs)
    z = (tens["actions"] - mean) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std).sum(dim=2) - G.TWO_LN_2PI
    xr = logp - tens["logp_old"]
    r, adv = torch.exp(xr), tens["adv"]
    lclip = -torch.minimum(r * adv, torch.clamp(r, 1.0 - clip, 1.0 + clip) * adv)
    if case.value:
        e1 = v - tens["ret"]
        if case.vclip > 0.0:
            e2 = tens["v_old"] + torch.clamp(v - tens["v_old"], -case.vclip, case.vclip) - tens["ret"]
            lv = 0.5 * torch.maximum(e1 * e1, e2 * e2)
        else:
            lv = 0.5 * e1 * e1
    else:
        lv = torch.zeros_like(v)
    ent = (log_std + 0.5 * (1.0 + np.log(2.0 * np.pi))).sum()
    loss = scale * (lclip.sum() + vf_coef * lv.sum() - ent_coef * ent * T * S)
    return loss, logp, v, lclip.sum(), (r - 1.0 - xr).sum(), lv.sum()


def torch_tensors(inp, T, S, dtype, device="cpu"):
    import torch
    out = {k: torch.tensor(inp[k][:T, :S], dtype=dtype, device=device) for k in ("x", "actions", "logp_old", "adv", "ret", "v_old")}
    out["done"] = torch.tensor(inp["done"][:T, :S], device=device)
    out["h0"] = torch.tensor(inp["h0"][:S], dtype=dtype, device=device)
    return out


def torch_grads(case, model):
    """the module's gradients as grad_errors takes them: (gru 4-tuple, head [(W, b)], grad_value or None, grad_log_std)"""
    cell, lins, critic, log_std = model
    n = lambda p: p.grad.detach().cpu().numpy()
    gv = np.concatenate([n(critic.weight).reshape(-1), n(critic.bias).reshape(-1)]) if case.value else None
    return ((n(cell.weight_ih), n(cell.weight_hh), n(cell.bias_ih), n(cell.bias_hh)), [(n(l.weight), n(l.bias)) for l in lins], gv, n(log_std))


def torch_errors(case, inp, T, S, dtype, each=False):
    """torch autograd of `dtype` on the CPU against the reference: (gradient, logp, V, sum L_clip, sum k3, sum L_V); each: the gradient's
    entry is the list of every tensor's error"""
    ref = ppo_seq(case, inp, T, S)
    model = torch_model(case, inp, dtype)
    loss, lp, v, lsum, kl, lvsum = torch_loss(case, torch_tensors(inp, T, S, dtype), T, S, model)
    loss.backward()
    errs = grad_errors(*torch_grads(case, model), ref)
    f = lambda a: float(a.detach())
    return (errs if each else max(errs), G.rel(lp.detach().numpy(), ref["logp"]), G.rel(v.detach().numpy(), ref["value"]),
            G.rel(f(lsum), ref["stats"][0]), G.rel(f(kl), ref["stats"][2]), G.rel(f(lvsum), ref["stats"][3]) if case.value else 0.0)


def find_seed(case, limit=4000):
    for seed in range(limit):
        if conditions(case, inputs(case, seed)) is None:
            return seed
    raise RuntimeError("no seed below %d meets the conditions of %s" % (limit, case.name))


# the seed of each case: the first that meets conditions() (python -m tests.policy_grad_seq_ref)
SEEDS = {
    'gru16-tanh': 0,
    'gru16-tanh-vclip': 2,
    'gru16-relu': 0,
    'gru16-relu-vclip': 2,
    'gru48x32-tanh': 1,
    'gru48x32-tanh-vclip': 1,
    'gru48x32-relu': 21,
    'gru48x32-relu-vclip': 23,
    'gru64x16x48-tanh': 0,
    'gru64x16x48-tanh-vclip': 20,
    'gru64x16x48-relu': 59,
    'gru64x16x48-relu-vclip': 154,
    'gru64x64x64-tanh': 0,
    'gru64x64x64-tanh-vclip': 49,
    'gru64x64x64-relu': 54,
    'gru64x64x64-relu-vclip': 2572,
    'gru64x16x48-tanh-d19': 3,
    'gru64x16x48-tanh-d19-vclip': 55,
    'gru48x32-relu-norm': 1,
    'gru48x32-relu-norm-vclip': 1,
    'gru16-tanh-nohead': 0,
    'gru64x64x64-relu-nohead': 54,
}

# per case and (T, S): torch fp32 autograd's (gradient, logp, V, sum L_clip, sum k3, sum L_V) errors against the reference
# (python -m tests.policy_grad_seq_ref; torch on the CPU)
BASELINE = {
    'gru16-tanh': {(1, 1): (9.49e-07, 5.53e-08, 1.52e-07, 2.6e-08, 8.25e-06, 1.87e-06), (1, 65): (7.59e-07, 1.17e-07, 1.59e-07, 6.11e-08, 1.97e-07, 2.64e-08), (2, 63): (7.77e-07, 1e-07, 1.35e-07, 2.16e-07, 2.48e-07, 2.95e-08), (5, 64): (4.28e-07, 1.62e-07, 1.58e-07, 2.61e-06, 1.76e-08, 4.58e-08), (5, 65): (5.01e-07, 1.62e-07, 1.58e-07, 3.34e-06, 4.29e-08, 4.07e-09), (6, 130): (4.88e-07, 1.62e-07, 1.27e-07, 4.83e-08, 7.75e-08, 1.03e-07)},
    'gru16-tanh-vclip': {(1, 1): (6.65e-07, 5.2e-08, 3.42e-07, 1.34e-07, 6.98e-07, 1.34e-06), (1, 65): (4.33e-07, 1.05e-07, 1.41e-07, 8.31e-08, 3.5e-07, 8.8e-08), (2, 63): (4.62e-07, 9.66e-08, 1.7e-07, 1.03e-06, 4.48e-07, 2.63e-08), (5, 64): (8.75e-07, 9.66e-08, 1.7e-07, 8.36e-08, 2.38e-07, 4.41e-08), (5, 65): (6.93e-07, 9.66e-08, 1.7e-07, 1.79e-07, 1.55e-07, 5.39e-08), (6, 130): (4.33e-07, 1.39e-07, 1.32e-07, 2.21e-07, 3.48e-08, 2.33e-08)},
    'gru16-relu': {(1, 1): (9.49e-07, 2.85e-08, 1.52e-07, 2.02e-08, 7.13e-06, 1.87e-06), (1, 65): (6.49e-07, 1.36e-07, 1.59e-07, 5.37e-07, 2.79e-08, 2.64e-08), (2, 63): (1.05e-06, 1.17e-07, 1.35e-07, 2.24e-07, 1.89e-07, 2.95e-08), (5, 64): (4.83e-07, 1e-07, 1.58e-07, 3.5e-06, 4.57e-08, 4.58e-08), (5, 65): (5.34e-07, 1e-07, 1.58e-07, 9.41e-06, 6.02e-09, 4.07e-09), (6, 130): (4.59e-07, 1e-07, 1.27e-07, 1.18e-07, 5.07e-08, 1.03e-07)},
    'gru16-relu-vclip': {(1, 1): (6.65e-07, 6.01e-08, 3.42e-07, 1.48e-07, 5.53e-07, 1.34e-06), (1, 65): (7.45e-07, 1.32e-07, 1.41e-07, 1.76e-07, 2.63e-07, 8.8e-08), (2, 63): (6.66e-07, 1.23e-07, 1.7e-07, 1.61e-06, 7.75e-07, 2.63e-08), (5, 64): (1.31e-06, 1.55e-07, 1.7e-07, 4.69e-08, 3.81e-07, 4.41e-08), (5, 65): (1.61e-06, 1.55e-07, 1.7e-07, 1.91e-07, 3.6e-07, 5.39e-08), (6, 130): (1.17e-06, 1.55e-07, 1.32e-07, 9.88e-08, 6.08e-08, 2.33e-08)},
    'gru48x32-tanh': {(1, 1): (3.83e-07, 8.59e-08, 1.91e-07, 1.53e-07, 7.94e-08, 9.28e-08), (1, 65): (5.03e-07, 1.68e-07, 1.68e-07, 1.54e-07, 1.38e-07, 4.16e-08), (2, 63): (1.09e-06, 1.52e-07, 1.95e-07, 2.75e-06, 3.01e-07, 3.29e-08), (5, 64): (1.21e-06, 1.52e-07, 2.16e-07, 1e-06, 1.14e-07, 1.06e-07), (5, 65): (1.46e-06, 1.52e-07, 2.16e-07, 5.06e-06, 2.09e-07, 2.29e-09), (6, 130): (9.42e-07, 1.57e-07, 2.39e-07, 1.16e-06, 1.38e-07, 1.35e-08)},
    'gru48x32-tanh-vclip': {(1, 1): (3.83e-07, 8.59e-08, 1.91e-07, 1.53e-07, 7.94e-08, 9.28e-08), (1, 65): (5.03e-07, 1.68e-07, 1.68e-07, 1.54e-07, 1.38e-07, 6.07e-08), (2, 63): (1.09e-06, 1.52e-07, 1.95e-07, 2.75e-06, 3.01e-07, 8.73e-09), (5, 64): (1.21e-06, 1.52e-07, 2.16e-07, 1e-06, 1.14e-07, 2.88e-08), (5, 65): (1.46e-06, 1.52e-07, 2.16e-07, 5.06e-06, 2.09e-07, 2.3e-08), (6, 130): (9.42e-07, 1.57e-07, 2.39e-07, 1.16e-06, 1.38e-07, 1.02e-08)},
    'gru48x32-relu': {(1, 1): (5.17e-07, 3.98e-09, 3.66e-07, 7.63e-09, 4.19e-07, 3.5e-07), (1, 65): (8.49e-07, 7.92e-08, 2.27e-07, 4.35e-07, 1.71e-07, 2.13e-08), (2, 63): (8.41e-07, 9.3e-08, 2.27e-07, 7.24e-07, 1.93e-07, 8.18e-09), (5, 64): (8.27e-07, 1.35e-07, 2.33e-07, 3.81e-07, 1.73e-07, 2.41e-08), (5, 65): (8.28e-07, 1.35e-07, 2.33e-07, 4.94e-07, 1.31e-07, 4.36e-08), (6, 130): (9.91e-07, 1.48e-07, 1.91e-07, 9.7e-08, 4.43e-08, 6.05e-08)},
    'gru48x32-relu-vclip': {(1, 1): (2.95e-07, 3.12e-08, 5.87e-08, 1.57e-07, 1.03e-05, 7.12e-08), (1, 65): (7.35e-07, 6.84e-08, 2.3e-07, 1.16e-07, 1.68e-07, 5.22e-08), (2, 63): (6.53e-07, 1.02e-07, 2.7e-07, 1.11e-07, 2.18e-08, 1.02e-07), (5, 64): (7.84e-07, 1.38e-07, 2.71e-07, 1.96e-07, 9.66e-08, 8.14e-08), (5, 65): (7.05e-07, 1.38e-07, 2.71e-07, 6.94e-08, 9.07e-08, 8.48e-08), (6, 130): (6.17e-07, 1.27e-07, 3.22e-07, 6.29e-07, 6.45e-08, 1.51e-08)},
    'gru64x16x48-tanh': {(1, 1): (1.07e-06, 5.27e-08, 1.76e-07, 1.06e-07, 7.17e-05, 2.17e-06), (1, 65): (9.82e-07, 1.53e-07, 1.44e-07, 7.18e-07, 6.59e-07, 4.24e-08), (2, 63): (7.88e-07, 1.53e-07, 2.12e-07, 2.81e-06, 4.37e-07, 6.37e-08), (5, 64): (9.4e-07, 1.36e-07, 2.41e-07, 7.45e-07, 1.94e-07, 1.14e-07), (5, 65): (9.06e-07, 1.36e-07, 2.41e-07, 7.76e-07, 1.03e-07, 4.18e-09), (6, 130): (8.11e-07, 1.16e-07, 2.41e-07, 8.79e-07, 5.82e-08, 5.99e-08)},
    'gru64x16x48-tanh-vclip': {(1, 1): (2.97e-07, 1.3e-08, 7.34e-07, 1.06e-07, 1.67e-06, 1.32e-07), (1, 65): (5.47e-07, 1.24e-07, 1.64e-07, 0.000119, 5.59e-07, 1.83e-08), (2, 63): (1.3e-06, 1.97e-07, 2.18e-07, 2.49e-06, 5.08e-07, 3e-08), (5, 64): (1.79e-06, 1.62e-07, 2.14e-07, 3.38e-06, 1.24e-07, 4.94e-09), (5, 65): (1.19e-06, 1.62e-07, 2.14e-07, 4.62e-06, 1.41e-07, 9.88e-08), (6, 130): (1.23e-06, 1.56e-07, 2.4e-07, 5.45e-07, 8.62e-08, 2.32e-08)},
    'gru64x16x48-relu': {(1, 1): (6.46e-07, 7.21e-08, 1.45e-07, 2.71e-07, 4.27e-06, 1.42e-06), (1, 65): (1.05e-06, 5.8e-08, 2.44e-07, 5.01e-05, 2.4e-07, 1.33e-08), (2, 63): (6.21e-07, 1.12e-07, 2.22e-07, 5.5e-07, 2.84e-07, 1.99e-08), (5, 64): (6.34e-07, 1.35e-07, 2.08e-07, 1.8e-07, 1.85e-07, 1.1e-08), (5, 65): (5.07e-07, 1.35e-07, 2.08e-07, 3.64e-07, 3.1e-07, 6.76e-08), (6, 130): (9.71e-07, 1.35e-07, 2.57e-07, 6.44e-07, 1.79e-07, 6.67e-08)},
    'gru64x16x48-relu-vclip': {(1, 1): (5.49e-07, 8.13e-08, 5.59e-08, 3.54e-07, 0.000318, 4.19e-07), (1, 65): (6.39e-07, 1.53e-07, 2.14e-07, 2.69e-07, 6.55e-07, 7.38e-08), (2, 63): (6.11e-07, 1.44e-07, 1.84e-07, 1.76e-07, 1.66e-07, 5.48e-08), (5, 64): (7.16e-07, 1.14e-07, 1.96e-07, 3.79e-07, 2.19e-07, 2.02e-08), (5, 65): (7.79e-07, 1.14e-07, 1.96e-07, 5.98e-07, 1.55e-07, 2.01e-08), (6, 130): (9.1e-07, 1.71e-07, 2.31e-07, 2.22e-07, 1.33e-08, 3.98e-09)},
    'gru64x64x64-tanh': {(1, 1): (3.7e-07, 9.59e-08, 3.05e-07, 2.29e-07, 2.06e-06, 3.97e-07), (1, 65): (8.68e-07, 1.36e-07, 2.13e-07, 1.28e-07, 3.5e-07, 6.78e-08), (2, 63): (1.01e-06, 1.36e-07, 2.21e-07, 1.45e-07, 2.92e-07, 5.62e-08), (5, 64): (9.66e-07, 1.69e-07, 3.03e-07, 3.73e-07, 6.71e-08, 3.28e-09), (5, 65): (9.65e-07, 1.69e-07, 3.03e-07, 5.78e-08, 6.78e-08, 6.39e-08), (6, 130): (6.03e-07, 1.86e-07, 2.99e-07, 6.65e-07, 6.25e-08, 4.22e-08)},
    'gru64x64x64-tanh-vclip': {(1, 1): (5.06e-07, 8.65e-08, 1.26e-07, 2.11e-07, 8.86e-07, 4.03e-07), (1, 65): (6.21e-07, 1.36e-07, 3e-07, 1.35e-07, 3.3e-07, 6.84e-09), (2, 63): (6.76e-07, 1.36e-07, 2.46e-07, 1.1e-07, 3.51e-07, 1.05e-07), (5, 64): (5.74e-07, 1.36e-07, 2.75e-07, 9.23e-08, 2.81e-07, 4.99e-08), (5, 65): (9.35e-07, 1.36e-07, 2.75e-07, 1.92e-08, 2.06e-07, 4.12e-09), (6, 130): (6.92e-07, 1.24e-07, 2.75e-07, 1.8e-08, 2.23e-07, 6.7e-08)},
    'gru64x64x64-relu': {(1, 1): (1.17e-06, 9.47e-09, 1.2e-07, 2.17e-08, 0.000471, 2.23e-06), (1, 65): (4.7e-07, 1.32e-07, 2.25e-07, 7.68e-09, 4.88e-07, 1.45e-07), (2, 63): (6.28e-07, 1.27e-07, 2.44e-07, 1.58e-07, 3.12e-07, 5.1e-08), (5, 64): (6.33e-07, 1.26e-07, 3.13e-07, 7.4e-08, 2.64e-07, 5.01e-08), (5, 65): (6.59e-07, 1.26e-07, 3.13e-07, 7.89e-08, 2.57e-07, 1.03e-07), (6, 130): (9.48e-07, 1.76e-07, 3.7e-07, 1.75e-07, 6.86e-08, 6.88e-08)},
    'gru64x64x64-relu-vclip': {(1, 1): (3.73e-07, 5.04e-08, 2.55e-07, 2.03e-07, 5.85e-07, 7.57e-07), (1, 65): (5.11e-07, 9.12e-08, 1.87e-07, 2.38e-08, 1.93e-07, 4.13e-08), (2, 63): (1.41e-06, 1.52e-07, 2.03e-07, 5.78e-07, 4.97e-08, 1.03e-07), (5, 64): (7.16e-07, 1.52e-07, 3.01e-07, 5.51e-06, 3.08e-08, 4.72e-08), (5, 65): (7.47e-07, 1.52e-07, 3.01e-07, 5.71e-07, 4.52e-11, 3.25e-08), (6, 130): (9.87e-07, 1.52e-07, 3.09e-07, 2.27e-07, 1.03e-08, 2.63e-08)},
    'gru64x16x48-tanh-d19': {(1, 1): (5.03e-07, 4.6e-08, 1.47e-07, 1.31e-07, 0.000397, 9.77e-07), (1, 65): (5.41e-07, 1.7e-07, 1.85e-07, 1.08e-07, 2.87e-08, 6.77e-08), (2, 63): (4.68e-07, 1.46e-07, 2.76e-07, 1.87e-07, 1.89e-07, 4.56e-08), (5, 64): (6.22e-07, 1.49e-07, 3.08e-07, 9.28e-08, 2.49e-07, 2.9e-08), (5, 65): (7.39e-07, 1.49e-07, 3.08e-07, 9e-08, 1.71e-07, 5.02e-08), (6, 130): (1.68e-06, 1.11e-07, 3.17e-07, 2.49e-07, 5.36e-08, 7.76e-08)},
    'gru64x16x48-tanh-d19-vclip': {(1, 1): (1.72e-06, 5.36e-08, 1.27e-06, 2.8e-07, 1.09e-06, 3.4e-06), (1, 65): (1.03e-06, 1.06e-07, 2.31e-07, 1.11e-07, 5.94e-07, 1.62e-08), (2, 63): (1.15e-06, 8.69e-08, 2.1e-07, 6.69e-08, 3e-07, 3.15e-10), (5, 64): (2.12e-06, 8.81e-08, 2.41e-07, 1.81e-06, 4.82e-08, 3.8e-08), (5, 65): (1.49e-06, 8.81e-08, 2.41e-07, 1.11e-06, 7.52e-08, 8.07e-09), (6, 130): (8.63e-07, 1.82e-07, 2.39e-07, 5.78e-07, 1.1e-07, 9.62e-08)},
    'gru48x32-relu-norm': {(1, 1): (2.72e-07, 2.86e-08, 4.04e-07, 5.76e-08, 1.92e-07, 8.45e-08), (1, 65): (7.57e-07, 1.62e-07, 2.39e-07, 2.16e-07, 5.67e-07, 1.81e-08), (2, 63): (1.65e-06, 1.47e-07, 3.03e-07, 9.02e-07, 4.33e-07, 2.68e-08), (5, 64): (7.31e-07, 1.8e-07, 2.52e-07, 1.99e-08, 5.4e-08, 1.31e-09), (5, 65): (9.08e-07, 1.8e-07, 2.52e-07, 1.32e-06, 8.01e-08, 3.1e-09), (6, 130): (7.76e-07, 1.7e-07, 4.22e-07, 5.18e-06, 1.05e-07, 1.37e-08)},
    'gru48x32-relu-norm-vclip': {(1, 1): (2.72e-07, 2.86e-08, 4.04e-07, 5.76e-08, 1.92e-07, 8.45e-08), (1, 65): (7.68e-07, 1.62e-07, 2.39e-07, 2.16e-07, 5.67e-07, 6.47e-08), (2, 63): (1.65e-06, 1.47e-07, 3.03e-07, 9.02e-07, 4.33e-07, 9.71e-08), (5, 64): (7.59e-07, 1.8e-07, 2.52e-07, 1.99e-08, 5.4e-08, 2.9e-08), (5, 65): (9.08e-07, 1.8e-07, 2.52e-07, 1.32e-06, 8.01e-08, 6.4e-08), (6, 130): (6.79e-07, 1.7e-07, 4.22e-07, 5.18e-06, 1.05e-07, 8.88e-09)},
    'gru16-tanh-nohead': {(1, 1): (1.66e-07, 5.53e-08, 1.52e-07, 2.6e-08, 8.25e-06, 0), (1, 65): (8.08e-07, 1.17e-07, 1.59e-07, 6.11e-08, 1.97e-07, 0), (2, 63): (7.77e-07, 1e-07, 1.35e-07, 2.16e-07, 2.48e-07, 0), (5, 64): (4.34e-07, 1.62e-07, 1.58e-07, 2.61e-06, 1.76e-08, 0), (5, 65): (4.98e-07, 1.62e-07, 1.58e-07, 3.34e-06, 4.29e-08, 0), (6, 130): (4.52e-07, 1.62e-07, 1.27e-07, 4.83e-08, 7.75e-08, 0)},
    'gru64x64x64-relu-nohead': {(1, 1): (3.15e-07, 9.47e-09, 1.2e-07, 2.17e-08, 0.000471, 0), (1, 65): (3.95e-07, 1.32e-07, 2.25e-07, 7.68e-09, 4.88e-07, 0), (2, 63): (6.85e-07, 1.27e-07, 2.44e-07, 1.58e-07, 3.12e-07, 0), (5, 64): (6.33e-07, 1.26e-07, 3.13e-07, 7.4e-08, 2.64e-07, 0), (5, 65): (8.63e-07, 1.26e-07, 3.13e-07, 7.89e-08, 2.57e-07, 0), (6, 130): (9.48e-07, 1.76e-07, 3.7e-07, 1.75e-07, 6.86e-08, 0)},
}

_INPUTS = {}


def case_inputs(name):
    """the case and its inputs at its seed, computed once and shared: treat them as read-only"""
    if name not in _INPUTS:
        _INPUTS[name] = inputs(CASES[name], SEEDS[name])
    return CASES[name], _INPUTS[name]


_REFS = {}


def case_ref(name, T, S):
    """ppo_seq of the case at its defaults on the prefix (T, S), computed once and shared: read-only"""
    if (name, T, S) not in _REFS:
        case, inp = case_inputs(name)
        _REFS[name, T, S] = ppo_seq(case, inp, T, S)
    return _REFS[name, T, S]


def bounds(name, T, S):
    """The device's bounds for the case at (T, S), FACTOR x torch fp32's errors: (gradient, logp, V, sum L_clip, sum k3, sum L_V).  As in
    A.bounds: the gradient's is the case's own at that size, and so are logp's and V's at more than one row; the true scalars -- the
    three sums at every size, logp and V at (1, 1) -- take the largest torch error over the cases at that size."""
    pooled = [max(BASELINE[c.name][T, S][k] for c in SEQ_CASES) for k in range(1, 6)]
    own = BASELINE[name][T, S]
    one = T * S == 1
    return (FACTOR * own[0], FACTOR * (pooled[0] if one else own[1]), FACTOR * (pooled[1] if one else own[2]),
            FACTOR * pooled[2], FACTOR * pooled[3], FACTOR * pooled[4])


if __name__ == "__main__":
    import torch
    seeds = {c.name: find_seed(c) for c in SEQ_CASES}
    print("SEEDS = {")
    for k, v in seeds.items():
        print("    %r: %d," % (k, v))
    print("}\n\nBASELINE = {")
    for c in SEQ_CASES:
        inp = inputs(c, seeds[c.name])
        print("    %r: {%s}," % (c.name, ", ".join("(%d, %d): (%s)" % (T, S, ", ".join("%.3g" % e for e in torch_errors(c, inp, T, S, torch.float32)))
                                                   for T, S in CONFIGS)))
    print("}")
