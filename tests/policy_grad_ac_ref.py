"""An fp64 restatement of the shared-trunk actor-critic gradient (gaq.h gaq_policy_eval_ac_dev, gaq_policy_grad_ppo_ac_dev) on fp32
inputs -- manual backprop through the trunk with both heads' deltas, in NumPy -- with the cases, the inputs and the bounds the CPU and
GPU tests share.  It extends tests/policy_grad_ref.py (G below): the nets, the observations, the actions, logp_old and the advantages
of a case are G.inputs' of the same net at this module's seed.

Loss per row: L = L_clip + VF_COEF * L_V - ENT_COEF * H, times scale, summed over the rows.  L_clip is G.ppo's surrogate.  With
e1 = V - ret: L_V = e1^2 / 2 when vclip == 0; when vclip > 0, c = clamp(V - v_old, +-vclip), e2 = e1 where the clamp does not bind
(c == V - v_old: the two errors are then the same number, a tie, and ties take e1) and v_old + c - ret where it does,
L_V = max(e1^2, e2^2) / 2 and dL_V/dV = e1 if e1^2 >= e2^2 else 0.  H = sum_k log_std_k + 2 (1 + ln 2 pi): state-independent, so its only
gradient is -ENT_COEF * scale * rows on every component of grad_log_std.

Cases: four hidden shapes x (tanh + output tanh, relu without), one net on a 19-wide observation and one behind the exact-table
normaliser of G's -norm case, each with vclip = 0 and vclip = 0.2; R = 453 rows, the smaller row counts are prefixes.

Inputs besides G.inputs', from RandomState(seed + 2000): a value head w ~ N(0, 1 / W), b; ret = V + 0.5 n and v_old = V + 0.25 n around
the reference's V.  The seed of each case (SEEDS) was searched on the CPU (`python -m tests.policy_grad_ac_ref`) so that conditions()
holds in the fp64 reference.

Bounds: BASELINE holds, per case and row count, torch fp32 autograd's error on the CPU against this reference on the same inputs:
(gradient, logp, V, sum L_clip, sum k3, sum L_V), each max|v - v64| / max|v64|, the gradient's the largest over the parameter tensors,
grad_value (one tensor of W + 1) and grad_log_std.  The device's bound is G.FACTOR = 8 x that, for the reason G states (bounds())."""
import numpy as np

from tests import policy_grad_ref as G

R, ROWS, CLIP, LOG_STD, FACTOR = G.R, G.ROWS, G.CLIP, G.LOG_STD, G.FACTOR
VF_COEF, ENT_COEF, VCLIP = 0.5, 0.01, 0.2
NETS = [[16], [64, 64], [48, 80, 32], [128, 128, 128]]


class AcCase:
    """a net of G's (policy, 4 outputs) with a value head, and the value clip of the call"""

    def __init__(self, widths, act, out_tanh, D=18, norm=False, vclip=0.0):
        self.net, self.vclip = G.Case(widths, act, out_tanh, D=D, norm=norm), float(vclip)
        self.widths, self.act, self.out_tanh, self.D, self.norm = self.net.widths, act, bool(out_tanh), D, norm
        self.name = "ac" + self.net.name[len("policy"):] + ("-vclip" if vclip > 0 else "")

    def __repr__(self):
        return self.name


_NETS = [(w, a, t, 18, False) for w in NETS for a, t in G.STYLES] + [([64, 64], "tanh", True, 19, False), ([64, 64], "relu", False, 18, True)]
AC_CASES = [AcCase(w, a, t, D=D, norm=nm, vclip=vc) for w, a, t, D, nm in _NETS for vc in (0.0, VCLIP)]
CASES = {c.name: c for c in AC_CASES}


def inputs(case, seed):
    """G.inputs of the net at `seed`, plus the value head (wv [W], bv), ret and v_old [R]"""
    inp = G.inputs(case.net, seed)
    rng = np.random.RandomState(seed + 2000)
    W = case.widths[-1]
    inp["wv"] = (rng.randn(W) / np.sqrt(W)).astype(np.float32)
    inp["bv"] = np.float32(0.1 * rng.randn())
    hs = G.forward(inp["layers"], case.act, case.out_tanh, inp["x"])[0]
    v = hs[-1] @ inp["wv"].astype(np.float64) + float(inp["bv"])
    inp["ret"] = (v + 0.5 * rng.randn(R)).astype(np.float32)
    inp["v_old"] = (v + 0.25 * rng.randn(R)).astype(np.float32)
    return inp


def value_loss(v, ret, v_old, vclip):
    """fp64: (L_V, dL_V/dV, cut, the rows where the clamp binds, e1, e2) per row"""
    e1 = v - ret
    if vclip <= 0.0:
        return 0.5 * e1 * e1, e1, np.zeros(len(v), bool), np.zeros(len(v), bool), e1, e1
    dvo = v - v_old
    c = np.clip(dvo, -vclip, vclip)
    bound = c != dvo
    e2 = np.where(bound, v_old + c - ret, e1)
    cut = ~(e1 * e1 >= e2 * e2)
    return 0.5 * np.maximum(e1 * e1, e2 * e2), np.where(cut, 0.0, e1), cut, bound, e1, e2


def backward_ac(layers, act, out_tanh, hs, mean, dmean, wv, dv):
    """dmean [rows, 4] and dv [rows]: the gradients with respect to the mean and to V -> ([(dW, db), ...], (dwv, dbv)), summed over
    the rows; the two deltas meet in the last hidden layer"""
    actd = (lambda h: 1.0 - h * h) if act == "tanh" else (lambda h: (h > 0.0).astype(np.float64))
    d = np.asarray(dmean, np.float64) * ((1.0 - mean * mean) if out_tanh else 1.0)
    y = hs[-1]
    grads = [(d.T @ y, d.sum(axis=0))]
    gvalue = (dv @ y, dv.sum())
    d = (d @ np.asarray(layers[-1][0], np.float64) + dv[:, None] * np.asarray(wv, np.float64)[None, :]) * actd(y)
    for l in range(len(layers) - 2, -1, -1):
        grads.append((d.T @ hs[l], d.sum(axis=0)))
        if l:
            d = (d @ np.asarray(layers[l][0], np.float64)) * actd(hs[l])
    return grads[::-1], gvalue


def ppo_ac(case, inp, rows, scale=None, clip=CLIP, vclip=None, vf_coef=VF_COEF, ent_coef=ENT_COEF, lo=0):
    """the fp64 reference of gaq_policy_grad_ppo_ac_dev on the rows [lo, lo + rows)"""
    scale = 1.0 / rows if scale is None else scale
    vclip = case.vclip if vclip is None else vclip
    sl = slice(lo, lo + rows)
    f64 = lambda k: np.asarray(inp[k][sl], np.float64)
    hs, pre, mean, zsum = G.forward(inp["layers"], case.act, case.out_tanh, inp["x"][sl])
    inv = np.exp(-LOG_STD.astype(np.float64))
    z = (f64("actions") - mean) * inv
    logp = (-0.5 * z * z - LOG_STD).sum(axis=1) - G.TWO_LN_2PI
    xr = logp - f64("logp_old")
    r, adv = np.exp(xr), f64("adv")
    s1, s2 = r * adv, np.clip(r, 1.0 - clip, 1.0 + clip) * adv
    dl = np.where(s1 <= s2, -adv * r, 0.0)
    dmean = scale * dl[:, None] * z * inv
    v = hs[-1] @ inp["wv"].astype(np.float64) + float(inp["bv"])
    lv, dlv, cut, bound, e1, e2 = value_loss(v, f64("ret"), f64("v_old"), vclip)
    dv = scale * vf_coef * dlv
    grads, gvalue = backward_ac(inp["layers"], case.act, case.out_tanh, hs, mean, dmean, inp["wv"], dv)
    return dict(logp=logp, mean=mean, value=v, ratio=r, active=s1 <= s2, dv=dv, cut=cut, bound=bound, e1=e1, e2=e2, pre=pre, zsum=zsum,
                grads=grads, gvalue=np.concatenate([gvalue[0], [gvalue[1]]]),
                glogstd=(scale * dl[:, None] * (z * z - 1.0)).sum(axis=0) - ent_coef * scale * rows,
                stats=np.array([(-np.minimum(s1, s2)).sum(), float((s2 < s1).sum()), (r - 1.0 - xr).sum(), lv.sum(), float(cut.sum()),
                                float(rows)]))


def conditions(case, inp):
    """None if the inputs meet the conditions in the fp64 reference, else what fails: G.conditions of the net (relu pre-activations,
    ratios off the clip range's edges, 10 % to 70 % of them outside, both signs of advantage, no saturation, rows 0 and 64 active); no
    |V - v_old| within 1e-4 of vclip; where the clamp binds, |e1^2 - e2^2| >= 1e-6 max(e1^2, e2^2) (where it does not, e2 is e1 by
    definition) -- the fp32 and fp64 branches then agree; 10 % to 70 % of the rows cut when vclip > 0; rows 0 and 64 have a value delta"""
    bad = G.conditions(case.net, inp)
    if bad is not None:
        return bad
    ref = ppo_ac(case, inp, R)
    if case.vclip > 0.0:
        dvo = np.abs(ref["value"] - np.asarray(inp["v_old"], np.float64))
        if float(np.abs(dvo - case.vclip).min()) < 1e-4:
            return "a |V - v_old| within 1e-4 of vclip"
        a, b = ref["e1"][ref["bound"]] ** 2, ref["e2"][ref["bound"]] ** 2
        if a.size and float((np.abs(a - b) / np.maximum(a, b)).min()) < 1e-6:
            return "e1^2 and e2^2 within 1e-6 relative"
        frac = float(ref["cut"].mean())
        if not 0.1 <= frac <= 0.7:
            return "%.3f of the rows' value gradients cut" % frac
    if ref["dv"][0] == 0.0 or ref["dv"][64] == 0.0:
        return "row 0 or row 64 has no value delta"
    return None


def grad_errors(got_layers, got_value, got_logstd, ref):
    """G.grad_errors' metric of every parameter tensor, then grad_value (one tensor) and grad_log_std"""
    return G.grad_errors(got_layers, None, ref) + [G.rel(got_value, ref["gvalue"]), G.rel(got_logstd, ref["glogstd"])]


def torch_model(case, inp, dtype):
    """the shared trunk with two Linear heads as a torch module of `dtype`, and log_std: (trunk, actor, critic, log_std)"""
    import torch
    import torch.nn as nn
    mods, prev = [], case.D
    for W, b in inp["layers"][:-1]:
        lin = nn.Linear(prev, W.shape[0])
        lin.weight.data, lin.bias.data = torch.tensor(W), torch.tensor(b)
        mods += [lin, nn.Tanh() if case.act == "tanh" else nn.ReLU()]
        prev = W.shape[0]
    actor, critic = nn.Linear(prev, 4), nn.Linear(prev, 1)
    actor.weight.data, actor.bias.data = torch.tensor(inp["layers"][-1][0]), torch.tensor(inp["layers"][-1][1])
    critic.weight.data, critic.bias.data = torch.tensor(inp["wv"][None, :]), torch.tensor(np.asarray(inp["bv"]).reshape(1))
    trunk = nn.Sequential(*mods)
    for m in (trunk, actor, critic):
        m.to(dtype)
    return trunk, actor, critic, torch.tensor(LOG_STD, dtype=dtype, requires_grad=True)


def torch_loss(case, inp, rows, dtype, model, scale=None, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF):
    """the combined loss through torch ops of `dtype`: (scale * sum L, logp, V, sum L_clip, sum k3, sum L_V)"""
    import torch
    trunk, actor, critic, log_std = model
    scale = 1.0 / rows if scale is None else scale
    t = lambda k: torch.tensor(inp[k][:rows], dtype=dtype)
    y = trunk(t("x"))
    mean = actor(y)
    mean = torch.tanh(mean) if case.out_tanh else mean
    v = critic(y)[:, 0]
    z = (t("actions") - mean) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std).sum(dim=1) - G.TWO_LN_2PI
    xr = logp - t("logp_old")
    r, adv = torch.exp(xr), t("adv")
    lclip = -torch.minimum(r * adv, torch.clamp(r, 1.0 - clip, 1.0 + clip) * adv)
    e1 = v - t("ret")
    if case.vclip > 0.0:
        e2 = t("v_old") + torch.clamp(v - t("v_old"), -case.vclip, case.vclip) - t("ret")
        lv = 0.5 * torch.maximum(e1 * e1, e2 * e2)
    else:
        lv = 0.5 * e1 * e1
    ent = (log_std + 0.5 * (1.0 + np.log(2.0 * np.pi))).sum()
    loss = scale * (lclip.sum() + vf_coef * lv.sum() - ent_coef * ent * rows)
    return loss, logp, v, lclip.sum(), (r - 1.0 - xr).sum(), lv.sum()


def torch_grads(case, model):
    """the module's gradients in the reference's shapes: ([(dW, db), ...], grad_value [W + 1], grad_log_std)"""
    trunk, actor, critic, log_std = model
    lins = [m for m in trunk if hasattr(m, "weight")] + [actor]
    return ([(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lins],
            np.concatenate([critic.weight.grad.numpy().reshape(-1), critic.bias.grad.numpy().reshape(-1)]), log_std.grad.numpy())


def torch_errors(case, inp, rows, dtype):
    """torch autograd of `dtype` on the CPU against the reference: (gradient, logp, V, sum L_clip, sum k3, sum L_V)"""
    ref = ppo_ac(case, inp, rows)
    model = torch_model(case, inp, dtype)
    loss, lp, v, lsum, kl, lvsum = torch_loss(case, inp, rows, dtype, model)
    loss.backward()
    g = max(grad_errors(*torch_grads(case, model), ref))
    return (g, G.rel(lp.detach().numpy(), ref["logp"]), G.rel(v.detach().numpy(), ref["value"]), G.rel(float(lsum.detach()), ref["stats"][0]),
            G.rel(float(kl.detach()), ref["stats"][2]), G.rel(float(lvsum.detach()), ref["stats"][3]))


def find_seed(case, limit=4000):
    for seed in range(limit):
        if conditions(case, inputs(case, seed)) is None:
            return seed
    raise RuntimeError("no seed below %d meets the conditions of %s" % (limit, case.name))


# the seed of each case: the first that meets conditions() (python -m tests.policy_grad_ac_ref)
SEEDS = {
    'ac-16-tanh': 0,
    'ac-16-tanh-vclip': 1,
    'ac-16-relu': 0,
    'ac-16-relu-vclip': 1,
    'ac-64x64-tanh': 0,
    'ac-64x64-tanh-vclip': 0,
    'ac-64x64-relu': 4,
    'ac-64x64-relu-vclip': 32,
    'ac-48x80x32-tanh': 0,
    'ac-48x80x32-tanh-vclip': 8,
    'ac-48x80x32-relu': 8,
    'ac-48x80x32-relu-vclip': 8,
    'ac-128x128x128-tanh': 0,
    'ac-128x128x128-tanh-vclip': 0,
    'ac-128x128x128-relu': 246,
    'ac-128x128x128-relu-vclip': 1160,
    'ac-64x64-tanh-d19': 1,
    'ac-64x64-tanh-d19-vclip': 3,
    'ac-64x64-relu-norm': 0,
    'ac-64x64-relu-norm-vclip': 0,
}

# per case and row count: torch fp32 autograd's (gradient, logp, V, sum L_clip, sum k3, sum L_V) errors against the reference
# (python -m tests.policy_grad_ac_ref; torch on the CPU)
BASELINE = {
    'ac-16-tanh': {1: (4.76e-07, 7.74e-08, 3.11e-08, 2.9e-07, 4.65e-06, 9.64e-07), 63: (9.28e-07, 1.59e-07, 9.03e-08, 4.65e-06, 2.05e-07, 5.13e-09), 64: (6.26e-07, 1.59e-07, 9.03e-08, 2.69e-06, 2.24e-07, 1.75e-08), 65: (5.94e-07, 1.59e-07, 9.03e-08, 1.78e-06, 2.23e-07, 2.9e-08), 453: (5.7e-07, 1.11e-07, 1.4e-07, 8.94e-08, 9.47e-08, 2e-08)},
    'ac-16-tanh-vclip': {1: (3.49e-07, 6.82e-08, 7.08e-08, 1.96e-07, 9.63e-06, 2.12e-07), 63: (5.31e-07, 7.76e-08, 9.25e-08, 1.58e-07, 5.83e-08, 3.82e-08), 64: (4.06e-07, 7.76e-08, 9.25e-08, 2.99e-07, 6.75e-08, 4.93e-08), 65: (3.29e-07, 7.76e-08, 9.25e-08, 2.01e-07, 6.23e-09, 5.76e-08), 453: (5.85e-07, 1.26e-07, 1.06e-07, 2.14e-07, 1.14e-07, 1.02e-09)},
    'ac-16-relu': {1: (5.86e-07, 1.85e-08, 4.38e-08, 7.43e-08, 9.86e-07, 1.18e-06), 63: (6.29e-07, 1.91e-07, 1.38e-07, 5.11e-06, 6.14e-08, 1.14e-07), 64: (5.45e-07, 1.91e-07, 1.38e-07, 3.13e-06, 9.95e-08, 2.29e-08), 65: (4.37e-07, 1.91e-07, 1.38e-07, 1.97e-06, 1e-07, 1.14e-08), 453: (1.62e-06, 1.23e-07, 1.06e-07, 5.2e-07, 5.23e-08, 2.83e-08)},
    'ac-16-relu-vclip': {1: (4.28e-07, 7.06e-08, 1.43e-07, 1.68e-07, 4.34e-06, 2.06e-07), 63: (2.67e-07, 8.09e-08, 1.28e-07, 2.85e-07, 6.9e-08, 2.95e-08), 64: (3.37e-07, 8.09e-08, 1.28e-07, 1.76e-07, 7.78e-08, 3.88e-08), 65: (3.1e-07, 8.09e-08, 1.28e-07, 1.31e-07, 1.31e-07, 4.13e-08), 453: (5.32e-07, 2.32e-07, 1.75e-07, 2.93e-07, 1.58e-07, 1.13e-09)},
    'ac-64x64-tanh': {1: (2.27e-07, 2.98e-08, 7.71e-08, 1.35e-07, 3.38e-06, 2.59e-07), 63: (3.38e-07, 2.04e-07, 1.38e-07, 4.91e-07, 2.63e-07, 7.88e-08), 64: (3.42e-07, 2.04e-07, 1.38e-07, 2.88e-07, 3.46e-07, 4.24e-08), 65: (3.91e-07, 2.04e-07, 1.38e-07, 1.79e-07, 3.44e-07, 8.81e-08), 453: (8.79e-07, 1.31e-07, 1.83e-07, 1.69e-08, 6.73e-08, 3.08e-08)},
    'ac-64x64-tanh-vclip': {1: (2.27e-07, 2.98e-08, 7.71e-08, 1.35e-07, 3.38e-06, 2.59e-07), 63: (3.31e-07, 2.04e-07, 1.38e-07, 4.91e-07, 2.63e-07, 6.85e-08), 64: (3.05e-07, 2.04e-07, 1.38e-07, 2.88e-07, 3.46e-07, 3.41e-08), 65: (4.28e-07, 2.04e-07, 1.38e-07, 1.79e-07, 3.44e-07, 7.74e-08), 453: (8.79e-07, 1.31e-07, 1.83e-07, 1.69e-08, 6.73e-08, 2.79e-08)},
    'ac-64x64-relu': {1: (5.78e-07, 7.27e-08, 1.19e-07, 1.38e-07, 4.76e-05, 5.29e-07), 63: (7.34e-07, 1e-07, 3.09e-07, 2.33e-09, 4.76e-07, 1.4e-08), 64: (7.71e-07, 1e-07, 3.09e-07, 2.58e-07, 6.38e-07, 5.33e-08), 65: (6.28e-07, 1e-07, 3.09e-07, 1.01e-07, 6.76e-07, 6.29e-09), 453: (6.15e-07, 1.03e-07, 2.22e-07, 7.33e-08, 3.46e-08, 9.57e-08)},
    'ac-64x64-relu-vclip': {1: (4.43e-07, 6.21e-08, 6.35e-07, 1.38e-07, 8.35e-06, 6.71e-07), 63: (8.71e-07, 1.83e-07, 1.84e-07, 1.12e-07, 3.18e-07, 1.26e-07), 64: (7.06e-07, 1.83e-07, 1.84e-07, 1.79e-07, 3.52e-07, 6.38e-08), 65: (1.12e-06, 1.83e-07, 1.84e-07, 1.98e-07, 4.38e-07, 2.44e-09), 453: (5.58e-07, 1.36e-07, 2.17e-07, 2.78e-06, 2.94e-08, 6.97e-09)},
    'ac-48x80x32-tanh': {1: (2.57e-07, 1.28e-08, 3.51e-08, 4.95e-08, 1.27e-06, 9.94e-08), 63: (8.39e-07, 9.87e-08, 1.44e-07, 5.52e-07, 4.61e-07, 1.25e-07), 64: (6.32e-07, 9.87e-08, 1.55e-07, 9.39e-07, 3.17e-07, 5.31e-08), 65: (6.38e-07, 9.87e-08, 1.55e-07, 5.59e-07, 3.18e-07, 5.88e-08), 453: (8.39e-07, 1.56e-07, 2.49e-07, 2.42e-07, 5.99e-08, 4.24e-08)},
    'ac-48x80x32-tanh-vclip': {1: (2.77e-07, 4e-10, 1.14e-07, 4.44e-08, 5.09e-06, 1.32e-07), 63: (5.2e-07, 1.42e-07, 2.08e-07, 3.95e-08, 2.12e-07, 2.7e-08), 64: (7.45e-07, 1.42e-07, 2.08e-07, 4.88e-07, 1.14e-07, 1.33e-07), 65: (5.59e-07, 1.42e-07, 2.08e-07, 3.09e-07, 1.57e-07, 1.46e-07), 453: (1.01e-06, 1.04e-07, 3.05e-07, 1.95e-07, 1.55e-07, 5.46e-10)},
    'ac-48x80x32-relu': {1: (2.51e-07, 1.59e-08, 5.26e-10, 8.96e-08, 3.88e-06, 1.06e-07), 63: (6.72e-07, 9.88e-08, 2.1e-07, 6.29e-07, 2.5e-07, 8.66e-08), 64: (6.43e-07, 9.88e-08, 2.1e-07, 4.57e-06, 3.04e-07, 8.68e-08), 65: (5.5e-07, 9.88e-08, 2.1e-07, 8.58e-07, 3.46e-07, 1.01e-07), 453: (8.09e-07, 1.36e-07, 2.84e-07, 5.85e-07, 1.1e-08, 3.88e-08)},
    'ac-48x80x32-relu-vclip': {1: (2.51e-07, 1.59e-08, 5.26e-10, 8.96e-08, 3.88e-06, 1.06e-07), 63: (7.29e-07, 9.88e-08, 2.1e-07, 6.29e-07, 2.5e-07, 2.79e-08), 64: (6.04e-07, 9.88e-08, 2.1e-07, 4.57e-06, 3.04e-07, 2.81e-08), 65: (5.44e-07, 9.88e-08, 2.1e-07, 8.58e-07, 3.46e-07, 6.43e-08), 453: (8.09e-07, 1.36e-07, 2.84e-07, 5.85e-07, 1.1e-08, 3.34e-09)},
    'ac-128x128x128-tanh': {1: (3.35e-07, 2.36e-08, 1.18e-09, 9.63e-08, 7.35e-07, 5.53e-08), 63: (9.86e-07, 1.39e-07, 2.57e-07, 1.03e-06, 4.61e-07, 9.69e-08), 64: (5.72e-07, 1.39e-07, 2.57e-07, 1.17e-06, 4.77e-07, 5.89e-08), 65: (7.02e-07, 1.39e-07, 2.57e-07, 9.25e-07, 4.75e-07, 1.79e-07), 453: (1e-06, 1.52e-07, 2.89e-07, 2.07e-08, 6.62e-08, 8.83e-09)},
    'ac-128x128x128-tanh-vclip': {1: (3.35e-07, 2.36e-08, 1.18e-09, 9.63e-08, 7.35e-07, 5.53e-08), 63: (9.86e-07, 1.39e-07, 2.57e-07, 1.03e-06, 4.61e-07, 1.08e-07), 64: (5.52e-07, 1.39e-07, 2.57e-07, 1.17e-06, 4.77e-07, 1.24e-07), 65: (7.02e-07, 1.39e-07, 2.57e-07, 9.25e-07, 4.75e-07, 8.68e-08), 453: (1e-06, 1.52e-07, 2.89e-07, 2.07e-08, 6.62e-08, 3.77e-08)},
    'ac-128x128x128-relu': {1: (1.59e-06, 5.18e-08, 5.09e-08, 1.91e-07, 4.15e-05, 3.17e-06), 63: (1.12e-06, 1.29e-07, 1.78e-07, 6.19e-07, 5.26e-07, 1.68e-08), 64: (9.93e-07, 1.29e-07, 1.78e-07, 5.96e-07, 4.24e-07, 1.82e-08), 65: (1.18e-06, 1.29e-07, 1.78e-07, 7.25e-07, 4.33e-07, 6.99e-08), 453: (9.58e-07, 1.43e-07, 2.25e-07, 6.22e-07, 1.2e-07, 4.09e-08)},
    'ac-128x128x128-relu-vclip': {1: (7.32e-07, 2.79e-08, 3.07e-07, 7.46e-08, 9.56e-05, 1.38e-06), 63: (7.74e-07, 1.12e-07, 3.53e-07, 4.49e-07, 5.58e-07, 2.62e-08), 64: (6.94e-07, 1.12e-07, 3.53e-07, 3.67e-07, 4.98e-07, 6.02e-08), 65: (6.21e-07, 1.12e-07, 3.53e-07, 2.91e-07, 4.97e-07, 5.81e-08), 453: (1.48e-06, 1.34e-07, 4.98e-07, 6.63e-07, 9.01e-08, 4.78e-08)},
    'ac-64x64-tanh-d19': {1: (2.67e-07, 3.46e-08, 9.02e-08, 1.52e-07, 6.7e-07, 2.07e-07), 63: (1.59e-06, 1.45e-07, 2.04e-07, 1.28e-07, 1.68e-08, 2.82e-08), 64: (1.95e-06, 1.45e-07, 2.04e-07, 8.16e-08, 8.06e-09, 9.84e-08), 65: (1.56e-06, 1.45e-07, 2.04e-07, 6.13e-08, 2.94e-08, 4.91e-08), 453: (6.34e-07, 1.69e-07, 1.63e-07, 1.79e-07, 8.76e-08, 8.13e-08)},
    'ac-64x64-tanh-d19-vclip': {1: (3.47e-07, 6.98e-08, 1.08e-07, 3.2e-07, 1.13e-05, 3.48e-09), 63: (7.71e-07, 1.11e-07, 2.36e-07, 8.63e-06, 4.51e-07, 9.95e-09), 64: (6.31e-07, 1.11e-07, 2.82e-07, 2.77e-06, 3.5e-07, 2.4e-09), 65: (8e-07, 1.11e-07, 2.82e-07, 2.63e-06, 4.68e-07, 1.82e-08), 453: (5.93e-07, 1.28e-07, 2.09e-07, 2.03e-08, 1.72e-07, 3.4e-08)},
    'ac-64x64-relu-norm': {1: (3.29e-07, 9.62e-08, 1.37e-07, 3.6e-07, 6.13e-06, 3.94e-07), 63: (6.68e-07, 1.8e-07, 1.68e-07, 3.47e-06, 1.29e-07, 7.42e-09), 64: (5.93e-07, 1.8e-07, 1.47e-07, 1.65e-06, 1.7e-07, 4.41e-08), 65: (5.3e-07, 1.8e-07, 1.47e-07, 8.38e-07, 1.71e-07, 9.73e-08), 453: (8.95e-07, 2.18e-07, 1.63e-07, 3.77e-07, 7.42e-08, 2.37e-08)},
    'ac-64x64-relu-norm-vclip': {1: (3.29e-07, 9.62e-08, 1.37e-07, 3.6e-07, 6.13e-06, 3.94e-07), 63: (6.73e-07, 1.8e-07, 1.68e-07, 3.47e-06, 1.29e-07, 1.68e-08), 64: (5.52e-07, 1.8e-07, 1.47e-07, 1.65e-06, 1.7e-07, 5.15e-08), 65: (5.09e-07, 1.8e-07, 1.47e-07, 8.38e-07, 1.71e-07, 7.83e-09), 453: (8.95e-07, 2.18e-07, 1.63e-07, 3.77e-07, 7.42e-08, 1.04e-07)},
}

_INPUTS = {}


def case_inputs(name):
    """the case and its inputs at its seed, computed once and shared: treat them as read-only"""
    if name not in _INPUTS:
        _INPUTS[name] = inputs(CASES[name], SEEDS[name])
    return CASES[name], _INPUTS[name]


def bounds(name, rows):
    """The device's bounds for the case at `rows`, FACTOR x torch fp32's errors: (gradient, logp, V, sum L_clip, sum k3, sum L_V).  As
    in G.bounds: the gradient's is the case's own at that row count, and so are logp's and V's at more than one row; the true scalars
    -- the three sums at every row count, logp and V at one row -- take the largest torch error over the cases at that row count."""
    pooled = [max(BASELINE[c.name][rows][k] for c in AC_CASES) for k in range(1, 6)]
    own = BASELINE[name][rows]
    return (FACTOR * own[0], FACTOR * (own[1] if rows > 1 else pooled[0]), FACTOR * (own[2] if rows > 1 else pooled[1]),
            FACTOR * pooled[2], FACTOR * pooled[3], FACTOR * pooled[4])


if __name__ == "__main__":
    import torch
    seeds = {c.name: find_seed(c) for c in AC_CASES}
    print("SEEDS = {")
    for k, v in seeds.items():
        print("    %r: %d," % (k, v))
    print("}\n\nBASELINE = {")
    for c in AC_CASES:
        inp = inputs(c, seeds[c.name])
        print("    %r: {%s}," % (c.name, ", ".join("%d: (%s)" % (r, ", ".join("%.3g" % e for e in torch_errors(c, inp, r, torch.float32)))
                                                   for r in ROWS)))
    print("}")
