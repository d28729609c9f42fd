"""An fp64 restatement of the gradients on the device (gaq.h gaq_policy_logp_dev, gaq_policy_grad_ppo_dev, gaq_critic_grad_mse_dev) on
fp32 inputs -- manual backprop in NumPy -- with the cases, the inputs and the bounds the CPU and GPU tests share.

Cases: five hidden shapes x (tanh + output tanh, relu without), one net on a 19-wide observation (a partial k-step of 3 rows) and one
behind an observation normaliser; the same hidden shapes with one output for the critic.  Every case has R = 453 = 64 * 7 + 5 rows; the
smaller row counts of the matrix are prefixes of them.

Inputs: mlp_ref._scaled_layers(seed) and, from RandomState(seed + 1000), Gaussian observations, behaviour means 0.15 sigma off the net's,
Gaussian advantages and value targets.  The seed of each case (SEEDS) was searched on the CPU (`python -m tests.policy_grad_ref`) so that
conditions() holds in the fp64 reference: then the fp32 and fp64 branch decisions agree, and the case has teeth.

Bounds: BASELINE holds, per case and row count, the error that torch fp32 autograd on the CPU shows against this reference on the same
inputs (`python -m tests.policy_grad_ref` measures it): (gradient, logp, loss sum, kl sum), each max|v - v64| / max|v64|, the gradient's
the largest over the parameter tensors and grad_log_std.  The device's bound is 8 x that number, applied to each tensor: the factor is the
margin for another summation order over up to 128 + 64 terms (bounds(), which also says how the scalar quantities are treated)."""
import numpy as np

from tests.mlp_ref import _scaled_layers, assert_not_saturated

R = 453
ROWS = [1, 63, 64, 65, R]
CLIP = 0.2
LOG_STD = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
TWO_LN_2PI = 2.0 * np.log(2.0 * np.pi)
NETS = [[16], [64, 64], [128, 128], [48, 80, 32], [128, 128, 128]]
STYLES = [("tanh", True), ("relu", False)]
FACTOR = 8.0


class Case:
    def __init__(self, widths, act, out_tanh, D=18, norm=False, n_out=4):
        self.widths, self.act, self.out_tanh, self.D, self.norm, self.n_out = list(widths), act, bool(out_tanh), D, norm, n_out
        self.name = "%s-%s-%s%s%s" % ("critic" if n_out == 1 else "policy", "x".join(map(str, widths)), act,
                                      "-d%d" % D if D != 18 else "", "-norm" if norm else "")

    def __repr__(self):
        return self.name


POLICY_CASES = [Case(w, a, t) for w in NETS for a, t in STYLES] + [Case([64, 64], "tanh", True, D=19), Case([64, 64], "relu", False, norm=True)]
CRITIC_CASES = [Case(w, a, False, n_out=1) for w in NETS for a, _ in STYLES]
CASES = {c.name: c for c in POLICY_CASES + CRITIC_CASES}


def norm_stats(D):
    """the normaliser of the -norm case: statistics whose fp32 table is exact (mean k / 8, inv_std 2, 1 or 1 / 2; eps = 0), clip 2.5"""
    k = np.arange(D)
    return ((k % 5 - 2) / 8.0), np.array([0.25, 1.0, 4.0])[k % 3], 0.0, 2.5


def normalised(x, D):
    """gaq.h's element expression in fp32: the subtraction and the product rounded separately, then the clamp"""
    mean, var, _, clip = norm_stats(D)
    inv = (1.0 / np.sqrt(var)).astype(np.float32)
    return np.clip((x - mean.astype(np.float32)).astype(np.float32) * inv, np.float32(-clip), np.float32(clip)).astype(np.float32)


def forward(layers, act, out_tanh, x):
    """fp64 forward on the fp32 weights: (the layers' inputs [x, h_0, ...], the hidden pre-activations, the output after the optional tanh)"""
    hs, pre, y = [np.asarray(x, np.float64)], [], np.asarray(x, np.float64)
    for W, b in layers[:-1]:
        v = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        pre.append(v)
        y = np.tanh(v) if act == "tanh" else np.maximum(v, 0.0)
        hs.append(y)
    W, b = layers[-1]
    z = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
    return hs, pre, (np.tanh(z) if out_tanh else z), z


def backward(layers, act, out_tanh, hs, out, dout):
    """dout [rows, n_out] = the gradient with respect to the output -> [(dW, db), ...] summed over the rows"""
    d = np.asarray(dout, np.float64) * ((1.0 - out * out) if out_tanh else 1.0)
    grads = []
    for l in range(len(layers) - 1, -1, -1):
        grads.append((d.T @ hs[l], d.sum(axis=0)))
        if l:
            h = hs[l]
            d = (d @ np.asarray(layers[l][0], np.float64)) * ((1.0 - h * h) if act == "tanh" else (h > 0.0))
    return grads[::-1]


def inputs(case, seed):
    """the case's fp32 inputs at `seed`: layers, obs (raw), x (what the net sees), and actions / logp_old / adv or target"""
    layers = _scaled_layers(case.widths, case.D, seed)
    if case.n_out == 1:
        layers = layers[:-1] + [(layers[-1][0][:1].copy(), layers[-1][1][:1].copy())]
    rng = np.random.RandomState(seed + 1000)
    obs = rng.randn(R, case.D).astype(np.float32)
    if case.norm:
        obs = (2.0 * obs + 0.25).astype(np.float32)
    x = normalised(obs, case.D) if case.norm else obs
    inp = dict(layers=layers, obs=obs, x=x)
    if case.n_out == 1:
        v = forward(layers, case.act, False, x)[2][:, 0]
        inp["target"] = (v + 0.5 * rng.randn(R)).astype(np.float32)
        return inp
    mean = forward(layers, case.act, case.out_tanh, x)[2]
    std = np.exp(LOG_STD.astype(np.float64))
    mean_b = mean + 0.15 * std * rng.randn(R, 4)
    z = rng.randn(R, 4)
    inp["actions"] = (mean_b + std * z).astype(np.float32)
    inp["logp_old"] = ((-0.5 * z * z - LOG_STD).sum(axis=1) - TWO_LN_2PI).astype(np.float32)
    inp["adv"] = rng.randn(R).astype(np.float32)
    return inp


def ppo(case, inp, rows, scale=None, clip=CLIP):
    """the fp64 reference of gaq_policy_grad_ppo_dev on the first `rows` rows"""
    scale = 1.0 / rows if scale is None else scale
    x, a = inp["x"][:rows], np.asarray(inp["actions"][:rows], np.float64)
    hs, pre, mean, zsum = forward(inp["layers"], case.act, case.out_tanh, x)
    inv = np.exp(-LOG_STD.astype(np.float64))
    z = (a - mean) * inv
    logp = (-0.5 * z * z - LOG_STD).sum(axis=1) - TWO_LN_2PI
    xr = logp - np.asarray(inp["logp_old"][:rows], np.float64)
    r, adv = np.exp(xr), np.asarray(inp["adv"][:rows], np.float64)
    s1, s2 = r * adv, np.clip(r, 1.0 - clip, 1.0 + clip) * adv
    dl = np.where(s1 <= s2, -adv * r, 0.0)
    dmean = scale * dl[:, None] * z * inv                       # with respect to the mean (after the output tanh)
    return dict(logp=logp, mean=mean, ratio=r, active=s1 <= s2, dmean=dmean, pre=pre, zsum=zsum,
                grads=backward(inp["layers"], case.act, case.out_tanh, hs, mean, dmean),
                glogstd=(scale * dl[:, None] * (z * z - 1.0)).sum(axis=0),
                stats=np.array([(-np.minimum(s1, s2)).sum(), float((s2 < s1).sum()), (r - 1.0 - xr).sum(), float(rows)]))


def mse(case, inp, rows, scale=None):
    """the fp64 reference of gaq_critic_grad_mse_dev on the first `rows` rows"""
    scale = 1.0 / rows if scale is None else scale
    hs, pre, v, _ = forward(inp["layers"], case.act, False, inp["x"][:rows])
    d = v[:, 0] - np.asarray(inp["target"][:rows], np.float64)
    dv = (scale * d)[:, None]
    return dict(value=v[:, 0], dv=dv, pre=pre, zsum=v, grads=backward(inp["layers"], case.act, False, hs, v, dv),
                stats=np.array([0.5 * (d * d).sum(), float(rows)]))


def conditions(case, inp):
    """None if the inputs meet the issue's conditions in the fp64 reference, else what fails.  Conditions on the inputs, not measurements:
    no relu pre-activation within 2e-5 of 0 and no ratio within 1e-4 of 1 +- CLIP (the fp32 and fp64 branches then agree); 10 % to 70 % of
    the ratios outside the clip range; both signs of advantage; units not saturated; and rows 0 and 64 -- the one-row case and the
    partial tile's only row -- have a gradient (an all-zero reference would leave the relative metric undefined)."""
    ref = ppo(case, inp, R) if case.n_out == 4 else mse(case, inp, R)
    if case.act == "relu" and min(float(np.abs(v).min()) for v in ref["pre"]) < 2e-5:
        return "a relu pre-activation within 2e-5 of 0"
    try:
        assert_not_saturated(ref["zsum"] if case.n_out == 4 else np.zeros(1), ref["pre"], case.act, case.name)
    except AssertionError as e:
        return str(e)
    if case.n_out == 1:
        return None
    r = ref["ratio"]
    if float(np.minimum(np.abs(r - (1.0 - CLIP)), np.abs(r - (1.0 + CLIP))).min()) < 1e-4:
        return "a ratio within 1e-4 of the clip range's edge"
    out = float(((r < 1.0 - CLIP) | (r > 1.0 + CLIP)).mean())
    if not 0.1 <= out <= 0.7:
        return "%.3f of the ratios outside the clip range" % out
    if not ((inp["adv"] > 0).any() and (inp["adv"] < 0).any()):
        return "one sign of advantage only"
    if not (ref["active"][0] and ref["active"][64]):
        return "row 0 or row 64 has no gradient"
    return None


def rel(got, want):
    """max|got - want| / max|want| of two arrays"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def grad_errors(got_layers, got_logstd, ref):
    """the metric of every parameter tensor (W and b of each layer, then grad_log_std if given)"""
    errs = []
    for (gW, gb), (rW, rb) in zip(got_layers, ref["grads"]):
        errs += [rel(gW, rW), rel(gb, rb)]
    if got_logstd is not None:
        errs.append(rel(got_logstd, ref["glogstd"]))
    return errs


def torch_net(case, inp, dtype):
    """the case's net as torch leaves of `dtype`: ([(W, b), ...], log_std, forward(x) -> output)"""
    import torch
    layers = [(torch.tensor(W, dtype=dtype, requires_grad=True), torch.tensor(b, dtype=dtype, requires_grad=True)) for W, b in inp["layers"]]
    log_std = torch.tensor(LOG_STD, dtype=dtype, requires_grad=True)

    def fwd(x):
        y = x
        for W, b in layers[:-1]:
            y = y @ W.T + b
            y = torch.tanh(y) if case.act == "tanh" else torch.relu(y)
        y = y @ layers[-1][0].T + layers[-1][1]
        return torch.tanh(y) if case.out_tanh else y
    return layers, log_std, fwd


def torch_loss(case, inp, rows, dtype, layers, log_std, fwd, scale=None, clip=CLIP):
    """the loss of the case through torch ops of `dtype`: (scale * sum L, logp or V, sum L, sum k3)"""
    import torch
    scale = 1.0 / rows if scale is None else scale
    x = torch.tensor(inp["x"][:rows], dtype=dtype)
    out = fwd(x)
    if case.n_out == 1:
        d = out[:, 0] - torch.tensor(inp["target"][:rows], dtype=dtype)
        L = 0.5 * d * d
        return scale * L.sum(), out[:, 0], L.sum(), None
    z = (torch.tensor(inp["actions"][:rows], dtype=dtype) - out) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std).sum(dim=1) - TWO_LN_2PI
    xr = logp - torch.tensor(inp["logp_old"][:rows], dtype=dtype)
    r, adv = torch.exp(xr), torch.tensor(inp["adv"][:rows], dtype=dtype)
    L = -torch.minimum(r * adv, torch.clamp(r, 1.0 - clip, 1.0 + clip) * adv)
    return scale * L.sum(), logp, L.sum(), (r - 1.0 - xr).sum()


def torch_errors(case, inp, rows, dtype):
    """torch autograd of `dtype` on the CPU against the reference: (gradient, logp or V, loss sum, kl sum or 0)"""
    import torch
    ref = ppo(case, inp, rows) if case.n_out == 4 else mse(case, inp, rows)
    layers, log_std, fwd = torch_net(case, inp, dtype)
    loss, lp, lsum, kl = torch_loss(case, inp, rows, dtype, layers, log_std, fwd)
    loss.backward()
    got = [(W.grad.numpy(), b.grad.numpy()) for W, b in layers]
    g = max(grad_errors(got, log_std.grad.numpy() if case.n_out == 4 else None, ref))
    return (g, rel(lp.detach().numpy(), ref["logp"] if case.n_out == 4 else ref["value"]), rel(float(lsum.detach()), ref["stats"][0]),
            rel(float(kl.detach()), ref["stats"][2]) if kl is not None else 0.0)


def find_seed(case, limit=4000):
    for seed in range(limit):
        if conditions(case, inputs(case, seed)) is None:
            return seed
    raise RuntimeError("no seed below %d meets the conditions of %s" % (limit, case.name))


# the seed of each case: the first that meets conditions() (python -m tests.policy_grad_ref)
SEEDS = {
    'policy-16-tanh': 0,
    'policy-16-relu': 0,
    'policy-64x64-tanh': 0,
    'policy-64x64-relu': 4,
    'policy-128x128-tanh': 0,
    'policy-128x128-relu': 4,
    'policy-48x80x32-tanh': 0,
    'policy-48x80x32-relu': 8,
    'policy-128x128x128-tanh': 0,
    'policy-128x128x128-relu': 246,
    'policy-64x64-tanh-d19': 1,
    'policy-64x64-relu-norm': 0,
    'critic-16-tanh': 0,
    'critic-16-relu': 0,
    'critic-64x64-tanh': 0,
    'critic-64x64-relu': 2,
    'critic-128x128-tanh': 0,
    'critic-128x128-relu': 4,
    'critic-48x80x32-tanh': 0,
    'critic-48x80x32-relu': 2,
    'critic-128x128x128-tanh': 0,
    'critic-128x128x128-relu': 83,
}

# per case and row count: torch fp32 autograd's (gradient, logp / V, loss sum, kl sum) errors against the reference
# (python -m tests.policy_grad_ref; torch on the CPU)
BASELINE = {
    'policy-16-tanh': {1: (1.79e-07, 3.24e-08, 1.35e-07, 2.97e-07), 63: (2.52e-07, 1.59e-07, 9.21e-08, 3.29e-07), 64: (2.82e-07, 1.59e-07, 4.98e-07, 2.86e-07), 65: (3.91e-07, 1.59e-07, 3.84e-07, 2.85e-07), 453: (4.67e-07, 1.11e-07, 9.16e-08, 9.47e-08)},
    'policy-16-relu': {1: (1.21e-07, 1.85e-08, 7.43e-08, 9.86e-07), 63: (4.69e-07, 1.91e-07, 5.97e-06, 5.57e-07), 64: (4.37e-07, 1.91e-07, 3.38e-06, 5.16e-07), 65: (3.6e-07, 1.91e-07, 2.19e-06, 5.14e-07), 453: (1.27e-06, 1.32e-07, 3.39e-07, 1.39e-07)},
    'policy-64x64-tanh': {1: (3.47e-07, 8.01e-08, 2.89e-07, 5.33e-06), 63: (6.04e-07, 1.42e-07, 9.22e-07, 7.73e-08), 64: (4.65e-07, 1.42e-07, 5.31e-07, 9.97e-08), 65: (6.34e-07, 1.42e-07, 4.72e-07, 9.86e-08), 453: (1.15e-06, 1.06e-07, 2.58e-07, 6.73e-08)},
    'policy-64x64-relu': {1: (2.37e-07, 3.33e-08, 1.02e-07, 4.76e-05), 63: (8.73e-07, 1.05e-07, 2.24e-07, 7.66e-07), 64: (7.44e-07, 1.05e-07, 3.48e-07, 1e-06), 65: (8.02e-07, 1.05e-07, 2.64e-07, 8.58e-07), 453: (1.28e-06, 1.12e-07, 7.33e-08, 1.29e-07)},
    'policy-128x128-tanh': {1: (3.43e-07, 7.25e-08, 2.57e-07, 4.95e-06), 63: (1.07e-06, 1.12e-07, 3.22e-06, 4.96e-07), 64: (8.02e-07, 1.12e-07, 2.79e-06, 5.17e-07), 65: (7.55e-07, 1.12e-07, 1.68e-06, 5.16e-07), 453: (7.51e-07, 1.92e-07, 1.7e-07, 5.97e-08)},
    'policy-128x128-relu': {1: (3.28e-07, 3.8e-08, 1.12e-07, 4.68e-05), 63: (6.88e-07, 8.28e-08, 1.44e-07, 1.19e-07), 64: (5.9e-07, 8.28e-08, 2.15e-08, 4.5e-08), 65: (7.49e-07, 8.28e-08, 1.12e-07, 6.77e-09), 453: (1.64e-06, 1.31e-07, 1.46e-08, 1.28e-07)},
    'policy-48x80x32-tanh': {1: (4.33e-07, 9.7e-08, 3.75e-07, 5.62e-06), 63: (6.6e-07, 9.4e-08, 2.28e-06, 2.75e-07), 64: (5.9e-07, 9.4e-08, 1.18e-06, 1.94e-07), 65: (6.4e-07, 9.4e-08, 5.59e-07, 1.95e-07), 453: (8.49e-07, 1.11e-07, 4.74e-10, 5.99e-08)},
    'policy-48x80x32-relu': {1: (3.34e-07, 7.02e-08, 1.97e-07, 3.88e-06), 63: (5.18e-07, 1.33e-07, 7.99e-07, 1.65e-07), 64: (5.43e-07, 1.33e-07, 3.4e-06, 1.39e-07), 65: (5.34e-07, 1.33e-07, 1.21e-06, 1.72e-08), 453: (9.51e-07, 1.36e-07, 6.53e-07, 1.1e-08)},
    'policy-128x128x128-tanh': {1: (7.58e-07, 1.33e-07, 5.21e-07, 7.98e-06), 63: (2.14e-06, 2.06e-07, 3.62e-06, 2.81e-07), 64: (1.81e-06, 2.06e-07, 2.39e-06, 2.61e-07), 65: (1.72e-06, 2.06e-07, 1.51e-06, 2.62e-07), 453: (1.1e-06, 1.52e-07, 2.81e-07, 1.25e-07)},
    'policy-128x128x128-relu': {1: (6.53e-07, 8.99e-08, 3.74e-07, 5.12e-05), 63: (9.02e-07, 1.29e-07, 5.59e-07, 7.14e-07), 64: (1.02e-06, 1.29e-07, 4.82e-07, 7.05e-07), 65: (1.15e-06, 1.29e-07, 7.25e-07, 7.14e-07), 453: (1.28e-06, 1.41e-07, 1.05e-06, 1.2e-07)},
    'policy-64x64-tanh-d19': {1: (4.21e-07, 5.12e-08, 2.41e-07, 7.63e-07), 63: (2.1e-06, 1.25e-07, 4.33e-07, 3.42e-07), 64: (2.5e-06, 1.25e-07, 5.41e-07, 2.79e-07), 65: (2.7e-06, 1.25e-07, 3.48e-07, 2.58e-07), 453: (6.76e-07, 1.93e-07, 3.75e-07, 8.76e-08)},
    'policy-64x64-relu-norm': {1: (5.08e-07, 1.23e-07, 4.9e-07, 6.94e-06), 63: (6.48e-07, 1.27e-07, 2.61e-06, 5.01e-07), 64: (6.24e-07, 1.27e-07, 9.2e-07, 6.01e-07), 65: (6.63e-07, 1.27e-07, 3.99e-07, 6.01e-07), 453: (8.7e-07, 2.18e-07, 1.06e-07, 2.13e-08)},
    'critic-16-tanh': {1: (1.93e-07, 1.79e-07, 3.29e-07, 0), 63: (7.11e-07, 1.41e-07, 3.42e-08, 0), 64: (7.13e-07, 1.41e-07, 1.04e-08, 0), 65: (4.47e-07, 1.41e-07, 7.43e-09, 0), 453: (1.1e-06, 1.62e-07, 2.48e-08, 0)},
    'critic-16-relu': {1: (8.95e-08, 5.33e-08, 1.16e-07, 0), 63: (3.01e-07, 6.49e-08, 3.59e-10, 0), 64: (2.33e-07, 6.49e-08, 2.6e-08, 0), 65: (2.72e-07, 6.49e-08, 2.64e-08, 0), 453: (3.8e-07, 1.19e-07, 4.76e-08, 0)},
    'critic-64x64-tanh': {1: (3.1e-07, 3.07e-07, 1.71e-07, 0), 63: (7.95e-07, 1.96e-07, 2.87e-08, 0), 64: (8.64e-07, 1.96e-07, 7.17e-08, 0), 65: (5.22e-07, 1.96e-07, 8.84e-08, 0), 453: (7.5e-07, 2.09e-07, 5.03e-08, 0)},
    'critic-64x64-relu': {1: (7.72e-07, 7.16e-07, 1.46e-06, 0), 63: (6.75e-07, 1.72e-07, 1.5e-07, 0), 64: (6.04e-07, 1.72e-07, 7.79e-08, 0), 65: (5.45e-07, 1.72e-07, 1.64e-07, 0), 453: (5.53e-07, 2.51e-07, 9.76e-08, 0)},
    'critic-128x128-tanh': {1: (2.42e-07, 1.92e-07, 2.36e-07, 0), 63: (6.65e-07, 2.46e-07, 5.27e-08, 0), 64: (8.83e-07, 2.46e-07, 4.83e-08, 0), 65: (4.92e-07, 2.46e-07, 5.46e-09, 0), 453: (6.57e-07, 2.49e-07, 4.67e-08, 0)},
    'critic-128x128-relu': {1: (2.24e-07, 6.83e-09, 6.11e-08, 0), 63: (3.58e-07, 2.8e-07, 9.17e-08, 0), 64: (3.6e-07, 2.8e-07, 3.92e-08, 0), 65: (5.3e-07, 2.8e-07, 1.93e-10, 0), 453: (6.93e-07, 2.76e-07, 6.22e-08, 0)},
    'critic-48x80x32-tanh': {1: (5.28e-07, 9.8e-08, 4.62e-07, 0), 63: (8.41e-07, 1.57e-07, 4.86e-08, 0), 64: (1.22e-06, 1.57e-07, 5.09e-08, 0), 65: (9.95e-07, 1.57e-07, 6.57e-08, 0), 453: (1.12e-06, 2e-07, 4.14e-08, 0)},
    'critic-48x80x32-relu': {1: (2.81e-07, 3.33e-08, 1.5e-07, 0), 63: (8.51e-07, 2.36e-07, 6.1e-09, 0), 64: (6.45e-07, 2.36e-07, 6.35e-08, 0), 65: (3.95e-06, 2.36e-07, 8.6e-08, 0), 453: (1.46e-06, 1.71e-07, 2.55e-08, 0)},
    'critic-128x128x128-tanh': {1: (5.05e-07, 4.59e-06, 3.38e-07, 0), 63: (5.19e-07, 2.75e-07, 1.15e-07, 0), 64: (7.88e-07, 2.68e-07, 1.68e-08, 0), 65: (7.32e-07, 2.68e-07, 1.86e-10, 0), 453: (8.98e-07, 2.6e-07, 4.52e-08, 0)},
    'critic-128x128x128-relu': {1: (7.51e-07, 1.39e-07, 5.75e-07, 0), 63: (3.82e-07, 2.82e-07, 9.2e-08, 0), 64: (4.04e-07, 2.82e-07, 1.15e-07, 0), 65: (4.19e-07, 2.82e-07, 8.25e-08, 0), 453: (6.28e-07, 3.63e-07, 3.27e-08, 0)},
}


def case_inputs(name):
    case = CASES[name]
    return case, inputs(case, SEEDS[name])


def bounds(name, rows):
    """The device's bounds for the case at `rows`, FACTOR x torch fp32's errors: (gradient, logp / V, loss sum, kl sum).  The gradient's
    is the case's own at that row count (a maximum over up to 9 tensors of many elements), and so is logp's / V's at more than one row
    (a maximum over at least 63 rows): stable numbers.  The loss and kl sums are single scalars at every row count, and logp / V is one
    at one row; a scalar's rounding error is a single draw -- at one row torch's kl error came out anywhere from 3e-7 to 5e-5 over the
    policy cases (r - 1 - x cancels to x^2 / 2, so logp's last bit decides it), and its loss-sum error as low as 2e-10.  For these true
    scalars alone the baseline is the largest torch error at that row count over the cases of the same family (the policies, or the
    critics): twelve (ten) draws of one quantity at one size."""
    family = POLICY_CASES if CASES[name].n_out == 4 else CRITIC_CASES
    pooled = [max(BASELINE[c.name][rows][k] for c in family) for k in (1, 2, 3)]
    own = BASELINE[name][rows]
    return (FACTOR * own[0], FACTOR * (own[1] if rows > 1 else pooled[0]), FACTOR * pooled[1], FACTOR * pooled[2])


if __name__ == "__main__":
    import torch
    seeds = {c.name: find_seed(c) for c in POLICY_CASES + CRITIC_CASES}
    print("SEEDS = {")
    for k, v in seeds.items():
        print("    %r: %d," % (k, v))
    print("}\n\nBASELINE = {")
    for c in POLICY_CASES + CRITIC_CASES:
        inp = inputs(c, seeds[c.name])
        print("    %r: {%s}," % (c.name, ", ".join("%d: (%s)" % (r, ", ".join("%.3g" % e for e in torch_errors(c, inp, r, torch.float32)))
                                                   for r in ROWS)))
    print("}")
