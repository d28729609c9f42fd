"""An fp64 reference of the device MLP policy (gaq.h gaq_policy: obs -> [Linear -> act] x n_hidden -> Linear -> 4 (-> tanh)) and random
nets whose units do not saturate, so that a wrong sum shows in the actions instead of hiding behind a tanh."""
import numpy as np


def _scaled_layers(widths, D=18, seed=0):
    """fp32 layers [(W [out, in], b [out]), ...] (the hidden layers, then 4 outputs): W = randn / sqrt(fan_in), b = 0.1 randn, as
    tests/gru_util.py _head draws them."""
    rng = np.random.RandomState(seed)
    dims = [D] + list(widths) + [4]
    return [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
            for k in range(len(dims) - 1)]


def _f64(a, like):
    """a as float64 in the array type of `like`: numpy for numpy, a torch tensor on like's device for a torch tensor"""
    if isinstance(like, np.ndarray):
        return np.asarray(a, np.float64)
    import torch
    return torch.as_tensor(np.asarray(a), device=like.device).to(torch.float64)


def forward64(layers, act, out_tanh, x, hidden=None):
    """The policy's forward pass in float64 on the fp32 weights: x [..., in] (numpy, or a torch tensor, which keeps the pass on its
    device) -> (actions [..., 4], the output sums before the output tanh [..., 4]).  With a list for `hidden`, each hidden layer's
    pre-activation [..., width] is appended to it."""
    numpy = isinstance(x, np.ndarray)
    if numpy:
        y = np.asarray(x, np.float64)
        tanh, relu = np.tanh, lambda v: np.maximum(v, 0.0)
    else:
        import torch
        y = x.to(torch.float64)
        tanh, relu = torch.tanh, torch.relu
    for W, b in layers[:-1]:
        y = y @ _f64(W, y).T + _f64(b, y)
        if hidden is not None:
            hidden.append(y)
        y = tanh(y) if act == "tanh" else relu(y)
    W, b = layers[-1]
    z = y @ _f64(W, y).T + _f64(b, y)
    return (tanh(z) if out_tanh else z), z


def saturation(z, hidden, act):
    """(the fraction of output sums with |z| < 1.5, the largest fraction of saturated pre-activations over the hidden layers: |v| > 3
    for tanh, v <= 0 for relu)"""
    def frac(m):
        return float(m.sum()) / float(m.numel() if hasattr(m, "numel") else m.size)
    live = frac(abs(z) < 1.5)
    sat = max([frac(abs(v) > 3.0) if act == "tanh" else frac(v <= 0.0) for v in hidden], default=0.0)
    return live, sat


def assert_not_saturated(z, hidden, act, what=""):
    """the case has teeth: at least half of the output sums are off the tanh's flat tails, and no hidden layer is more than 90 % flat"""
    live, sat = saturation(z, hidden, act)
    assert live >= 0.5, "%s: only %.3f of the output sums have |z| < 1.5" % (what, live)
    assert sat <= 0.9, "%s: a hidden layer is %.3f saturated" % (what, sat)
