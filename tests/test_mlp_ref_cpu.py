"""The fp64 reference of the device MLP policy (tests/mlp_ref.py forward64) pinned to a torch float64 nn.Sequential with the same weights
and to the documented packed layout (pack_weights read back as the device routine indexes it).  No GPU needed."""
import numpy as np
import pytest

from gym_art_amd.policy import pack_weights
from tests.mlp_ref import _scaled_layers, assert_not_saturated, forward64, saturation
from tests.test_policy_cpu import _forward_packed

NETS = [([48], "tanh", True), ([240, 80], "relu", False), ([16, 48, 240], "tanh", False), ([144, 48], "relu", True)]


def _x(D, n=33, seed=5):
    return (1.5 * np.random.RandomState(seed).randn(n, D)).astype(np.float32)


def _sequential64(layers, act, out_tanh):
    import torch
    nn = torch.nn
    mods = []
    for k, (W, b) in enumerate(layers):
        lin = nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W).double())
            lin.bias.copy_(torch.from_numpy(b).double())
        mods.append(lin)
        if k < len(layers) - 1:
            mods.append(nn.Tanh() if act == "tanh" else nn.ReLU())
    if out_tanh:
        mods.append(nn.Tanh())
    return nn.Sequential(*mods)


@pytest.mark.parametrize("D", [13, 22, 108])
@pytest.mark.parametrize("widths,act,out_tanh", NETS)
def test_forward64_is_the_torch_float64_sequential(widths, act, out_tanh, D):
    torch = pytest.importorskip("torch")
    layers = _scaled_layers(widths, D, seed=D)
    x = _x(D)
    hidden = []
    a, z = forward64(layers, act, out_tanh, x, hidden)
    net = _sequential64(layers, act, out_tanh)
    with torch.no_grad():
        ref = net(torch.from_numpy(x).double()).numpy()
        zref = net[:2 * len(widths) + 1](torch.from_numpy(x).double()).numpy()
    assert a.dtype == np.float64 and a.shape == (len(x), 4)
    np.testing.assert_allclose(a, ref, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(z, zref, rtol=1e-13, atol=1e-13)
    assert [h.shape[1] for h in hidden] == list(widths)
    # the torch form of the same pass, on the tensor's device, gives the same numbers
    a2, z2 = forward64(layers, act, out_tanh, torch.from_numpy(x))
    np.testing.assert_allclose(a2.numpy(), a, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(z2.numpy(), z, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("D", [13, 22, 108])
@pytest.mark.parametrize("widths,act,out_tanh", NETS)
def test_forward64_reads_the_packed_layout(widths, act, out_tanh, D):
    layers = _scaled_layers(widths, D, seed=D + 1)
    x = _x(D, seed=D)
    packed = pack_weights(layers)
    f = np.tanh if act == "tanh" else (lambda v: np.maximum(v, 0.0))
    got = _forward_packed(packed.astype(np.float64), widths, D, x.astype(np.float64), f, out_tanh)
    np.testing.assert_allclose(forward64(layers, act, out_tanh, x)[0], got, rtol=1e-12, atol=1e-12)


def test_scaled_layers_do_not_saturate():
    """the point of the scaling: on inputs of unit size the sums stay off the tanh's tails, where the unscaled randn nets sit"""
    from tests.policy_util import _layers
    x = np.random.RandomState(0).randn(256, 108).astype(np.float32)
    for act in ("tanh", "relu"):
        hidden = []
        _, z = forward64(_scaled_layers([240, 80], 108), act, True, x, hidden)
        assert_not_saturated(z, hidden, act, act)
    hidden = []
    _, z = forward64(_layers([240, 80], 108), "tanh", True, x, hidden)
    live, sat = saturation(z, hidden, "tanh")
    assert live < 0.5 and sat > 0.5

