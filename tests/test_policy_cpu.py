"""Host side of the device MLP policy (gym_art_amd/policy.py): the packed weight layout of include/gaq.h, the checks that refuse what the
device routine cannot run, the nn.Sequential reader and the multi-device refusal.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd.policy import _Desc, check_layers, pack_weights, torch_layers
from tests.policy_util import _layers


def _forward_packed(packed, widths, D, x, act=np.tanh, out_tanh=False):
    """The device routine's indexing of the packed layout, in NumPy: per hidden layer W'[c][k][j] then bias, output W'[k][o] then bias."""
    off, h, I = 0, x, D
    for w in widths:
        Wp = packed[off:off + w * I].reshape(w // 16, I, 16); off += w * I
        b = packed[off:off + w]; off += w
        W = Wp.transpose(0, 2, 1).reshape(w, I)
        h, I = act(h @ W.T + b), w
    Wo = packed[off:off + 4 * I].reshape(I, 4); off += 4 * I
    y = h @ Wo + packed[off:off + 4]
    assert off + 4 == packed.size
    return np.tanh(y) if out_tanh else y


@pytest.mark.parametrize("widths", [[16], [64, 64], [128, 32, 48]])
def test_packed_layout_is_the_documented_one(widths):
    layers = _layers(widths)
    packed = pack_weights(layers)
    x = np.random.RandomState(1).randn(7, 18).astype(np.float32)
    ref = x
    for W, b in layers[:-1]:
        ref = np.tanh(ref @ W.T + b)
    ref = ref @ layers[-1][0].T + layers[-1][1]
    np.testing.assert_allclose(_forward_packed(packed, widths, 18, x), ref, rtol=1e-5, atol=1e-5)


def test_weight_count_matches_the_packing():
    lib = _lib.load()
    for widths in ([16], [64, 64], [128, 128, 128]):
        d = _Desc()
        d.struct_size = C.sizeof(_Desc)
        d.in_dim, d.n_hidden = 18, len(widths)
        for k, w in enumerate(widths):
            d.width[k] = w
        assert lib.gaq_policy_weight_count(C.byref(d)) == pack_weights(_layers(widths)).size
    d.width[0] = 24
    assert lib.gaq_policy_weight_count(C.byref(d)) == -1
    d.width[0], d.n_hidden = 16, 4
    assert lib.gaq_policy_weight_count(C.byref(d)) == -1


@pytest.mark.parametrize("widths,D,msg", [([24], 18, "multiples of 16"), ([256], 18, "multiples of 16"), ([64], 17, "inputs"),
                                          ([], 18, "1 to 3"), ([16, 16, 16, 16], 18, "1 to 3")])
def test_layers_the_device_cannot_run_are_refused(widths, D, msg):
    with pytest.raises(ValueError, match=msg):
        check_layers(_layers(widths, D=D), 18, "tanh")
    with pytest.raises(ValueError, match="tanh"):
        check_layers(_layers([16]), 18, "gelu")


def test_torch_sequential_reader():
    torch = pytest.importorskip("torch")
    nn = torch.nn
    m = nn.Sequential(nn.Linear(18, 32), nn.ReLU(), nn.Linear(32, 16), nn.ReLU(), nn.Linear(16, 4), nn.Tanh())
    layers, act, out_tanh = torch_layers(m)
    assert act == "relu" and out_tanh and [W.shape for W, _ in layers] == [(32, 18), (16, 32), (4, 16)]
    np.testing.assert_array_equal(layers[1][0], m[2].weight.detach().numpy())
    with pytest.raises(ValueError, match="same activation"):
        torch_layers(nn.Sequential(nn.Linear(18, 16), nn.ReLU(), nn.Linear(16, 16), nn.Tanh(), nn.Linear(16, 4)))
    with pytest.raises(ValueError, match="Tanh and ReLU"):
        torch_layers(nn.Sequential(nn.Linear(18, 16), nn.GELU(), nn.Linear(16, 4)))
    with pytest.raises(ValueError, match="end with a Linear"):
        torch_layers(nn.Sequential(nn.Linear(18, 16), nn.ReLU()))


def test_multi_device_env_refuses_policy_rollouts():
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.multi_device import multi_device_class
    cls = multi_device_class(QuadrotorEnv)
    with pytest.raises(NotImplementedError, match="rollout_policy_dev"):
        cls.rollout_policy_dev(object.__new__(cls), None, None, None, None)
