"""Host side of the MFMA policy engine (gaq_policy_desc_ex, gym_art_amd/policy.py engine="mfma" / "auto"): the weight count and
refusals of the _ex entry points, check_layers for 256-wide nets, the packed layout at width 256 and the "auto" rule.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd.policy import _Desc, _DescEx, check_layers, pack_weights, resolve_engine
from tests.policy_util import _desc_ex, _layers


def test_desc_ex_is_desc_plus_engine():
    assert C.sizeof(_DescEx) == C.sizeof(_Desc) + 4
    assert _DescEx.engine.offset == C.sizeof(_Desc)


@pytest.mark.parametrize("widths", [[256], [256, 256], [256, 256, 256], [256, 128, 64], [256, 16], [16], [64, 64], [144, 48]])
def test_weight_count_ex_matches_the_packing(widths):
    lib = _lib.load()
    assert lib.gaq_policy_weight_count_ex(C.byref(_desc_ex(widths, "mfma"))) == pack_weights(_layers(widths)).size


@pytest.mark.parametrize("widths", [[16], [64, 64], [128, 128, 128], [32, 128, 16]])
def test_weight_count_ex_for_valu_nets_is_the_valu_count(widths):
    lib = _lib.load()
    d = _Desc()
    d.struct_size = C.sizeof(_Desc)
    d.in_dim, d.n_hidden = 18, len(widths)
    for k, w in enumerate(widths):
        d.width[k] = w
    n = lib.gaq_policy_weight_count(C.byref(d))
    assert n == pack_weights(_layers(widths)).size
    assert lib.gaq_policy_weight_count_ex(C.byref(_desc_ex(widths, "valu"))) == n
    assert lib.gaq_policy_weight_count_ex(C.byref(_desc_ex(widths, "mfma"))) == n


def test_weight_count_ex_refusals():
    lib = _lib.load()

    def count(d):
        return lib.gaq_policy_weight_count_ex(C.byref(d))
    assert count(_desc_ex([256], "valu")) == -1
    assert count(_desc_ex([272], "mfma")) == -1
    assert count(_desc_ex([24], "mfma")) == -1
    assert count(_desc_ex([64, 0], "mfma")) == -1
    d = _desc_ex([64, 64, 64], "mfma")
    d.n_hidden = 4
    assert count(d) == -1
    assert count(_desc_ex([64, 64], 2)) == -1
    assert count(_desc_ex([64, 64], -1)) == -1
    d = _desc_ex([64, 64], "mfma")
    d.struct_size = C.sizeof(_Desc)
    assert count(d) == -1
    d.struct_size = C.sizeof(_DescEx) + 4
    assert count(d) == -1
    # the plain entry point still refuses width 256 and 4 hidden layers
    p = _Desc()
    p.struct_size = C.sizeof(_Desc)
    p.in_dim, p.n_hidden, p.width[0] = 18, 1, 256
    assert lib.gaq_policy_weight_count(C.byref(p)) == -1


def test_engine_of_a_null_policy_is_refused():
    assert _lib.load().gaq_policy_engine(None) == -1


def test_check_layers_mfma_widths():
    for widths in ([256, 256, 256], [256, 16], [256], [16, 256, 48]):
        check_layers(_layers(widths), 18, "relu", engine="mfma")
    for widths, msg in (([272], "multiples of 16"), ([24], "multiples of 16"), ([256, 256, 256, 256], "1 to 3")):
        with pytest.raises(ValueError, match=msg):
            check_layers(_layers(widths), 18, "tanh", engine="mfma")
    with pytest.raises(ValueError, match="multiples of 16 in \\[16, 128\\]$"):
        check_layers(_layers([256]), 18, "tanh")                    # the default engine keeps its limits and its words
    with pytest.raises(ValueError, match="engine"):
        check_layers(_layers([64]), 18, "tanh", engine="tensor")


def test_auto_engine_rule():
    for widths in ([16], [64, 64], [128, 128, 128], [32, 128, 16]):
        assert resolve_engine(_layers(widths), 18, "tanh") == "valu"
        assert resolve_engine(_layers(widths), 18, "tanh", "mfma") == "mfma"
    for widths in ([256], [256, 256], [144, 64], [64, 256, 16]):
        assert resolve_engine(_layers(widths), 18, "relu") == "mfma"
        with pytest.raises(ValueError, match="128"):
            resolve_engine(_layers(widths), 18, "relu", "valu")
    for widths in ([272], [24], [64] * 4):
        with pytest.raises(ValueError):
            resolve_engine(_layers(widths), 18, "tanh")
    with pytest.raises(ValueError, match="inputs"):
        resolve_engine(_layers([256], D=17), 18, "tanh")
    with pytest.raises(ValueError, match="engine"):
        resolve_engine(_layers([64]), 18, "tanh", "fast")


@pytest.mark.parametrize("widths", [[256], [256, 256], [256, 256, 256], [256, 128, 64], [48, 256]])
def test_packed_layout_at_width_256(widths):
    """pack_weights through the documented indexing (per hidden layer W'[c][k][j] then bias; output W'[k][o] then bias), in NumPy."""
    layers = _layers(widths, seed=len(widths))
    packed = pack_weights(layers)
    x = np.random.RandomState(2).randn(9, 18).astype(np.float32)
    off, h, I = 0, x.astype(np.float64), 18
    for li, w in enumerate(widths):
        Wp = packed[off:off + w * I].reshape(w // 16, I, 16); off += w * I
        b = packed[off:off + w]; off += w
        for c, k, j in ((0, 0, 0), (w // 16 - 1, I - 1, 15), (w // 32, I // 2, 7)):
            assert Wp[c, k, j] == layers[li][0][16 * c + j, k]
        h, I = np.tanh(h @ Wp.transpose(0, 2, 1).reshape(w, I).T.astype(np.float64) + b), w
    Wo = packed[off:off + 4 * I].reshape(I, 4); off += 4 * I
    y = h @ Wo + packed[off:off + 4]
    assert off + 4 == packed.size
    ref = x.astype(np.float64)
    for W, b in layers[:-1]:
        ref = np.tanh(ref @ W.T.astype(np.float64) + b)
    ref = ref @ layers[-1][0].T.astype(np.float64) + layers[-1][1]
    np.testing.assert_allclose(y, ref, rtol=1e-12, atol=1e-12)
