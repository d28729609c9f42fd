"""Host side of the bf16 policy engine (GAQ_POLICY_ENGINE_MFMA_BF16, MLPPolicy(engine="bf16")): the weight count and refusals of engine 3,
check_layers and the "auto" rule, and the reference helper's bf16 rounding against torch.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_art_amd import _lib
from gym_art_amd.policy import ENGINES, _Desc, check_layers, pack_weights, resolve_engine
from tests.policy_bf16_ref import bf16_round, forward
from tests.policy_util import _desc_ex, _layers


def test_engine_value():
    assert ENGINES["bf16"] == 3


@pytest.mark.parametrize("widths", [[16], [64, 64], [256], [256, 256], [256, 256, 256], [256, 128, 64], [48, 256, 16], [144, 48]])
def test_weight_count_bf16_is_the_fp32_count(widths):
    lib = _lib.load()
    n = lib.gaq_policy_weight_count_ex(C.byref(_desc_ex(widths, "mfma")))
    assert n == pack_weights(_layers(widths)).size
    assert lib.gaq_policy_weight_count_ex(C.byref(_desc_ex(widths, "bf16"))) == n


def test_weight_count_bf16_refusals():
    lib = _lib.load()

    def count(d):
        return lib.gaq_policy_weight_count_ex(C.byref(d))
    for widths in ([272], [24], [8], [64, 40], [64, 0], [512]):
        assert count(_desc_ex(widths, "bf16")) == -1, widths
    d = _desc_ex([64, 64, 64], "bf16")
    d.n_hidden = 4
    assert count(d) == -1
    d.n_hidden = 0
    assert count(d) == -1
    d = _desc_ex([64, 64], "bf16")
    d.struct_size = C.sizeof(_Desc)
    assert count(d) == -1


def test_unassigned_engine_values_stay_refused():
    """2 was refused as unknown before the bf16 engine and stays so; so do 4 and negative values"""
    lib = _lib.load()
    for engine in (2, 4, 7, -1):
        assert lib.gaq_policy_weight_count_ex(C.byref(_desc_ex([64, 64], engine))) == -1, engine
    assert lib.gaq_policy_weight_count_ex(C.byref(_desc_ex([64, 64], 3))) == pack_weights(_layers([64, 64])).size


def test_check_layers_bf16_widths():
    for widths in ([256, 256, 256], [256, 16], [16], [48, 256, 16]):
        check_layers(_layers(widths), 18, "relu", engine="bf16")
    for widths, msg in (([272], "multiples of 16"), ([24], "multiples of 16"), ([256, 256, 256, 256], "1 to 3")):
        with pytest.raises(ValueError, match=msg):
            check_layers(_layers(widths), 18, "tanh", engine="bf16")
    with pytest.raises(ValueError, match="bf16 engine"):
        check_layers(_layers([272]), 18, "tanh", engine="bf16")


def test_auto_never_picks_bf16():
    for widths in ([16], [64, 64], [128, 128, 128], [256], [256, 256], [256, 256, 256], [48, 256, 16]):
        assert resolve_engine(_layers(widths), 18, "tanh") != "bf16"
        assert resolve_engine(_layers(widths), 18, "relu", "bf16") == "bf16"
    assert resolve_engine(_layers([64, 64]), 18, "tanh") == "valu"
    assert resolve_engine(_layers([256, 256]), 18, "tanh") == "mfma"
    with pytest.raises(ValueError, match="256"):
        resolve_engine(_layers([272]), 18, "tanh", "bf16")


def _bits(x):
    return x.contiguous().view(torch.int32)


def test_bf16_round_matches_torch_bit_for_bit():
    rng = np.random.RandomState(0)
    u = rng.randint(0, 2 ** 32, size=1 << 18, dtype=np.uint64).astype(np.uint32)
    specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF,
                         0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,        # ties: to even (down), to even (up), both signs
                         0x3F807FFF, 0x3F808001, 0x00008000, 0x80018000, 0x7F7F8000, 0x7F7F7FFF], np.uint32)
    # every tie of a spread of exponents: low 16 bits exactly 0x8000, mantissa lsb 0 and 1
    ties = (np.arange(0, 1 << 16, 97, dtype=np.uint32) << 16) | 0x8000
    x = torch.from_numpy(np.concatenate([u, specials, ties]).view(np.float32).copy())
    fin = ~torch.isnan(x)
    ours, ref = bf16_round(x), x.to(torch.bfloat16).to(torch.float32)
    assert torch.equal(_bits(ours[fin]), _bits(ref[fin]))
    assert torch.isnan(ours[~fin]).all()
    z = bf16_round(torch.tensor([0.0, -0.0]))
    assert _bits(z).tolist() == [0, -(1 << 31)]


def test_bf16_round_is_idempotent_on_bf16_values():
    x = torch.randn(4096).to(torch.bfloat16).to(torch.float32)
    assert torch.equal(_bits(bf16_round(x)), _bits(x))


def test_reference_forward_rounds_weights_and_inputs():
    """The helper against an independent spelling of the contract through torch's own bf16 conversion."""
    layers = _layers([64, 32], seed=3)
    obs = torch.from_numpy(np.random.RandomState(4).randn(33, 18).astype(np.float32))
    y = forward(layers, "tanh", True, obs)
    h = obs
    for k, (W, b) in enumerate(layers):
        Wb = torch.from_numpy(W).to(torch.bfloat16).double()
        z = h.to(torch.bfloat16).double() @ Wb.T + torch.from_numpy(b).double()
        h = torch.tanh(z).float() if k < 2 else torch.tanh(z)
    assert torch.equal(y, h)
