"""Host side of "an encoder in front of the cell" (gaq.h gaq_policy_desc_rnn_enc, GRUPolicy / LSTMPolicy.with_encoder): the encoder block's
packing and its inverse, the weight-count formula against the packing, the refusals of the description by text, the Python-side refusals
that need no device, and the fp64 reference the GPU tests use (tests/enc_util.py) against torch fp64.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd.policy import (GRUPolicy, LSTMPolicy, _DescRnn, _DescRnnEnc, check_encoder_layers, encoder_weight_count,
                                pack_encoder_weights, pack_weights, torch_encoder, unpack_encoder_weights)
from tests.enc_util import _cell, _desc_enc, _encoder, reference_rollout, yardstick_parts
from tests.gru_util import _desc_rnn, _head

SHAPES = [(18, (16,)), (19, (48,)), (18, (80,)), (19, (256,)), (18, (240, 80)), (13, (32, 256)), (108, (256, 256))]


def _err():
    return _lib.load().gaq_last_error().decode()


def test_descriptor_and_symbols():
    lib = _lib.load()
    assert C.sizeof(_DescRnnEnc) == C.sizeof(_DescRnn) + 16                 # enc_in_dim, enc_layers, enc_width[2]
    for name in ("gaq_policy_create_rnn_enc", "gaq_policy_encoder_weight_count", "gaq_policy_set_encoder_weights",
                 "gaq_policy_set_encoder_weights_dev", "gaq_policy_get_encoder_weights", "gaq_policy_encoder_width"):
        assert hasattr(lib, name), name
    assert lib.gaq_abi_version() == _lib.ABI_VERSION == 5                   # additive: the version stays


@pytest.mark.parametrize("D,widths", SHAPES)
def test_pack_unpack_round_trip_and_count(D, widths):
    """the block is the MLP's hidden-layer layout -- W'[W/16][in][16] then the bias, per layer -- and its size is the library's count"""
    lib = _lib.load()
    enc = _encoder(D, widths, seed=3)
    p = pack_encoder_weights(enc)
    want = sum(w * i + w for w, i in zip(widths, (D,) + tuple(widths[:-1])))
    assert p.size == want == encoder_weight_count(D, widths)
    assert lib.gaq_policy_encoder_weight_count(C.byref(_desc_enc([64], widths, enc_in=D))) == want
    # the same floats as the hidden layers of an MLP with these layers in front of any output layer
    out = (np.zeros((4, widths[-1]), np.float32), np.zeros(4, np.float32))
    assert np.array_equal(p, pack_weights(enc + [out])[:want])
    W0 = enc[0][0]
    first = p[:widths[0] * D].reshape(widths[0] // 16, D, 16)
    for c in range(widths[0] // 16):
        assert np.array_equal(first[c], W0[16 * c:16 * c + 16].T)
    assert np.array_equal(p[widths[0] * D:widths[0] * D + widths[0]], enc[0][1])
    back = unpack_encoder_weights(p, D, widths)
    assert len(back) == len(enc)
    for (W, b), (W2, b2) in zip(enc, back):
        assert np.array_equal(W, W2) and np.array_equal(b, b2)
    import torch
    for (W, b), (W2, b2) in zip(enc, unpack_encoder_weights(torch.from_numpy(p), D, widths)):
        assert np.array_equal(W, W2.numpy()) and np.array_equal(b, b2.numpy())
    with pytest.raises(ValueError, match="packs into"):
        unpack_encoder_weights(p[:-1], D, widths)


def test_the_cell_and_head_count_is_the_rnn_count_on_E_inputs():
    lib = _lib.load()
    for cell, G in ((1, 3), (3, 4)):
        n = lib.gaq_policy_weight_count_rnn(C.byref(_desc_rnn([48, 32], cell=cell, in_dim=80)))
        assert n == G * 48 * (80 + 48) + 2 * G * 48 + pack_weights(_head(48, (32,))).size


def test_description_refusals_say_encoder():
    lib = _lib.load()

    def count(d):
        return lib.gaq_policy_encoder_weight_count(C.byref(d))
    assert count(_desc_enc([64], (48,))) == 48 * 18 + 48
    assert count(_desc_enc([64, 32], (240, 80), cell=3)) == 240 * 18 + 240 + 80 * 240 + 80
    for widths in ((24,), (272,), (0,), (64, 8), (64, 264)):                # widths outside the family
        assert count(_desc_enc([64], widths)) == -1 and "encoder" in _err() and "enc_width" in _err(), widths
    for layers in (0, 3, -1):                                               # enc_layers outside 1..2
        d = _desc_enc([64], (48,))
        d.enc_layers = layers
        assert count(d) == -1 and "encoder" in _err() and "enc_layers" in _err()
    assert count(_desc_enc([64], (48,), in_dim=18)) == -1 and "encoder" in _err() and "last width" in _err()
    assert count(_desc_enc([64], (48, 80), in_dim=48)) == -1 and "last width" in _err()
    d = _desc_enc([64], (48,))
    d.struct_size = C.sizeof(_DescRnn)                                      # a wrong struct_size
    assert count(d) == -1 and "encoder" in _err() and "size mismatch" in _err()
    assert count(_desc_enc([64], (48,), enc_in=0)) == -1 and "encoder" in _err()
    # the recurrent description's own refusals keep their own texts
    assert count(_desc_enc([64], (48,), cell=2)) == -1 and "unknown recurrent cell" in _err()
    assert count(_desc_enc([64], (48,), engine=3)) == -1 and "MFMA engine only" in _err()
    assert count(_desc_enc([24], (48,))) == -1 and "multiples of 16" in _err()
    # null arguments
    h = C.c_void_p()
    assert lib.gaq_policy_create_rnn_enc(None, C.byref(_desc_enc([64], (48,))), C.byref(h)) == -1
    assert lib.gaq_policy_encoder_width(None) == -1
    assert lib.gaq_policy_set_encoder_weights(None, None) == -1 and lib.gaq_policy_get_encoder_weights(None, None) == -1


def test_check_encoder_layers():
    assert check_encoder_layers(_encoder(18, (48,)), 18) == [48]
    assert check_encoder_layers(_encoder(19, (240, 80)), 19) == [240, 80]
    for bad, text in (([], "1 or 2"), (_encoder(18, (16, 16)) + _encoder(16, (16,)), "1 or 2"), (_encoder(18, (24,)), "multiples of 16"),
                      (_encoder(18, (272,)), "multiples of 16"), (_encoder(17, (48,)), "obs_dim"), (_encoder(18, (48,)) + _encoder(32, (16,)), "takes 32")):
        with pytest.raises(ValueError, match="encoder") as e:
            check_encoder_layers(bad, 18)
        assert text in str(e.value), (text, str(e.value))
    with pytest.raises(ValueError, match="encoder"):
        check_encoder_layers([(np.zeros((16, 18)), np.zeros(15))], 18)


class _FakeEnv:
    """what the constructors read before they reach the device"""
    obs_dim, device, num_envs, _handle = 18, 0, 4, None


@pytest.mark.parametrize("cls,cell", [(GRUPolicy, "gru"), (LSTMPolicy, "lstm")])
def test_constructor_refusals_before_the_device(cls, cell):
    env = _FakeEnv()
    with pytest.raises(ValueError, match="encoder"):                        # a width outside the family
        cls.with_encoder(env, _encoder(18, (24,)), _cell(cell, 32, 24), _head(32))
    with pytest.raises(ValueError, match="encoder"):                        # the encoder does not take the observation
        cls.with_encoder(env, _encoder(19, (48,)), _cell(cell, 32, 48), _head(32))
    with pytest.raises(ValueError, match="encoder's last width"):           # the cell does not take the encoder's last width
        cls.with_encoder(env, _encoder(18, (48,)), _cell(cell, 32, 18), _head(32))
    with pytest.raises(ValueError, match="encoder"):                        # three layers
        cls.with_encoder(env, _encoder(18, (16, 16)) + _encoder(16, (16,)), _cell(cell, 32, 16), _head(32))
    # without an encoder the texts are the ones they were, and the constructor takes no such keyword: its parameters are the parent's
    with pytest.raises(ValueError, match="expected the env's obs_dim 18"):
        cls(env, _cell(cell, 32, 48), _head(32))
    with pytest.raises(TypeError):
        cls(env, _cell(cell, 32, 48), _head(32), encoder=_encoder(18, (48,)))


def test_torch_encoder_and_from_torch_refusals():
    import torch
    nn = torch.nn
    torch.manual_seed(0)
    layers, act = torch_encoder(nn.Sequential(nn.Linear(18, 64), nn.ReLU(), nn.Linear(64, 32), nn.ReLU()))
    assert act == "relu" and [W.shape for W, _ in layers] == [(64, 18), (32, 64)] and layers[0][0].dtype == np.float32
    assert torch_encoder(nn.Sequential(nn.Linear(18, 16, bias=False), nn.Tanh()))[0][0][1].tolist() == [0.0] * 16
    for bad in (nn.Sequential(nn.Linear(18, 64)), nn.Sequential(nn.Linear(18, 64), nn.ELU()), nn.Sequential(nn.Tanh(), nn.Linear(18, 64)),
                nn.Sequential(nn.Linear(18, 64), nn.Tanh(), nn.Linear(64, 32), nn.ReLU()), nn.Linear(18, 64),
                nn.Sequential(*[m for _ in range(3) for m in (nn.Linear(16, 16), nn.Tanh())])):
        with pytest.raises(ValueError, match="encoder"):
            torch_encoder(bad)
    env = _FakeEnv()
    head = nn.Sequential(nn.Linear(32, 16), nn.Tanh(), nn.Linear(16, 4))
    with pytest.raises(ValueError, match="encoder's activation"):           # the encoder's activation is not the head's
        GRUPolicy.from_torch_encoder(nn.Sequential(nn.Linear(18, 64), nn.ReLU()), nn.GRUCell(64, 32), head, env)
    with pytest.raises(ValueError, match="encoder's last width"):
        LSTMPolicy.from_torch_encoder(nn.Sequential(nn.Linear(18, 64), nn.Tanh()), nn.LSTMCell(48, 32), head, env)


@pytest.mark.parametrize("cell,widths,act,out_tanh,head,norm", [("gru", (48,), "tanh", True, (), False), ("gru", (240, 80), "relu", False, (32,), True),
                                                                ("lstm", (80,), "tanh", False, (32,), True), ("lstm", (16, 32), "relu", True, (), False)])
def test_reference_against_torch_fp64(cell, widths, act, out_tanh, head, norm):
    """tests/enc_util.py reference_rollout == nn.Sequential + nn.GRUCell / nn.LSTMCell + the head in torch float64, stepped by hand with
    the rollout's semantics, to 1e-12: actions, final states, V per step with the bootstrap row, terminal values"""
    import torch
    nn = torch.nn
    D, H, N, T = 19, 32, 7, 6
    rng = np.random.RandomState(11)
    enc, weights, layers = _encoder(D, widths, 1), _cell(cell, H, widths[-1], 2), _head(H, head, 3)
    value = ((rng.randn(head[-1] if head else H) / 4).astype(np.float32), np.float32(0.3))
    nm = (rng.randn(D), np.exp(0.3 * rng.randn(D)), 2.5) if norm else None
    obs0, obs, term = rng.randn(N, D), rng.randn(T, N, D), rng.randn(T, N, D)
    done = (rng.rand(T, N) < 0.3).astype(np.uint8)
    assert done.any() and done[T - 1].any()
    state0 = tuple(0.5 * rng.randn(N, H) for _ in range(2 if cell == "lstm" else 1))
    ref = reference_rollout(cell, enc, weights, layers, act, out_tanh, obs0, obs, done, state0, value, term, nm)

    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    A = nn.Tanh if act == "tanh" else nn.ReLU
    mods, prev = [], D
    for W, b in enc:
        lin = nn.Linear(prev, W.shape[0]).double()
        lin.weight.data, lin.bias.data, prev = t64(W), t64(b), W.shape[0]
        mods += [lin, A()]
    tenc = nn.Sequential(*mods)
    tcell = (nn.GRUCell if cell == "gru" else nn.LSTMCell)(prev, H).double()
    for p, a in zip((tcell.weight_ih, tcell.weight_hh, tcell.bias_ih, tcell.bias_hh), weights):
        p.data = t64(a)

    def trunk(h):
        for W, b in layers[:-1]:
            h = A()(nn.functional.linear(h, t64(W), t64(b)))
        return h

    def feats(x):
        x = t64(x)
        if nm:
            x = torch.clamp((x - t64(nm[0])) * t64(nm[1]), -nm[2], nm[2])
        return tenc(x)

    def step(x, s):
        out = tcell(feats(x), s[0] if cell == "gru" else s)
        return (out,) if cell == "gru" else tuple(out)
    V = lambda h: trunk(h) @ t64(value[0]) + float(value[1])
    with torch.no_grad():
        s = tuple(t64(x) for x in state0)
        for t in range(T + 1):
            new = step(obs0 if t == 0 else obs[t - 1], s)
            assert np.max(np.abs(V(new[0]).numpy() - ref["v"][t])) < 1e-12
            if t == T:
                break
            z = nn.functional.linear(trunk(new[0]), t64(layers[-1][0]), t64(layers[-1][1]))
            assert np.max(np.abs((torch.tanh(z) if out_tanh else z).numpy() - ref["a"][t])) < 1e-12
            d = torch.from_numpy(done[t] != 0)
            tv = np.zeros(N)
            if d.any():
                tv[d.numpy()] = V(step(term[t][d.numpy()], tuple(x[d] for x in new))[0]).numpy()
            assert np.max(np.abs(tv - ref["tv"][t])) < 1e-12
            s = tuple(torch.where(d[:, None], torch.zeros_like(x), x) for x in new)
        assert np.max(np.abs(s[0].numpy() - ref["h"])) < 1e-12
        if cell == "lstm":
            assert np.max(np.abs(s[1].numpy() - ref["c"])) < 1e-12
    # the yardstick runs the same rollout in torch fp32: close to the reference, and not the reference
    yard = reference_rollout(cell, enc, weights, layers, act, out_tanh, obs0, obs, done, state0, value, term, nm,
                             parts=yardstick_parts(cell, enc, weights, layers, act, out_tanh, value, nm))
    for k in ref:
        e = np.max(np.abs(yard[k] - ref[k]))
        assert 0.0 < e < 1e-4, (k, e)
