"""Host side of the separate critic (gaq.h gaq_critic, gaq_step_policy_critic_many_dev; gym_art_amd.policy.MLPCritic): the packed layout,
the weight count, every validation error, the declarations in header and binding, and the refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd.policy import MLPCritic, _CriticDesc, check_critic_layers, pack_critic_weights, pack_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gaq_critic_create": 3, "gaq_critic_weight_count": 1, "gaq_critic_set_weights": 2, "gaq_critic_set_weights_dev": 2,
       "gaq_critic_destroy": 1, "gaq_critic_eval_dev": 5, "gaq_step_policy_critic_many_dev": 12}


def _critic_layers(widths, D=18, seed=0):
    rng = np.random.RandomState(seed)
    dims = [D] + list(widths) + [1]
    return [(rng.randn(dims[k + 1], dims[k]).astype(np.float32), rng.randn(dims[k + 1]).astype(np.float32)) for k in range(len(dims) - 1)]


def _desc(widths, in_dim=18, act=0):
    d = _CriticDesc()
    d.struct_size = C.sizeof(_CriticDesc)
    d.in_dim, d.n_hidden, d.hidden_act = in_dim, len(widths), act
    for k, w in enumerate(widths[:3]):
        d.width[k] = w
    return d


def _stub_env(D=18):
    """what MLPCritic reads of an env before it touches the library: the validation comes first"""
    return types.SimpleNamespace(obs_dim=D, device=0, _handle=None)


def test_packed_layout_against_a_hand_built_example():
    """D = 2, one hidden layer of 16 units, then the 1-output layer: W'[c][k][j] = W[16c + j][k], bias, then w[16], then its bias"""
    W = np.arange(32, dtype=np.float32).reshape(16, 2)              # W[j][k] = 2 j + k
    b = 100 + np.arange(16, dtype=np.float32)
    w = 200 + np.arange(16, dtype=np.float32).reshape(1, 16)
    packed = pack_critic_weights([(W, b), (w, np.array([300.0], np.float32))])
    want = [2 * j + 0 for j in range(16)] + [2 * j + 1 for j in range(16)] + [100 + j for j in range(16)] + [200 + j for j in range(16)] + [300]
    assert packed.dtype == np.float32 and packed.flags["C_CONTIGUOUS"] and packed.tolist() == [float(x) for x in want]
    # two chunks of 16 units: chunk c holds the units 16 c .. 16 c + 15
    W2 = np.arange(64, dtype=np.float32).reshape(32, 2)
    p2 = pack_critic_weights([(W2, np.zeros(32, np.float32)), (np.zeros((1, 32), np.float32), np.zeros(1, np.float32))])
    assert p2[:64].tolist() == [float(2 * (16 * c + j) + k) for c in range(2) for k in range(2) for j in range(16)]
    # the hidden layers are packed exactly as a policy's, and the last layer as a value head (weights, then the bias)
    layers = _critic_layers([48, 32])
    pol = pack_weights(layers[:-1] + [(np.zeros((4, 32), np.float32), np.zeros(4, np.float32))])
    got = pack_critic_weights(layers)
    nh = 48 * 18 + 48 + 32 * 48 + 32
    assert np.array_equal(got[:nh], pol[:nh])
    assert np.array_equal(got[nh:nh + 32], layers[-1][0].reshape(-1)) and got[nh + 32] == layers[-1][1][0] and got.size == nh + 33


@pytest.mark.parametrize("n_out", [4, 1])
@pytest.mark.parametrize("widths", [[16], [32], [48, 256], [256, 48]])
def test_weight_layout_is_what_pack_and_unpack_use(widths, n_out):
    """the total is pack_weights' size, and each section starts where unpack_weights finds that layer's (distinct) values"""
    from gym_art_amd.policy import unpack_weights, weight_layout
    dims = [18] + widths + [n_out]
    layers = [(1000.0 * k + np.arange(o * i, dtype=np.float32).reshape(o, i) % 997, 1000.0 * k + 998 + np.zeros(o, np.float32))
              for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))]
    packed = pack_weights(layers)
    offs, total = weight_layout(18, widths, n_out)
    assert total == packed.size and len(offs) == len(layers) and offs[0] == 0
    for k, ((W, b), off) in enumerate(zip(layers, offs)):
        section = packed[off:off + W.size + b.size]
        assert section.min() >= 1000.0 * k and section.max() < 1000.0 * (k + 1) and np.array_equal(section[W.size:], b)
    for (W, b), (W2, b2) in zip(layers, unpack_weights(packed, 18, widths, n_out)):
        assert np.array_equal(W, W2) and np.array_equal(b, b2)
    with pytest.raises(ValueError, match="multiples of 16"):
        weight_layout(18, [24], n_out)


@pytest.mark.parametrize("widths", [[16], [48], [240, 80], [256, 256, 256], [32, 128, 16]])
def test_weight_count_against_the_formula(widths):
    lib = _lib.load()
    for D in (18, 19):
        want, prev = 0, D
        for w in widths:
            want += w * prev + w
            prev = w
        want += prev + 1
        assert lib.gaq_critic_weight_count(C.byref(_desc(widths, D))) == want
        assert pack_critic_weights(_critic_layers(widths, D)).size == want


def test_description_errors_name_the_field():
    lib = _lib.load()

    def refused(d, text):
        assert lib.gaq_critic_weight_count(C.byref(d)) == -1
        assert text in lib.gaq_last_error(), lib.gaq_last_error()

    d = _desc([48])
    d.struct_size -= 4
    refused(d, b"struct_size")
    assert lib.gaq_critic_weight_count(None) == -1
    for bad, which in (([24], b"width[0]"), ([272], b"width[0]"), ([48, 8], b"width[1]"), ([48, 48, 0], b"width[2]"), ([-16], b"width[0]")):
        refused(_desc(bad), which)
    for nh in (0, 4, -1):
        d = _desc([48, 48, 48])
        d.n_hidden = nh
        refused(d, b"n_hidden")
    refused(_desc([48], act=2), b"hidden_act")
    refused(_desc([48], in_dim=0), b"in_dim")
    # create: the description is checked before anything else is touched, and nothing is created
    h = C.c_void_p(123)
    assert lib.gaq_critic_create(None, C.byref(_desc([48])), C.byref(h)) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_critic_destroy(None) == 0


def test_mlpcritic_refuses_malformed_layers_with_the_offending_shape():
    env = _stub_env()
    good = _critic_layers([48, 32])
    check_critic_layers(good, 18, "tanh")
    check_critic_layers(_critic_layers([256, 256, 256], 19), 19, "relu")

    def refused(layers, text, act="tanh"):
        for build in (lambda: check_critic_layers(layers, 18, act), lambda: MLPCritic.from_arrays(env, layers, act), lambda: MLPCritic(env, layers, act)):
            with pytest.raises(ValueError, match=text):
                build()

    refused(good, "'tanh' or 'relu'", act="gelu")
    refused(good[-1:], "1 to 3 hidden layers and an output layer, got 1")
    refused(_critic_layers([16, 16, 16, 16]), "got 5 Linear layers")
    refused(_critic_layers([48], D=19), "layer 0 takes 19 inputs, expected 18")
    refused([good[0], (good[1][0][:, :-1], good[1][1]), good[2]], "layer 1 takes 47 inputs, expected 48")
    refused([(good[0][0], good[0][1][:-1])] + good[1:], r"layer 0: W must be \[out, in\] and b \[out\], got \(48, 18\) and \(47,\)")
    refused([(good[0][0].reshape(-1), good[0][1])] + good[1:], r"layer 0: W must be \[out, in\]")
    refused(_critic_layers([24]), r"hidden layer 0 has width 24: widths must be multiples of 16 in \[16, 256\]")
    refused(_critic_layers([48, 272]), "hidden layer 1 has width 272")
    refused(_critic_layers([8]), "hidden layer 0 has width 8")
    four = _critic_layers([48])
    refused([four[0], (np.zeros((4, 48), np.float32), np.zeros(4, np.float32))], "output layer must have 1 output, has 4")
    refused([four[0], (np.zeros((2, 48), np.float32), np.zeros(2, np.float32))], "has 2")


def test_from_torch_rejects_what_it_must():
    import torch
    nn = torch.nn
    env = _stub_env()

    def seq(widths, acts=None, out=1, tail=()):
        mods, prev = [], 18
        for k, w in enumerate(widths):
            mods += [nn.Linear(prev, w), (acts[k] if acts else nn.Tanh)()]
            prev = w
        return nn.Sequential(*(mods + [nn.Linear(prev, out)] + [m() for m in tail]))

    for module, text in ((seq([48], out=4), "1 output, has 4"),
                         (seq([48, 48], out=2), "1 output, has 2"),
                         (seq([48, 48], acts=[nn.Tanh, nn.ReLU]), "same activation"),
                         (seq([24]), "width 24"),
                         (seq([48, 272]), "width 272"),
                         (seq([16, 16, 16, 16]), "got 5 Linear layers"),
                         (seq([48], tail=(nn.Tanh,)), "not squashed"),
                         (seq([48], acts=[nn.Sigmoid]), "only Tanh and ReLU"),
                         (nn.Sequential(nn.Linear(18, 48), nn.ReLU()), "must end with a Linear"),
                         (nn.Sequential(nn.Linear(19, 48), nn.Tanh(), nn.Linear(48, 1)), "takes 19 inputs, expected 18")):
        with pytest.raises(ValueError, match=text):
            MLPCritic.from_torch(module, env)


def _header_arity():
    src = open(os.path.join(ROOT, "include", "gaq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(gaq_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src)}


def test_entry_points_are_declared_in_header_and_binding_with_matching_arity():
    header = _header_arity()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    res = {n: r for n, r, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name, arity in NEW.items():
        assert header.get(name) == arity, (name, header.get(name))
        assert len(sig[name]) == arity, name
        assert hasattr(lib, name), name
    assert res["gaq_critic_weight_count"] is C.c_int64 and sig["gaq_critic_eval_dev"][1] is C.c_int64
    # gaq_step_policy_ac_term_many_dev's arguments with the critic after the policy
    assert len(sig["gaq_step_policy_critic_many_dev"]) == len(sig["gaq_step_policy_ac_term_many_dev"]) + 1
    assert sig["gaq_step_policy_critic_many_dev"][3] is C.c_int32
    # every declaration of the header still has the binding's arity (the new section broke none)
    for name, args in sig.items():
        assert header[name] == max(1, len(args)), name
    src = open(os.path.join(ROOT, "include", "gaq.h")).read()
    assert "never" in src[src.index("separate critic"):src.index("gaq_critic_create")] and "hidden state" in src     # feed-forward, said so
    assert C.sizeof(_CriticDesc) == 4 * 7


def test_entry_points_refuse_null_arguments():
    lib = _lib.load()
    assert lib.gaq_critic_set_weights(None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_critic_set_weights_dev(None, None) == -1
    assert lib.gaq_critic_eval_dev(None, 4, None, None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_step_policy_critic_many_dev(None, None, None, 4, None, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.gaq_last_error()


def test_critic_is_a_keyword_only_argument_with_default_none():
    from gym_art_amd import QuadrotorEnv
    par = inspect.signature(QuadrotorEnv.rollout_policy_dev).parameters
    assert par["critic"].default is None and par["critic"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "critic" in QuadrotorEnv.rollout_policy_dev.__doc__
    for name in ("values", "logp", "term_values"):                  # ... beside the ones that were there
        assert par[name].default is None and par[name].kind is inspect.Parameter.KEYWORD_ONLY


def test_multi_device_env_refuses_a_critic():
    from gym_art_amd.multi_device import _MultiDeviceMixin as M
    with pytest.raises(NotImplementedError, match="critic="):
        M.rollout_policy_dev(M.__new__(M), critic=object())
    with pytest.raises(NotImplementedError, match="values="):       # as it refuses values=
        M.rollout_policy_dev(M.__new__(M), values=object())
