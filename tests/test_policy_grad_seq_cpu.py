"""The recurrent learner's reference (tests/policy_grad_seq_ref.py) against torch fp64 autograd of the same loss on a GRUCell loop with
torch.where resets, a Linear head and a value Linear; the conditions its cases meet; and the surface of the new entry points -- no GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P
from tests import policy_grad_seq_ref as R
from tests.gru_util import _gru, _head

IDS = [c.name for c in R.SEQ_CASES]


@pytest.mark.parametrize("case", R.SEQ_CASES, ids=IDS)
def test_reference_agrees_with_torch_fp64_autograd(case):
    """<= 1e-12 relative per parameter tensor (weight_ih, bias_ih, weight_hh, bias_hh and the head's separately), for grad_value and
    grad_log_std, and for logp and V, at every (T, S)"""
    import torch
    _, inp = R.case_inputs(case.name)
    for T, S in R.CONFIGS:
        errs, lp, v = R.torch_errors(case, inp, T, S, torch.float64, each=True)[:3]
        assert len(errs) == 4 + 2 * len(inp["head"]) + (2 if case.value else 1)
        assert max(errs) <= 1e-12 and lp <= 1e-12 and v <= 1e-12, (T, S, errs, lp, v)


@pytest.mark.parametrize("case", R.SEQ_CASES, ids=IDS)
def test_inputs_meet_the_conditions(case):
    """conditions on the inputs, not measurements: G's and A's, the done pattern of every T >= 5 size, and rows 0 and 64 carrying a
    gradient at t = 0 through a later step: the reference's gradient of those rows' first step into h (dh0 of a call on steps 1 ..)
    is non-zero"""
    _, inp = R.case_inputs(case.name)
    assert R.conditions(case, inp) is None
    for T, S in R.CONFIGS:
        if T >= 5:
            assert R.done_conditions(inp["done"], T, S) is None
            d = inp["done"][:T, :S] != 0
            assert d[0].any() and d[T - 2].any() and (d[:-1] & d[1:]).any() and d[T - 1].any() and not d[:, 0].any()
            assert S <= 64 or not d[:, 64].any()
    ref = R.ppo_seq(case, inp, R.TMAX, R.SMAX)
    clipped = float(((ref["ratio"] < 1 - R.CLIP) | (ref["ratio"] > 1 + R.CLIP)).mean())
    assert 0.1 <= clipped <= 0.7 and (inp["adv"] > 0).any() and (inp["adv"] < 0).any()
    cut = float(ref["cut"].mean())
    assert (0.1 <= cut <= 0.7) if case.vclip > 0 else cut == 0.0
    later = R.ppo_seq(case, inp, R.TMAX - 1, R.SMAX, t_lo=1, scale=1.0)       # what steps 1 .. send back into step 0's output
    assert np.abs(later["dh0"][0]).max() > 0 and np.abs(later["dh0"][64]).max() > 0
    assert set(R.BASELINE[case.name]) == set(R.CONFIGS)


def test_the_case_list_is_the_stated_one():
    names = set(R.CASES)
    for shape in ("gru16", "gru48x32", "gru64x16x48", "gru64x64x64"):
        for style in ("tanh", "relu"):
            assert {"%s-%s" % (shape, style), "%s-%s-vclip" % (shape, style)} <= names
    assert sum(c.D == 19 for c in R.SEQ_CASES) == 2 and sum(c.norm for c in R.SEQ_CASES) == 2
    assert sum(not c.value for c in R.SEQ_CASES) == 2 and len(R.SEQ_CASES) == 22
    assert R.CONFIGS == [(1, 1), (1, 65), (2, 63), (5, 64), (5, 65), (6, 130)]


def test_a_done_cuts_the_reference_in_two():
    """with done[1] set everywhere the gradient is that of steps 0 .. 1 from h0 plus that of steps 2 .. from 0, and without the value
    terms grad_value is 0"""
    case, inp = R.case_inputs("gru48x32-tanh-vclip")
    done = inp["done"].copy()
    done[1, :] = 1
    T, S = 5, 65
    whole = R.ppo_seq(case, inp, T, S, scale=1.0, done=done)
    a = R.ppo_seq(case, inp, 2, S, scale=1.0, done=done)
    b = R.ppo_seq(case, inp, 3, S, scale=1.0, done=done, t_lo=2, h0=np.zeros((S, case.H)))
    for w, x, y in zip(R.tensors(whole), R.tensors(a), R.tensors(b)):
        assert np.allclose(w, x + y, rtol=1e-12, atol=1e-14 * np.abs(w).max())
    assert not R.ppo_seq(case, inp, T, S, vf_coef=0.0)["gvalue"].any()


def test_one_committed_baseline_is_what_torch_fp32_gives_here():
    """maxima over many elements within a factor of 8 of the committed numbers, the single scalars below the pooled bound"""
    import torch
    case, inp = R.case_inputs("gru64x16x48-tanh-vclip")
    T, S = R.CONFIGS[-1]
    got, want = R.torch_errors(case, inp, T, S, torch.float32), R.BASELINE[case.name][T, S]
    print("torch fp32 at (%d, %d): %s, committed %s" % (T, S, got, want))
    for g, w in zip(got[:3], want[:3]):
        assert w / 8.0 <= g <= w * 8.0, (got, want)
    for g, b in zip(got[3:], R.bounds(case.name, T, S)[3:]):
        assert g <= b, (got, R.bounds(case.name, T, S))


def test_entry_points_are_declared_bound_and_refuse_null_handles():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    for name, nargs in {"gaq_policy_eval_seq_dev": 12, "gaq_policy_grad_ppo_seq_dev": 21}.items():
        assert len(sig[name]) == nargs and sig[name][1] is C.c_int32 and sig[name][2] is C.c_int64 and name + "(" in header, name
        assert hasattr(lib, name)
    assert sig["gaq_policy_grad_ppo_seq_dev"][11:16] == [C.c_float] * 5
    assert lib.gaq_abi_version() == 5                              # additive entry points: the ABI version stays
    assert lib.gaq_policy_eval_seq_dev(None, 2, 4, *[None] * 9) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_grad_ppo_seq_dev(None, 2, 4, *[None] * 8, 0.2, 0.2, 0.5, 0.01, 1.0, *[None] * 5) == -1
    assert b"null" in lib.gaq_last_error()


@pytest.mark.parametrize("H,D,head", [(16, 18, ()), (48, 19, (32,)), (64, 18, (16, 48))])
def test_unpack_gru_weights_round_trips(H, D, head):
    import torch
    gru, layers = _gru(H, D, 3), _head(H, head, 4)
    packed = P.pack_gru_weights(gru, layers)
    for flat in (packed, torch.tensor(packed)):
        (W_ih, W_hh, b_ih, b_hh), got = P.unpack_gru_weights(flat, D, H, head)
        for a, b in zip((W_ih, W_hh, b_ih, b_hh), gru):
            assert tuple(a.shape) == b.shape and np.array_equal(np.asarray(a), b)
        assert len(got) == len(layers)
        for (W, b), (W0, b0) in zip(got, layers):
            assert np.array_equal(np.asarray(W), W0) and np.array_equal(np.asarray(b), b0)
        assert isinstance(W_ih, type(flat))
    assert np.array_equal(P.pack_gru_weights(*P.unpack_gru_weights(packed, D, H, head)), packed)
    with pytest.raises(ValueError, match="packs into"):
        P.unpack_gru_weights(packed[:-1], D, H, head)


def test_python_surface():
    def sig(f):
        return str(inspect.signature(f))
    assert sig(P.GRUPolicy.evaluate_seq_dev) == "(self, obs, actions, done, h0, logp=None, value=None, mean=None, h_out=None, stream=None)"
    assert sig(P.GRUPolicy.ppo_seq_grad_dev) == ("(self, obs, actions, done, h0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, "
                                                 "vf_coef=0.5, ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, "
                                                 "stats=None, stream=None)")
    assert sig(P.unpack_gru_weights) == "(packed, in_dim, hidden_size, head_widths=())"
    assert sig(P.GRUPolicy.set_weights) == "(self, gru, head_layers)" and sig(P.GRUPolicy.set_weights_dev) == "(self, packed)"
    for f in (P.GRUPolicy.evaluate_seq_dev, P.GRUPolicy.ppo_seq_grad_dev, P.unpack_gru_weights, P.GRUPolicy.set_weights,
              P.GRUPolicy.set_weights_dev):
        assert f.__doc__
    assert not hasattr(P.LSTMPolicy, "ppo_seq_grad_dev")
