"""The LSTM learner's reference (tests/policy_grad_lstm_ref.py) against torch fp64 autograd of the same loss on an LSTMCell loop with
torch.where resets of h and c, a Linear head and a value Linear; the conditions its cases meet; the committed baseline table; the LDS
formula of gaq.h; and the surface of the three new entry points -- no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P
from tests import policy_grad_lstm_ref as R
from tests.gru_util import _head
from tests.lstm_util import _lstm

IDS = [c.name for c in R.LSTM_CASES]


@pytest.mark.parametrize("case", R.LSTM_CASES, ids=IDS)
def test_reference_agrees_with_torch_fp64_autograd(case):
    """<= 1e-12 relative per parameter tensor (weight_ih, bias_ih, weight_hh, bias_hh and the head's separately), for grad_value and
    grad_log_std, and for logp and V, at every (T, S)"""
    import torch
    _, inp = R.case_inputs(case.name)
    for T, S in R.CONFIGS:
        errs, lp, v = R.torch_errors(case, inp, T, S, torch.float64, each=True)[:3]
        assert len(errs) == 4 + 2 * len(inp["head"]) + (2 if case.value else 1)
        assert max(errs) <= 1e-12 and lp <= 1e-12 and v <= 1e-12, (T, S, errs, lp, v)


@pytest.mark.parametrize("case", R.LSTM_CASES, ids=IDS)
def test_inputs_meet_the_conditions(case):
    """conditions on the inputs, not measurements: the GRU reference's, the done pattern of every T >= 5 size, non-zero h0 and c0, and
    rows 0 and 64 carrying a gradient at t = 0 through a later step, by both paths: the reference's gradient of those rows' first step
    into h and into c (dh0 and dc0 of a call on steps 1 ..) is non-zero.  The baseline table has every config."""
    _, inp = R.case_inputs(case.name)
    assert R.conditions(case, inp) is None
    assert np.abs(inp["h0"]).min() > 0 and np.abs(inp["c0"]).min() > 0
    for T, S in R.CONFIGS:
        if T >= 5:
            assert R.done_conditions(inp["done"], T, S) is None
    ref = R.ppo_seq(case, inp, R.TMAX, R.SMAX)
    clipped = float(((ref["ratio"] < 1 - R.CLIP) | (ref["ratio"] > 1 + R.CLIP)).mean())
    assert 0.1 <= clipped <= 0.7 and (inp["adv"] > 0).any() and (inp["adv"] < 0).any()
    cut = float(ref["cut"].mean())
    assert (0.1 <= cut <= 0.7) if case.vclip > 0 else cut == 0.0
    later = R.ppo_seq(case, inp, R.TMAX - 1, R.SMAX, t_lo=1, scale=1.0)       # what steps 1 .. send back into step 0's outputs
    for s in (0, 64):
        assert np.abs(later["dh0"][s]).max() > 0 and np.abs(later["dc0"][s]).max() > 0
    assert set(R.BASELINE[case.name]) == set(R.CONFIGS) and case.name in R.SEEDS
    assert all(len(v) == 6 and all(np.isfinite(v)) and v[0] > 0 for v in R.BASELINE[case.name].values())


def test_the_case_list_is_the_stated_one():
    names = set(R.CASES)
    for shape in ("lstm16", "lstm48x32", "lstm64x16x48", "lstm64x64x64"):
        for style in ("tanh", "relu"):
            assert {"%s-%s" % (shape, style), "%s-%s-vclip" % (shape, style)} <= names
    assert sum(c.D == 19 for c in R.LSTM_CASES) == 2 and sum(c.norm for c in R.LSTM_CASES) == 2
    assert sum(not c.value for c in R.LSTM_CASES) == 2 and len(R.LSTM_CASES) == 22
    assert R.CONFIGS == [(1, 1), (1, 65), (2, 63), (5, 64), (5, 65), (6, 130)] and (R.TMAX, R.SMAX) == (6, 130)
    assert set(R.SEEDS) == names == set(R.BASELINE)


def test_a_done_cuts_the_reference_in_two():
    """with done[1] set everywhere the gradient is that of steps 0 .. 1 from (h0, c0) plus that of steps 2 .. from (0, 0); at T = 1 from
    c0 = 0 the f-gate rows are exactly 0, and with c0 != 0 they are not"""
    case, inp = R.case_inputs("lstm48x32-tanh-vclip")
    done = inp["done"].copy()
    done[1, :] = 1
    T, S, H = 5, 65, case.H
    whole = R.ppo_seq(case, inp, T, S, scale=1.0, done=done)
    a = R.ppo_seq(case, inp, 2, S, scale=1.0, done=done)
    b = R.ppo_seq(case, inp, 3, S, scale=1.0, done=done, t_lo=2, h0=np.zeros((S, H)), c0=np.zeros((S, H)))
    for w, x, y in zip(R.tensors(whole), R.tensors(a), R.tensors(b)):
        assert np.allclose(w, x + y, rtol=1e-12, atol=1e-14 * np.abs(w).max())
    assert not R.ppo_seq(case, inp, T, S, vf_coef=0.0)["gvalue"].any()
    zero = R.ppo_seq(case, inp, 1, S, h0=np.zeros((S, H)), c0=np.zeros((S, H)))
    assert not zero["g_lstm"][1].any() and not zero["g_lstm"][0][H:2 * H].any() and not zero["g_lstm"][2][H:2 * H].any()
    assert zero["g_lstm"][0][:H].any() and R.ppo_seq(case, inp, 1, S, h0=np.zeros((S, H)))["g_lstm"][0][H:2 * H].any()


def test_one_committed_baseline_is_what_torch_fp32_gives_here():
    """maxima over many elements within a factor of 8 of the committed numbers, the single scalars below the pooled bound"""
    import torch
    case, inp = R.case_inputs("lstm64x16x48-tanh-vclip")
    T, S = R.CONFIGS[-1]
    got, want = R.torch_errors(case, inp, T, S, torch.float32), R.BASELINE[case.name][T, S]
    print("torch fp32 at (%d, %d): %s, committed %s" % (T, S, got, want))
    for g, w in zip(got[:3], want[:3]):
        assert w / 8.0 <= g <= w * 8.0, (got, want)
    for g, b in zip(got[3:], R.bounds(case.name, T, S)[3:]):
        assert g <= b, (got, R.bounds(case.name, T, S))


def lds_bytes(in_dim, H, head, bwd=True, idx=False):
    """gaq.h's formula: 8.25 KiB + 272 B x (in_dim rounded up to 16 + 3 H + max(4 H, H + the head widths)), + 256 B for the idx form;
    the forward call: 8.25 KiB + 272 B x (in_dim rounded up to 16 + 2 H + the head widths)"""
    kx = (in_dim + 15) & ~15
    rows = kx + (3 * H + max(4 * H, H + sum(head)) if bwd else 2 * H + sum(head))
    return 8448 + 272 * rows + (256 if idx else 0)


def test_the_lds_formula():
    """135.75 KiB at 18-LSTM64-64-64 as gaq.h states, under the 160 KiB cap with the idx form's 256 B; H = 80, the first refused width,
    would be over the cap as well"""
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    assert lds_bytes(18, 64, (64, 64)) == 135.75 * 1024 and "135.75 KiB at 18-LSTM64-64-64" in header
    assert lds_bytes(18, 64, (64, 64), idx=True) <= 160 * 1024
    assert lds_bytes(18, 80, (64, 64)) > 160 * 1024 and lds_bytes(18, 80, ()) > 160 * 1024
    assert lds_bytes(18, 64, (64, 64), bwd=False) < lds_bytes(18, 64, (64, 64))
    src = open(os.path.join(_lib._HERE, "csrc", "gaq_policy_grad_seq.hip")).read()
    assert "(bwd ? (lstm ? 3 : 2) : 1) * H + (bwd ? std::max(4 * H, head) : head)" in src and "kGradLdsMax" in src


def test_entry_points_are_declared_bound_and_refuse_null_handles():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    want = {"gaq_policy_eval_lstm_seq_dev": 14, "gaq_policy_grad_ppo_lstm_seq_dev": 22, "gaq_policy_grad_ppo_lstm_seq_idx_dev": 24}
    for name, nargs in want.items():
        assert len(sig[name]) == nargs and sig[name][1] is C.c_int32 and sig[name][2] is C.c_int64 and name + "(" in header, name
        assert hasattr(lib, name)
    assert sig["gaq_policy_grad_ppo_lstm_seq_dev"][12:17] == [C.c_float] * 5
    assert sig["gaq_policy_grad_ppo_lstm_seq_idx_dev"][3:5] == [C.c_void_p, C.c_int64]
    assert sig["gaq_policy_grad_ppo_lstm_seq_idx_dev"][14:19] == [C.c_float] * 5
    assert lib.gaq_abi_version() == 5                              # additive entry points: the ABI version stays
    assert lib.gaq_policy_eval_lstm_seq_dev(None, 2, 4, *[None] * 11) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_grad_ppo_lstm_seq_dev(None, 2, 4, *[None] * 9, 0.2, 0.2, 0.5, 0.01, 1.0, *[None] * 5) == -1
    assert b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_grad_ppo_lstm_seq_idx_dev(None, 2, 4, None, 4, *[None] * 9, 0.2, 0.2, 0.5, 0.01, 1.0, *[None] * 5) == -1
    assert b"null" in lib.gaq_last_error()


@pytest.mark.parametrize("H,D,head", [(16, 18, ()), (48, 19, (32,)), (64, 18, (16, 48))])
def test_unpack_lstm_weights_round_trips_a_gradient_shaped_vector(H, D, head):
    """pack -> unpack is the identity on the tensors, on a NumPy array and on a torch tensor, and unpack -> pack on an arbitrary vector
    of the packed size (what a gradient is): the four gate blocks land in nn.LSTMCell's shapes and order"""
    import torch
    lstm, layers = _lstm(H, D, 3), _head(H, head, 4)
    packed = P.pack_lstm_weights(lstm, layers)
    for flat in (packed, torch.tensor(packed)):
        (W_ih, W_hh, b_ih, b_hh), got = P.unpack_lstm_weights(flat, D, H, head)
        for a, b in zip((W_ih, W_hh, b_ih, b_hh), lstm):
            assert tuple(a.shape) == b.shape and np.array_equal(np.asarray(a), b)
        assert tuple(W_ih.shape) == (4 * H, D) and tuple(W_hh.shape) == (4 * H, H) and tuple(b_ih.shape) == (4 * H,)
        for (W, b), (W0, b0) in zip(got, layers):
            assert np.array_equal(np.asarray(W), W0) and np.array_equal(np.asarray(b), b0)
        assert isinstance(W_ih, type(flat))
    grad = np.random.RandomState(5).randn(packed.size).astype(np.float32)
    assert np.array_equal(P.pack_lstm_weights(*P.unpack_lstm_weights(grad, D, H, head)), grad)
    with pytest.raises(ValueError, match="packs into"):
        P.unpack_lstm_weights(packed[:-1], D, H, head)
