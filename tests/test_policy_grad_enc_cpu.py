"""The fp64 reference of the learner's passes for a recurrent policy with an encoder (tests/policy_grad_enc_ref.py) against torch fp64
autograd; its inputs against the conditions; its cut; one committed baseline entry recomputed; and the surface of the two new gradient
entry points and of the Python methods -- no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P
from tests import policy_grad_enc_ref as R

G = R.G
IDS = [c.name for c in R.ENC_CASES]


@pytest.mark.parametrize("case", R.ENC_CASES, ids=IDS)
def test_reference_agrees_with_torch_fp64_autograd(case):
    """<= 1e-12 relative per parameter tensor -- the cell's four, the head's, grad_value, grad_log_std, and every W and b of the encoder
    -- and for logp, V and the sums, at three sizes; dfeat's product with the features' inputs is the parent reference's own dW_ih"""
    import torch
    _, inp = R.case_inputs(case.name)
    for T, S in ((1, 1), (5, 65), (6, 130)):
        errs = R.torch_errors(case, inp, T, S, torch.float64, each=True)
        flat = list(errs[0]) + list(errs[1]) + list(errs[2:])
        assert max(flat) <= 1e-12, (case.name, T, S, flat)
        ref = R.case_ref(case.name, T, S)
        g = ref["g_gru" if case.cell == "gru" else "g_lstm"][0]
        assert G.rel(ref["g_wih_check"], g) <= 1e-13
        assert ref["dfeat"].shape == (T, S, case.enc[-1]) and len(ref["g_enc"]) == len(case.enc)


@pytest.mark.parametrize("case", R.ENC_CASES, ids=IDS)
def test_inputs_meet_the_conditions(case):
    _, inp = R.case_inputs(case.name)
    assert R.conditions(case, inp) is None
    assert inp["done"].shape == (R.TMAX, R.SMAX) and (R.TMAX, R.SMAX) == (6, 130)
    assert float(np.abs(R.case_ref(case.name, 6, 130)["dfeat"]).max()) > 0.0
    # every tensor of the encoder carries a gradient that is not within the bounds of zero
    for gW, gb in R.case_ref(case.name, 6, 130)["g_enc"]:
        assert np.abs(gW).max() > 1e-4 and np.abs(gb).max() > 1e-4


def test_the_case_list_is_the_stated_one():
    encs = {c.enc for c in R.ENC_CASES}
    assert {(16,), (48,), (80,), (32, 64), (128,)} <= encs
    assert any(c.enc == (128,) and c.cell == "gru" and c.H == 16 for c in R.ENC_CASES)
    assert {c.D for c in R.ENC_CASES} == {18, 19} and sum(c.norm for c in R.ENC_CASES) == 1
    assert {(c.act, c.out_tanh) for c in R.ENC_CASES} == {("tanh", True), ("relu", False)}
    assert {c.H for c in R.ENC_CASES} == {16, 64} and {c.cell for c in R.ENC_CASES} == {"gru", "lstm"}
    assert {c.value for c in R.ENC_CASES} == {True, False} and sum(c.vclip > 0 for c in R.ENC_CASES) == 2
    assert R.CONFIGS == [(1, 1), (1, 65), (2, 63), (5, 64), (5, 65), (6, 130)] and R.FACTOR == 8.0
    assert set(R.SEEDS) == set(R.BASELINE) == set(R.CASES)
    assert all(set(R.BASELINE[n]) == set(R.CONFIGS) and all(len(v) == 7 for v in R.BASELINE[n].values()) for n in R.CASES)
    # every backward call of the family fits the sequence kernel's LDS (gaq.h's formula), the idx form's 256 B included
    for c in R.ENC_CASES:
        E, H, hd = c.enc[-1], c.H, sum(c.head)
        assert 8448 + 272 * (E + (3 if c.cell == "lstm" else 2) * H + max(4 * H, H + hd)) + 256 <= 160 * 1024, c.name


@pytest.mark.parametrize("name", ["enc80-gru64x64-tanh-vclip", "enc32x64-lstm16-relu-norm"])
def test_a_done_cuts_the_reference_in_two(name):
    """with done[2] set everywhere every gradient of T = 6 is that of steps 0 .. 2 from the given states plus that of steps 3 .. 5 from
    zero states, the encoder's tensors included"""
    case, inp = R.case_inputs(name)
    T, S = R.TMAX, R.SMAX
    done = inp["done"].copy()
    done[2] = 1
    whole = R.ppo_enc_seq(case, inp, T, S, done=done)
    a = R.ppo_enc_seq(case, inp, 3, S, scale=1.0 / (T * S), done=done)
    zero = dict(inp, **{k: np.zeros_like(inp[k]) for k in ("h0", "c0") if k in inp})
    b = R.ppo_enc_seq(case, zero, 3, S, scale=1.0 / (T * S), t_lo=3, done=done)
    for (wW, wb), (aW, ab), (bW, bb) in zip(whole["g_enc"], a["g_enc"], b["g_enc"]):
        assert G.rel(aW + bW, wW) <= 1e-13 and G.rel(ab + bb, wb) <= 1e-13
    assert G.rel(np.concatenate([a["dfeat"], b["dfeat"]]), whole["dfeat"]) <= 1e-13
    # and without the cut the two halves do not add up: the gradient does flow across t = 2 where done[2] is clear
    whole2 = R.ppo_enc_seq(case, inp, T, S)
    a2 = R.ppo_enc_seq(case, inp, 3, S, scale=1.0 / (T * S))
    assert G.rel(a2["dfeat"], whole2["dfeat"][:3]) > 1e-3


def test_one_committed_baseline_is_what_torch_fp32_gives_here():
    """maxima over many elements within a factor of 8 of the committed numbers, the single scalars below the pooled bound"""
    import torch
    name = "enc80-gru64x64-tanh-vclip"
    case, inp = R.case_inputs(name)
    T, S = 6, 130
    now = R.torch_errors(case, inp, T, S, torch.float32)
    was = R.BASELINE[name][T, S]
    bounds = R.bounds(name, T, S)
    print("baseline %s (6, 130): now %s | committed %s" % (name, " ".join("%.3g" % e for e in now), " ".join("%.3g" % e for e in was)))
    for k in range(4):
        assert was[k] / 8 <= now[k] <= 8 * was[k], (k, now[k], was[k])
    for k in range(4, 7):
        assert now[k] <= bounds[k], (k, now[k], bounds[k])


def test_entry_points_are_declared_bound_and_refuse_null_handles():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    # the LSTM forms' arguments plus grad_enc_out after grad_out
    for name, parent in (("gaq_policy_grad_ppo_enc_seq_dev", "gaq_policy_grad_ppo_lstm_seq_dev"),
                         ("gaq_policy_grad_ppo_enc_seq_idx_dev", "gaq_policy_grad_ppo_lstm_seq_idx_dev")):
        assert len(sig[name]) == len(sig[parent]) + 1 and "int " + name + "(" in header and hasattr(lib, name), name
        k = len(sig[parent]) - 4                                     # grad_out's place: before grad_value, grad_log_std, stats, stream
        assert sig[name][:k] == sig[parent][:k] and sig[name][k] is C.c_void_p and sig[name][k + 1:] == sig[parent][k:]
    assert "float* grad_out_dev, float* grad_enc_out_dev," in header
    assert lib.gaq_abi_version() == 5
    assert lib.gaq_policy_grad_ppo_enc_seq_dev(None, 2, 4, *[None] * 9, 0.2, 0.2, 0.5, 0.01, 1.0, *[None] * 6) == -1
    assert b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_grad_ppo_enc_seq_idx_dev(None, 2, 4, None, 4, *[None] * 9, 0.2, 0.2, 0.5, 0.01, 1.0, *[None] * 6) == -1
    assert b"null" in lib.gaq_last_error()


def test_the_python_surface():
    """the parent methods' parameters plus grad_encoder=None, on both classes under the same names; thin methods over one private body"""
    sig = lambda f: str(inspect.signature(f))
    for cls, parent, parent_idx in ((P.GRUPolicy, "ppo_seq_grad_dev", "ppo_seq_grad_idx_dev"),
                                    (P.LSTMPolicy, "ppo_bptt_grad_dev", "ppo_bptt_grad_idx_dev")):
        for new, old in (("ppo_enc_seq_grad_dev", parent), ("ppo_enc_seq_grad_idx_dev", parent_idx)):
            assert sig(getattr(cls, new)) == sig(getattr(cls, old))[:-1] + ", grad_encoder=None)", (cls, new)
            assert "_ppo_enc_grad" in inspect.getsource(getattr(cls, new)) and "grad_encoder" in getattr(cls, new).__doc__
    assert hasattr(P._RecurrentPolicy, "_ppo_enc_grad")


def test_the_optimiser_entry_points_are_declared_bound_and_refuse_null_handles():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    assert sig["gaq_optim_create_policy_enc"] == sig["gaq_optim_create_policy"] and "int gaq_optim_create_policy_enc(" in header
    # gaq_optim_step_dev's arguments with grad_enc after grad
    assert sig["gaq_optim_step_enc_dev"] == sig["gaq_optim_step_dev"][:2] + [C.c_void_p] + sig["gaq_optim_step_dev"][2:]
    assert "int gaq_optim_step_enc_dev(gaq_optim* opt, const float* grad_dev, const float* grad_enc_dev," in header
    for words in ("FOURTH group placed after log_std", "Groups 0 .. 2 keep their indices", "joint over all"):
        assert words in header, words
    d, h = P.optim_desc(), C.c_void_p()
    assert lib.gaq_optim_create_policy_enc(None, C.byref(d), C.byref(h)) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_optim_step_enc_dev(None, None, None, None, None, None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_abi_version() == 5
    # the three- and the four-group kernels are the same text: each kernel defined once, a template over the group count, launched at both
    src = open(os.path.join(_lib._HERE, "csrc", "gaq_optim.hip")).read()
    for kernel in ("optim_sumsq_kernel", "optim_update_kernel", "optim_step_one_kernel"):
        assert len(re.findall(r"template <int NG> __global__ [^;{]*\bvoid %s\(OptimDevT<NG> d\) \{" % kernel, src)) == 1, kernel
        assert len(re.findall(r"\bvoid %s\(" % kernel, src)) == 1, kernel
        assert kernel + "<kOptGroups>" in src and kernel + "<kOptGroupsEnc>" in src, kernel
    assert "GAQ_OPTIM_KERNELS" not in src and "_enc_kernel" not in src


def test_adam_enc_dev_surface():
    sig = lambda f: str(inspect.signature(f))
    assert issubclass(P.AdamEncDev, P.AdamDev)
    assert sig(P.AdamEncDev.__init__) == sig(P.AdamDev.__init__)
    assert sig(P.AdamEncDev.step) == "(self, grad, grad_encoder, grad_value=None, grad_log_std=None, stats=None, stream=None, sync_log_std=True)"
    for name in ("state_dict", "load_state_dict", "set_lr", "sync_log_std", "close"):
        assert getattr(P.AdamEncDev, name) is getattr(P.AdamDev, name)
    assert "fourth group" in P.AdamEncDev.__doc__ and "gaq_optim_create_policy_enc" in P.AdamEncDev.__doc__
    with pytest.raises(ValueError, match="encoder"):
        P.AdamEncDev(object())
