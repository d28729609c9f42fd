"""The shared-trunk actor-critic gradient's reference (tests/policy_grad_ac_ref.py) against torch fp64 autograd of the same combined
loss on a shared trunk with two Linear heads, the conditions its cases meet, and the surface of the new entry points -- no GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P
from tests import policy_grad_ac_ref as A

IDS = [c.name for c in A.AC_CASES]


@pytest.mark.parametrize("case", A.AC_CASES, ids=IDS)
def test_reference_agrees_with_torch_fp64_autograd(case):
    """<= 1e-12 relative, per parameter tensor, for grad_value and grad_log_std, logp, V and the three sums, at every row count"""
    import torch
    _, inp = A.case_inputs(case.name)
    for rows in A.ROWS:
        assert max(A.torch_errors(case, inp, rows, torch.float64)) <= 1e-12, rows


@pytest.mark.parametrize("case", A.AC_CASES, ids=IDS)
def test_inputs_meet_the_conditions(case):
    """conditions on the inputs, not measurements: those of the net, the margins of the value clip's branches, 10 % to 70 % of the
    value gradients cut under the clip (and none without), a value delta in rows 0 and 64"""
    _, inp = A.case_inputs(case.name)
    assert A.conditions(case, inp) is None
    ref = A.ppo_ac(case, inp, A.R)
    cut = float(ref["cut"].mean())
    assert (0.1 <= cut <= 0.7) if case.vclip > 0 else cut == 0.0
    assert ref["stats"][4] == ref["cut"].sum() and ref["dv"][0] != 0.0 and ref["dv"][64] != 0.0
    assert set(A.BASELINE[case.name]) == set(A.ROWS) and (A.VF_COEF, A.ENT_COEF, A.VCLIP) == (0.5, 0.01, 0.2)


def test_the_case_list_is_the_stated_one():
    nets = {c.net.name for c in A.AC_CASES}
    for w in ("16", "64x64", "48x80x32", "128x128x128"):
        assert {"policy-%s-tanh" % w, "policy-%s-relu" % w} <= nets
    assert {"policy-64x64-tanh-d19", "policy-64x64-relu-norm"} <= nets and len(A.AC_CASES) == 2 * len(nets) == 20
    assert sorted({c.vclip for c in A.AC_CASES}) == [0.0, 0.2] and A.ROWS == [1, 63, 64, 65, 453]


def test_without_the_value_terms_the_reference_is_the_ppo_reference():
    """vf_coef = 0, ent_coef = 0: the trunk's gradient, grad_log_std and the first three sums are tests/policy_grad_ref.py's, and the
    value head's gradient is zero; the tie rule: where the clamp does not bind the gradient is e1"""
    case, inp = A.case_inputs("ac-48x80x32-relu-vclip")
    got, want = A.ppo_ac(case, inp, A.R, vf_coef=0.0, ent_coef=0.0), A.G.ppo(case.net, inp, A.R)
    for (a, b), (c, d) in zip(got["grads"], want["grads"]):
        assert np.array_equal(a, c) and np.array_equal(b, d)
    assert np.array_equal(got["glogstd"], want["glogstd"]) and np.array_equal(got["stats"][:3], want["stats"][:3])
    assert not got["gvalue"].any()
    full = A.ppo_ac(case, inp, A.R)
    free = ~full["bound"]
    assert free.any() and not full["cut"][free].any() and np.array_equal(full["e1"][free], full["e2"][free])


def test_one_committed_baseline_is_what_torch_fp32_gives_here():
    """as tests/test_policy_grad_cpu.py holds its table: maxima over many elements within a factor of 8 of the committed numbers, the
    single scalars below the pooled bound"""
    import torch
    case, inp = A.case_inputs("ac-64x64-tanh-vclip")
    got, want = A.torch_errors(case, inp, A.R, torch.float32), A.BASELINE[case.name][A.R]
    print("torch fp32 at %d rows: %s, committed %s" % (A.R, got, want))
    for g, w in zip(got[:3], want[:3]):
        assert w / 8.0 <= g <= w * 8.0, (got, want)
    for g, b in zip(got[3:], A.bounds(case.name, A.R)[3:]):
        assert g <= b, (got, A.bounds(case.name, A.R))


def test_entry_points_are_declared_bound_and_refuse_null_handles():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    for name, nargs in {"gaq_policy_eval_ac_dev": 8, "gaq_policy_grad_ppo_ac_dev": 18}.items():
        assert len(sig[name]) == nargs and sig[name][1] is C.c_int64 and name + "(" in header, name
    assert sig["gaq_policy_grad_ppo_ac_dev"][8:13] == [C.c_float] * 5
    assert lib.gaq_abi_version() == 5                              # additive entry points: the ABI version stays
    assert lib.gaq_policy_eval_ac_dev(None, 4, None, None, None, None, None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_grad_ppo_ac_dev(None, 4, None, None, None, None, None, None, 0.2, 0.2, 0.5, 0.01, 1.0, None, None, None, None,
                                          None) == -1 and b"null" in lib.gaq_last_error()


def test_python_surface():
    def sig(f):
        return str(inspect.signature(f))
    assert sig(P.MLPPolicy.evaluate_dev) == "(self, obs, actions, logp=None, value=None, mean=None, stream=None)"
    assert sig(P.MLPPolicy.ppo_ac_grad_dev) == ("(self, obs, actions, logp_old, adv, ret, v_old=None, clip=0.2, vclip=None, vf_coef=0.5, "
                                                "ent_coef=0.0, scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, "
                                                "stream=None)")
    assert sig(P.MLPPolicy.set_value_head_dev) == "(self, packed)"
    for f in (P.MLPPolicy.evaluate_dev, P.MLPPolicy.ppo_ac_grad_dev, P.MLPPolicy.set_value_head_dev):
        assert f.__doc__
