"""The wide learner's case list and interface without a GPU: the committed seeds meet the parents' conditions, one BASELINE entry is
torch's error today, the LDS formula's three quoted sizes, the three methods' signatures and the three entry points' declarations."""
import inspect

import numpy as np
import pytest

from tests import policy_grad_wide as W


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_committed_seeds_meet_the_conditions(name):
    case, inp = W.case_inputs(name)
    assert W.SEEDS[name] < W.SEED_LIMIT
    assert W.conditions(case, inp) is None
    assert set(W.BASELINE[name]) == set(W.ROWS)


def test_the_case_list_is_the_issues():
    assert len(W.AC_CASES) == 16 and len(W.POLICY_CASES) == 8 and len(W.CRITIC_CASES) == 8
    assert set(W.SEEDS) == set(W.CASES) == set(W.BASELINE)
    assert all(max(c.widths) > 128 and W.lds_rows(c.D, c.widths) <= W.WIDE_ROWS for c in W.CASES.values())
    assert W.SEEDS["ac-256x256-relu"] == 224 and W.SEEDS["critic-256x128x128-relu"] == 233 and W.SEEDS["ac-256x128x128-relu"] == 481


def test_one_baseline_entry_recomputed():
    """as tests/test_policy_grad_ac_cpu.py holds its table: maxima over many elements (the gradient's, logp's, V's) within a factor of 8
    of the committed numbers, the single scalars below the pooled bound"""
    import torch
    for name, first in (("ac-144-tanh-vclip", 3), ("critic-256-relu", 2)):
        case, inp = W.case_inputs(name)
        got, want = W.torch_errors(case, inp, W.R, torch.float32), W.BASELINE[name][W.R]
        print("%s: torch fp32 at %d rows: %s, committed %s" % (name, W.R, got, want))
        assert len(got) == len(want)
        for g, w in zip(got[:first], want[:first]):
            assert w / 8.0 <= g <= w * 8.0, (got, want)
        for g, b in zip(got[first:], W.bounds(name, W.R)[first:]):
            assert g <= b, (got, W.bounds(name, W.R))


def test_the_reference_adds_over_row_ranges():
    """reference(lo=) is the reference of that range: 65 rows = rows 0-63 + row 64 at one scale (what the GPU additivity test leans on)"""
    for name in ("ac-144-tanh-vclip", "policy-144-tanh", "critic-144-tanh"):
        case, inp = W.case_inputs(name)
        whole, lo, hi = W.reference(case, inp, 65), W.reference(case, inp, 64), W.reference(case, inp, 1, lo=64)
        for (a, b), (c, d), (e, f) in zip(whole["grads"], lo["grads"], hi["grads"]):
            assert np.allclose(a * 65, c * 64 + e, rtol=1e-9, atol=1e-12) and np.allclose(b * 65, d * 64 + f, rtol=1e-9, atol=1e-12)


def test_the_loops_inputs_stay_off_the_branch_edges_for_ten_steps():
    """LOOP_SEED meets loop_conditions(), and is below the search limit; the matrix's own seed of that case does not (a ratio comes
    within 1.5e-5 of the clip range's edge before step 8 of the reference trajectory): the condition has teeth"""
    case, inp = W.loop_inputs()
    assert W.LOOP_SEED < W.SEED_LIMIT and W.loop_conditions(case, inp) is None
    bad = W.loop_conditions(*W.case_inputs(W.LOOP_CASE))
    print("the matrix seed of %s: %s" % (W.LOOP_CASE, bad))
    assert bad is not None and bad.startswith("step")
    assert len(W.LOOP_BASELINE) == 6 and W.loop_bounds()[0] == W.FACTOR * W.LOOP_BASELINE[0]


def test_the_loops_forward_is_the_references_at_the_start():
    """loop_forward() restates the forward pass and the ratio on the twin module: before the first step its ratios, V and smallest
    pre-activation are A.ppo_ac's, so the margins loop_conditions() holds are margins of the reference's own quantities"""
    import torch
    for name in (W.LOOP_CASE, "ac-256x128x128-relu-vclip", "ac-256x256-relu-norm"):
        case, inp = W.loop_inputs() if name == W.LOOP_CASE else W.case_inputs(name)
        ref = W.A.ppo_ac(case, inp, W.R)
        pre, r, v = W.loop_forward(case, inp, W.A.torch_model(case, inp, torch.float64))
        assert np.allclose(r, ref["ratio"], rtol=1e-11, atol=0) and np.allclose(v, ref["value"], rtol=1e-11, atol=1e-13)
        assert abs(pre - min(float(np.abs(p).min()) for p in ref["pre"])) <= 1e-13


def test_lds_formula():
    assert W.lds_bytes(18, [256, 256]) == 156672
    assert W.lds_rows(18, [256, 256, 16]) == 560 and W.lds_bytes(18, [256, 256, 16]) == 161024 <= W.LDS_MAX
    assert W.lds_rows(18, [256, 256, 32]) == 576 and W.lds_bytes(18, [256, 256, 32]) == 165376 > W.LDS_MAX
    assert W.lds_rows(18, [256, 256, 256]) > W.WIDE_ROWS
    assert W.lds_bytes(18, [128, 128, 128], idx=False) == int(118.75 * 1024)     # the narrow actor-critic form's, as its unit states it


def test_signatures():
    from gym_art_amd.policy import MLPCritic, MLPPolicy

    def sig(f):
        return [(p.name, p.kind == p.KEYWORD_ONLY, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]
    assert sig(MLPPolicy.evaluate_wide_dev) == [("obs", False, inspect.Parameter.empty), ("actions", False, inspect.Parameter.empty),
                                                ("logp", False, None), ("value", False, None), ("mean", False, None), ("stream", False, None)]
    e = inspect.Parameter.empty
    assert sig(MLPPolicy.ppo_wide_grad_dev) == [
        ("obs", False, e), ("actions", False, e), ("logp_old", False, e), ("adv", False, e), ("ret", False, None), ("v_old", False, None),
        ("idx", True, None), ("clip", True, 0.2), ("vclip", True, None), ("vf_coef", True, 0.5), ("ent_coef", True, 0.0), ("scale", True, None),
        ("grad", True, None), ("grad_value", True, None), ("grad_log_std", True, None), ("stats", True, None), ("stream", True, None)]
    assert sig(MLPCritic.mse_wide_grad_dev) == [("obs", False, e), ("target", False, e), ("idx", True, None), ("scale", True, None),
                                                ("grad", True, None), ("stats", True, None), ("stream", True, None)]


def test_lib_declares_the_entry_points():
    import ctypes as C
    from gym_art_amd import _lib
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    P = C.c_void_p
    assert table["gaq_policy_eval_wide_dev"] == (C.c_int, [P, C.c_int64, P, P, P, P, P, P])
    assert table["gaq_policy_grad_ppo_wide_dev"] == (C.c_int, [P, C.c_int64, P, C.c_int64, P, P, P, P, P, P] + [C.c_float] * 5 + [P] * 5)
    assert table["gaq_critic_grad_mse_wide_dev"] == (C.c_int, [P, C.c_int64, P, C.c_int64, P, P, C.c_float, P, P, P])
    header = open(_lib.__file__.replace("gym_art_amd/_lib.py", "include/gaq.h")).read()
    for name in ("gaq_policy_eval_wide_dev", "gaq_policy_grad_ppo_wide_dev", "gaq_critic_grad_mse_wide_dev"):
        assert "int %s(" % name in header
    assert "#define GAQ_ABI_VERSION 5" in header
