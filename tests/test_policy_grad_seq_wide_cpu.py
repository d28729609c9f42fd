"""The wide recurrent learner's case list and interface without a GPU: the committed seeds meet the conditions, the single-row BASELINE
entries and one large one are torch's error today at several thread counts, the Python copy of the LDS formula at its three sizes, the two
methods' signatures and the two entry points' declarations."""
import inspect
import os
import re

import pytest

from tests import policy_grad_seq_wide as W

R = W.R


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_committed_seeds_meet_the_conditions(name):
    case, inp = W.case_inputs(name)
    assert W.SEEDS[name] < W.SEED_LIMIT
    assert R.conditions(case, inp) is None and W.conditions(case, inp) is None
    assert set(W.BASELINE[name]) == set(W.CONFIGS)
    assert all(W.conditions(case, R.inputs(case, s)) is not None for s in range(max(0, W.SEEDS[name] - 3), W.SEEDS[name]))   # (the first)


def test_the_single_row_condition_has_teeth():
    """seed 0 of gru112x16x48-tanh meets the parents' conditions and misses this list's: V and ret nearly cancel at row 0"""
    case = W.CASES["gru112x16x48-tanh"]
    inp = R.inputs(case, 0)
    bad = W.conditions(case, inp)
    print(bad)
    assert R.conditions(case, inp) is None and bad is not None and bad.startswith("|V / (V - ret)| = 57")
    case, inp = W.edge_inputs()
    assert W.conditions(case, inp) is None and len(W.EDGE_BASELINE) == 6 and W.edge_bounds()[0] == W.FACTOR * W.EDGE_BASELINE[0]


def test_the_case_list_is_the_issues():
    assert len(W.SEQ_CASES) == 20 and set(W.SEEDS) == set(W.CASES) == set(W.BASELINE)
    assert W.FACTOR == 8 and W.CONFIGS is R.CONFIGS
    nets = {(c.H, c.head, c.act, c.out_tanh, c.D, c.norm) for c in W.SEQ_CASES}
    assert nets == {(80, (), "tanh", False, 18, False), (128, (), "tanh", False, 18, False), (128, (), "relu", False, 18, False),
                    (96, (64,), "relu", False, 18, False), (112, (16, 48), "tanh", True, 18, False),
                    (128, (64, 64), "tanh", False, 18, False), (128, (64, 64), "relu", False, 18, False),
                    (128, (64, 64), "tanh", False, 19, False), (96, (64,), "relu", False, 18, True)}
    for net in nets:                                              # each with and without vclip
        assert {c.vclip for c in W.SEQ_CASES if (c.H, c.head, c.act, c.out_tanh, c.D, c.norm) == net and c.value} == {0.0, W.VCLIP}
    assert sorted(c.name for c in W.SEQ_CASES if not c.value) == ["gru128x64x64-relu-nohead", "gru80-tanh-nohead"]
    # every net is out of the narrow calls' reach and within this one's LDS, the idx form included
    assert all(64 < c.H <= 128 and c.H % 16 == 0 and W.lds_bytes(c.D, c.H, c.head, idx=True) <= W.LDS_MAX for c in W.SEQ_CASES)


def test_baseline_entries_recomputed():
    """The gradient's entry -- the one bound that is a case's own at every size -- recomputed at 1, 2 and torch's default threads: at the
    single-row size of every case, where one draw decides it, and at (6, 130) of one case, within a factor of 2 of the committed
    number; the single scalars below the pooled bound."""
    import torch
    default = torch.get_num_threads()
    try:
        for threads in (1, 2, default):
            torch.set_num_threads(threads)
            for name, (T, S) in [(c.name, (1, 1)) for c in W.SEQ_CASES] + [("gru80-tanh-vclip", (R.TMAX, R.SMAX))]:
                case, inp = W.case_inputs(name)
                got, want = R.torch_errors(case, inp, T, S, torch.float32), W.BASELINE[name][T, S]
                assert want[0] / 2.0 <= got[0] <= want[0] * 2.0, (threads, name, T, S, got, want)
                for g, b in zip(got[3:], W.bounds(name, T, S)[3:]):
                    assert g <= b, (threads, name, got, W.bounds(name, T, S))
    finally:
        torch.set_num_threads(default)


def test_lds_formula():
    """gaq.h's three sizes: 18-GRU128-64-64 is 156 416 B, the idx form 256 B more, and at H = 128 the first in_dim refused is the one
    the formula names; at one group the formula is the narrow kernel's.  This holds the Python copy (W.lds_bytes) only: what ties it
    to the library's own figure is tests/test_gpu_policy_grad_seq_wide.py's test_the_lds_edge_on_a_swarm, where 60-GRU112 (the top
    of this formula) runs and 60-GRU128 (the first it refuses) is refused."""
    assert W.lds_bytes(18, 128, (64, 64)) == 156416 <= W.LDS_MAX
    assert W.lds_bytes(18, 128, (64, 64), idx=True) == 156416 + 256 <= W.LDS_MAX
    first = next(D for D in range(1, 4096) if W.lds_bytes(D, 128, (64, 64)) > W.LDS_MAX)
    assert first == 49 and W.lds_bytes(49, 128, (64, 64)) == 165120 and W.lds_bytes(48, 128, (64, 64)) == 160768
    assert next(D for D in range(1, 4096) if W.lds_bytes(D, 128, ()) > W.LDS_MAX) == 49       # the planes, not the head, set the rows
    assert W.lds_bytes(60, 112, ()) == 156416 and W.lds_bytes(60, 128, ()) == 165120 > W.LDS_MAX    # the swarm edge of the GPU test
    assert W.lds_bytes(18, 64, (64, 64)) == int(118.75 * 1024)     # the narrow form's figure, as its unit states it
    assert W.lds_bytes(18, 128, (64, 64), bwd=False) == 8448 + 272 * (32 + 128 + 256)
    # four planes of 128 rows, the form r32 could not fit
    assert 8448 + 272 * (32 + 2 * 128 + 4 * 128) > 200 * 1024


def test_signatures():
    from gym_art_amd.policy import GRUPolicy

    def sig(f):
        return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]
    assert sig(GRUPolicy.evaluate_seq_wide_dev) == sig(GRUPolicy.evaluate_seq_dev)
    assert sig(GRUPolicy.ppo_seq_wide_grad_dev) == sig(GRUPolicy.ppo_seq_grad_dev) + [("idx", None)]
    assert sig(GRUPolicy.ppo_seq_grad_idx_dev)[1:] == sig(GRUPolicy.ppo_seq_grad_dev)          # (the idx twin's own order: idx first)


def test_lib_declares_the_entry_points():
    import ctypes as C
    from gym_art_amd import _lib
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert table["gaq_policy_eval_seq_wide_dev"] == table["gaq_policy_eval_seq_dev"]
    assert table["gaq_policy_grad_ppo_seq_wide_dev"] == table["gaq_policy_grad_ppo_seq_idx_dev"]
    assert table["gaq_policy_grad_ppo_seq_wide_dev"][1][:5] == [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "gaq.h")).read()

    def params(name):
        """the declaration's parameter types, names dropped"""
        decl = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        return [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())) for a in decl.split(",")]
    assert params("gaq_policy_eval_seq_wide_dev") == params("gaq_policy_eval_seq_dev")
    assert params("gaq_policy_grad_ppo_seq_wide_dev") == params("gaq_policy_grad_ppo_seq_idx_dev")
    assert "#define GAQ_ABI_VERSION 5" in header
