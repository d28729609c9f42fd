"""The edge cases of the encoder learner (tests/policy_grad_enc_edges.py): their committed seeds against the conditions, the fp64
reference of every case against torch fp64 autograd, one committed baseline row recomputed, and the LDS table from gaq.h's formulas --
the largest accepted launch, the first refused width and the encoder backward above 64 KiB -- no GPU."""
import os

import numpy as np
import pytest

from gym_art_amd import _lib
from tests import policy_grad_enc_edges as E
from tests import policy_grad_enc_ref as R

G = R.G
IDS = [c.name for c in E.EDGE_CASES]


@pytest.mark.parametrize("case", E.EDGE_CASES, ids=IDS)
def test_committed_seeds_meet_the_conditions(case):
    _, inp = E.case_inputs(case.name)
    assert R.conditions(case, inp) is None
    assert inp["done"].shape == (E.TMAX, E.SMAX) == (6, 130)
    ref = E.case_ref(case.name, 6, 130)
    assert float(np.abs(ref["dfeat"]).max()) > 0.0
    # every tensor of the encoder carries a gradient that is not within the bounds of zero
    for gW, gb in ref["g_enc"]:
        assert np.abs(gW).max() > 1e-4 and np.abs(gb).max() > 1e-4


@pytest.mark.parametrize("case", E.EDGE_CASES, ids=IDS)
def test_reference_agrees_with_torch_fp64_autograd(case):
    """tests/test_policy_grad_enc_cpu.py's tolerance: <= 1e-12 relative per parameter tensor, the encoder's included, and for logp, V
    and the sums, at every size; dfeat's product with the features is the parent reference's own dW_ih to 1e-13"""
    import torch
    _, inp = E.case_inputs(case.name)
    for T, S in E.CONFIGS:
        errs = R.torch_errors(case, inp, T, S, torch.float64, each=True)
        flat = list(errs[0]) + list(errs[1]) + list(errs[2:])
        assert max(flat) <= 1e-12, (case.name, T, S, flat)
        ref = E.case_ref(case.name, T, S)
        g = ref["g_gru" if case.cell == "gru" else "g_lstm"][0]
        assert G.rel(ref["g_wih_check"], g) <= 1e-13
        assert ref["dfeat"].shape == (T, S, case.enc[-1]) and len(ref["g_enc"]) == len(case.enc)


def test_one_committed_baseline_is_what_torch_fp32_gives_here():
    """the parent's rule: maxima over many elements within a factor of 8 of the committed numbers, the single scalars below the pooled
    bound"""
    import torch
    name = "enc112-lstm64x64x64-tanh-vclip"
    case, inp = E.case_inputs(name)
    T, S = 6, 130
    now = R.torch_errors(case, inp, T, S, torch.float32)
    was = E.BASELINE[name][T, S]
    bounds = E.bounds(name, T, S)
    print("baseline %s (6, 130): now %s | committed %s" % (name, " ".join("%.3g" % e for e in now), " ".join("%.3g" % e for e in was)))
    for k in range(4):
        assert was[k] / 8 <= now[k] <= 8 * was[k], (k, now[k], was[k])
    for k in range(4, 7):
        assert now[k] <= bounds[k], (k, now[k], bounds[k])


def test_the_case_list_is_the_stated_one():
    assert {"enc112-lstm64x64x64-tanh-vclip", "enc128x128-gru64x64-relu", "enc64x32-lstm48x32-tanh-vclip-d19", "enc128x16-gru48-relu-norm",
            "enc16x16-gru16-tanh-nohead"} <= set(E.CASES)
    assert E.CONFIGS == [(1, 1), (5, 65), (6, 130)] and set(E.CONFIGS) <= set(R.CONFIGS) and E.FACTOR == 8.0
    assert set(E.SEEDS) == set(E.BASELINE) == set(E.CASES) and not set(E.CASES) & set(R.CASES)
    assert all(s < 400 for s in E.SEEDS.values())
    assert all(set(E.BASELINE[n]) == set(E.CONFIGS) and all(len(v) == 7 for v in E.BASELINE[n].values()) for n in E.CASES)
    # what the list is for: H = 48 on both cells, a narrowing pair, the smallest pair, both layers at the limit
    assert {c.cell for c in E.EDGE_CASES if c.H == 48} == {"gru", "lstm"}
    assert any(len(c.enc) == 2 and c.enc[0] > c.enc[1] for c in E.EDGE_CASES) and (128, 16) in {c.enc for c in E.EDGE_CASES}
    assert (16, 16) in {c.enc for c in E.EDGE_CASES} and (128, 128) in {c.enc for c in E.EDGE_CASES}
    assert not {c.enc for c in E.EDGE_CASES} & {c.enc for c in R.ENC_CASES}
    assert not any(c.H == 48 for c in R.ENC_CASES)
    # the pooled entries of bounds() are the largest over BOTH lists at that size
    for T, S in E.CONFIGS:
        rows = [E.BASELINE[n][T, S] for n in E.CASES] + [R.BASELINE[n][T, S] for n in R.CASES]
        b = E.bounds("enc16x16-gru16-tanh-nohead", T, S)
        own = E.BASELINE["enc16x16-gru16-tanh-nohead"][T, S]
        assert b[:2] == (8 * own[0], 8 * own[1])
        assert b[4:] == tuple(8 * max(r[k] for r in rows) for k in (4, 5, 6))
        assert b[2:4] == (tuple(8 * max(r[k] for r in rows) for k in (2, 3)) if T * S == 1 else (8 * own[2], 8 * own[3]))


def test_the_lds_table():
    """gaq.h's formulas: the sequence kernel 8448 + 272 x (E + carried H + max(4 H, H + head)) (+ 256: the idx form), the encoder's
    backward 272 x (obs_dim rounded up to 16 + the encoder's widths), against 160 KiB -- and 64 KiB, past which a launch needs
    hipFuncSetAttribute"""
    assert E.LDS_MAX == 163840
    top = E.CASES["enc112-lstm64x64x64-tanh-vclip"]
    assert E.case_lds(top)[0] == 160768 and E.case_lds(top, idx=True)[0] == 161024 and 161024 <= E.LDS_MAX
    # the first refused width before the same cell: encoder widths are multiples of 16
    assert E.seq_lds(128, True, 64, (64, 64)) == 165120 > E.LDS_MAX
    assert E.seq_lds(128, True, 64, (64, 64), bwd=False) <= E.LDS_MAX            # ... which the forward call still takes
    # no accepted shape of the family asks for more: H and head widths <= 64, E a multiple of 16
    assert E.seq_lds(112, False, 64, (64, 64), idx=True) < 161024
    # the parent's formulas hold at its own figures (gaq.h: 118.75 KiB at 18-GRU64-64-64, 135.75 KiB at 18-LSTM64-64-64, 127.25 and
    # 144.25 KiB behind E = 64)
    assert E.seq_lds(18, False, 64, (64, 64)) == 121600 and E.seq_lds(18, True, 64, (64, 64)) == 139008
    assert E.seq_lds(64, False, 64, (64, 64)) == 130304 and E.seq_lds(64, True, 64, (64, 64)) == 147712
    for D in (18, 19):
        assert E.grad_feat_lds(D, (128, 128)) == 78336 > 65536
        assert E.grad_feat_lds(D, (128, 128), idx=True) == 78592
    assert max(E.grad_feat_lds(c.D, c.enc, True) for c in R.ENC_CASES) < 44 * 1024    # the parent list stays below
    for c in E.EDGE_CASES:
        seq, feat = E.case_lds(c, idx=True)
        print("%s: sequence kernel %d B (idx %d B), encoder backward %d B (idx %d B)" % (c.name, E.case_lds(c)[0], seq, E.case_lds(c)[1], feat))
        assert seq <= E.LDS_MAX and feat <= E.LDS_MAX
    assert [c.name for c in E.EDGE_CASES if E.case_lds(c)[1] > 65536] == ["enc128x128-gru64x64-relu"]
    # the header names the refusal, the limit and the largest accepted shape
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    for words in ("LSTM64-64-64 behind E = 128 is refused", "in_dim too large", "E = 112", "157 KiB"):
        assert words in header, words
