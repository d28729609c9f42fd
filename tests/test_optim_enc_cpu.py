"""The reference of the encoder policies' optimiser (tests/optim_enc_ref.py) against torch.optim.Adam / AdamW with clip_grad_norm_ in
fp64, the properties of its case list from the element counts, the conditions its gradients meet, one committed torch fp32 row
recomputed and the state layout against the library's counts -- no GPU."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P
from tests import optim_enc_ref as R
from tests import optim_ref as O
from tests.enc_util import CELLS, _desc_enc

IDS = [c.name for c in R.CASES]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_reference_agrees_with_torch_fp64(case):
    """theta, m and v of every group after each of the ten steps, and every step's norm and coef: <= 1e-12 relative"""
    import torch
    errs, scal = R.torch_errors(case, torch.float64, at=tuple(range(1, R.STEPS + 1)))
    worst = max(max(e) for k in errs for e in errs[k].values())
    print("%s: torch fp64 differs by %.3g (theta, m, v), %.3g (norm, coef)" % (case.name, worst, scal))
    assert worst <= 1e-12 and scal <= 1e-12


def test_the_case_list_is_the_stated_one():
    """each property the list is for, from the element counts: group k is [end[k-1], end[k]) of an index space cut every 2048"""
    sizes, ends = {c.name: c.sizes for c in R.CASES}, {c.name: c.ends for c in R.CASES}
    K = R.CHUNK
    assert K == 2048 and R.STEPS == 10 and R.AT == (1, 2, 10) and R.FACTOR == 8.0
    # all four groups in one chunk
    assert sizes["enc16-gru16-head-logstd"] == (1700, 17, 4, 304) and ends["enc16-gru16-head-logstd"][3] == 2025 <= K
    # both middle groups empty, with a log_std that is not learned and with none
    for name, ls in (("enc16-gru16-frozen-nohead", "frozen"), ("enc16-lstm16-det-nohead", None)):
        e = ends[name]
        assert e[0] == e[1] == e[2] < e[3] and R.BY_NAME[name].log_std == ls and not R.BY_NAME[name].head
    # the boundary inside the weights, the encoder's group wholly in the second chunk
    e = ends["enc16-lstm16-det-nohead"]
    assert sizes["enc16-lstm16-det-nohead"] == (2244, 0, 0, 304) and e[0] > K and K < e[2] and e[3] <= 2 * K
    # only the head empty; only log_std empty; each with the boundary inside the encoder's group
    e = ends["enc16x16-gru16-nohead"]
    assert e[0] == e[1] < e[2] and (e[2], e[3]) == (1704, 2280) and e[2] < K < e[3]
    e = ends["enc16x16-gru16-head-frozen"]
    assert e[0] < e[1] == e[2] and (e[2], e[3]) == (1717, 2293) and e[2] < K < e[3]
    # all four with the boundary inside the encoder's group
    e = ends["enc16x16-gru16-head-logstd"]
    assert e[0] < e[1] < e[2] and (e[2], e[3]) == (1721, 2297) and e[2] < K < e[3]
    # many chunks, the last one partial, the encoder at both width limits
    big = R.BY_NAME["enc128x128-gru16-head-logstd"]
    assert big.enc == (128, 128) and big.D == 19 and big.sizes == (7076, 17, 4, 19072) and big.ends[3] == 26169
    assert big.ends[3] > 12 * K and big.ends[3] % K and big.ends[2] // K != (big.ends[3] - 1) // K
    # no group of any case ends on a wave or chunk boundary by accident of the sizes being round
    assert all(e % 64 for c in R.CASES for e in set(c.ends))
    assert {c.cell for c in R.CASES} == {"gru", "lstm"}
    assert set(R.BASELINE) == set(sizes) and all(set(R.BASELINE[n]) == set(R.AT) for n in sizes)
    assert all(len(R.BASELINE[n][k][w]) == 4 for n in sizes for k in R.AT for w in ("theta", "m", "v"))
    # an empty group has no error to bound, a present one has
    for c in R.CASES:
        for k in R.AT:
            for w in ("theta", "m", "v"):
                assert [x > 0 for x in R.BASELINE[c.name][k][w]] == [s > 0 for s in c.sizes], (c.name, k, w)


def test_the_hyper_parameters_vary_as_the_parents_do():
    assert sorted(c.clip for c in R.CASES if c.clip) == ["above", "below"]
    assert any(c.hp["weight_decay"] > 0 and c.log_std == "learn" for c in R.CASES) and any(c.hp["weight_decay"] == 0 for c in R.CASES)
    assert any(c.hp["max_grad_norm"] is None for c in R.CASES)
    assert any(c.hp["betas"] != (0.9, 0.999) for c in R.CASES) and any(c.hp["eps"] != 1e-8 for c in R.CASES)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_inputs_meet_the_conditions(case):
    """tests/test_optim_cpu.py's conditions: magnitudes over [1e-6, 10], about 5 % exact zeros, gradients that change from step to
    step, the stated side of the clip at every step"""
    g = [np.concatenate(R.gradients(case, k)) for k in range(R.STEPS)]
    for x in g:
        nz = np.abs(x[x != 0])
        assert 1e-6 * 0.999 <= nz.min() and nz.max() <= 10.0 and nz.min() < 1e-4 and nz.max() > 1.0
        assert 0.01 <= float((x == 0).mean()) <= 0.1
    assert not np.array_equal(g[0], g[1])
    assert [x.size for x in R.gradients(case, 0)] == list(case.sizes) == [x.size for x in R.theta0(case)]
    stats = [r[3] for r in R.reference(case.name)]
    if case.clip == "above":
        assert all(s[0] > 20.0 * case.hp["max_grad_norm"] and s[1] < 0.05 for s in stats)
    if case.clip == "below":
        assert all(s[0] < 0.05 * case.hp["max_grad_norm"] and s[1] == 1.0 for s in stats)
    assert [s[2] for s in stats] == list(range(1, R.STEPS + 1)) and not any(s[3] for s in stats)


def test_the_encoder_rides_behind_the_weights_with_their_arithmetic():
    """the four-group reference is optim_ref's step on [weights | encoder], head, log_std: the joint norm is over all four, weight
    decay reaches the encoder and never log_std"""
    case = R.BY_NAME["enc16x16-gru16-head-logstd"]
    th, g = R.theta0(case), R.gradients(case, 0)
    got = R.trajectory(case, 1)[0]
    norm = float(np.sqrt(sum(np.sum(x.astype(np.float64) ** 2) for x in g)))
    assert abs(got[3][0] - norm) <= 1e-12 * norm
    st = O.State([th[3], np.zeros(0), th[2]])                      # the encoder alone in slot 0, log_std in its slot: no clip
    O.step(st, [g[3], np.zeros(0), g[2]], **case.hp)
    assert np.array_equal(st.theta[0], got[0][3]) and np.array_equal(st.theta[2], got[0][2])
    nodecay = R.Case("enc16x16-gru16-head-logstd", "gru", (16, 16), [16])
    other = R.trajectory(nodecay, 1)[0]
    assert np.array_equal(other[0][2], got[0][2]) and not np.array_equal(other[0][3], got[0][3])


def test_one_committed_baseline_is_what_torch_fp32_gives_here():
    """the parent's rule: maxima over many elements within a factor of 8 of the committed numbers"""
    import torch
    case = R.BY_NAME["enc128x128-gru16-head-logstd"]
    got, _ = R.torch_errors(case, torch.float32)
    want = R.BASELINE[case.name]
    print("torch fp32: %s, committed %s" % (got, want))
    for k in R.AT:
        for what in ("theta", "m", "v"):
            for group in (0, 3):
                g, w = got[k][what][group], want[k][what][group]
                assert w / 8.0 <= g <= w * 8.0, (k, what, group, got, want)
    assert R.bound(case.name, 1, "theta", 3) == max(8.0 * want[1]["theta"][3], 2.0 ** -24)
    assert R.bound("enc16-lstm16-det-nohead", R.STEPS, "theta", 1) == R.STEPS * 2.0 ** -24     # the floor: one rounding per step


def test_the_counts_are_the_librarys():
    lib = _lib.load()
    for case in R.CASES:
        nw, nh, nl, ne = case.sizes
        assert ne == P.encoder_weight_count(case.D, case.enc)
        d = _desc_enc(case.widths, case.enc, enc_in=case.D, cell=CELLS[case.cell])
        assert lib.gaq_policy_encoder_weight_count(C.byref(d)) == ne
        dr = P._fill_desc(P._DescRnn(), case.enc[-1], case.widths, "tanh", out_tanh=0, engine=P.ENGINES["mfma"],
                          cell=P.CELL_GRU if case.cell == "gru" else P.CELL_LSTM)
        assert lib.gaq_policy_weight_count_rnn(C.byref(dr)) == nw
        groups, total = P.optim_groups(nw, case.widths[-1] if case.head else None, case.log_std == "learn")
        assert total == nw + nh + nl == case.ends[2] and total + ne == case.ends[3]
        assert [g[0] for g in groups] == [n for n, s in zip(R.GROUPS[:3], case.sizes[:3]) if s]
