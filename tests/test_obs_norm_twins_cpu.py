"""The argument of tests/test_gpu_obs_norm_twins.py made checkable without a GPU (tests/obs_norm_twins_plan.py): the table it attaches
publishes its power-of-two scales exactly, scaling the observation and scaling the first layer's weights give the same bits in a float32
fmaf chain and after rounding to bf16, the three ways a twin could be wrong that the identity table cannot see each change nearly every
first-layer sum, and the GPU file's case lists reach the shapes its docstring claims."""
import os
import re

import numpy as np
import pytest

from tests import obs_norm_ref as R
from tests import obs_norm_twins_plan as P
from tests.test_gpu_policy_shapes import OBS, _batches, _style

UNITS = 16                                       # one chunk of a first layer


def _rows(D, rows=256, seed=0):
    """random fp32 rows of the size of observations, with exact zeros and -0.0 sprinkled in (an env at rest, a padded feature)"""
    rng = np.random.RandomState(100 * D + seed)
    x = (rng.randn(rows, D) * (1.0 + np.arange(D) % 4)).astype(np.float32)
    hit = rng.rand(rows, D)
    x[hit < 0.05] = 0.0
    x[hit > 0.95] = -0.0
    assert np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any()
    return x


def _layer(D, seed=0):
    rng = np.random.RandomState(7000 + 10 * D + seed)
    return (rng.randn(UNITS, D) / np.sqrt(D)).astype(np.float32), (0.1 * rng.randn(UNITS)).astype(np.float32)


def test_widths_are_the_env_layouts():
    assert [d for _, _, d in OBS] == R.WIDTHS == P.WIDTHS and len(P.WIDTHS) == 11


@pytest.mark.parametrize("D", R.WIDTHS)
def test_the_table_publishes_the_scales_exactly(D):
    s = P.scales(D)
    assert s.dtype == np.float32 and set(s.tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0}
    assert np.all(s[1:] != s[:-1])                                  # adjacent columns differ
    assert s[D - 1] != s[0] or s[D - 1] != s[1]
    var = s.astype(np.float64) ** -2
    assert np.array_equal(1.0 / var, s.astype(np.float64) ** 2)     # the variances are exact in float64
    mean32, inv32 = R.table(1.0, np.zeros(D), var, 0.0)
    assert np.array_equal(P.bits(inv32), P.bits(s)) and np.array_equal(P.bits(mean32), P.bits(np.zeros(D, np.float32)))
    # and the element expression under it is the exact scaling, signed zeros included
    x = _rows(D)
    z = R.normalize(x, mean32, inv32, np.inf)
    assert np.array_equal(P.bits(z), P.bits(P.staged(x, s)))
    assert np.array_equal(z.astype(np.float64), x.astype(np.float64) * s.astype(np.float64))
    assert np.array_equal(np.signbit(z), np.signbit(x))
    ones, zeros = np.ones((1, D), np.float32), np.zeros((1, D), np.float32)
    assert np.array_equal(R.normalize(ones, mean32, inv32, np.inf)[0], s) and not P.bits(R.normalize(zeros, mean32, inv32, np.inf)).any()


@pytest.mark.parametrize("D", R.WIDTHS)
def test_scaling_the_input_or_the_weights_gives_the_same_bits(D):
    """one ascending fmaf chain per unit: (x s, W) against (x, W s)"""
    s = P.scales(D)
    for seed in range(3):
        x, (W, b) = _rows(D, seed=seed), _layer(D, seed)
        Ws = (W * s[None, :]).astype(np.float32)
        assert np.array_equal(Ws.astype(np.float64), W.astype(np.float64) * s[None, :].astype(np.float64))       # exact
        a, c = P.fmaf_chain(P.staged(x, s), W, b), P.fmaf_chain(x, Ws, b)
        assert np.isfinite(a).all() and np.array_equal(P.bits(a), P.bits(c)), (D, seed)
        assert not np.array_equal(P.bits(a), P.bits(P.fmaf_chain(x, W, b)))      # (the scales do something)


def _bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("D", R.WIDTHS)
def test_the_same_after_rounding_to_bf16(D):
    """the bf16 engine rounds the staged value and the weights (torch's CPU bfloat16 is the rounding): rounding commutes with the
    power-of-two scaling, and the chain on the rounded values gives the same bits either way"""
    s = P.scales(D)
    x, (W, b) = _rows(D), _layer(D)
    xs_b, x_b = _bf16(P.staged(x, s)), _bf16(x)
    W_b, Ws_b = _bf16(W), _bf16((W * s[None, :]).astype(np.float32))
    assert np.array_equal(P.bits(xs_b), P.bits(x_b * s[None, :])) and np.array_equal(P.bits(Ws_b), P.bits(W_b * s[None, :]))
    assert not np.array_equal(x_b, x)                               # (the rounding does something)
    a, c = P.fmaf_chain(xs_b, W_b, b), P.fmaf_chain(x_b, Ws_b, b)
    assert np.isfinite(a).all() and np.array_equal(P.bits(a), P.bits(c))


@pytest.mark.parametrize("mutant", P.MUTANTS)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_a_wrong_twin_changes_nearly_every_first_layer_sum(D, mutant):
    """the scale taken from column k + 1, the scale dropped, and `dim` off by one: the identity table (mean 0, scale 1) hides all
    three; under these scales each changes the first layer's sums in more than 99 % of the rows"""
    s = P.scales(D)
    x, (W, b) = _rows(D), _layer(D)
    good = P.bits(P.fmaf_chain(P.staged(x, s), W, b))
    bad = P.bits(P.fmaf_chain(P.staged(x, s, mutant), W, b))
    changed = (good != bad).any(axis=1).mean()
    assert changed > 0.99, (D, mutant, changed)
    one = np.ones(D, np.float32)                                    # ... and under the identity table the first two change nothing
    if mutant != "dim_minus_one":                                   # (the last column of "next_column" reads the clip)
        assert np.array_equal(P.bits(P.staged(x, one, mutant)[:, :-1]), P.bits(P.staged(x, one)[:, :-1]))


# ---- the case lists -----------------------------------------------------------------------------------------------------------------
def _all_cases():
    out = [c for obs in OBS for _, cases in P.sweep(obs) for c in cases]
    return out + [c for _, c in P.extras()]


def test_what_each_width_reaches():
    want_partial = {13: 1, 14: 2, 18: 2, 19: 3, 20: 0, 22: 2, 25: 1, 24: 0, 36: 0, 60: 0, 108: 0}
    want_bf16 = {13: 1, 14: 1, 18: 1, 19: 1, 20: 1, 22: 1, 25: 1, 24: 1, 36: 2, 60: 2, 108: 4}
    for D in R.WIDTHS:
        assert P.partial_k_step(D) == want_partial[D] and P.bf16_k_steps(D) == want_bf16[D], D
        assert 4 * (P.k_steps(D) - 1) < D <= 4 * P.k_steps(D) and 32 * (P.bf16_k_steps(D) - 1) < D <= 32 * P.bf16_k_steps(D)
    assert {P.partial_k_step(D) for D in R.WIDTHS} == {0, 1, 2, 3}
    assert all(P.k_steps(D) % 2 == 1 and P.partial_k_step(D) == 0 for D in (20, 36, 60, 108))      # no padding, an odd count
    assert P.k_steps(24) == 6 and {P.bf16_k_steps(D) for D in (36, 60, 108)} == {2, 4}


def test_every_family_runs_at_every_width_and_every_twin_is_reached():
    assert len(P.KERNELS) == 13 == len(set(P.KERNELS))
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "gym_art_amd", "csrc", "gaq_policy.hip")).read()
    # each name of P.KERNELS labels the <PolObsNorm> instantiation of one __global__ template: those that take the normaliser parameter
    taking = re.findall(r"^template <[^\n]*>\n__global__[^\n]*\nvoid (\w+)\([^)]*\bNorm\.\.\. nm\)", src, re.M)
    assert sorted(taking) == sorted({k.replace("_norm_kernel", "_kernel") for k in P.KERNELS})
    assert not re.search(r"\w+_norm_kernel\b", src)                 # and none is written out a second time
    for obs in OBS:
        fams = P.sweep(obs)
        assert [f for f, _ in fams] == list(P.FAMILIES)
        assert {k for f, _ in fams for k in P.FAMILIES[f].kernels} == set(P.KERNELS), obs
        for family, cases in fams:
            want = _batches(obs[1])
            assert [c.N for c in cases] == (want if family in P.BIG_BATCH_FAMILIES else want[:3]), (obs, family)
            assert all(c.D == obs[2] and c.layout == "alias" and not c.stagger and not c.single for c in cases)
            assert all(n % max(1, obs[1]) == 0 for n in want)       # whole swarms
    assert P.BIG_BATCH_FAMILIES == ("mlp_ac", "lstm_ac")
    for family, fam in P.FAMILIES.items():
        assert ("tv" in fam.ask) == any("term" in k for k in fam.kernels), family
        assert fam.critic == any(k.startswith("critic_") for k in fam.kernels), family


def test_the_nets_are_the_smallest_that_reach_each_path():
    assert P.MLP_NETS == [[48], [80, 48]] and P.BF16_NETS == [[48, 48], [144, 48]]
    assert P.REC_H == [48, 80] and P.REC_HEADS == [(), (16, 80)]
    n = len(R.WIDTHS)
    for family, fam in P.FAMILIES.items():
        nets = [P.net_of(family, i) for i in range(n)]
        if fam.kind in ("mlp", "bf16"):
            seen = {(tuple(net.widths), _style(net.k)[0]) for net in nets}
            assert len(seen) == 4, (family, seen)                   # both nets with both activations
        else:
            assert {(net.H, net.head) for net in nets} == {(H, h) for H in P.REC_H for h in P.REC_HEADS}, family
            assert {_style(net.k)[0] for net in nets if net.head} == {"tanh", "relu"}, family
        assert {_style(net.k)[1] for net in nets} == {True, False}, family
        assert all((net.critic is not None) == fam.critic for net in nets)
    # chunks of wave w: (width / 16 - w + 3) / 4 -- wave 3 idle at 3 chunks; 5 chunks give wave 0 a second one
    assert [(w // 16 - 3 + 3) // 4 for w in (48, 80)] == [0, 1] and [(w // 16 - 0 + 3) // 4 for w in (48, 80)] == [1, 2]


def test_the_extra_cases():
    ex = dict(P.extras())
    assert len(ex) == len(P.extras())
    for family in ("gru_ac", "lstm_ac"):
        for n in (1, 63, 65):
            c = ex["d20-%s-n%d" % (family, n)]
            assert (c.family, c.D, c.N, c.single) == (family, 20, n, False)
        for n in (16, 2096):
            c = ex["d108-%s-h256-n%d" % (family, n)]
            assert (c.D, c.N, c.net.H, c.net.head) == (108, n, 256, ()) and "v" in P.FAMILIES[c.family].ask
    # the LDS is at its limit there: 157 KiB of the CU's 160
    assert P.recurrent_ac_lds(108, 256) == 157 * 1024 <= 160 * 1024
    assert P.recurrent_ac_lds(108, 256, (16, 80)) == 157 * 1024 and P.recurrent_ac_lds(18, 256) == 2048 + 256 * (20 + 512)
    c = ex["d108-mlp256x3-critic256x2"]
    assert (c.family, c.D, c.net.widths, c.net.critic) == ("mlp_critic", 108, [256, 256, 256], [256, 256]) and c.N == _batches(16)[2]
    for family in P.FAMILIES:                                       # one staggered case per family: passes of 67 and 63 rows
        c = ex["d19-%s-staggered" % family]
        assert (c.family, c.D, c.N, c.stagger) == (family, 19, 130, True) and P.partial_k_step(c.D) == 3
        assert (c.N - P.STAGGER_MASKED, P.STAGGER_MASKED) == (67, 63) and P.STAGGER_AFTER == 5
    for D in (13, 108):
        for family in ("mlp_ac", "lstm_ac"):
            assert {ex["d%d-%s-%s" % (D, family, layout)].layout for layout in ("alias", "plain")} == {"alias", "plain"}
    assert sum(1 for c in ex.values() if c.layout == "plain") == 4


def test_every_multi_step_call_is_16_byte_aligned():
    """a T > 1 call needs N D 4 bytes to be a multiple of 16; the cases that are not run their window as calls of one step"""
    cases = _all_cases()
    assert len(cases) == 11 * (9 * 3 + 2) + len(P.extras())
    for c in cases:
        assert c.single == ((c.N * c.D) % 4 != 0), c
        assert c.family in P.FAMILIES and c.D in R.WIDTHS and P.T == 20
    assert [(c.D, c.N) for c in cases if c.single] == [(19, 130)] * len(P.FAMILIES)
    assert all((n * 20) % 4 == 0 for n in (1, 63, 65))
