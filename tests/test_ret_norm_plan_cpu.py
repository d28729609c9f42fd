"""tests/test_gpu_ret_norm_sizes.py without a GPU (tests/ret_norm_plan.py): that each batch size reaches what its GPU case names, that
the device's order of operations (the numpy emulation) passes every assertion the GPU file makes at every shape it runs -- the cases
are the SAME functions, driven through ret_norm_plan.Emulated instead of RetNorm --, that each of the six wrong orders
(ret_norm_plan.MUTANTS) fails one of those assertions at a named shape, that the K-aware bars are never smaller than the plain ones
for a K inside the samples, and that every kind of bar rejects an fp32 recurrence with fp32 sums by more than 100x."""
import functools

import numpy as np
import pytest

from tests import obs_norm_plan as OP
from tests import ret_norm_plan as P
from tests import ret_norm_ref as R


def _new(mutant=None):
    return functools.partial(P.Emulated, mutant=mutant)


# ---- 1. what each size reaches ----------------------------------------------------------------------------------------------------------
def test_plan_of_the_existing_sizes():
    """N = 68 and 2096, the sizes of tests/test_gpu_ret_norm.py: chunk = 1, at least 247 row groups empty, and a last workgroup whose
    waves 1 to 3 are entirely past N or (2096) not there at all"""
    assert P.plan(68) == P.Plan(1, 1, 1, 0, 255, (64, 4, 0, 0))
    assert P.plan(2096) == P.Plan(9, 1, 9, 0, 247, (48, 0, 0, 0))


def test_plan_of_the_chunk_sizes():
    """a: 257 partials are 128 full runs of two, ONE run of one and 127 empty row groups; 512 fill every row group with two; 769 are
    192 runs of four, one of one and 63 empty row groups.  Training batches of 65 536 to 2^20 envs give chunk = 1 to 16."""
    assert P.plan(65537) == P.Plan(257, 2, 128, 1, 127, (1, 0, 0, 0))
    assert P.plan(131072) == P.Plan(512, 2, 256, 0, 0, (64, 64, 64, 64))
    assert P.plan(196609) == P.Plan(769, 4, 192, 1, 63, (1, 0, 0, 0))
    assert [P.plan(n).chunk for n in (65536, 65537, 2 ** 20)] == [1, 2, 16] and P.plan(2 ** 20).empty == 0
    assert P.CHUNK_SIZES == [65537, 131072, 196609]


def test_plan_of_the_edge_sizes():
    """b: lane 0 alone; a wave one lane short, full, and one lane into the next; a workgroup whose wave 3 is partial, a full one, and one
    lane into a second workgroup whose waves 1 to 3 are past N"""
    last = {N: P.plan(N).last for N in P.EDGE_SIZES}
    assert last == {1: (1, 0, 0, 0), 63: (63, 0, 0, 0), 64: (64, 0, 0, 0), 65: (64, 1, 0, 0), 255: (64, 64, 64, 63),
                    256: (64, 64, 64, 64), 257: (1, 0, 0, 0)}
    assert [P.plan(N).nb for N in P.EDGE_SIZES] == [1, 1, 1, 1, 1, 1, 2] and {T % 4 for T in P.EDGE_STEPS} == {0, 1, 2, 3}


# ---- 2. the emulation passes every assertion of the GPU file -------------------------------------------------------------------------------
@pytest.mark.parametrize("T", P.CHUNK_STEPS)
@pytest.mark.parametrize("N", P.CHUNK_SIZES)
def test_emulation_at_the_chunk_sizes(N, T):
    P.case_chunks(_new(), N, T)


@pytest.mark.parametrize("N", P.EDGE_SIZES)
def test_emulation_at_the_edge_sizes(N):
    P.case_edges(_new(), N)
    if N == 1:
        P.case_edges(_new(), N, big=True)


def test_emulation_gamma_and_long_windows():
    for N, T in P.SHIFT_SHAPES:
        P.case_gamma_zero(_new(), N, T)
        P.case_gamma_one_dones(_new(), N)
    P.case_gamma_one_long(_new())


@pytest.mark.parametrize("N,T", P.SHIFT_SHAPES)
def test_emulation_at_the_shift_limits(N, T):
    """d.1 to d.4; d.1's relative M2 error in the device's order is about 2e-4, a hundred thousand times the plain bar"""
    figures = []
    P.case_shift_far(_new(), N, T, figures)
    (_, _, rel, over), = figures
    assert 1e-5 < rel < 1e-2 and over > 1e3, (rel, over)
    P.case_shift_empty_state(_new(), N, T)
    P.case_shift_outlier(_new(), N, T)
    P.case_shift_jump(_new(), N, T)


def test_emulation_running_merge():
    P.case_long_run(_new())
    for name in P.PRIORS:
        P.case_prior(_new(), name)


# ---- 3. every mutant dies on an assertion of the GPU file, at a named shape ----------------------------------------------------------------
def _killed(word, case, *args, **kw):
    with pytest.raises(AssertionError, match="^" + word):
        case(*args, **kw)


def test_mutant_drop_last():
    """the count is wrong at N = 65 537 (case a) and nothing is wrong at nb <= 256, where every run holds one partial"""
    _killed("count", P.case_chunks, _new("drop_last"), 65537, 2)
    _killed("count", P.case_chunks, _new("drop_last"), 196609, 5)
    P.case_edges(_new("drop_last"), 257)
    P.case_long_run(_new("drop_last"))


def test_mutant_own_K():
    """the count is right and the mean leaves its bar wherever there is a second workgroup: N = 257 (case b); N = 256 has one"""
    _killed("bars", P.case_edges, _new("own_K"), 257)
    _killed("bars", P.case_chunks, _new("own_K"), 65537, 2)
    P.case_edges(_new("own_K"), 256)


def test_mutant_no_guard():
    """the count is wrong wherever N % 256 != 0: N = 1, 63, 257 (case b); at N = 256 the mutant is the kernel"""
    for N in (1, 63, 257):
        _killed("count", P.case_edges, _new("no_guard"), N, steps=[1, 8])
    P.case_edges(_new("no_guard"), 256)


def test_mutant_done_first():
    """the carry is right and the statistics leave their bars: N = 256 (case b), T = 8 (row 1 all done)"""
    _killed("bars", P.case_edges, _new("done_first"), 256, steps=[8])
    _killed("bars", P.case_chunks, _new("done_first"), 131072, 5)


def test_mutant_stale_mean_K():
    """a state stored as count 0, mean 7 (case d.2), at both shapes: a one-valued window's M2 == 0.0 breaks -- the window of 1e-3, not
    the window of 1.7, whose shifted sums are exact under a K of 7 too (shown here), which is why d.2 runs both.  The third part of d.2
    (a stored (0, 7, 3) against a fresh object's bits on an ordinary window) is NOT a second killer of this mutant: under it the fresh
    object shifts by fp32(0) = 0 instead of reward[0], and at these shapes sums shifted by 7 and by 0 come out with the same bits
    (shown here); that part pins the unread mean and M2 of the merge instead.  Every other case has count > 0 or a stored mean of 0."""
    for N, T in P.SHIFT_SHAPES:
        rew = np.full((T, N), 1.7, np.float32)
        state, _ = P.emulate_update(rew, np.zeros((T, N), np.uint8), 0.0, None, (0.0, 7.0, 3.0), "stale_mean_K")
        assert state == (float(T * N), float(np.float32(1.7)), 0.0)
        _killed("one value: 0.001", P.case_shift_empty_state, _new("stale_mean_K"), N, T)
        rew, done = R.rollout(T, N)
        stored, fresh = (P.emulate_update(rew, done, R.GAMMA, None, st, "stale_mean_K")[0] for st in ((0.0, 7.0, 3.0), (0.0, 0.0, 0.0)))
        assert stored == fresh != P.emulate_update(rew, done, R.GAMMA, None, (0.0, 7.0, 3.0))[0]
    P.case_edges(_new("stale_mean_K"), 65)


def test_mutant_fma_carry():
    """R = fma(gamma, R, r): the inputs of N = 65, T = 8 (case b) make carry bits differ, and the carry assertion says so"""
    rew, done, _, carry = P.chain(8, 65, (0, 1, 2))[0]
    _, fused = P.emulate_update(rew, done, R.GAMMA, None, (0.0, 0.0, 0.0), "fma_carry")
    differ = int((fused.view(np.uint64) != carry.view(np.uint64)).sum())
    assert differ >= 1 and np.allclose(fused, carry, rtol=1e-15, atol=0.0), differ
    _killed("carry", P.case_edges, _new("fma_carry"), 65, steps=[8])


# ---- 4. the bars ------------------------------------------------------------------------------------------------------------------------
def test_shifted_bars_are_never_smaller_and_equal_inside_the_range():
    """stat_bars_shifted >= stat_bars for every K, and EQUAL for min R <= K <= max R: a case whose K is inside its samples loses
    nothing by using the plain bars"""
    rng = np.random.RandomState(3)
    for samples in (rng.randn(50, 37), 1e3 + 1e-2 * rng.randn(5, 68), P.chain(5, 2096, (0, 1))[0][2], np.full((3, 3), 1.7)):
        plain = R.stat_bars(samples)
        for K in (samples.min(), samples.max(), samples.flat[0], float(np.clip(np.float32(samples.mean()), samples.min(), samples.max())), 0.5 * (samples.min() + samples.max())):
            assert R.stat_bars_shifted(samples, K) == plain
        for K in (samples.min() - 1.0, samples.max() + 1e5, -1e6):
            shifted = R.stat_bars_shifted(samples, K)
            assert shifted[0] >= plain[0] and shifted[1] > plain[1]


def _fp32_moments(rew, done, gamma, carry=None):
    """(mean, M2) of an fp32 recurrence whose samples are summed in sequence in fp32: sum R and sum R^2, unshifted"""
    g32 = np.float32(gamma)
    ret = np.zeros(rew.shape[1], np.float32) if carry is None else np.asarray(carry, np.float32)
    samples = np.empty(rew.shape, np.float32)
    for t in range(rew.shape[0]):
        ret = (ret * g32 + rew[t]).astype(np.float32)
        samples[t] = ret
        ret = np.where(done[t] != 0, np.float32(0.0), ret)
    flat = samples.reshape(-1)
    s32 = np.add.accumulate(flat, dtype=np.float32)[-1]
    q32 = np.add.accumulate(flat * flat, dtype=np.float32)[-1]
    n = np.float32(flat.size)
    mean32 = np.float32(s32 / n)
    return float(mean32), float(np.float32(q32 - n * mean32 * mean32)), ret


def _rejected(what, got, ref, bars):
    fm, f2 = abs(got[0] - ref[1]) / bars[0], abs(got[1] - ref[2]) / bars[1]
    print("%s: fp32 arithmetic / bar: mean %.3g, M2 %.3g" % (what, fm, f2))
    assert fm > 100 and f2 > 100, (what, fm, f2)


def test_bars_reject_fp32_arithmetic():
    """tests/test_ret_norm_cpu.py::test_bars_reject_fp32_arithmetic's criterion on every kind of bar the GPU file uses, at a shape it
    uses it at: stat_bars (a, the smallest chunked size); stat_bars_shifted (d.1, both shapes); merge_bars fed the K-aware bars (d.4)
    and the plain ones (e, SB3's start); the 200-update bars (e).  Where a batch merges into a state, the fp32 batch moments go through
    the fp64 chan_merge, as in tests/test_obs_norm_plan_cpu.py.  On a prior count of 1e12 (e) the M2 bar rejects the fp32 batch like
    every other -- M2_b enters the merged M2 unscaled, and delta^2 na nb / n carries the batch mean's error at full size --, and the
    MEAN bar alone cannot: the merged mean takes the batch mean's error scaled by nb / n = 1e-8, below a bar that holds the prior
    mean's own roundings.  Both are asserted."""
    rew, done, s1, _ = P.chain(2, 65537, (0, 1))[0]
    _rejected("a", _fp32_moments(rew, done, R.GAMMA), R.moments(s1), R.stat_bars(s1))
    for N, T in P.SHIFT_SHAPES:
        rew, done, before = P.steady_window(T, N)
        samples, _ = R.returns(rew, done, R.GAMMA, before)
        _rejected("d.1 N=%d" % N, _fp32_moments(rew, done, R.GAMMA, before), R.moments(samples), R.stat_bars_shifted(samples, rew[0, 0]))
        low, done1, high, done2 = P.jump_windows(T, N)
        s1, c1 = R.returns(low, done1, 0.0)
        s2, _ = R.returns(high, done2, 0.0, c1)
        state, batch = R.moments(s1), R.moments(s2)
        m32, q32, _ = _fp32_moments(high, done2, 0.0, c1)
        bad = R.merge(state, (batch[0], m32, q32))
        _rejected("d.4 N=%d" % N, bad[1:], R.merge(state, batch), OP.merge_bars(state, batch, R.stat_bars_shifted(s2, np.float32(state[1]))))
    rew, done = R.rollout(P.LONG_T, P.LONG_N)
    samples, _ = R.returns(rew, done, R.GAMMA)
    state, batch = (1e-4, 0.0, 1e-4), R.moments(samples)
    m32, q32, _ = _fp32_moments(rew, done, R.GAMMA)
    _rejected("e sb3", R.merge(state, (batch[0], m32, q32))[1:], R.merge(state, batch), OP.merge_bars(state, batch, R.stat_bars(samples)))
    state = P.PRIORS["1e12"]["load"]
    bars = OP.merge_bars(state, batch, R.stat_bars(samples))
    ref = R.merge(state, batch)
    both, only_m2, only_mean = (R.merge(state, (batch[0], m, q)) for m, q in ((m32, q32), (batch[1], q32), (m32, batch[2])))
    fm, f2 = abs(both[1] - ref[1]) / bars[0], abs(both[2] - ref[2]) / bars[1]
    print("e 1e12: fp32 arithmetic / bar: mean %.3g, M2 %.3g (fp32 M2 alone %.3g, fp32 mean alone %.3g)"
          % (fm, f2, abs(only_m2[2] - ref[2]) / bars[1], abs(only_mean[2] - ref[2]) / bars[1]))
    assert f2 > 100 and abs(only_m2[2] - ref[2]) > 100 * bars[1] and abs(only_mean[2] - ref[2]) > 100 * bars[1]
    assert abs(m32 - batch[1]) > 100 * R.stat_bars(samples)[0] and batch[0] / (state[0] + batch[0]) < 2e-8 and fm < 1.0
    windows, ref, bars, _ = P.long_run()
    rew, done = np.concatenate([w[0] for w in windows]), np.concatenate([w[1] for w in windows])
    _rejected("e 200 updates", _fp32_moments(rew, done, R.GAMMA), ref, bars)
