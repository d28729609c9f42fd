"""The return normaliser's update (gaq_learn.hip: gaq_ret_norm_update_dev = ret_norm_partial_kernel, then obs_norm_merge_kernel with
D = 1) restated in numpy fp64: what a batch size N reaches (plan), the device's order of operations with six wrong orders
(emulate_update, MUTANTS), and the cases of tests/test_gpu_ret_norm_sizes.py written once against a small interface (Emulated here,
RetNorm on the device there), so that tests/test_ret_norm_plan_cpu.py runs THE SAME assertions on the emulation and on its mutants
without a GPU: a mutant is dead when the assertion the GPU file makes at a named shape fails on it.

emulate_update is NOT expected to equal the device's statistics bit for bit: the device computes q += d d as one fma, and the compiler
may contract the expressions of obs_moments_merge where numpy rounds twice.  It has the device's ORDER, so its distance from a two-pass
reference is what the algorithm as written costs.  The carry IS bit-exact: the kernel forbids contraction of R = gamma R + r."""
import collections
import fractions
import functools

import numpy as np

from tests import obs_norm_plan as P
from tests import ret_norm_ref as R
from tests.test_gpu_ret_norm import _bits

BLOCK = 256                  # kBlock: lanes of a workgroup of ret_norm_partial_kernel, one env each
WAVE = 64
GROUPS = 256                 # kObsNormBlock / D with D = 1: the row groups of obs_norm_merge_kernel

Plan = collections.namedtuple("Plan", "nb chunk full partial empty last")
MUTANTS = ["drop_last", "own_K", "no_guard", "done_first", "stale_mean_K", "fma_carry"]


def plan(N):
    """What N envs reach: nb = ceil(N / 256) workgroups (never capped), chunk = ceil(nb / 256) partials per row group of the merge
    launch, the row groups whose run [g chunk, min((g + 1) chunk, nb)) is full (chunk partials), partial (fewer, not none) and empty,
    and `last`, the live lanes of the last workgroup's four waves."""
    nb = -(-N // BLOCK)
    chunk = -(-nb // GROUPS)
    runs = [min((g + 1) * chunk, nb) - min(g * chunk, nb) for g in range(GROUPS)]
    live = N - (nb - 1) * BLOCK
    last = tuple(min(max(live - WAVE * w, 0), WAVE) for w in range(BLOCK // WAVE))
    return Plan(nb, chunk, runs.count(chunk), sum(1 for r in runs if 0 < r < chunk), runs.count(0), last)


# ---- the device's order -----------------------------------------------------------------------------------------------------------------
def _merge1(a, b):
    """obs_moments_merge on Python floats (fp64), with its two early returns"""
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n, delta = a[0] + b[0], b[1] - a[1]
    return n, a[1] + delta * (b[0] / n), a[2] + b[2] + delta * delta * (a[0] * b[0] / n)


def _fma(a, b, c):
    """a b + c with ONE rounding, element by element (exact rational arithmetic, then the correctly rounded float)"""
    F = fractions.Fraction
    return np.array([float(F(float(a)) * F(float(y)) + F(float(z))) for y, z in zip(b, c)], np.float64)


def emulate_update(rew, done, gamma, carry, state, mutant=None):
    """((count, mean, M2), carry [N]) in float64 after gaq_ret_norm_update_dev of rew [T, N] (fp32) and done [T, N] on the running
    `state` = (count, mean, M2) and the per-env `carry` (None: zeros), in the device's order.
    ret_norm_partial_kernel: K = fp32(state mean) where count > 0, else reward[0, 0]; lane i < N runs R = gamma R + r (product and sum
    rounded separately), d = R - K, s += d, q += d d over t ascending, then R = 0 where done; its shifted moments are
    (T, s / T, max(q - s^2 / T, 0)), a lane with i >= N holds (0, 0, 0).  The __shfl_down tree o = 1, 2, ... 32 leaves in lane 0 of each
    wave the pairwise tree merge(merge(l0, l1), merge(l2, l3)) ... of its 64 lanes; the four waves merge in ascending order into one
    partial per workgroup.  obs_norm_merge_kernel, D = 1: row group g merges partials [g chunk, min((g + 1) chunk, nb)) in ascending
    order, the 256 row groups merge in ascending order, K is added to the mean and the batch merges into the state.
    mutant -- "drop_last": a row group's run stops one partial early where it holds more than one; "own_K": workgroup b shifts by
    reward[0, 256 b] while the merge adds back workgroup 0's; "no_guard": a lane with i >= N contributes T samples of value K;
    "done_first": R is cleared before it is sampled; "stale_mean_K": K = fp32(state mean) even where count = 0; "fma_carry":
    R = fma(gamma, R, r), one rounding."""
    assert mutant is None or mutant in MUTANTS, mutant
    rew, done = np.asarray(rew, np.float32), np.asarray(done) != 0
    T, N = rew.shape
    p = plan(N)
    L = p.nb * BLOCK
    g = np.float64(np.float32(gamma))
    count, smean, sm2 = (float(v) for v in state)
    K0 = np.float64(np.float32(smean) if (count > 0 or mutant == "stale_mean_K") else rew[0, 0])
    lane = np.arange(L)
    if mutant == "own_K":
        K0 = np.float64(rew[0, 0])
        K = rew[0, BLOCK * (lane // BLOCK)].astype(np.float64)
    else:
        K = np.full(L, K0)
    live = lane < N
    Rv = np.zeros(L)
    if carry is not None:
        Rv[:N] = np.asarray(carry, np.float64)
    x, dn = np.zeros((T, L)), np.zeros((T, L), bool)
    x[:, :N], dn[:, :N] = rew, done
    s, q = np.zeros(L), np.zeros(L)
    for t in range(T):
        if mutant == "fma_carry":
            Rv = _fma(g, Rv, x[t])
        else:
            Rv = g * Rv
            Rv = Rv + x[t]
        cleared = np.where(dn[t], 0.0, Rv)
        d = (cleared if mutant == "done_first" else Rv) - K
        s = s + d
        q = q + d * d
        Rv = cleared
    cnt = float(T)
    m2 = np.maximum(q - s * s / cnt, 0.0)
    if mutant == "no_guard":
        m = (np.full(L, cnt), np.where(live, s / cnt, 0.0), np.where(live, m2, 0.0))
    else:
        m = (np.where(live, cnt, 0.0), np.where(live, s / cnt, 0.0), np.where(live, m2, 0.0))
    m = tuple(v.reshape(p.nb, BLOCK // WAVE, WAVE) for v in m)
    o = 1
    while o < WAVE:                                                            # lane l takes lane l + o: pairs, pairs of pairs, ...
        m = P._merge(tuple(v[..., 0::2] for v in m), tuple(v[..., 1::2] for v in m))
        o <<= 1
    part = tuple(v[:, 0, 0] for v in m)
    for w in range(1, BLOCK // WAVE):
        part = P._merge(part, tuple(v[:, w, 0] for v in m))                    # [nb]
    gi = np.arange(GROUPS)[:, None]
    b = gi * p.chunk + np.arange(p.chunk)[None, :]                             # [G, chunk]: the partial row group g merges j-th
    b1 = np.minimum((gi + 1) * p.chunk, p.nb)
    if mutant == "drop_last":
        b1 = np.where(b1 - gi * p.chunk > 1, b1 - 1, b1)
    run = tuple(np.where(b < b1, v[np.minimum(b, p.nb - 1)], 0.0) for v in part)               # n = 0: merged as nothing
    mine = tuple(np.zeros(GROUPS) for _ in range(3))
    for j in range(p.chunk):
        mine = P._merge(mine, tuple(v[:, j] for v in run))
    batch = (0.0, 0.0, 0.0)
    for k in range(GROUPS):
        batch = _merge1(batch, tuple(float(v[k]) for v in mine))
    batch = (batch[0], batch[1] + float(K0), batch[2])
    return _merge1((count, smean, sm2), batch), Rv[:N].copy()


class Emulated:
    """emulate_update behind the interface the cases below drive (tests/test_gpu_ret_norm_sizes.py has the device's)"""

    def __init__(self, N, gamma=R.GAMMA, from_stats=None, mutant=None):
        self.N, self.gamma, self.mutant = N, gamma, mutant
        self.state, self.carry = (0.0, 0.0, 0.0), np.zeros(N)
        if from_stats is not None:
            var, count, mean = from_stats
            self.load(count, mean, float(var) * float(count))

    def load(self, count, mean, m2, returns=None):
        self.state = (float(count), float(mean), float(m2))
        if returns is not None:
            self.carry = np.array(returns, np.float64)

    def update(self, rew, done):
        self.state, self.carry = emulate_update(rew, done, self.gamma, self.carry, self.state, self.mutant)

    def stats(self):
        return self.state

    def returns(self):
        return self.carry

    def table(self):
        pass

    def close(self):
        pass


# ---- the shapes and data of tests/test_gpu_ret_norm_sizes.py --------------------------------------------------------------------------
CHUNK_SIZES = [65537, 131072, 196609]     # a: nb = 257, 512, 769
CHUNK_STEPS = [2, 5]
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257]
EDGE_STEPS = [1, 2, 3, 4, 7, 8]           # around the loop's unroll of 4
SHIFT_SHAPES = [(2096, 5), (68, 20)]      # c, d: the two sizes of tests/test_gpu_ret_norm.py, where the present bars were measured
LONG_N, LONG_T, LONG_UPDATES = 2096, 5, 200
CARRY_1E5 = 1e5                           # d.1: the steady state of rewards of 1e3 at gamma 0.99


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def chain(T, N, seeds, gamma=R.GAMMA, big=False):
    """successive windows of R.rollout(T, N, seed) from a zero carry: a list of (rew, done, samples so far [k T, N], carry), read-only.
    big: every env at 1e3 + 1e-2 randn (R.rollout leaves N = 1 with unit normals only)"""
    out, carry, seen = [], None, []
    for seed in seeds:
        rew, done = R.rollout(T, N, seed)
        if big:
            rew = (1e3 + 1e-2 * np.random.RandomState(7 + T + seed).randn(T, N)).astype(np.float32)
        samples, carry = R.returns(rew, done, gamma, carry)
        seen.append(samples)
        out.append(_ro(rew, done, np.concatenate(seen), carry))
    return out


def steady_window(T, N):
    """d.1: (rew, done, carry before) -- rewards 1e3 +- 1e-2, no dones, every env's return loaded at its steady state 1e5"""
    rew = (1e3 + 1e-2 * np.random.RandomState(11 * T + N).randn(T, N)).astype(np.float32)
    return _ro(rew, np.zeros((T, N), np.uint8), np.full(N, CARRY_1E5))


def jump_windows(T, N):
    """d.4: unit-normal rewards, then rewards at 1e5 +- 0.1; the dones of R.rollout (gamma is 0: the samples are the rewards)"""
    rng = np.random.RandomState(13 * T + N)
    low = rng.randn(T, N).astype(np.float32)
    high = (1e5 + 0.1 * rng.randn(T, N)).astype(np.float32)
    return _ro(low, R.rollout(T, N)[1], high, R.rollout(T, N, 1)[1])


def long_rewards(T=1000, N=68):
    """c: rewards 1 + 0.5 randn without dones: at gamma = 1 the returns grow to about T"""
    rew = (1.0 + 0.5 * np.random.RandomState(17).randn(T, N)).astype(np.float32)
    return _ro(rew, np.zeros((T, N), np.uint8))


@functools.lru_cache(maxsize=None)
def long_run():
    """e: LONG_UPDATES windows of R.rollout(LONG_T, LONG_N, seed) -> ([(rew, done)], two-pass moments of all samples, bars, carry).
    The bars are obs_norm_plan.steps_bars of the samples as one column: 8 (n + updates) u times max|R| (mean) and n range^2 (M2)."""
    windows, seen, carry = [], [], None
    for seed in range(LONG_UPDATES):
        rew, done = R.rollout(LONG_T, LONG_N, seed)
        samples, carry = R.returns(rew, done, R.GAMMA, carry)
        windows.append((rew, done))
        seen.append(samples)
    s = np.concatenate(seen).reshape(-1)
    bars = tuple(float(b[0]) for b in P.steps_bars(s[:, None], LONG_UPDATES))
    return windows, R.moments(s), bars, _ro(carry)[0]


# ---- the assertions ---------------------------------------------------------------------------------------------------------------------
def _frac(err, bar):
    return float(err / bar) if bar > 0 else (0.0 if err == 0 else float("inf"))


def check(norm, ref, bars, carry, what, worst=None):
    """the count exact, the carry bit for bit `carry`, mean and M2 within bars = (mean, M2) of ref = (count, mean, M2); the published
    table through norm.table(); -> (mean error / bar, M2 error / bar), folded into `worst`.  A bar of 0 demands equality."""
    count, mean, m2 = norm.stats()
    em, e2 = abs(mean - ref[1]), abs(m2 - ref[2])
    fr = (_frac(em, bars[0]), _frac(e2, bars[1]))
    assert count == ref[0], "count: %s: %r, expected %r" % (what, count, ref[0])
    got = norm.returns()
    assert got.shape == np.shape(carry) and np.array_equal(_bits(got), _bits(carry)), "carry: %s: not the fp64 recurrence bit for bit" % (what,)
    assert em <= bars[0] and e2 <= bars[1], "bars: %s: error / bar: mean %.3g, M2 %.3g" % (what, fr[0], fr[1])
    norm.table()
    if worst is not None:
        worst[0], worst[1] = max(worst[0], fr[0]), max(worst[1], fr[1])
    return fr


def _in_range(K, samples):
    return samples.min() <= K <= samples.max()


def _report(group, what, worst):
    print("%s %s: worst error / bar: mean %.3g, M2 %.3g" % (group, what, worst[0], worst[1]))
    return tuple(worst)


def case_chunks(new, N, T):
    """a. one update (two fresh objects: the same bits) and two updates on top of each other at nb > 256"""
    (rew, done, s1, c1), (rew2, done2, s12, c2) = chain(T, N, (0, 1))
    worst, pair = [0.0, 0.0], []
    for _ in range(2):
        norm = new(N)
        norm.update(rew, done)
        check(norm, R.moments(s1), R.stat_bars(s1), c1, "N=%d T=%d" % (N, T), worst)
        pair.append(norm.stats())
        norm.close()
    assert all(_bits(u) == _bits(v) for u, v in zip(*pair)), "bits: N=%d T=%d: two fresh objects differ" % (N, T)
    norm = new(N)
    norm.update(rew, done)
    norm.update(rew2, done2)
    check(norm, R.moments(s12), R.stat_bars(s12), c2, "N=%d T=%d+%d" % (N, T, T), worst)
    norm.close()
    return _report("a", "N=%d T=%d" % (N, T), worst)


def case_edges(new, N, steps=EDGE_STEPS, big=False):
    """b. three consecutive updates at every T, checked after each: the carry crosses the calls and K becomes the running mean"""
    worst = [0.0, 0.0]
    for T in steps:
        norm = new(N)
        for k, (rew, done, seen, carry) in enumerate(chain(T, N, (0, 1, 2), R.GAMMA, big)):
            norm.update(rew, done)
            check(norm, R.moments(seen), R.stat_bars(seen), carry, "N=%d T=%d update %d%s" % (N, T, k, " at 1e3" if big else ""), worst)
        norm.close()
    return _report("b", "N=%d%s" % (N, " at 1e3" if big else ""), worst)


def case_gamma_zero(new, N, T):
    """c. gamma = 0: every sample is its reward and the carry the last reward widened (0 where that step was done)"""
    rew, done = R.rollout(T, N)
    samples, carry = R.returns(rew, done, 0.0)
    assert np.array_equal(samples, rew.astype(np.float64)) and np.array_equal(carry, np.where(done[-1] != 0, 0.0, rew[-1].astype(np.float64)))
    norm = new(N, gamma=0.0)
    norm.update(rew, done)
    fr = check(norm, R.moments(samples), R.stat_bars(samples), carry, "gamma=0 N=%d T=%d" % (N, T))
    norm.close()
    return _report("c", "gamma=0 N=%d T=%d" % (N, T), fr)


def case_gamma_one_long(new):
    """c. gamma = 1 over T = 1000 steps without a done: the returns grow to about 1e3, K = reward[0, 0] is about 1"""
    rew, done = long_rewards()
    samples, carry = R.returns(rew, done, 1.0)
    assert 800.0 < samples[-1].min() and samples.max() < 1200.0 and _in_range(rew[0, 0], samples)
    norm = new(rew.shape[1], gamma=1.0)
    norm.update(rew, done)
    fr = check(norm, R.moments(samples), R.stat_bars(samples), carry, "gamma=1 N=%d T=%d" % rew.shape[::-1])
    norm.close()
    return _report("c", "gamma=1 T=1000", fr)


def case_gamma_one_dones(new, N, T=20):
    """c. gamma = 1 with dones at p = 0.1: two updates, the undiscounted carry crossing the call"""
    worst = [0.0, 0.0]
    norm = new(N, gamma=1.0)
    for k, (rew, done, seen, carry) in enumerate(chain(T, N, (0, 1), 1.0)):
        norm.update(rew, done)
        check(norm, R.moments(seen), R.stat_bars(seen), carry, "gamma=1 N=%d T=%d update %d" % (N, T, k), worst)
    norm.close()
    return _report("c", "gamma=1 dones N=%d" % N, worst)


def case_shift_far(new, N, T, figures=None):
    """d.1: fresh statistics beside a loaded carry of 1e5: K = reward[0, 0] = 1e3 lies 1e5 from samples whose spread is about 1e-2.
    Inside stat_bars_shifted; OUTSIDE the plain stat_bars' M2 (the documented limit of the shifted one-pass sum, not an accident)."""
    rew, done, before = steady_window(T, N)
    samples, carry = R.returns(rew, done, R.GAMMA, before)
    ref, K = R.moments(samples), float(rew[0, 0])
    assert not _in_range(K, samples) and np.abs(samples - K).max() > 9e4 and samples.max() - samples.min() < 1.0
    assert all(u >= v for u, v in zip(R.stat_bars_shifted(samples, K), R.stat_bars(samples)))
    norm = new(N)
    norm.load(0.0, 0.0, 0.0, returns=before)
    norm.update(rew, done)
    fr = check(norm, ref, R.stat_bars_shifted(samples, K), carry, "far K N=%d T=%d" % (N, T))
    e2 = abs(norm.stats()[2] - ref[2])
    plain = R.stat_bars(samples)[1]
    print("d.1 N=%d T=%d: relative M2 error %.3g (M2 %.6g), %.3g x the plain bar" % (N, T, e2 / ref[2], ref[2], e2 / plain))
    if figures is not None:
        figures.append((N, T, e2 / ref[2], e2 / plain))
    assert e2 > plain, "plain bar: far K N=%d T=%d: the M2 error %.3g is inside the plain bar %.3g" % (N, T, e2, plain)
    norm.close()
    return _report("d", "far K N=%d T=%d" % (N, T), fr)


def case_shift_empty_state(new, N, T):
    """d.2: a state stored as count 0, mean 7, M2 3, then a window of one value (1.7, and 1e-3), and an ordinary one: neither stored
    number has any effect.  The window of 1.7 alone cannot see a K of 7: 1.7f - 7 has 26 significant bits, its square is exact in fp64
    and q - s^2 / T is 0 either way; 1e-3f - 7 has 36, and shifted by 7 its M2 comes out at 1e-11 instead of 0."""
    done = R.rollout(T, N)[1]
    for value in (1.7, 1e-3):
        rew = np.full((T, N), value, np.float32)
        norm = new(N, gamma=0.0)
        norm.load(0.0, 7.0, 3.0)
        norm.update(rew, done)
        count, mean, m2 = norm.stats()
        assert count == T * N, "count: one value N=%d T=%d: %r" % (N, T, count)
        assert m2 == 0.0 and mean == float(np.float32(value)), "one value: %g N=%d T=%d: mean %r, M2 %r" % (value, N, T, mean, m2)
        assert np.array_equal(_bits(norm.returns()), _bits(R.returns(rew, done, 0.0)[1])), "carry: one value N=%d T=%d" % (N, T)
        norm.table()
        norm.close()
    rew, done = R.rollout(T, N)
    runs = []
    for stored in ((0.0, 7.0, 3.0), None):
        norm = new(N)
        if stored is not None:
            norm.load(*stored)
        norm.update(rew, done)
        runs.append(norm.stats())
        norm.close()
    assert all(_bits(u) == _bits(v) for u, v in zip(*runs)), "stored: N=%d T=%d: %r, a fresh object %r" % ((N, T) + tuple(runs))


def case_shift_outlier(new, N, T):
    """d.3: reward[0, 0] = 1e6 in an otherwise ordinary first update: K is an outlier, but a sample, so the plain bars hold"""
    rew, done = R.rollout(T, N)
    rew = rew.copy()
    rew[0, 0] = 1e6
    samples, carry = R.returns(rew, done, R.GAMMA)
    assert _in_range(rew[0, 0], samples) and samples[0, 0] == 1e6
    norm = new(N)
    norm.update(rew, done)
    fr = check(norm, R.moments(samples), R.stat_bars(samples), carry, "outlier K N=%d T=%d" % (N, T))
    norm.close()
    return _report("d", "outlier K N=%d T=%d" % (N, T), fr)


def case_shift_jump(new, N, T):
    """d.4: the return level jumps from 0 to 1e5 between two updates: the second is summed shifted by K = fp32(the first's mean)"""
    low, done1, high, done2 = jump_windows(T, N)
    s1, c1 = R.returns(low, done1, 0.0)
    s2, c2 = R.returns(high, done2, 0.0, c1)
    norm = new(N, gamma=0.0)
    norm.update(low, done1)
    check(norm, R.moments(s1), R.stat_bars(s1), c1, "jump, before, N=%d T=%d" % (N, T))
    state = norm.stats()
    K = float(np.float32(state[1]))
    assert not _in_range(K, s2) and abs(K) < 0.1
    batch = R.moments(s2)
    norm.update(high, done2)
    fr = check(norm, R.merge(state, batch), P.merge_bars(state, batch, R.stat_bars_shifted(s2, K)), c2, "jump N=%d T=%d" % (N, T))
    norm.close()
    return _report("d", "jump N=%d T=%d" % (N, T), fr)


def case_long_run(new):
    """e. 200 successive updates against ONE two-pass over all 2 096 000 samples"""
    windows, ref, bars, carry = long_run()
    norm = new(LONG_N)
    for rew, done in windows:
        norm.update(rew, done)
    fr = check(norm, ref, bars, carry, "%d updates of T=%d N=%d" % (LONG_UPDATES, LONG_T, LONG_N))
    norm.close()
    return _report("e", "%d updates" % LONG_UPDATES, fr)


PRIORS = {"1e12": dict(load=(1e12, 3.0, 2e12)), "sb3": dict(from_stats=(1.0, 1e-4, 0.0))}


def case_prior(new, name, N=LONG_N, T=LONG_T):
    """e. one window on a state of count 1e12 (mean 3, var 2), and on SB3's RunningMeanStd start (count 1e-4, mean 0, var 1) through
    from_stats: against chan_merge(state, two-pass moments).  K = fp32(the state's mean) lies inside the window's samples."""
    rew, done = R.rollout(T, N)
    samples, carry = R.returns(rew, done, R.GAMMA)
    prior = PRIORS[name]
    if "load" in prior:
        state = prior["load"]
        norm = new(N)
        norm.load(*state)
    else:
        var, count, mean = prior["from_stats"]
        state = (count, mean, var * count)
        norm = new(N, from_stats=prior["from_stats"])
    assert tuple(norm.stats()) == state and _in_range(np.float32(state[1]), samples)
    batch = R.moments(samples)
    norm.update(rew, done)
    fr = check(norm, R.merge(state, batch), P.merge_bars(state, batch, R.stat_bars(samples)), carry, "prior %s N=%d T=%d" % (name, N, T))
    norm.close()
    return _report("e", "prior %s" % name, fr)
