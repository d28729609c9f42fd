"""Reference arithmetic of the return normaliser (include/gaq.h gaq_ret_norm) in numpy fp64: the per-env recurrence exactly as the header
states it, the list of samples it produces, their statistics through tests/obs_norm_ref.py (moments / chan_merge / table, one column;
the table's mean column is not used), the element expression, the error bars of the device's statistics (stat_bars for a shift K among
the samples, stat_bars_shifted for any K), and the synthetic rollouts the GPU tests share."""
import numpy as np

from tests import obs_norm_ref as O

U64 = 2.0 ** -52
GAMMA, EPS, CLIP = 0.99, 1e-8, 10.0          # RetNorm's defaults (SB3's)


def returns(rew, done, gamma, carry=None):
    """(samples [T, N] float64, carry [N] float64): R = gamma R + r with the product and the sum rounded separately (numpy evaluates the
    two in turn), gamma the fp32 value widened; R is a sample, then R = 0 where done is set"""
    rew, done = np.asarray(rew, np.float32), np.asarray(done)
    g = np.float64(np.float32(gamma))
    R = np.zeros(rew.shape[1], np.float64) if carry is None else np.array(carry, np.float64)
    samples = np.empty(rew.shape, np.float64)
    for t in range(rew.shape[0]):
        R = g * R
        R = R + rew[t].astype(np.float64)
        samples[t] = R
        R = np.where(done[t] != 0, 0.0, R)
    return samples, R


def moments(samples):
    """two-pass (count, mean, M2) of every sample as floats"""
    n, mean, m2 = O.moments(np.asarray(samples, np.float64).reshape(-1, 1))
    return n, float(mean[0]), float(m2[0])


def merge(a, b):
    n, mean, m2 = O.chan_merge((a[0], np.float64(a[1]), np.float64(a[2])), (b[0], np.float64(b[1]), np.float64(b[2])))
    return n, float(mean), float(m2)


def inv_std(count, m2, eps):
    """the published fp32 inv_std of fp64 statistics: fp32(1 / sqrt(M2 / count + eps)), the variance 1 before any update"""
    return O.table(count, np.zeros(1), np.array([m2], np.float64), eps)[1][0]


def normalize(r, inv32, clip):
    """min(max(r * inv_std, -clip), clip) in fp32: the device's expression rounding for rounding"""
    c = np.float32(clip)
    return np.minimum(np.maximum(np.asarray(r, np.float32) * np.float32(inv32), -c), c)


def stat_bars(samples):
    """(bar of the mean, bar of M2) against the two-pass fp64 values: tests/test_gpu_obs_norm._stat_bars for one column of n = T N
    samples.  The device adds n shifted terms in fp64 and merges partials; a sum of n terms carries at most (n - 1) u of relative error
    on the sum of magnitudes (u = 2^-52), the merges, the K + s / n and numpy's own sums add a few roundings: 8 n u is taken.  mean:
    magnitudes <= max|R|.  M2: n terms d^2 <= range^2.  Samples of one value (range 0) must give exactly 0."""
    s = np.asarray(samples, np.float64).reshape(-1)
    n = s.size
    return 8 * n * U64 * np.abs(s).max(), 8 * n * U64 * n * (s.max() - s.min()) ** 2


def stat_bars_shifted(samples, K):
    """(bar of the mean, bar of M2) for samples summed SHIFTED by a K that may lie far from them: stat_bars' derivation with the terms
    the device really adds.  It adds n terms d = R - K and n terms d^2, 8 u per term as in stat_bars: the d are at most
    max(max|R|, |K|) in magnitude on the way back to the mean (K + s / n rounds at that magnitude), the d^2 at most max|R - K|^2, and
    q - s^2 / n cancels sums of that size, so M2 is accurate relative to n max|R - K|^2, not to n range^2 -- the one-pass shifted
    algorithm's limit, about u (Delta / sigma)^2 relative for a K at Delta from samples of spread sigma.  For min R <= K <= max R,
    |R - K| <= range and |K| <= max|R|: the bars ARE stat_bars' (never smaller for any K), which tests/test_ret_norm_plan_cpu.py
    asserts.  K is far from the samples after a carry loaded next to fresh statistics, or a jump of the return level between two
    updates (K = fp32 of the OLD mean); an outlier at reward[0] is a K inside the range."""
    s = np.asarray(samples, np.float64).reshape(-1)
    n, K = s.size, float(K)
    reach = max(s.max() - s.min(), np.abs(s - K).max())
    return 8 * n * U64 * max(np.abs(s).max(), abs(K)), 8 * n * U64 * n * reach ** 2


def rollout(T, N, seed=0):
    """a synthetic rollout (rew [T, N] float32, done [T, N] uint8): rewards 1e3 + 1e-2 randn in the first half of the envs (a large mean
    with a small spread) and unit normals in the other; dones at p = 0.1 and, where T allows, row 1 all done and row 3 all clear"""
    rng = np.random.RandomState(100003 * T + N + seed)
    rew = rng.randn(T, N)
    rew[:, :N // 2] = 1e3 + 1e-2 * rew[:, :N // 2]
    done = (rng.rand(T, N) < 0.1).astype(np.uint8)
    if T > 3:
        done[1], done[3] = 1, 0
    rew = rew.astype(np.float32)
    rew.setflags(write=False); done.setflags(write=False)
    return rew, done
