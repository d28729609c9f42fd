"""Reference arithmetic of the observation normaliser (include/gaq.h gaq_obs_norm) in numpy, and the case table its GPU tests share:
Chan's parallel merge of (count, mean, M2), the published table, the element expression in a chosen precision, per-width statistics
with a different mean and scale in every column, and stand-in observations that reach +clip, -clip and the interior."""
import numpy as np

CLIP = 5.0
EPS = 1e-5
# every observation width the env layouts of tests/test_gpu_policy_shapes.py produce (the GPU tests check this list against the envs)
WIDTHS = [13, 14, 18, 19, 20, 22, 25, 24, 36, 60, 108]


def moments(x):
    """direct two-pass (count, mean [D], M2 [D]) of rows x [rows, D] in float64"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=0)
    return float(x.shape[0]), mean, ((x - mean) ** 2).sum(axis=0)


def chan_merge(a, b):
    """Chan, Golub & LeVeque: the moments of the union of two samples a = (n, mean, M2), b likewise"""
    (na, ma, sa), (nb, mb, sb) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    delta = np.asarray(mb, np.float64) - np.asarray(ma, np.float64)
    return n, ma + delta * (nb / n), sa + sb + delta * delta * (na * nb / n)


def table(count, mean, m2, eps):
    """the published fp32 table of fp64 statistics: (fp32(mean), fp32(1 / sqrt(var + eps))), var = M2 / count (1 before any update)"""
    mean, m2 = np.asarray(mean, np.float64), np.asarray(m2, np.float64)
    var = m2 / count if count > 0 else np.ones_like(mean)
    return mean.astype(np.float32), (1.0 / np.sqrt(var + np.float64(np.float32(eps)))).astype(np.float32)


def normalize(x, mean32, inv32, clip, dtype=np.float32):
    """min(max((x - mean[k]) * inv_std[k], -clip), clip) in `dtype`: float32 is the device's expression rounding for rounding (two
    roundings, then the clamp), float64 the reference the actors are compared with"""
    x, m, s = (np.asarray(a).astype(dtype) for a in (x, mean32, inv32))
    c = dtype(clip)
    return np.minimum(np.maximum((x - m) * s, -c), c)


def case_stats(D):
    """(mean [D], var [D]) of the case table: every column its own mean and scale (a wrong column index cannot survive), scales from
    0.05 to 0.35 so that unit-sized inputs land on both clamps and between them"""
    k = np.arange(D)
    mean = 0.25 * ((k % 5) - 2) + 0.01 * k
    std = 0.05 * (1 + (k % 7)) + 0.001 * k
    return mean.astype(np.float64), (std * std).astype(np.float64)


def stand_in_obs(rows, D, seed=0):
    """unit-normal stand-in observations [rows, D] float32"""
    return np.random.RandomState(1000 * D + seed).randn(rows, D).astype(np.float32)


def clip_census(z, clip=CLIP):
    """(elements at +clip, at -clip, strictly inside)"""
    z = np.asarray(z)
    return int((z == clip).sum()), int((z == -clip).sum()), int((np.abs(z) < clip).sum())
