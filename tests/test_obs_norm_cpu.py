"""Observation normalisation without a GPU: the numpy restatement of Chan's merge and of the element expression (tests/obs_norm_ref.py)
against a direct two-pass fp64 mean / variance, the teeth of the GPU tests' case table in every observation width, and the public
signatures of ObsNorm and set_obs_norm."""
import inspect

import numpy as np
import pytest

from tests import obs_norm_ref as R


@pytest.mark.parametrize("sizes", [(1,), (1, 1), (65, 4097), (7, 1, 300, 2), (4097, 65, 64)])
def test_chan_merge_equals_two_pass(sizes):
    """batches merged one after the other (and as a tree) against the two-pass moments of their concatenation; a column of mean 1e3 and
    spread 1e-2 and a constant column included.  Bar: a few fp64 roundings per merge, relative to the size of the quantity"""
    rng = np.random.RandomState(len(sizes))
    D = 5
    batches = []
    for n in sizes:
        x = rng.randn(n, D)
        x[:, 1] = 1e3 + 1e-2 * rng.randn(n)
        x[:, 2] = 1.5
        batches.append(x.astype(np.float32).astype(np.float64))
    n_ref, mean_ref, m2_ref = R.moments(np.concatenate(batches))
    run = (0.0, np.zeros(D), np.zeros(D))
    for x in batches:
        run = R.chan_merge(run, R.moments(x))
    parts = [R.moments(x) for x in batches]
    while len(parts) > 1:
        parts = [R.chan_merge(parts[k], parts[k + 1]) if k + 1 < len(parts) else parts[k] for k in range(0, len(parts), 2)]
    u = 2.0 ** -52
    for n, mean, m2 in (run, parts[0]):
        assert n == n_ref
        assert np.all(np.abs(mean - mean_ref) <= 16 * len(sizes) * u * np.maximum(np.abs(mean_ref), 1.0))
        assert np.all(np.abs(m2 - m2_ref) <= 1e-9 * np.maximum(m2_ref, 1e-12) + 64 * u * n_ref * 1e-4)
        assert m2[2] == 0.0 and mean[2] == 1.5


def test_element_expression():
    """identity at mean 0, inv_std 1, clip inf on every kind of fp32 value, -0 included; two roundings, not an fma; the clamp"""
    x = np.array([0.0, -0.0, 1.0, -1.5, 3.4e38, -3.4e38, 1e-45, -1e-45, np.inf, -np.inf], np.float32)
    z = R.normalize(x, np.zeros(x.size, np.float32), np.ones(x.size, np.float32), np.inf)
    assert z.dtype == np.float32 and np.array_equal(z.view(np.uint32), x.view(np.uint32))
    a, m, s = np.float32(1.0000001), np.float32(0.33333334), np.float32(3.0000002)
    two = np.float32(np.float32(a - m) * s)
    assert R.normalize([a], [m], [s], 100.0)[0] == two
    assert list(R.normalize([10.0, -10.0, 0.5], [0.0] * 3, [1.0] * 3, 5.0)) == [5.0, -5.0, 0.5]
    mean32, inv32 = R.table(0.0, np.zeros(3), np.zeros(3), R.EPS)
    assert np.all(mean32 == 0) and np.all(inv32 == np.float32(1.0 / np.sqrt(1.0 + np.float64(np.float32(R.EPS)))))


@pytest.mark.parametrize("D", R.WIDTHS)
def test_case_table_has_teeth(D):
    """the GPU tests' statistics and stand-in observations: in every width some elements clip at +clip, some at -clip, some not at
    all; every column has its own (mean, inv_std) pair, and shifting the table by one column changes the result"""
    mean, var = R.case_stats(D)
    mean32, inv32 = R.table(1.0, mean, var, R.EPS)
    assert len({(float(a), float(b)) for a, b in zip(mean32, inv32)}) == D
    for rows in (1, 63, 64, 65, 130):
        z = R.normalize(R.stand_in_obs(rows, D), mean32, inv32, R.CLIP)
        hi, lo, inside = R.clip_census(z)
        if rows >= 63:
            assert hi > 0 and lo > 0 and inside > 0, (D, rows, hi, lo, inside)
        assert not np.array_equal(z, R.normalize(R.stand_in_obs(rows, D), mean32, np.roll(inv32, -1), R.CLIP))
    z1 = R.normalize(R.stand_in_obs(1, D), mean32, inv32, R.CLIP)
    assert np.abs(z1).max() == R.CLIP and np.abs(z1).min() < R.CLIP


def test_public_signatures():
    from gym_art_amd import policy as P
    sig = lambda f: str(inspect.signature(f))
    assert sig(P.ObsNorm.__init__) == "(self, env, eps=1e-05, clip=5.0)"
    assert sig(P.ObsNorm.update_dev) == "(self, obs, stream=None)"
    assert sig(P.ObsNorm.normalize_dev) == "(self, obs, out=None, stream=None)"
    assert sig(P.ObsNorm.from_stats.__func__) == "(cls, env, mean, var, count=1.0, eps=1e-05, clip=5.0)"
    for name in ("count", "mean", "var"):
        assert isinstance(getattr(P.ObsNorm, name), property)
    for name in ("state_dict", "load_state_dict", "close"):
        assert callable(getattr(P.ObsNorm, name))
    for cls in (P.MLPPolicy, P.GRUPolicy, P.LSTMPolicy, P.MLPCritic):
        assert sig(cls.set_obs_norm) == "(self, norm)", cls
    assert P.MLPPolicy.set_obs_norm is P._DevicePolicy.set_obs_norm
    assert "obs_norm=None" in sig(P.MLPPolicy.__init__)


def test_symbols_are_bound():
    from gym_art_amd import _lib
    names = {s[0] for s in _lib.SYMBOLS}
    for n in ("create", "update_dev", "apply_dev", "get_stats", "set_stats", "destroy"):
        assert "gaq_obs_norm_" + n in names
    assert {"gaq_policy_set_obs_norm", "gaq_critic_set_obs_norm"} <= names
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib._HERE), "include", "gaq.h")).read()
    for n in names:
        if "obs_norm" in n:
            assert n + "(" in header, n
