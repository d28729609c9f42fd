"""Return normalisation without a GPU: the new entry points are exported, bound and refuse null arguments; the reference's one-pass
moments (tests/ret_norm_ref.py) against an independent SB3-style loop; the teeth of the GPU tests' error bars; RetNorm's signatures."""
import ctypes as C
import inspect
import os

import numpy as np

from tests import ret_norm_ref as R

NAMES = ("create", "update_dev", "apply_dev", "reset_returns_dev", "get_stats", "set_stats", "get_returns", "set_returns", "destroy")


def test_symbols_are_exported_and_bound():
    from gym_art_amd import _lib
    lib = _lib.load()
    bound = {s[0] for s in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    for n in NAMES:
        assert "gaq_ret_norm_" + n in bound, n
        assert hasattr(lib, "gaq_ret_norm_" + n), n
        assert "gaq_ret_norm_" + n + "(" in header, n
    assert lib.gaq_abi_version() == 5


def test_entry_points_refuse_null_arguments():
    from gym_art_amd import _lib
    lib = _lib.load()
    h, d = C.c_void_p(), C.c_double()
    calls = [lambda: lib.gaq_ret_norm_create(None, 0.99, 1e-8, 10.0, C.byref(h)),
             lambda: lib.gaq_ret_norm_update_dev(None, 4, None, None, None),
             lambda: lib.gaq_ret_norm_apply_dev(None, 4, None, None, None),
             lambda: lib.gaq_ret_norm_reset_returns_dev(None, None, None),
             lambda: lib.gaq_ret_norm_get_stats(None, C.byref(d), C.byref(d), C.byref(d)),
             lambda: lib.gaq_ret_norm_set_stats(None, 1.0, 0.0, 1.0),
             lambda: lib.gaq_ret_norm_get_returns(None, None),
             lambda: lib.gaq_ret_norm_set_returns(None, None)]
    for call in calls:
        assert call() == -1 and b"null" in lib.gaq_last_error()
    assert not h.value
    assert lib.gaq_ret_norm_destroy(None) == 0


class _RunningMeanStd:
    """SB3's RunningMeanStd.update / update_from_moments for scalars, started at count 0 instead of SB3's pseudo-count of 1e-4 (so the
    count is the number of samples)"""

    def __init__(self):
        self.mean, self.var, self.count = 0.0, 1.0, 0.0

    def update(self, x):
        batch_mean, batch_var, batch_count = float(np.mean(x)), float(np.var(x)), x.shape[0]
        delta = batch_mean - self.mean
        tot = self.count + batch_count
        m2 = self.var * self.count + batch_var * batch_count + delta * delta * self.count * batch_count / tot
        self.mean, self.var, self.count = self.mean + delta * batch_count / tot, m2 / tot, tot


def _vec_normalize_loop(rew, done, gamma):
    """VecNormalize.step_wait's reward half, one RunningMeanStd.update per step"""
    rms, ret = _RunningMeanStd(), np.zeros(rew.shape[1])
    for t in range(rew.shape[0]):
        ret = ret * np.float64(np.float32(gamma)) + rew[t]
        rms.update(ret)
        ret[done[t] != 0] = 0.0
    return rms, ret


def test_one_pass_moments_equal_the_per_step_loop():
    rng = np.random.RandomState(5)
    T, N = 50, 37
    rew = rng.randn(T, N).astype(np.float32)
    done = (rng.rand(T, N) < 0.1).astype(np.uint8)
    assert 0 < done.sum() < T * N
    samples, carry = R.returns(rew, done, R.GAMMA)
    n, mean, m2 = R.moments(samples)
    rms, ret = _vec_normalize_loop(rew, done, R.GAMMA)
    bar_mean, bar_m2 = R.stat_bars(samples)
    assert rms.count == n == T * N
    assert np.array_equal(ret.view(np.uint64), carry.view(np.uint64))
    assert abs(rms.mean - mean) <= bar_mean and abs(rms.var - m2 / n) <= bar_m2 / n
    # and split in two with the carry handed over, merged with Chan's formula
    a, mid = R.returns(rew[:17], done[:17], R.GAMMA)
    b, end = R.returns(rew[17:], done[17:], R.GAMMA, mid)
    assert np.array_equal(np.concatenate([a, b]), samples) and np.array_equal(end, carry)
    n2, mean2, m22 = R.merge(R.moments(a), R.moments(b))
    assert n2 == n and abs(mean2 - mean) <= bar_mean and abs(m22 - m2) <= bar_m2


def test_recurrence_order_and_rounding():
    """a done clears the carry AFTER its sample; gamma is the fp32 value; product and sum are rounded separately"""
    samples, carry = R.returns(np.array([[1.0], [2.0], [4.0]], np.float32), np.array([[0], [1], [0]], np.uint8), 0.5)
    assert samples[:, 0].tolist() == [1.0, 2.5, 4.0] and carry.tolist() == [4.0]
    g = np.float64(np.float32(0.99))
    assert g != 0.99
    s, _ = R.returns(np.array([[0.1], [0.3]], np.float32), np.zeros((2, 1), np.uint8), 0.99)
    assert s[1, 0] == g * np.float64(np.float32(0.1)) + np.float64(np.float32(0.3))


def test_bars_reject_fp32_arithmetic():
    """rewards of mean 1e3 and spread 1e-2: an fp32 recurrence with fp32 sums misses both bars by more than 100x"""
    rng = np.random.RandomState(6)
    T, N = 50, 37
    rew = (1e3 + 1e-2 * rng.randn(T, N)).astype(np.float32)
    done = (rng.rand(T, N) < 0.1).astype(np.uint8)
    samples, _ = R.returns(rew, done, R.GAMMA)
    n, mean, m2 = R.moments(samples)
    bar_mean, bar_m2 = R.stat_bars(samples)
    g32, ret = np.float32(R.GAMMA), np.zeros(N, np.float32)
    s32, q32 = np.float32(0.0), np.float32(0.0)
    for t in range(T):
        ret = (ret * g32 + rew[t]).astype(np.float32)
        for v in ret:
            s32 = np.float32(s32 + v)
            q32 = np.float32(q32 + v * v)
        ret[done[t] != 0] = 0.0
    mean32 = np.float32(s32 / np.float32(n))
    m2_32 = np.float32(q32 - np.float32(n) * mean32 * mean32)
    print("fp32 arithmetic / bar: mean %.3g, M2 %.3g" % (abs(mean32 - mean) / bar_mean, abs(m2_32 - m2) / bar_m2))
    assert abs(mean32 - mean) > 100 * bar_mean and abs(m2_32 - m2) > 100 * bar_m2


def test_element_expression_and_table():
    x = np.array([0.0, -0.0, 1.0, -1.5, 3.4e38, -3.4e38, 1e-45, -1e-45, np.inf, -np.inf], np.float32)
    fresh = R.inv_std(0.0, 0.0, R.EPS)
    assert fresh == np.float32(1.0)                                # 1 / sqrt(1 + 1e-8) rounds to 1: fresh statistics are the identity
    z = R.normalize(x, fresh, np.inf)
    assert z.dtype == np.float32 and np.array_equal(z.view(np.uint32), x.view(np.uint32))
    assert R.inv_std(4.0, 1.0, 0.0) == np.float32(2.0)
    assert list(R.normalize([30.0, -30.0, 0.5], np.float32(0.5), 10.0)) == [10.0, -10.0, 0.25]


def test_public_signatures():
    from gym_art_amd import policy as P
    sig = lambda f: str(inspect.signature(f))
    assert sig(P.RetNorm.__init__) == "(self, env, gamma=0.99, eps=1e-08, clip=10.0)"
    assert sig(P.RetNorm.update_dev) == "(self, rew, done, stream=None)"
    assert sig(P.RetNorm.normalize_dev) == "(self, rew, out=None, stream=None)"
    assert sig(P.RetNorm.reset_returns) == "(self, mask=None)"
    assert sig(P.RetNorm.from_stats.__func__) == "(cls, env, var, count=1.0, mean=0.0, gamma=0.99, eps=1e-08, clip=10.0)"
    for name in ("count", "mean", "var", "returns"):
        assert isinstance(getattr(P.RetNorm, name), property)
    for name in ("state_dict", "load_state_dict", "close"):
        assert callable(getattr(P.RetNorm, name))


def test_policy_reexports_the_classes_of_norm():
    """gym_art_amd.norm is the home of both normalisers; gym_art_amd.policy hands out the same classes"""
    from gym_art_amd import norm, policy
    assert policy.ObsNorm is norm.ObsNorm and policy.RetNorm is norm.RetNorm
    assert issubclass(norm.ObsNorm, norm._RunningNorm) and issubclass(norm.RetNorm, norm._RunningNorm)
