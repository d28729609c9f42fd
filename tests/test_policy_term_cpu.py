"""Host side of time-limit bootstrapping (gaq.h gaq_step_policy_ac_term_many_dev, gaq_gae_term_dev): the entry points and the Python
arguments exist, and the fp64 reference the GPU tests use is the plain one without terminal values and the closed form with them."""
import ctypes as C
import inspect

import numpy as np
import pytest

from gym_art_amd import _lib
from tests import ac_ref, term_ref


def _rollout(T, N, seed, p_done):
    rng = np.random.RandomState(seed)
    return rng.randn(T, N), (rng.rand(T, N) < p_done).astype(np.uint8), rng.randn(T + 1, N), rng.randn(T, N)


def test_library_exports_the_entry_points_with_the_documented_argument_counts():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    assert len(sig["gaq_step_policy_ac_term_many_dev"]) == 11       # gaq_step_policy_ac_many_dev's 10 + term_value_out before the stream
    assert len(sig["gaq_gae_term_dev"]) == 11                       # gaq_gae_dev's 10 + term_value after value
    assert sig["gaq_gae_term_dev"][6:8] == [C.c_float, C.c_float]
    assert lib.gaq_step_policy_ac_term_many_dev(None, None, 4, None, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.gaq_last_error()
    assert lib.gaq_gae_term_dev(None, 4, None, None, None, None, 0.99, 0.95, None, None, None) == -1
    assert b"null" in lib.gaq_last_error()


def test_python_methods_accept_term_values():
    from gym_art_amd import QuadrotorEnv
    for name in ("rollout_policy_dev", "gae_dev"):
        par = inspect.signature(getattr(QuadrotorEnv, name)).parameters
        assert "term_values" in par and par["term_values"].default is None, name
        assert par["term_values"].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert "absorbing" in QuadrotorEnv.gae_dev.__doc__             # what happens without term_values is said


def test_multi_device_env_refuses_term_values():
    from gym_art_amd.multi_device import _MultiDeviceMixin as M
    for name in ("rollout_policy_dev", "gae_dev"):
        with pytest.raises(NotImplementedError, match="term_values"):
            getattr(M, name)(M.__new__(M), term_values=object())


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.99, 0.0), (0.9, 1.0), (1.0, 1.0)])
def test_gae_term64_with_zero_terminal_values_is_gae64(gamma, lam):
    rew, done, val, _ = _rollout(17, 23, 0, 0.2)
    assert done.sum() > 0
    adv, ret = term_ref.gae_term64(rew, done, val, np.zeros_like(rew), gamma, lam)
    adv0, ret0 = ac_ref.gae64(rew, done, val, gamma, lam)
    assert np.array_equal(adv, adv0) and np.array_equal(ret, ret0)
    # ... and what the entries of envs that did not finish hold is never used
    junk = np.where(done != 0, 0.0, np.nan)
    adv1, _ = term_ref.gae_term64(rew, done, val, junk, gamma, lam)
    assert np.array_equal(adv1, adv0)


def test_gae_term64_on_a_hand_built_three_step_case():
    """env 0 finishes in step 1, env 1 never: closed-form truncation-bootstrapped advantages"""
    g, l = 0.9, 0.8
    r = np.array([[1.0, 0.5], [2.0, -1.0], [3.0, 0.25]])
    V = np.array([[0.5, 1.0], [1.5, -2.0], [-1.0, 3.0], [2.0, 0.75]])
    d = np.array([[0, 0], [1, 0], [0, 0]], np.uint8)
    tv = np.array([[np.nan, np.nan], [4.0, np.nan], [np.nan, np.nan]])
    adv, ret = term_ref.gae_term64(r, d, V, tv, g, l)
    # env 0: the step-1 target looks at V(terminal observation) = 4, the chain is cut between steps 1 and 2
    a2 = 3.0 + g * 2.0 - (-1.0)
    a1 = 2.0 + g * 4.0 - 1.5
    a0 = 1.0 + g * 1.5 - 0.5 + g * l * a1
    assert np.allclose(adv[:, 0], [a0, a1, a2], rtol=0, atol=1e-14)
    # env 1: no done, plain GAE
    b2 = 0.25 + g * 0.75 - 3.0
    b1 = -1.0 + g * 3.0 - (-2.0) + g * l * b2
    b0 = 0.5 + g * (-2.0) - 1.0 + g * l * b1
    assert np.allclose(adv[:, 1], [b0, b1, b2], rtol=0, atol=1e-14)
    assert np.allclose(ret, adv + V[:3], rtol=0, atol=1e-14)
    # against today's cut: the advantage at the done step grows by gamma * term_value, the one before by gamma lam times that
    adv0, _ = ac_ref.gae64(r, d, V, g, l)
    assert np.allclose(adv[:, 0] - adv0[:, 0], [g * l * g * 4.0, g * 4.0, 0.0], rtol=0, atol=1e-14)
    assert np.array_equal(adv[:, 1], adv0[:, 1])


def test_gae_term_bar_is_gae_bar_with_the_terminal_values_in_M():
    T = 8
    rew, done, val, tv = _rollout(T, 5, 2, 0.3)
    assert done.sum() > 0
    tv = 10.0 * tv                                                  # large enough to matter
    adv, _ = term_ref.gae_term64(rew, done, val, tv, 0.99, 0.95)
    M = (np.abs(rew) + np.abs(val[:T]) + np.abs(val[1:]) + np.abs(adv) + np.where(done != 0, np.abs(tv), 0.0)).max(axis=0)
    assert np.allclose(term_ref.gae_term_bar(rew, done, val, tv, adv, 0.99, 0.95), 4 * 2.0 ** -24 * M / (1 - 0.99 * 0.95))
    assert np.allclose(term_ref.gae_term_bar(rew, done, val, tv, adv, 1.0, 1.0), 4 * 2.0 ** -24 * M * T)
    assert (term_ref.gae_term_bar(rew, done, val, tv, adv, 0.99, 0.95) >= ac_ref.gae_bar(rew, val, adv, 0.99, 0.95)).all()
    # entries of envs that did not finish do not enter (they may be NaN)
    junk = np.where(done != 0, tv, np.nan)
    assert np.array_equal(term_ref.gae_term_bar(rew, done, val, junk, adv, 0.99, 0.95), term_ref.gae_term_bar(rew, done, val, tv, adv, 0.99, 0.95))


def test_fp32_recursion_stays_inside_the_derived_bar():
    """the device's formula emulated in fp32 (each fma as the fp32 rounding of the fp64 result) on 4000 envs: every element inside the bar"""
    T, N, gamma, lam = 64, 4000, 0.99, 0.95
    rew, done, val, tv = _rollout(T, N, 4, 0.05)
    rew, val, tv = (x.astype(np.float32) for x in (rew, val, 3.0 * tv))
    d = done != 0
    g32 = np.float32(gamma)
    gl = np.float32(g32 * np.float32(lam))
    a = np.zeros(N, np.float32)
    out = np.zeros((T, N), np.float32)
    for t in range(T - 1, -1, -1):
        vnext = np.where(d[t], tv[t], val[t + 1]).astype(np.float64)
        delta = ((np.float64(g32) * vnext + rew[t].astype(np.float64)).astype(np.float32) - val[t]).astype(np.float32)
        a = (np.where(d[t], 0.0, np.float64(gl)) * a.astype(np.float64) + delta.astype(np.float64)).astype(np.float32)
        out[t] = a
    ref, _ = term_ref.gae_term64(rew, done, val, tv, gamma, lam)
    bar = term_ref.gae_term_bar(rew, done, val, tv, ref, gamma, lam)
    err = np.abs(out.astype(np.float64) - ref)
    assert (err <= bar[None]).all(), float((err / bar[None]).max())
    assert float((err / bar[None]).max()) > 1e-3                    # the bar is not vacuous


def test_gru_term_reference_is_the_next_value_of_an_uncut_episode():
    """with the terminal row equal to the observation the rollout went on with and the done flag cleared, the terminal value IS
    gru_means_values64's next value: the reference steps h as that function does"""
    from tests.gru_util import _gru, _head

    class Net:
        pass
    H, N, T = 32, 6, 5
    net = Net()
    net.gru, net.layers, net.act, net.out_tanh, net.H = _gru(H), _head(H, (16,)), "relu", True, H
    net.value = ac_ref.value_head(16, 9)
    rng = np.random.RandomState(2)
    obs0, obs = rng.randn(N, 18), rng.randn(T, N, 18)
    none = np.zeros((T, N), np.uint8)
    _, values, _ = ac_ref.gru_means_values64(net.gru, net.layers, net.act, net.out_tanh, net.value, obs0, obs, none, np.zeros((N, H)))
    at = np.array([0, 1, 2, 3, 4, 2])
    rows = obs[at, np.arange(N)]
    tv = term_ref.gru_term_values64(net, obs0, obs, none, np.zeros((N, H)), at, rows)
    assert np.allclose(tv, values[at + 1, np.arange(N)], rtol=0, atol=1e-13)
