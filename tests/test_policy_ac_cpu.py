"""Host side of the actor-critic rollouts (gaq.h gaq_policy_set_value_head, gaq_step_policy_ac_many_dev, gaq_gae_dev): the fp64 references
the GPU tests use, the value-head checks of the Python side, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd.policy import check_value_head, torch_value
from tests import ac_ref


def _rollout(T, N, seed, p_done):
    rng = np.random.RandomState(seed)
    return rng.randn(T, N), (rng.rand(T, N) < p_done).astype(np.uint8), rng.randn(T + 1, N)


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.99, 0.0), (0.9, 1.0), (1.0, 1.0)])
def test_gae64_equals_the_plain_double_loop(gamma, lam):
    T, N = 17, 23
    rew, done, val = _rollout(T, N, 0, 0.2)
    assert done.sum() > 0
    adv, ret = ac_ref.gae64(rew, done, val, gamma, lam)
    for i in range(N):
        a = 0.0
        for t in range(T - 1, -1, -1):
            nd = 0.0 if done[t, i] else 1.0
            a = rew[t, i] + gamma * nd * val[t + 1, i] - val[t, i] + gamma * lam * nd * a
            assert abs(adv[t, i] - a) <= 1e-12 * max(1.0, abs(a))
            assert abs(ret[t, i] - (a + val[t, i])) <= 1e-12 * max(1.0, abs(a))


def test_gae64_at_lambda_one_without_dones_is_reward_to_go_minus_value():
    T, N, gamma = 12, 9, 0.97
    rew, done, val = _rollout(T, N, 1, 0.0)
    assert done.sum() == 0
    adv, ret = ac_ref.gae64(rew, done, val, gamma, 1.0)
    for t in range(T):
        togo = sum(gamma ** (k - t) * rew[k] for k in range(t, T)) + gamma ** (T - t) * val[T]
        assert np.allclose(adv[t], togo - val[t], rtol=0, atol=1e-12)
        assert np.allclose(ret[t], togo, rtol=0, atol=1e-12)


def test_gae_bar_is_the_derived_formula():
    rew, done, val = _rollout(8, 5, 2, 0.1)
    adv, _ = ac_ref.gae64(rew, done, val, 0.99, 0.95)
    M = (np.abs(rew) + np.abs(val[:8]) + np.abs(val[1:]) + np.abs(adv)).max(axis=0)
    assert np.allclose(ac_ref.gae_bar(rew, val, adv, 0.99, 0.95), 4 * 2.0 ** -24 * M / (1 - 0.99 * 0.95))
    adv1, _ = ac_ref.gae64(rew, done, val, 1.0, 1.0)
    M1 = (np.abs(rew) + np.abs(val[:8]) + np.abs(val[1:]) + np.abs(adv1)).max(axis=0)
    assert np.allclose(ac_ref.gae_bar(rew, val, adv1, 1.0, 1.0), 4 * 2.0 ** -24 * M1 * 8)


@pytest.mark.parametrize("log_std", [(-2, -2, -2, -2), (-1, -1, -1, -1), (0, 0, 0, 0), (-2, 0, -1, -0.5)])
def test_fp32_log_prob_formula_stays_inside_the_derived_bar(log_std):
    """the device's formula emulated in fp32 on 2 10^5 draws, against logp64 on a = fl32(m + std z): every element inside the bar"""
    rng = np.random.RandomState(3)
    n = 200000
    z = rng.randn(n, 4).astype(np.float32)
    m = np.tanh(rng.randn(n, 4)).astype(np.float32)
    std = ac_ref.std_of(log_std)
    a = (std * z.astype(np.float64) + m.astype(np.float64)).astype(np.float32)      # one fma
    ref, bar = ac_ref.logp64(a, m, log_std)
    err = np.abs(ac_ref.logp32(z, log_std).astype(np.float64) - ref)
    assert (err <= bar).all(), float((err / bar).max())
    assert float((err / bar).max()) > 1e-3                  # the bar is not vacuous: the rounding it allows for is there


def test_with_value_is_a_fifth_output_unit():
    from tests.mlp_ref import _scaled_layers, forward64
    layers = _scaled_layers([48, 32], 18, 0)
    v = ac_ref.value_head(32, 5)
    x = np.random.RandomState(1).randn(7, 18)
    means, V, z = ac_ref.mlp_means_values64(layers, "tanh", True, v, x)
    a, z0 = forward64(layers, "tanh", True, x)
    assert np.array_equal(means, a) and np.array_equal(z, z0)
    hidden = []
    forward64(layers, "tanh", True, x, hidden)
    assert np.allclose(V, np.tanh(hidden[-1]) @ v[0].astype(np.float64) + np.float64(v[1]), rtol=0, atol=1e-14)


def test_gru_reference_with_value_agrees_with_reference_rollout():
    from tests.gru_util import _gru, _head, reference_rollout
    H, N, T = 32, 6, 5
    gru, layers = _gru(H), _head(H, (16,))
    rng = np.random.RandomState(2)
    obs0, obs, done = rng.randn(N, 18), rng.randn(T, N, 18), (rng.rand(T, N) < 0.3).astype(np.uint8)
    v = ac_ref.value_head(16, 9)
    means, values, _ = ac_ref.gru_means_values64(gru, layers, "relu", True, v, obs0, obs, done, np.zeros((N, H)))
    acts, _ = reference_rollout(gru, layers, "relu", True, obs0, obs, done, np.zeros((N, H)))
    assert np.allclose(means, acts, rtol=0, atol=1e-14) and values.shape == (T + 1, N)


def test_check_value_head():
    w = np.arange(48, dtype=np.float32)
    for ww, bb in ((w, 0.5), (w.reshape(1, 48), np.float32(0.5)), (w.astype(np.float64), np.array([0.5]))):
        packed = check_value_head(48, "mfma", ww, bb)
        assert packed.dtype == np.float32 and packed.shape == (49,) and packed.flags["C_CONTIGUOUS"]
        assert np.array_equal(packed[:48], w) and packed[48] == np.float32(0.5)
    for bad in (w[:47], w.reshape(48, 1), w.reshape(2, 24), np.zeros(64, np.float32)):
        with pytest.raises(ValueError, match="weights"):
            check_value_head(48, "mfma", bad, 0.0)
    with pytest.raises(ValueError, match="bias"):
        check_value_head(48, "mfma", w, np.zeros(2))
    with pytest.raises(ValueError, match="valu"):
        check_value_head(48, "valu", w, 0.0)
    with pytest.raises(ValueError, match="bf16"):
        check_value_head(48, "bf16", w, 0.0)
    with pytest.raises(ValueError, match="engine"):
        check_value_head(48, "auto", w, 0.0)


def test_torch_value_parsing():
    import torch
    nn = torch.nn
    torch.manual_seed(0)
    lin = nn.Linear(48, 1)
    w, b = torch_value(lin)
    assert w.shape == (48,) and np.array_equal(w, lin.weight.detach().numpy()[0]) and b == lin.bias.detach().numpy()[0]
    check_value_head(48, "mfma", w, b)
    w, b = torch_value(nn.Linear(32, 1, bias=False))
    assert w.shape == (32,) and b == 0.0
    for bad in (nn.Linear(48, 2), nn.Sequential(nn.Linear(48, 1)), nn.Tanh(), (np.zeros(48), 0.0), "critic"):
        with pytest.raises(ValueError, match=r"Linear\(W, 1\)"):
            torch_value(bad)


def test_new_entry_points_refuse_null_arguments():
    lib = _lib.load()
    assert lib.gaq_policy_set_value_head(None, None) == -1
    assert lib.gaq_policy_set_value_head_dev(None, None) == -1
    assert lib.gaq_policy_value_width(None) == -1
    assert lib.gaq_step_policy_ac_many_dev(None, None, 4, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.gaq_last_error()
    assert lib.gaq_gae_dev(None, 4, None, None, None, 0.99, 0.95, None, None, None) == -1
    assert b"null" in lib.gaq_last_error()


def test_binding_declares_the_new_entry_points():
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"gaq_policy_set_value_head", "gaq_policy_set_value_head_dev", "gaq_policy_value_width", "gaq_step_policy_ac_many_dev",
            "gaq_gae_dev"} <= names
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    assert len(sig["gaq_step_policy_ac_many_dev"]) == 10 and sig["gaq_gae_dev"][5:7] == [C.c_float, C.c_float]


def test_multi_device_env_names_the_new_method():
    from gym_art_amd.multi_device import _MultiDeviceMixin as M
    for name in ("rollout_policy_dev", "gae_dev"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(M, name)(M.__new__(M))
