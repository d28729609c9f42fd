"""Closed-loop rollouts (QuadrotorEnv.rollout_policy_dev / gaq_step_policy_many_dev): a device MLP picks every action from the previous
observation, fused into one launch on the alias layouts (policy_rollout_kernel<F>) and as policy launch + step launch per step elsewhere."""
import ctypes as C

import numpy as np
import pytest

from tests.policy_util import _bufs, _closed_loop, _dev, _net, _replay, environ

pytestmark = pytest.mark.gpu

N, T = 2088, 64          # 2088 = 32 tiles + a 40-lane tail tile


def _launched(kind):
    from gym_art_amd import _lib
    buf = (C.c_uint32 * 64)()
    k = _lib.load().gaq_launched_variants(kind, buf, 64)
    return {int(buf[i]) for i in range(k)}


BASE = dict(num_envs=N, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True)
LOG_STD = np.log([0.1, 0.2, 0.3, 0.4]).astype(np.float32)


@pytest.mark.parametrize("path", ["fused", "fallback"])
def test_replay_of_the_recorded_actions_is_bit_exact(path):
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    with environ(GAQ_NO_FUSED="1" if path == "fallback" else "0"):
        env, twin = QuadrotorEnv(**BASE), QuadrotorEnv(**BASE)
    pol = MLPPolicy.from_torch(_net([64, 64]), env, log_std=LOG_STD)
    _, o, r, d, a = _closed_loop(env, pol, T)
    assert int(d.sum()) > N                                  # auto-resets inside the rollout
    o2, r2, d2 = _replay(twin, a)
    assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2)
    if path == "fused":                                       # policy_rollout_kernel<F> of the alias kernel (launch record kind 2)
        assert _launched(2) & (set(range(16, 24)) | set(range(48, 56)))
    # and the state after the call is the same: one more open-loop step on both
    x = torch.rand((1, N, 4), device=_dev()) * 2 - 1
    s1, s2 = _bufs(env, T_=1), _bufs(twin, T_=1)
    env.step_many_dev(x, *s1[:3]); twin.step_many_dev(x, *s2[:3])
    assert all(torch.equal(u, v) for u, v in zip(s1[:3], s2[:3]))
    pol.close(); env.close(); twin.close()


@pytest.mark.parametrize("widths,act,out_tanh,precision,alias", [
    ([64, 64], "tanh", True, "fp64", True),
    ([16], "relu", False, "fp64", True),
    ([128, 128, 128], "tanh", False, "fp32", True),
    ([32, 128, 16], "relu", True, "fp64", False),
    ([128, 128], "relu", True, "fp64", False),
])
def test_actions_are_the_torch_policy_on_the_previous_observation(widths, act, out_tanh, precision, alias):
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    env = QuadrotorEnv(**dict(BASE, alias_obs=alias, precision=precision))
    net = _net(widths, act, out_tanh, seed=len(widths) + widths[0]).to(_dev())
    pol = MLPPolicy.from_torch(net, env)
    o0, o, r, d, a = _closed_loop(env, pol, T_=16)
    assert int(d.sum()) > 0                                  # an env's action after its reset comes from the reset observation
    prev = torch.cat([o0[None], o[:-1]])
    with torch.no_grad():
        ref = net(prev)
    err = float((a - ref).abs().max())
    assert err < 1e-5, err
    pol.close(); env.close()


def test_fused_equals_fallback():
    """The fused path and the fallback run the same policy routine: on the same observation (the first step) their actions -- exploration
    included -- are bit-equal.  After that the physics of the two paths is what gaq_step_many_dev's fused and per-step paths already are to
    each other (tests/test_gpu_kernel_coverage.py: within an fp32 ulp per step), so the trajectories agree to that precision."""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    for precision in ("fp32", "fp64"):
        kw = dict(BASE, precision=precision)
        fused = QuadrotorEnv(**kw)
        with environ(GAQ_NO_FUSED="1"):
            fb = QuadrotorEnv(**kw)
        net = _net([64, 64])
        p1, p2 = MLPPolicy.from_torch(net, fused, log_std=LOG_STD), MLPPolicy.from_torch(net, fb, log_std=LOG_STD)
        _, o, r, d, a = _closed_loop(fused, p1, T_=4)
        _, o2, r2, d2, a2 = _closed_loop(fb, p2, T_=4)
        assert torch.equal(a[0], a2[0]), precision
        tol = 2e-5 if precision == "fp32" else 1e-6
        assert torch.allclose(o, o2, rtol=tol, atol=tol) and torch.allclose(a, a2, rtol=1e-4, atol=1e-4), precision
        for x in (p1, p2, fused, fb):
            x.close()


@pytest.mark.parametrize("case", ["plain", "info", "sense_noise", "per_env_rerandomized"])
def test_fallback_configurations_replay_bit_exact(case):
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    kw = dict(BASE, alias_obs=False)
    if case == "info":
        kw["info"] = True
    elif case == "sense_noise":
        kw["sense_noise"] = "default"
    elif case == "per_env_rerandomized":
        kw.update(dynamics_params="RandomQuad", dynamics_randomize_every=1)
    env, twin = QuadrotorEnv(**kw), QuadrotorEnv(**kw)
    pol = MLPPolicy.from_torch(_net([64, 64], "relu"), env, log_std=LOG_STD)
    _, o, r, d, a = _closed_loop(env, pol, T_=24)
    assert int(d.sum()) > 0
    o2, r2, d2 = _replay(twin, a)
    assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), case
    pol.close(); env.close(); twin.close()


def test_exploration_noise_statistics_and_keying():
    import torch
    from scipy import stats
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    n, steps = 16384, 64                                     # 2^20 env-steps
    env = QuadrotorEnv(**dict(BASE, num_envs=n))
    zero = [(np.zeros((16, 18), np.float32), np.zeros(16, np.float32)), (np.zeros((4, 16), np.float32), np.zeros(4, np.float32))]
    pol = MLPPolicy.from_arrays(env, zero, log_std=LOG_STD)
    _, _, _, _, a = _closed_loop(env, pol, T_=steps)
    z = a.reshape(-1, 4).double().cpu().numpy()
    sd = np.exp(LOG_STD.astype(np.float64))
    for k in range(4):
        assert abs(z[:, k].mean()) < 0.01 * sd[k], k
        assert abs(z[:, k].std() / sd[k] - 1) < 0.01, k
        assert stats.kstest(z[:, k] / sd[k], "norm").pvalue > 1e-3, k
    pol.close(); env.close()
    # the draws of global env g do not depend on the handle it runs in
    off = 128
    full = QuadrotorEnv(**dict(BASE, num_envs=256))
    part = QuadrotorEnv(**dict(BASE, num_envs=128, env_id_offset=off))
    pf, pp = MLPPolicy.from_arrays(full, zero, log_std=LOG_STD), MLPPolicy.from_arrays(part, zero, log_std=LOG_STD)
    af = _closed_loop(full, pf, T_=8)[4]
    ap = _closed_loop(part, pp, T_=8)[4]
    assert torch.equal(af[:, off:], ap)
    for x in (pf, pp, full, part):
        x.close()


def test_refusals_launch_nothing():
    import torch
    from gym_art_amd import QuadrotorEnv, _lib
    from gym_art_amd.policy import MLPPolicy, _Desc
    lib = _lib.load()
    kw = dict(BASE, num_envs=256)
    env, twin = QuadrotorEnv(**kw), QuadrotorEnv(**kw)
    for e in (env, twin):
        e.reset_dev(torch.empty((256, 18), device=_dev()))
    o, r, d, a = _bufs(env, T_=4)

    def desc(in_dim=18, widths=(64, 64)):
        x = _Desc()
        x.struct_size = C.sizeof(_Desc)
        x.in_dim, x.n_hidden = in_dim, len(widths)
        for k, w in enumerate(widths):
            x.width[k] = w
        return x
    h = C.c_void_p()
    assert lib.gaq_policy_create(env._handle, C.byref(desc(in_dim=17)), C.byref(h)) == -1
    assert lib.gaq_policy_create(env._handle, C.byref(desc(widths=(24,))), C.byref(h)) == -1
    assert lib.gaq_policy_create(env._handle, C.byref(desc(widths=(256,))), C.byref(h)) == -1
    assert lib.gaq_policy_create(env._handle, C.byref(desc()), C.byref(h)) == 0          # weights never set
    assert lib.gaq_step_policy_many_dev(env._handle, h, 4, _lib.ptr(o), _lib.ptr(r), _lib.ptr(d), _lib.ptr(a), None) == -1
    lib.gaq_policy_destroy(h)
    pol = MLPPolicy.from_torch(_net([64, 64]), env)
    assert lib.gaq_step_policy_many_dev(env._handle, pol.handle, 0, _lib.ptr(o), _lib.ptr(r), _lib.ptr(d), _lib.ptr(a), None) == -1
    with pytest.raises(ValueError):
        MLPPolicy.from_torch(_net([64], D=17), env)
    mell = QuadrotorEnv(**dict(kw, raw_control=False))
    assert lib.gaq_policy_create(mell._handle, C.byref(desc()), C.byref(h)) == -1
    mell.close()
    # nothing was launched: env and its twin still step alike
    x = torch.rand((4, 256, 4), device=_dev()) * 2 - 1
    s1, s2 = _bufs(env, T_=4), _bufs(twin, T_=4)
    env.step_many_dev(x, *s1[:3]); twin.step_many_dev(x, *s2[:3])
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(s1[:3], s2[:3]))
    pol.close(); env.close(); twin.close()
