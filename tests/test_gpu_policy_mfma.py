"""The MFMA policy engine (GAQ_POLICY_ENGINE_MFMA, MLPPolicy(engine="mfma")): policy_mfma_kernel + the ordinary step launch per step.
Bit-equal to the VALU engine on every net both accept, the torch forward pass on 256-wide nets, bit-exact replays, shard-independent
exploration and refusals that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from tests.policy_util import _bufs, _closed_loop, _dev, _net, _replay, environ

pytestmark = pytest.mark.gpu

N = 2088                 # 32 tiles + a 40-lane tail tile

BASE = dict(num_envs=N, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True)
LOG_STD = np.log([0.1, 0.2, 0.3, 0.4]).astype(np.float32)

EQ_CASES = [([64, 64], "tanh", True, "fp64", True), ([16], "relu", False, "fp64", True), ([128, 128, 128], "tanh", False, "fp32", True),
            ([32, 128, 16], "relu", True, "fp64", False)]


@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("widths,act,out_tanh,precision,alias", EQ_CASES)
def test_mfma_is_bit_equal_to_the_valu_engine(widths, act, out_tanh, precision, alias, explore):
    """Same weights, same reset: the MFMA engine's whole trajectory (obs, reward, done, actions) equals the VALU per-step path's."""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    kw = dict(BASE, precision=precision, alias_obs=alias)
    env = QuadrotorEnv(**kw)
    with environ(GAQ_NO_FUSED="1"):
        ref = QuadrotorEnv(**kw)
    net = _net(widths, act, out_tanh, seed=len(widths) + widths[0])
    ls = LOG_STD if explore else None
    pm, pv = MLPPolicy.from_torch(net, env, log_std=ls, engine="mfma"), MLPPolicy.from_torch(net, ref, log_std=ls)
    assert pm.engine == "mfma" and pv.engine == "valu"
    _, o, r, d, a = _closed_loop(env, pm, 24)
    _, o2, r2, d2, a2 = _closed_loop(ref, pv, 24)
    assert int(d.sum()) > 0
    assert torch.equal(a, a2) and torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2)
    for x in (pm, pv, env, ref):
        x.close()


def test_mfma_is_bit_equal_to_the_valu_engine_in_graph_safe_mode():
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    env = QuadrotorEnv(**BASE)
    with environ(GAQ_NO_FUSED="1"):
        ref = QuadrotorEnv(**BASE)
    for e in (env, ref):
        e.set_graph_safe(True)
    net = _net([64, 64])
    pm, pv = MLPPolicy.from_torch(net, env, log_std=LOG_STD, engine="mfma"), MLPPolicy.from_torch(net, ref, log_std=LOG_STD)
    outs = []
    for e, p in ((env, pm), (ref, pv)):
        o0 = torch.empty((N, 18), device=_dev())
        e.reset_dev(o0)
        run = []
        for _ in range(3):                                          # the device step counter advances across calls
            o, r, d, a = _bufs(e, 8)
            e.rollout_policy_dev(p, o, r, d, a)
            run.append((o, r, d, a))
        torch.cuda.synchronize()
        outs.append(run)
    for x, y in zip(*outs):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    for x in (pm, pv, env, ref):
        x.close()


def test_first_actions_equal_the_fused_valu_path():
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    for precision in ("fp32", "fp64"):
        kw = dict(BASE, precision=precision)
        fused, env = QuadrotorEnv(**kw), QuadrotorEnv(**kw)
        net = _net([64, 64])
        pf, pm = MLPPolicy.from_torch(net, fused, log_std=LOG_STD), MLPPolicy.from_torch(net, env, log_std=LOG_STD, engine="mfma")
        a = _closed_loop(fused, pf, 4)[4]
        a2 = _closed_loop(env, pm, 4)[4]
        assert torch.equal(a[0], a2[0]), precision
        for x in (pf, pm, fused, env):
            x.close()


WIDE = [([256, 256], "tanh", True, "fp32", True), ([256, 256, 256], "relu", False, "fp64", True),
        ([256, 128, 64], "tanh", False, "fp64", False), ([256, 16], "relu", True, "fp32", False),
        ([256, 256], "relu", False, "fp64", False), ([256, 256, 256], "tanh", True, "fp32", False),
        ([256, 128, 64], "relu", True, "fp32", True), ([256, 16], "tanh", False, "fp64", True)]


def _torch_check(env, widths, act, out_tanh, T_):
    import torch
    from gym_art_amd.policy import MLPPolicy
    net = _net(widths, act, out_tanh, seed=len(widths) + widths[-1]).to(_dev())
    pol = MLPPolicy.from_torch(net, env)
    assert pol.engine == "mfma"
    o0, o, r, d, a = _closed_loop(env, pol, T_)
    prev = torch.cat([o0[None], o[:-1]])
    with torch.no_grad():
        ref = torch.cat([net(prev[t]) for t in range(T_)]).reshape(a.shape)
    err = float((a - ref).abs().max())
    pol.close()
    return err, d


@pytest.mark.parametrize("widths,act,out_tanh,precision,alias", WIDE)
def test_wide_actions_are_the_torch_policy_on_the_previous_observation(widths, act, out_tanh, precision, alias):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(**dict(BASE, alias_obs=alias, precision=precision))
    err, d = _torch_check(env, widths, act, out_tanh, 16)
    assert int(d.sum()) > 0
    assert err < 1e-5, err
    env.close()


def test_wide_actions_at_2_pow_20_envs():
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(**dict(BASE, num_envs=1 << 20))
    err, _ = _torch_check(env, [256, 256, 256], "tanh", True, 2)
    assert err < 1e-5, err
    env.close()


@pytest.mark.parametrize("case", ["alias", "plain", "info", "sense_noise", "per_env_rerandomized"])
def test_wide_replay_is_bit_exact(case):
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    kw = dict(BASE, alias_obs=case == "alias")
    if case == "info":
        kw["info"] = True
    elif case == "sense_noise":
        kw["sense_noise"] = "default"
    elif case == "per_env_rerandomized":
        kw.update(dynamics_params="RandomQuad", dynamics_randomize_every=1)
    env = QuadrotorEnv(**kw)
    # an MFMA policy always steps with the per-step launch; in the alias layout step_many_dev would fuse the replay into the open-loop
    # rollout kernel, whose physics is that launch's within an fp32 ulp (tests/test_gpu_policy_rollout.py test_fused_equals_fallback)
    with environ(GAQ_NO_FUSED="1"):
        twin = QuadrotorEnv(**kw)
    pol = MLPPolicy.from_torch(_net([256, 256], "relu"), env, log_std=LOG_STD)
    assert pol.engine == "mfma"
    _, o, r, d, a = _closed_loop(env, pol, 24)
    assert int(d.sum()) > 0
    o2, r2, d2 = _replay(twin, a)
    assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), case
    pol.close(); env.close(); twin.close()


def test_wide_exploration_is_keyed_by_the_global_env_id():
    """A zero 256-256 net: the actions are the exploration draws alone, and global env g draws the same ones in either handle."""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    off = 128
    full = QuadrotorEnv(**dict(BASE, num_envs=256))
    part = QuadrotorEnv(**dict(BASE, num_envs=128, env_id_offset=off))
    zero = [(np.zeros((256, 18), np.float32), np.zeros(256, np.float32)), (np.zeros((256, 256), np.float32), np.zeros(256, np.float32)),
            (np.zeros((4, 256), np.float32), np.zeros(4, np.float32))]
    pf, pp = MLPPolicy.from_arrays(full, zero, log_std=LOG_STD), MLPPolicy.from_arrays(part, zero, log_std=LOG_STD)
    assert pf.engine == pp.engine == "mfma"
    af = _closed_loop(full, pf, 8)[4]
    ap = _closed_loop(part, pp, 8)[4]
    assert torch.equal(af[:, off:], ap)
    assert float(af[..., 3].std()) > 0.3
    for x in (pf, pp, full, part):
        x.close()


def test_refusals_launch_nothing():
    import torch
    from gym_art_amd import QuadrotorEnv, _lib
    from gym_art_amd.policy import ENGINES, _DescEx
    lib = _lib.load()
    kw = dict(BASE, num_envs=256)
    env, twin = QuadrotorEnv(**kw), QuadrotorEnv(**kw)
    for e in (env, twin):
        e.reset_dev(torch.empty((256, 18), device=_dev()))

    def desc(in_dim=18, widths=(256, 256), engine=ENGINES["mfma"]):
        x = _DescEx()
        x.struct_size = C.sizeof(_DescEx)
        x.in_dim, x.n_hidden = in_dim, len(widths)
        for k, w in enumerate(widths):
            x.width[k] = w
        x.engine = engine
        return x
    h = C.c_void_p()
    assert lib.gaq_policy_create_ex(env._handle, C.byref(desc(engine=ENGINES["valu"])), C.byref(h)) == -1
    assert lib.gaq_policy_create_ex(env._handle, C.byref(desc(engine=7)), C.byref(h)) == -1
    assert lib.gaq_policy_create_ex(env._handle, C.byref(desc(in_dim=17)), C.byref(h)) == -1
    assert lib.gaq_policy_create_ex(env._handle, C.byref(desc(widths=(272,))), C.byref(h)) == -1
    bad = desc()
    bad.struct_size -= 4
    assert lib.gaq_policy_create_ex(env._handle, C.byref(bad), C.byref(h)) == -1
    mell = QuadrotorEnv(**dict(kw, raw_control=False))
    assert lib.gaq_policy_create_ex(mell._handle, C.byref(desc()), C.byref(h)) == -1
    mell.close()
    o, r, d, a = _bufs(env, 4)
    assert lib.gaq_policy_create_ex(env._handle, C.byref(desc()), C.byref(h)) == 0            # weights never set
    assert lib.gaq_policy_engine(h) == ENGINES["mfma"]
    assert lib.gaq_step_policy_many_dev(env._handle, h, 4, _lib.ptr(o), _lib.ptr(r), _lib.ptr(d), _lib.ptr(a), None) == -1
    lib.gaq_policy_destroy(h)
    # nothing was launched: env and its twin still step alike
    x = torch.rand((4, 256, 4), device=_dev()) * 2 - 1
    s1, s2 = _bufs(env, 4), _bufs(twin, 4)
    env.step_many_dev(x, *s1[:3]); twin.step_many_dev(x, *s2[:3])
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(s1[:3], s2[:3]))
    env.close(); twin.close()


def test_policy_engine_reports_the_engine_in_use():
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    env = QuadrotorEnv(**dict(BASE, num_envs=256))
    small, wide = MLPPolicy.from_torch(_net([64, 64]), env), MLPPolicy.from_torch(_net([256, 256]), env)
    assert small.engine == "valu" and wide.engine == "mfma"
    forced = MLPPolicy.from_torch(_net([64, 64]), env, engine="mfma")
    assert forced.engine == "mfma"
    with pytest.raises(ValueError, match="128"):
        MLPPolicy.from_torch(_net([256, 256]), env, engine="valu")
    for x in (small, wide, forced, env):
        x.close()
