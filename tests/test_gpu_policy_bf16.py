"""The bf16 policy engine (GAQ_POLICY_ENGINE_MFMA_BF16, MLPPolicy(engine="bf16")): policy_mfma_bf16_kernel + the ordinary step launch per
step.  Actions against the contract's reference forward (tests/policy_bf16_ref.py), against a bf16 torch actor, bit-exact replays,
determinism, shard-independent exploration and refusals that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from tests.policy_bf16_ref import forward
from tests.policy_util import _bufs, _closed_loop, _dev, _net, _replay, environ

pytestmark = pytest.mark.gpu

N = 2088                 # 32 tiles + a 40-lane tail tile: the last workgroup is partial

BASE = dict(num_envs=N, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True)
LOG_STD = np.log([0.1, 0.2, 0.3, 0.4]).astype(np.float32)
NETS = [[64, 64], [256, 256], [256, 256, 256]]
# contract tolerances: a different fp32 summation order can flip a hidden unit's bf16 rounding (one bf16 ulp of that activation, times
# its weights downstream); everything else agrees to fp32 rounding of the sums.  Measured on MI355X over every case below: worst error
# 1.1e-3, at least 99.68 % of the actions within 1e-4.  The all-actions bound is tightened from the contract's 1e-2 to 5e-3 (4x margin).
ATOL_ALL, ATOL_MOST, FRAC_MOST = 5e-3, 1e-4, 0.99


@pytest.mark.parametrize("n", [N, 1 << 20])
@pytest.mark.parametrize("out_tanh", [True, False])
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("widths", NETS)
def test_first_actions_follow_the_contract(widths, act, out_tanh, n):
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy, torch_layers
    env = QuadrotorEnv(**dict(BASE, num_envs=n))
    net = _net(widths, act, out_tanh, seed=len(widths) + widths[-1])
    pol = MLPPolicy.from_torch(net, env, engine="bf16")
    assert pol.engine == "bf16"
    o0, _, _, _, a = _closed_loop(env, pol, 1)
    layers, _, _ = torch_layers(net)
    ref = forward(layers, act, out_tanh, o0)
    err = (a[0].double() - ref).abs()
    worst, frac = float(err.max()), float((err <= ATOL_MOST).double().mean())
    print("bf16 contract %s %s out_tanh=%d n=%d: max %.3g, within %.0e: %.5f" % (widths, act, out_tanh, n, worst, ATOL_MOST, frac))
    assert worst <= ATOL_ALL, worst
    assert frac >= FRAC_MOST, frac
    pol.close(); env.close()


@pytest.mark.parametrize("case", ["alias", "fp64_planes", "graph_safe"])
def test_replay_is_bit_exact(case):
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    kw = dict(BASE)
    if case == "fp64_planes":
        kw.update(alias_obs=False, precision="fp64")
    env = QuadrotorEnv(**kw)
    # the replay must take the per-step launch too: in the alias layout step_many_dev would otherwise fuse it into the open-loop rollout
    # kernel (tests/test_gpu_policy_mfma.py test_wide_replay_is_bit_exact)
    with environ(GAQ_NO_FUSED="1"):
        twin = QuadrotorEnv(**kw)
    if case == "graph_safe":
        env.set_graph_safe(True); twin.set_graph_safe(True)
    pol = MLPPolicy.from_torch(_net([256, 256], "relu"), env, log_std=LOG_STD, engine="bf16")
    _, o, r, d, a = _closed_loop(env, pol, 64)
    assert int(d.sum()) > 0
    o2, r2, d2 = _replay(twin, a)
    assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), case
    pol.close(); env.close(); twin.close()


def test_rollouts_are_deterministic():
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    net = _net([256, 256, 256], "tanh", True)
    runs = []
    for _ in range(2):
        env = QuadrotorEnv(**BASE)
        pol = MLPPolicy.from_torch(net, env, log_std=LOG_STD, engine="bf16")
        runs.append(_closed_loop(env, pol, 32))
        pol.close(); env.close()
    assert all(torch.equal(x, y) for x, y in zip(*runs))


BF16_ULPS = 4


def test_bf16_torch_actor():
    """from_torch on a bf16 module loses nothing in the weights; its actions agree with the module's own bf16 forward pass (which rounds
    every Linear's output and every activation to bf16) within BF16_ULPS bf16 ulps of 1, the output tanh's range."""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    env = QuadrotorEnv(**BASE)
    net = _net([256, 256], "tanh", True, seed=11).to(torch.bfloat16)
    pol = MLPPolicy.from_torch(net, env, engine="bf16")
    o0, _, _, _, a = _closed_loop(env, pol, 1)
    with torch.no_grad():
        ref = net.to(_dev())(o0.to(torch.bfloat16)).float()
    err = float((a[0] - ref).abs().max())
    print("bf16 torch actor: max |a - module(obs)| = %.3g" % err)
    assert err <= BF16_ULPS * 2.0 ** -8, err
    pol.close(); env.close()


def test_exploration_is_keyed_by_the_global_env_id():
    """A zero 256-256 net: the actions are the exploration draws alone, and global env g draws the same ones in either handle."""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    off = 128
    full = QuadrotorEnv(**dict(BASE, num_envs=384))
    part = QuadrotorEnv(**dict(BASE, num_envs=256, env_id_offset=off))
    zero = [(np.zeros((256, 18), np.float32), np.zeros(256, np.float32)), (np.zeros((256, 256), np.float32), np.zeros(256, np.float32)),
            (np.zeros((4, 256), np.float32), np.zeros(4, np.float32))]
    pf = MLPPolicy.from_arrays(full, zero, log_std=LOG_STD, engine="bf16")
    pp = MLPPolicy.from_arrays(part, zero, log_std=LOG_STD, engine="bf16")
    af = _closed_loop(full, pf, 8)[4]
    ap = _closed_loop(part, pp, 8)[4]
    assert torch.equal(af[:, off:], ap)
    assert float(af[..., 3].std()) > 0.3
    # and they are the draws of the fp32 MFMA engine
    ref = QuadrotorEnv(**dict(BASE, num_envs=384))
    pm = MLPPolicy.from_arrays(ref, zero, log_std=LOG_STD, engine="mfma")
    assert torch.equal(_closed_loop(ref, pm, 8)[4], af)
    for x in (pf, pp, pm, full, part, ref):
        x.close()


def test_refusals_launch_nothing():
    import torch
    from gym_art_amd import QuadrotorEnv, _lib
    from gym_art_amd.policy import ENGINES, MLPPolicy, _DescEx
    lib = _lib.load()
    kw = dict(BASE, num_envs=256)
    env, twin = QuadrotorEnv(**kw), QuadrotorEnv(**kw)
    for e in (env, twin):
        e.reset_dev(torch.empty((256, 18), device=_dev()))

    def desc(in_dim=18, widths=(256, 256), engine=ENGINES["bf16"]):
        x = _DescEx()
        x.struct_size = C.sizeof(_DescEx)
        x.in_dim, x.n_hidden = in_dim, len(widths)
        for k, w in enumerate(widths):
            x.width[k] = w
        x.engine = engine
        return x
    h = C.c_void_p()
    four = desc(widths=(64, 64, 64))
    four.n_hidden = 4
    for bad in (desc(in_dim=17), desc(widths=(272,)), desc(widths=(24,)), four):
        assert lib.gaq_policy_create_ex(env._handle, C.byref(bad), C.byref(h)) == -1
    mell = QuadrotorEnv(**dict(kw, raw_control=False))
    assert lib.gaq_policy_create_ex(mell._handle, C.byref(desc()), C.byref(h)) == -1
    with pytest.raises(Exception):
        MLPPolicy.from_torch(_net([256, 256]), mell, engine="bf16")
    mell.close()
    o, r, d, a = _bufs(env, 4)
    assert lib.gaq_policy_create_ex(env._handle, C.byref(desc()), C.byref(h)) == 0            # weights never set
    assert lib.gaq_policy_engine(h) == 3
    assert lib.gaq_step_policy_many_dev(env._handle, h, 4, _lib.ptr(o), _lib.ptr(r), _lib.ptr(d), _lib.ptr(a), None) == -1
    lib.gaq_policy_destroy(h)
    # nothing was launched: env and its twin still step alike
    x = torch.rand((4, 256, 4), device=_dev()) * 2 - 1
    s1, s2 = _bufs(env, 4), _bufs(twin, 4)
    env.step_many_dev(x, *s1[:3]); twin.step_many_dev(x, *s2[:3])
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(s1[:3], s2[:3]))
    env.close(); twin.close()


def test_policy_engine_reports_bf16():
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    env = QuadrotorEnv(**dict(BASE, num_envs=256))
    p = MLPPolicy.from_torch(_net([64, 64]), env, engine="bf16")
    assert p.engine == "bf16" and p._lib.gaq_policy_engine(p.handle) == 3
    auto = MLPPolicy.from_torch(_net([256, 256]), env)
    assert auto.engine == "mfma"
    for x in (p, auto, env):
        x.close()
