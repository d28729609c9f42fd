"""The GRU policy engine (gaq_policy_desc_rnn, gym_art_amd.policy.GRUPolicy): policy_gru_kernel + the ordinary step launch per step.
Actions and state against an fp64 torch-semantics reference, bit-exact replays, rollouts split into calls, the done masking and
reset_hidden, exploration shared with the MLP engines, graph capture and refusals that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from tests.gru_util import _gru, _head, reference_rollout
from tests.policy_util import _bufs, _closed_loop, _dev, _replay, environ

pytestmark = pytest.mark.gpu

N = 2088                 # 32 tiles + a 40-lane tail tile

BASE = dict(num_envs=N, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True)
LOG_STD = np.log([0.1, 0.2, 0.3, 0.4]).astype(np.float32)


def _policy(env, H, head=(), act="tanh", out_tanh=True, log_std=None, seed=0):
    from gym_art_amd.policy import GRUPolicy
    return GRUPolicy(env, _gru(H, env.obs_dim, seed), _head(H, head, seed + 1), act, out_tanh, log_std)


def _rollout(env, pol, T_, h0=None):
    """reset_dev, .hidden <- h0 (zero by default), one closed-loop rollout: (obs0, obs, done, actions, final hidden) on the host"""
    import torch
    o0 = torch.empty((env.num_envs, env.obs_dim), device=_dev())
    env.reset_dev(o0)
    o0c = o0.clone()
    if h0 is None:
        pol.reset_hidden()
    else:
        pol.set_hidden(h0)
    o, r, d, a = _bufs(env, T_)
    env.rollout_policy_dev(pol, o, r, d, a)
    torch.cuda.synchronize()
    return o0c.cpu().numpy(), o.cpu().numpy(), d.cpu().numpy(), a.cpu().numpy(), pol.hidden.cpu().numpy()


TORCH_CASES = [(16, (), "tanh", True, True), (128, (), "tanh", False, False), (128, (64,), "relu", True, True),
               (256, (), "relu", False, True), (256, (128,), "tanh", True, False)]


@pytest.mark.parametrize("H,head,act,out_tanh,alias", TORCH_CASES)
def test_gru_against_torch(H, head, act, out_tanh, alias):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(**dict(BASE, alias_obs=alias))
    pol = _policy(env, H, head, act, out_tanh)
    gru, layers = _gru(H, env.obs_dim, 0), _head(H, head, 1)
    # one step from a random registered state
    h0 = (0.8 * np.random.RandomState(3).randn(N, H)).astype(np.float32)
    o0, o, d, a, h = _rollout(env, pol, 1, h0)
    ra, rh = reference_rollout(gru, layers, act, out_tanh, o0, o, d, h0)
    assert np.max(np.abs(a - ra)) < 1e-5 and np.max(np.abs(h - rh)) < 1e-5
    # 20 steps with auto-resets inside the window (an episode is 16 steps)
    o0, o, d, a, h = _rollout(env, pol, 20)
    assert 0 < int(d[:-1].sum())
    ra, rh = reference_rollout(gru, layers, act, out_tanh, o0, o, d, np.zeros((N, H)))
    assert np.max(np.abs(a - ra)) < 5e-5 and np.max(np.abs(h - rh)) < 5e-5
    pol.close(); env.close()


def test_gru_from_torch_modules():
    """GRUPolicy.from_torch of nn.GRU / nn.GRUCell and a Linear head gives torch's own forward pass (fp32, within 1e-5)"""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import GRUPolicy
    env = QuadrotorEnv(**BASE)
    torch.manual_seed(0)
    gru, head = torch.nn.GRU(18, 64), torch.nn.Sequential(torch.nn.Linear(64, 4), torch.nn.Tanh())
    pol = GRUPolicy.from_torch(gru, head, env)
    assert pol.hidden_size == 64 and tuple(pol.hidden.shape) == (N, 64)
    o0, o, d, a, h = _rollout(env, pol, 3)
    cell = torch.nn.GRUCell(18, 64)
    cell.load_state_dict({k[:-3]: v for k, v in gru.state_dict().items()})
    with torch.no_grad():
        hh = torch.zeros(N, 64)
        x = torch.from_numpy(o0)
        for t in range(3):
            hh = cell(x, hh)
            assert np.max(np.abs(head(hh).numpy() - a[t])) < 1e-5
            hh = torch.where(torch.from_numpy(d[t]).bool()[:, None], torch.zeros_like(hh), hh)
            x = torch.from_numpy(o[t])
    assert np.max(np.abs(hh.numpy() - h)) < 1e-5
    pol.close(); env.close()


@pytest.mark.parametrize("case", ["alias", "plain_info", "sense_noise", "per_env_rerandomized", "swarm"])
def test_gru_replay_is_bit_exact(case):
    import torch
    from gym_art_amd import QuadrotorEnv
    kw = dict(BASE)
    if case == "plain_info":
        kw.update(alias_obs=False, info=True)
    elif case == "sense_noise":
        kw["sense_noise"] = "default"
    elif case == "per_env_rerandomized":
        kw.update(dynamics_params="RandomQuad", dynamics_randomize_every=1)
    elif case == "swarm":
        kw["swarm"] = dict(agents=4)
    env = QuadrotorEnv(**kw)
    with environ(GAQ_NO_FUSED="1"):                   # the replay steps with the per-step launch too
        twin = QuadrotorEnv(**kw)
    pol = _policy(env, 128, (64,), "relu", True, LOG_STD)
    _, o, r, d, a = _closed_loop(env, pol, 24)
    assert int(d.sum()) > 0
    o2, r2, d2 = _replay(twin, a)
    assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), case
    pol.close(); env.close(); twin.close()


def test_split_rollout_is_invisible():
    import torch
    from gym_art_amd import QuadrotorEnv
    envs = [QuadrotorEnv(**BASE) for _ in range(2)]
    pols = [_policy(e, 64, (), "tanh", True, LOG_STD) for e in envs]
    outs = []
    for e, p, splits in zip(envs, pols, ([32], [16, 16])):
        o0 = torch.empty((N, 18), device=_dev())
        e.reset_dev(o0)
        o, r, d, a = _bufs(e, 32)
        t = 0
        for k in splits:
            e.rollout_policy_dev(p, o[t:t + k], r[t:t + k], d[t:t + k], a[t:t + k])
            t += k
        torch.cuda.synchronize()
        outs.append((o, a, d, p.hidden.clone()))
    assert int(outs[0][2].sum()) > 0
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    for x in pols + envs:
        x.close()


def test_done_masking_and_reset_hidden():
    import torch
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(**BASE)
    pol = _policy(env, 64)
    o0 = torch.empty((N, 18), device=_dev())
    env.reset_dev(o0)
    o, r, d, a = _bufs(env, 10)
    env.rollout_policy_dev(pol, o, r, d, a)
    # stagger the episodes: half the envs start over, so that the next window's last step finishes only some of them
    half = torch.from_numpy(np.random.RandomState(0).rand(N) < 0.5).to(_dev(), torch.uint8)
    env.reset_dev(o0, half)
    pol.reset_hidden(half)
    o, r, d, a = _bufs(env, 16)                                   # the reset half finishes in the last step, the rest at t = 5
    env.rollout_policy_dev(pol, o, r, d, a)
    torch.cuda.synchronize()
    last = d[-1].bool()
    assert 0 < int(last.sum()) < N
    zero_rows = (pol.hidden == 0).all(dim=1)
    assert torch.equal(zero_rows, last)
    # reset_hidden(mask) zeroes exactly the masked rows
    h0 = torch.randn(N, 64, device=_dev()) + 3.0
    pol.set_hidden(h0)
    m = np.random.RandomState(1).rand(N) < 0.3
    pol.reset_hidden(m)
    torch.cuda.synchronize()
    mt = torch.from_numpy(m).to(_dev())
    assert torch.equal(pol.hidden[mt], torch.zeros_like(pol.hidden[mt])) and torch.equal(pol.hidden[~mt], h0[~mt])
    pol.reset_hidden()
    torch.cuda.synchronize()
    assert not pol.hidden.any()
    pol.close(); env.close()


def test_exploration_equals_the_mlp_engines():
    """Zero weights: the GRU policy's actions are the exploration draws alone, the same as a zero MLPPolicy's"""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import GRUPolicy, MLPPolicy
    env, twin = QuadrotorEnv(**BASE), QuadrotorEnv(**BASE)
    H = 32
    z = np.zeros
    pg = GRUPolicy(env, (z((3 * H, 18)), z((3 * H, H)), z(3 * H), z(3 * H)), [(z((4, H)), z(4))], log_std=LOG_STD)
    pm = MLPPolicy.from_arrays(twin, [(z((H, 18)), z(H)), (z((4, H)), z(4))], log_std=LOG_STD, engine="mfma")
    _, o, r, d, a = _closed_loop(env, pg, 24)
    _, o2, r2, d2, a2 = _closed_loop(twin, pm, 24)
    assert int(d.sum()) > 0 and bool(a.any())
    assert torch.equal(a, a2) and torch.equal(o, o2) and torch.equal(d, d2)
    for x in (pg, pm, env, twin):
        x.close()


@pytest.mark.parametrize("alias", [True, None])
def test_graph_captured_gru_rollout(alias):
    """graph-safe mode: a captured 8-step GRU rollout replayed twice equals two eager calls on a twin, .hidden included"""
    import torch
    from gym_art_amd import QuadrotorEnv
    kw = dict(BASE, alias_obs=alias)
    graphed, eager = QuadrotorEnv(**kw), QuadrotorEnv(**kw)
    pols = [_policy(e, 64, (), "tanh", False, LOG_STD) for e in (graphed, eager)]
    bufs = []
    for e in (graphed, eager):
        e.set_graph_safe(True)
        o0 = torch.empty((N, 18), device=_dev())
        e.reset_dev(o0)
        bufs.append(_bufs(e, 8))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # warm-up on a side stream (torch's capture protocol)
        graphed.rollout_policy_dev(pols[0], *bufs[0])
    torch.cuda.current_stream().wait_stream(side)
    eager.rollout_policy_dev(pols[1], *bufs[1])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*bufs))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.rollout_policy_dev(pols[0], *bufs[0])
    dones = 0
    for _ in range(2):
        g.replay()
        eager.rollout_policy_dev(pols[1], *bufs[1])
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(*bufs))
        assert torch.equal(pols[0].hidden, pols[1].hidden)
        dones += int(bufs[0][2].sum())
    assert dones > 0
    for x in pols + [graphed, eager]:
        x.close()


def test_refusals_launch_nothing():
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    env, twin, other = QuadrotorEnv(**BASE), QuadrotorEnv(**BASE), QuadrotorEnv(**BASE)
    lib = _lib.load()
    pol, pol_other = _policy(env, 64), _policy(other, 64)
    for e in (env, twin, other):
        e.reset_dev(torch.empty((N, 18), device=_dev()))
    o, r, d, a = _bufs(env, 4)
    # a feed-forward policy has no hidden state
    mlp = MLPPolicy.from_arrays(env, [(np.zeros((16, 18)), np.zeros(16)), (np.zeros((4, 16)), np.zeros(4))], engine="mfma")
    assert lib.gaq_policy_cell(mlp.handle) == 0 and lib.gaq_policy_cell(pol.handle) == 1
    assert lib.gaq_policy_set_hidden_dev(mlp.handle, _lib.ptr(pol.hidden)) == -1
    assert lib.gaq_policy_reset_hidden_dev(mlp.handle, None, None) == -1
    # a misaligned buffer is refused and the registration stays
    assert lib.gaq_policy_set_hidden_dev(pol.handle, C.c_void_p(pol.hidden.data_ptr() + 4)) == -1
    # a policy of another env
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gaq_step_policy_many_dev(env._handle, pol_other.handle, 4, _lib.ptr(o), _lib.ptr(r), _lib.ptr(d), _lib.ptr(a), st) == -1
    with pytest.raises(ValueError):
        env.rollout_policy_dev(pol_other, o, r, d, a)
    # no registered buffer: GAQ_ERR_STATE
    _lib.check(lib.gaq_policy_set_hidden_dev(pol.handle, None))
    with pytest.raises(_lib.GaqError):
        env.rollout_policy_dev(pol, o, r, d, a)
    with pytest.raises(_lib.GaqError):
        pol.reset_hidden()
    torch.cuda.synchronize()
    # nothing moved: the env and its twin step alike
    acts = torch.rand((6, N, 4), device=_dev()) * 2 - 1
    o1, r1, d1, _ = _bufs(env, 6)
    o2, r2, d2, _ = _bufs(twin, 6)
    env.step_many_dev(acts, o1, r1, d1)
    twin.step_many_dev(acts, o2, r2, d2)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    for x in (mlp, pol, pol_other, env, twin, other):
        x.close()
