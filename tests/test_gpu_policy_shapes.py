"""Every device-policy engine against an fp64 reference at the shapes its kernels branch on: each observation width the env offers (an odd
number of full k-steps, partial k-steps of 0 to 3 rows, bf16 first layers of 1 to 4 k-steps), widths of an odd number of 16-unit chunks
(waves with different chunk counts, or none), single partial tiles, one full tile, one tile plus a sliver, and the GRU engine's largest LDS
footprint.  Each rollout's action[t] is checked against the reference run on the device's recorded obs[t - 1], on nets whose units do not
saturate (tests/mlp_ref.py), and each case asserts that it has teeth."""
import ctypes as C

import numpy as np
import pytest

from tests.gru_util import _gru, _head, reference_rollout
from tests.mlp_ref import _scaled_layers, assert_not_saturated, forward64
from tests.policy_bf16_ref import forward as bf16_forward
from tests.policy_util import _bufs, _closed_loop, _dev, environ
from tests.test_gpu_policy_bf16 import ATOL_ALL, ATOL_MOST, FRAC_MOST

pytestmark = pytest.mark.gpu

T = 20                   # an episode is 15 steps at ep_time=0.15: every env auto-resets inside the window

# (obs_repr, swarm agents, obs_dim): every distinct observation width.  fp32 k-steps of 4 inputs: 13 -> 3 full (odd) + 1 row, 14 -> 3 + 2,
# 18 -> 4 + 2, 19 -> 4 + 3, 20 -> 5 (odd) + 0, 22 -> 5 + 2, 25 -> 6 + 1, 24 -> 6, 36 -> 9 (odd), 60 -> 15 (odd), 108 -> 27 (odd);
# bf16 k-steps of 32 inputs: 1 up to 24, 2 at 36 and 60, 4 at 108
OBS = [("xyz_vxyz_quat_omega", 0, 13), ("xyzr_vxyzr_quat_omega_h", 0, 14), ("xyz_vxyz_R_omega", 0, 18), ("xyz_vxyz_R_omega_h", 0, 19),
       ("xyz_vxyz_R_omega_t2w_t2t", 0, 20), ("xyz_vxyz_R_omega_act", 0, 22), ("xyz_vxyz_R_omega_acc_act", 0, 25),
       ("xyz_vxyz_R_omega", 2, 24), ("xyz_vxyz_R_omega", 4, 36), ("xyz_vxyz_R_omega", 8, 60), ("xyz_vxyz_R_omega", 16, 108)]
OBS_IDS = ["d%d" % d for _, _, d in OBS]

# nets of both fp32 engines (VALU widths stop at 128), then the MFMA engine's wider ones; 48, 80, 144 and 240 are 3, 5, 9 and 15 chunks
FP32_NETS = [[16], [48], [80, 48], [32, 128, 16], [128, 128, 128]]
MFMA_NETS = [[144], [240, 80], [48, 256, 16], [256, 256, 256]]
BF16_NETS = [[16], [48, 48], [208], [240, 80], [48, 256, 16], [144, 48]]
GRU_H, GRU_HEADS = [48, 80, 240], [(), (48,), (16, 80)]

# Worst |device - fp64 reference| measured on MI355X over every case of this file: 3.2e-6 for the fp32 engines (VALU, MFMA and the fused
# VALU path alike), 8.0e-7 for the GRU engine (actions and state); the bounds leave 4.6x and 5x of margin
ATOL_FP32 = 1.5e-5
ATOL_GRU = 4e-6
# bf16: test_gpu_policy_bf16's tolerances, which are bf16 ulps of 1.  A relu unit is unbounded, and where the device's fp32 sum rounds it
# to the other bf16 neighbour than the reference's fp64 sum, that costs one ulp of the unit: at full scale relu units reach 4 (ulp 2^-5)
# and the worst action was off by 7.7e-3.  So the relu nets of the bf16 cases run their first layer at RELU_BF16_SCALE, which keeps
# their units near the range of tanh's (worst measured below, in the test's output)
RELU_BF16_SCALE = 0.4


def _batches(agents):
    """a single partial tile, one full tile, one tile + a sliver, 32 tiles + a 48-env tail; multiples of 4 (T > 1 with an odd obs_dim)
    and of the swarm's agents"""
    q = max(4, agents)
    return [q, 64, 64 + q, 2096]


def _kw(obs, n):
    rep, agents, _ = obs
    kw = dict(num_envs=n, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True, obs_repr=rep)
    if agents:
        kw["swarm"] = dict(agents=agents)
    return kw


def _env(obs, n, fused=True):
    from gym_art_amd import QuadrotorEnv
    if fused:
        env = QuadrotorEnv(**_kw(obs, n))
    else:
        with environ(GAQ_NO_FUSED="1"):
            env = QuadrotorEnv(**_kw(obs, n))
    assert env.obs_dim == obs[2], (obs, env.obs_dim)
    return env


def _style(k):
    """the hidden activation and the output tanh of the k-th case: all four combinations in turn"""
    return ("tanh", "relu")[k % 2], (k // 2) % 2 == 0


def _obs_scale(env):
    """per input, max(1, RMS over the envs of a reset observation): folded into the first layer (as gym_art_amd.policy asks for
    observation normalisation) so that large inputs -- accelerations, angular rates -- do not saturate the first layer"""
    import torch
    o0 = torch.empty((env.num_envs, env.obs_dim), device=_dev())
    env.reset_dev(o0)
    torch.cuda.synchronize()
    x = o0.double().cpu().numpy()
    return np.maximum(1.0, np.sqrt((x * x).mean(axis=0)))


def _mlp(widths, D, seed, scale):
    layers = _scaled_layers(widths, D, seed)
    W, b = layers[0]
    return [((W / scale[None, :]).astype(np.float32), b)] + layers[1:]


def _runs(env, pol):
    """a 1-step rollout from reset, then a T-step one: [(the observations the actions were taken on [t, N, D], actions [t, N, 4],
    observations [t, N, D])]"""
    import torch
    out = []
    for steps in (1, T):
        o0, o, _, d, a = _closed_loop(env, pol, steps)
        if steps == T:
            assert int(d[:-1].sum()) > 0                     # auto-resets inside the window
        out.append((torch.cat([o0[None], o[:-1]]), a, o))
    return out


def _check_fp32(layers, act, out_tanh, prev, a, what, worst):
    hidden = []
    ref, z = forward64(layers, act, out_tanh, prev, hidden)
    assert_not_saturated(z, hidden, act, what)
    err = float((a.double() - ref).abs().max())
    worst[0] = max(worst[0], err)
    assert err <= ATOL_FP32, (what, err)


@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_fp32_engines_against_fp64(obs):
    """VALU (the per-step policy_kernel) and fp32 MFMA against forward64, and bit-equal to each other on every net both accept"""
    import torch
    from gym_art_amd.policy import MLPPolicy
    D, worst = obs[2], [0.0]
    for n in _batches(obs[1]):
        ev, em = _env(obs, n, fused=False), _env(obs, n)
        scale = _obs_scale(ev)
        _obs_scale(em)                                          # the same calls on both envs: the same resets
        for k, widths in enumerate(FP32_NETS + MFMA_NETS):
            act, out_tanh = _style(k + D)
            layers = _mlp(widths, D, 100 + k, scale)
            pm = MLPPolicy.from_arrays(em, layers, act, out_tanh, engine="mfma")
            runs = _runs(em, pm)
            for prev, a, _ in runs:
                _check_fp32(layers, act, out_tanh, prev, a, "mfma %s %s %d n=%d" % (widths, act, out_tanh, n), worst)
            if widths in FP32_NETS:                             # (these come first: ev and em see the same calls up to here)
                pv = MLPPolicy.from_arrays(ev, layers, act, out_tanh, engine="valu")
                for (_, a_m, o_m), (prev, a, o) in zip(runs, _runs(ev, pv)):
                    _check_fp32(layers, act, out_tanh, prev, a, "valu %s %s %d n=%d" % (widths, act, out_tanh, n), worst)
                    assert torch.equal(a, a_m) and torch.equal(o, o_m), ("mfma != valu", widths, n)
                pv.close()
            pm.close()
        ev.close(); em.close()
    print("fp32 engines d=%d: worst |a - forward64| %.3g" % (D, worst[0]))


@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_bf16_engine_against_its_contract(obs):
    """the bf16 engine against tests/policy_bf16_ref.py with test_gpu_policy_bf16's tolerances: every action within ATOL_ALL and, over
    all actions of this observation width, at least FRAC_MOST within ATOL_MOST"""
    import torch
    from gym_art_amd.policy import MLPPolicy
    D, errs = obs[2], []
    for n in _batches(obs[1]):
        env = _env(obs, n)
        scale = _obs_scale(env)
        for k, widths in enumerate(BF16_NETS):
            act, out_tanh = _style(k + D)
            layers = _mlp(widths, D, 200 + k, scale)
            if act == "relu":
                W, b = layers[0]
                layers[0] = ((RELU_BF16_SCALE * W).astype(np.float32), (RELU_BF16_SCALE * b).astype(np.float32))
            pol = MLPPolicy.from_arrays(env, layers, act, out_tanh, engine="bf16")
            for prev, a, _ in _runs(env, pol):
                x = prev.reshape(-1, D)
                hidden = []
                _, z = forward64(layers, act, out_tanh, x, hidden)
                what = "bf16 %s %s %d n=%d" % (widths, act, out_tanh, n)
                assert_not_saturated(z, hidden, act, what)
                err = (a.reshape(-1, 4).double() - bf16_forward(layers, act, out_tanh, x)).abs()
                assert float(err.max()) <= ATOL_ALL, (what, float(err.max()))
                errs.append(err.reshape(-1))
            pol.close()
        env.close()
    err = torch.cat(errs)
    frac = float((err <= ATOL_MOST).double().mean())
    print("bf16 d=%d: worst %.3g, within %.0e: %.5f of %d" % (D, float(err.max()), ATOL_MOST, frac, err.numel()))
    assert frac >= FRAC_MOST, frac


def _gru_policy(env, H, head, act, out_tanh, seed, scale):
    """a GRU cell whose gates stay off their tails (weights ~ 1 / sqrt(inputs), the observation scaled as in _mlp) and a _head"""
    from gym_art_amd.policy import GRUPolicy
    D = env.obs_dim
    W_ih, W_hh, b_ih, b_hh = _gru(H, D, seed, scale=1.0 / np.sqrt(D + H))
    gru = ((W_ih / scale[None, :]).astype(np.float32), W_hh, b_ih, b_hh)
    layers = _head(H, head, seed + 1)
    return GRUPolicy(env, gru, layers, act, out_tanh), gru, layers


def _gru_check(env, pol, gru, layers, act, out_tanh, what, worst):
    """a 1-step rollout from a random state, then a T-step one from zero; actions and final state against reference_rollout"""
    import torch
    n, H = env.num_envs, pol.hidden_size
    h0 = (0.5 * np.random.RandomState(n + H).randn(n, H)).astype(np.float32)
    for steps, h_init in ((1, h0), (T, None)):
        o0 = torch.empty((n, env.obs_dim), device=_dev())
        env.reset_dev(o0)
        o0 = o0.clone()
        if h_init is None:
            pol.reset_hidden()
        else:
            pol.set_hidden(h_init)
        o, r, d, a = _bufs(env, steps)
        env.rollout_policy_dev(pol, o, r, d, a)
        torch.cuda.synchronize()
        o0, o, d, a, h = (x.cpu().numpy() for x in (o0, o, d, a, pol.hidden))
        if steps == T:
            assert 0 < int(d[:-1].sum())
        ra, rh = reference_rollout(gru, layers, act, out_tanh, o0, o, d, np.zeros((n, H)) if h_init is None else h_init)
        # teeth: the gates of the first step, the head's sums
        W_ih, W_hh, b_ih, b_hh = (np.asarray(x, np.float64) for x in gru)
        hs = np.zeros((n, H)) if h_init is None else h_init.astype(np.float64)
        gi, gh = o0.astype(np.float64) @ W_ih.T + b_ih, hs @ W_hh.T + b_hh
        r_ = 1.0 / (1.0 + np.exp(-(gi[:, :H] + gh[:, :H])))
        gates = [gi[:, :2 * H] + gh[:, :2 * H], gi[:, 2 * H:] + r_ * gh[:, 2 * H:]]
        hidden = []
        _, z = forward64(layers, act, out_tanh, rh, hidden)
        assert_not_saturated(z, hidden, act, what)
        assert_not_saturated(z, gates, "tanh", what + " gates")
        err = max(float(np.max(np.abs(a - ra))), float(np.max(np.abs(h - rh))))
        worst[0] = max(worst[0], err)
        assert err <= ATOL_GRU, (what, steps, err)


@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_gru_engine_against_fp64(obs):
    """every H of 3, 5 and 15 chunks at this observation width, the heads in turn"""
    D, worst = obs[2], [0.0]
    for n in _batches(obs[1]):
        env = _env(obs, n)
        scale = _obs_scale(env)
        for j, H in enumerate(GRU_H):
            head = GRU_HEADS[(j + D) % 3]
            act, out_tanh = _style(j + D)
            pol, gru, layers = _gru_policy(env, H, head, act, out_tanh, 300 + j, scale)
            _gru_check(env, pol, gru, layers, act, out_tanh, "gru H=%d head=%s %s %d n=%d" % (H, head, act, out_tanh, n), worst)
            pol.close()
        env.close()
    print("gru d=%d: worst |a - ref|, |h - ref| %.3g" % (D, worst[0]))


@pytest.mark.parametrize("n", [16, 2096])
def test_gru_largest_lds_footprint(n):
    """H = 256 on a 16-agent swarm's 108 inputs: 1 KiB + 256 B x (108 + 256 + 256) = 156 KiB of LDS, the largest the engine accepts"""
    obs, worst = OBS[-1], [0.0]
    env = _env(obs, n)
    scale = _obs_scale(env)
    pol, gru, layers = _gru_policy(env, 256, (48,), "tanh", True, 400, scale)
    _gru_check(env, pol, gru, layers, "tanh", True, "gru H=256 d=108 n=%d" % n, worst)
    print("gru H=256 d=108 n=%d: worst %.3g" % (n, worst[0]))
    pol.close(); env.close()


def _launched(kind):
    from gym_art_amd import _lib
    buf = (C.c_uint32 * 64)()
    k = _lib.load().gaq_launched_variants(kind, buf, 64)
    return {int(buf[i]) for i in range(k)}


@pytest.mark.parametrize("n", [4, 64, 68])
def test_fused_valu_path_at_tiny_batches(n):
    """policy_rollout_kernel<F> (launch record kind 2) at one partial tile, one full tile and one tile + a sliver: actions against
    forward64, and its first actions bit-equal to the per-step fallback's"""
    import torch
    from gym_art_amd.policy import MLPPolicy
    obs, worst = OBS[2], [0.0]
    fused, fb = _env(obs, n), _env(obs, n, fused=False)
    scale = _obs_scale(fused)
    _obs_scale(fb)
    for k, widths in enumerate(FP32_NETS):
        act, out_tanh = _style(k)
        layers = _mlp(widths, 18, 500 + k, scale)
        pf = MLPPolicy.from_arrays(fused, layers, act, out_tanh)
        pb = MLPPolicy.from_arrays(fb, layers, act, out_tanh)
        assert pf.engine == pb.engine == "valu"
        for (prev, a, _), (_, a2, _) in zip(_runs(fused, pf), _runs(fb, pb)):
            _check_fp32(layers, act, out_tanh, prev, a, "fused %s %s %d n=%d" % (widths, act, out_tanh, n), worst)
            assert torch.equal(a[0], a2[0]), (widths, n)
        pf.close(); pb.close()
    assert _launched(2) & (set(range(16, 24)) | set(range(48, 56)))
    print("fused valu n=%d: worst |a - forward64| %.3g" % (n, worst[0]))
    fused.close(); fb.close()
