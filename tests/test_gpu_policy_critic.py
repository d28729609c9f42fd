"""A separate critic on the device (gaq.h gaq_critic, gaq_step_policy_critic_many_dev; gym_art_amd.policy.MLPCritic): values_dev against
fp64 at the kernel's edge shapes, a bit-level anchor against the value head of the existing engine, asking for a critic changes nothing
else, log-probabilities do not depend on where V comes from, rollout values / bootstrap row / terminal values are values_dev of the
recorded rows bit for bit (fused and two-launch forms alike), splitting, advantages, and the refusals.
Rollouts: T = 20 at ep_time=0.15 (episodes of 16 steps), so every env finishes inside the window; each test asserts that.
On an MI355X: 29 passed in 4.3 s.  Worst |V - V_ref| printed: values_dev 6.67e-7 (240-80 relu, D = 19), over
the rollouts 6.73e-7 (GRU actor + critic 48, N = 2096), both under 5 % of the bar ATOL_FP32 = 1.5e-5; advantages worst error / bar 0.040.
The kernels' edge shapes are tests/test_gpu_policy_critic_shapes.py's."""
import ctypes as C

import numpy as np
import pytest

from tests import ac_ref, term_ref
from tests.mlp_ref import assert_not_saturated, forward64
from tests.policy_util import _bufs, _dev, environ
from tests.test_gpu_policy_ac import BATCHES, LAYOUTS, LOG_STD, T, _ac_bufs, _env, _Net, _reset, _same
from tests.test_gpu_policy_shapes import ATOL_FP32, _mlp, _obs_scale
from tests.test_gpu_policy_term import REGIMES, _one_done_each, _start, _term_buf, _tv_buf, _zeros_are_plus_zero

pytestmark = pytest.mark.gpu

TRUNKS = [[16], [48], [240, 80], [256, 256, 256]]
ACTS = ["tanh", "relu"]
# (actor, critic trunk): the LDS of the fused launch is sized by the critic, by the actor, by both alike; then a GRU actor
PAIRS = [(("mlp", [16]), [256, 256]), (("mlp", [256, 256, 256]), [16]), (("mlp", [240, 80]), [240, 80]), (("gru", 48, (16, 80)), [48])]
PAIR_IDS = ["mlp16+c256x2", "mlp256x3+c16", "mlp240-80+c240-80", "gru48-16-80+c48"]
CASES = [(BATCHES[0], LAYOUTS[0]), (BATCHES[1], LAYOUTS[1]), (BATCHES[0], LAYOUTS[1]), (BATCHES[1], LAYOUTS[0])]   # N = 68 and 2096, alias and plain


class _CNet:
    """a critic trunk with its 1-output layer, buildable on several (twin) envs, and its fp64 reference"""

    def __init__(self, widths, scale, k, D=18, act=None):
        self.widths, self.act = list(widths), (ACTS[k % 2] if act is None else act)   # (act: a trunk whose activation is not its seed's)
        full = _mlp(widths, D, 800 + k, scale)
        self.hidden, self.out4 = full[:-1], full[-1]                # (the 4-output layer: the twin policy's; forward64 wants one)
        self.value = ac_ref.value_head(widths[-1], 950 + k)
        self.layers = self.hidden + [(self.value[0].reshape(1, -1), np.asarray([self.value[1]], np.float32))]

    def build(self, env, fused=True):
        from gym_art_amd.policy import MLPCritic
        if fused:
            return MLPCritic.from_arrays(env, self.layers, self.act)
        with environ(GAQ_NO_FUSED_CRITIC="1"):
            return MLPCritic.from_arrays(env, self.layers, self.act)

    def twin_policy(self, env, log_std=LOG_STD):
        """an "mfma" MLPPolicy of the same hidden layers, an arbitrary 4-output layer and the critic's last layer as its value head"""
        from gym_art_amd.policy import MLPPolicy
        return MLPPolicy.from_arrays(env, self.hidden + [self.out4], self.act, True, log_std=log_std, engine="mfma", value=self.value)

    def ref64(self, x, what=""):
        """V in float64: mlp_ref.forward64 on the hidden layers, then the output dot product"""
        hidden = []
        forward64(self.hidden + [self.out4], self.act, False, np.asarray(x, np.float64), hidden)
        assert_not_saturated(np.zeros(1), hidden, self.act, what)   # (the hidden layers: the critic has no output tanh to hide behind)
        y = np.tanh(hidden[-1]) if self.act == "tanh" else np.maximum(hidden[-1], 0.0)
        return y @ self.value[0].astype(np.float64) + np.float64(self.value[1])


def _window(env, pol, crit, regime="aligned", steps=T, term=True):
    """reset (and the staggered regime's prelude), then one window with everything asked for from the critic"""
    import torch
    o0 = _start(env, pol, regime)
    tt = _term_buf(env)
    env.set_terminal_obs(tt)
    o, r, d, a = _bufs(env, steps)
    v, lp = _ac_bufs(env, steps)
    tv = _tv_buf(env, steps) if term else None
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp, term_values=tv, critic=crit)
    torch.cuda.synchronize()
    return dict(o0=o0, o=o, r=r, d=d, a=a, v=v, lp=lp, tv=tv, tt=tt)


def _close(*xs):
    for x in xs:
        x.close()


# ---- 1. values_dev against fp64 -------------------------------------------------------------------------------------------------
_WORST = [0.0]


@pytest.mark.parametrize("D", [18, 19])
def test_values_dev_against_fp64(D):
    """single partial tiles, one full tile, a tile plus one row, two tiles plus two; D = 19 pads the first layer's last k-step with -0"""
    import torch
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(num_envs=8, ep_time=0.15, seed=7, obs_repr="xyz_vxyz_R_omega" if D == 18 else "xyz_vxyz_R_omega_h")
    assert env.obs_dim == D
    rng = np.random.RandomState(5)
    for k, (widths, act) in enumerate((w, a) for w in TRUNKS for a in ACTS):
        net = _CNet(widths, np.ones(D), 2 * k + ACTS.index(act), D)
        assert net.act == act
        crit = net.build(env)
        for M in (1, 63, 64, 65, 130):
            x = rng.randn(M, D).astype(np.float32)
            got = crit.values_dev(torch.from_numpy(x).to(_dev()))
            torch.cuda.synchronize()
            what = "critic %s %s D=%d M=%d" % (widths, act, D, M)
            ref = net.ref64(x, what)
            assert got.shape == (M,) and got.dtype == torch.float32
            assert float(np.mean(np.abs(ref) > ATOL_FP32)) > 0.9, what                  # teeth
            err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - ref)))
            _WORST[0] = max(_WORST[0], err)
            print("%s: worst |V - V_ref| %.3g (bar %.3g); so far %.3g" % (what, err, ATOL_FP32, _WORST[0]))
            assert err <= ATOL_FP32, (what, err)
        # [..., D] inputs, an `out` of the caller's, and no rows at all
        x = rng.randn(3, 5, D).astype(np.float32)
        xd = torch.from_numpy(x).to(_dev())
        out = torch.full((3, 5), float("nan"), device=_dev())
        assert crit.values_dev(xd, out=out) is out
        assert crit.values_dev(torch.empty((0, D), device=_dev())).shape == (0,)
        torch.cuda.synchronize()
        ref = net.ref64(x, "3x5")
        assert float(np.mean(np.abs(ref) > ATOL_FP32)) > 0.9
        assert float(np.max(np.abs(out.cpu().numpy().astype(np.float64) - ref))) <= ATOL_FP32
        assert torch.equal(out.reshape(-1), crit.values_dev(xd.reshape(15, D)))             # a row's V does not depend on its slot
        crit.close()
    env.close()


# ---- 2. bit anchor against the existing engine ----------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", TRUNKS, ids=["c16", "c48", "c240-80", "c256x3"])
def test_values_dev_is_the_value_head_of_an_mfma_policy_twin_bit_for_bit(widths):
    import torch
    for act_k in (0, 1):
        for n, layout in CASES[:2]:
            env = _env(n, layout)
            net = _CNet(widths, _obs_scale(env), 2 * TRUNKS.index(widths) + act_k)
            crit, twin = net.build(env), net.twin_policy(env)
            _, o0 = _reset(env, twin)
            o, r, d, a = _bufs(env, 1)
            v, _ = _ac_bufs(env, 1)
            env.rollout_policy_dev(twin, o, r, d, a, values=v)
            got = crit.values_dev(o0)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(v).all()) and float(v[0].abs().max()) > 0
            assert torch.equal(got, v[0]), (widths, net.act, n, layout)
            assert torch.equal(crit.values_dev(o[0]), v[1]), (widths, net.act, n, layout)      # the bootstrap row too
            _close(crit, twin, env)


# ---- 3. asking for a critic changes nothing else --------------------------------------------------------------------------------
@pytest.mark.parametrize("graph_safe", [False, True], ids=["eager", "graph_safe"])
@pytest.mark.parametrize("pair", [PAIRS[2], PAIRS[3]], ids=[PAIR_IDS[2], PAIR_IDS[3]])
def test_asking_for_a_critic_changes_nothing_else(pair, graph_safe):
    import torch
    spec, cw = pair
    k = PAIRS.index(pair)
    for n, layout in CASES:
        plain, asked = _env(n, layout, graph_safe), _env(n, layout, graph_safe)
        scale = _obs_scale(plain)
        _obs_scale(asked)                                           # the same calls on both envs
        net, cnet = _Net(spec, scale, k), _CNet(cw, scale, k)
        pp, pa = net.build(plain, value=False), net.build(asked, value=False)
        crit = cnet.build(asked)
        _reset(plain, pp)
        plain.set_terminal_obs(_term_buf(plain))                    # (as _window does on the other env)
        o, r, d, a = _bufs(plain, T)
        plain.rollout_policy_dev(pp, o, r, d, a)
        w = _window(asked, pa, crit)
        what = (pair, layout, graph_safe, n)
        _one_done_each(w["d"], what)
        assert torch.equal(o, w["o"]) and torch.equal(r, w["r"]) and torch.equal(d, w["d"]) and torch.equal(a, w["a"]), what
        assert bool(torch.isfinite(w["v"]).all()) and bool(torch.isfinite(w["lp"]).all()), what
        _zeros_are_plus_zero(w["tv"], w["d"], what)
        if net.kind == "gru":
            assert torch.equal(pp.hidden, pa.hidden), what
        assert _same(plain.state_dict(), asked.state_dict()), what
        # ... and nothing later either: the next plain call of both gives the same bits
        o2, r2, d2, a2 = _bufs(asked, T)
        plain.rollout_policy_dev(pp, o, r, d, a)
        asked.rollout_policy_dev(pa, o2, r2, d2, a2)
        torch.cuda.synchronize()
        assert torch.equal(o, o2) and torch.equal(a, a2) and torch.equal(d, d2) and torch.equal(r, r2), what
        _close(pp, pa, crit, plain, asked)


# ---- 4. logp does not depend on where V comes from ------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_logp_with_a_critic_is_logp_of_the_value_head_call(pair):
    import torch
    spec, cw = pair
    k = PAIRS.index(pair)
    for n, layout in CASES[:2]:
        env, twin = _env(n, layout), _env(n, layout)
        scale = _obs_scale(env)
        _obs_scale(twin)
        net, cnet = _Net(spec, scale, k), _CNet(cw, scale, k)
        pol, pt = net.build(env, value=False), net.build(twin, value=True)
        crit = cnet.build(env)
        w = _window(env, pol, crit)
        _reset(twin, pt)
        twin.set_terminal_obs(_term_buf(twin))                      # (as _window does on the other env)
        o, r, d, a = _bufs(twin, T)
        v, lp = _ac_bufs(twin, T)
        twin.rollout_policy_dev(pt, o, r, d, a, values=v, logp=lp)
        torch.cuda.synchronize()
        what = (pair, n, layout)
        _one_done_each(w["d"], what)
        assert bool(torch.isfinite(lp).all()) and torch.equal(lp, w["lp"]), what
        assert torch.equal(a, w["a"]) and torch.equal(o, w["o"]), what
        assert not torch.equal(v, w["v"]), what                     # (two different value functions)
        _close(pol, pt, crit, env, twin)


# ---- 5. rollout values: fused, two-launch and standalone agree ------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_rollout_values_are_values_dev_of_the_recorded_rows(pair):
    import torch
    spec, cw = pair
    k = PAIRS.index(pair)
    for n, layout in CASES[:2] if k % 2 == 0 else CASES[2:]:
        runs = []
        for fused in (True, False):
            env = _env(n, layout)
            scale = _obs_scale(env)
            net, cnet = _Net(spec, scale, k), _CNet(cw, scale, k)
            pol, crit = net.build(env, value=False), cnet.build(env, fused)
            w = _window(env, pol, crit)
            what = (pair, n, layout, "fused" if fused else "two launches")
            _one_done_each(w["d"], what)
            rows = torch.cat([w["o0"][None], w["o"]])               # row t: what action t (and value t) saw; row T: where the call ends
            alone = crit.values_dev(rows)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(w["v"]).all()), what
            assert torch.equal(w["v"], alone), what
            assert torch.equal(w["v"][T], crit.values_dev(w["o"][T - 1])), what
            ref = cnet.ref64(rows.cpu().numpy(), str(what))
            assert float(np.mean(np.abs(ref) > ATOL_FP32)) > 0.9, what
            err = float(np.max(np.abs(w["v"].cpu().numpy().astype(np.float64) - ref)))
            print("%s: worst |V - V_ref| over the rollout %.3g (bar %.3g)" % (what, err, ATOL_FP32))
            assert err <= ATOL_FP32, (what, err)
            runs.append(w)
            _close(pol, crit, env)
        for key in ("o", "r", "d", "a", "v", "lp", "tv"):
            assert torch.equal(runs[0][key], runs[1][key]), (pair, n, layout, key)


# ---- 6. splitting the rollout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[3]], ids=[PAIR_IDS[0], PAIR_IDS[3]])
def test_splitting_the_rollout_changes_nothing(pair):
    import torch
    spec, cw = pair
    k = PAIRS.index(pair)
    for n, layout in CASES[:2]:
        whole = _env(n, layout)
        scale = _obs_scale(whole)
        net, cnet = _Net(spec, scale, k), _CNet(cw, scale, k)
        pw, cwh = net.build(whole, value=False), cnet.build(whole)
        w = _window(whole, pw, cwh)
        what = (pair, n, layout)
        at = _one_done_each(w["d"], what)
        first_done = int(at.min())
        assert first_done + 1 < T
        for h in (T // 2, first_done + 1):
            split = _env(n, layout)
            _obs_scale(split)                                       # the same calls as on `whole`
            ps, cs = net.build(split, value=False), cnet.build(split)
            _start(split, ps, "aligned")
            split.set_terminal_obs(_term_buf(split))
            o2, r2, d2, a2 = _bufs(split, T)
            va, lpa = _ac_bufs(split, h)
            vb, lpb = _ac_bufs(split, T - h)
            tv2 = _tv_buf(split)
            split.rollout_policy_dev(ps, o2[:h], r2[:h], d2[:h], a2[:h], values=va, logp=lpa, term_values=tv2[:h], critic=cs)
            split.rollout_policy_dev(ps, o2[h:], r2[h:], d2[h:], a2[h:], values=vb, logp=lpb, term_values=tv2[h:], critic=cs)
            torch.cuda.synchronize()
            assert torch.equal(w["o"], o2) and torch.equal(w["r"], r2) and torch.equal(w["d"], d2) and torch.equal(w["a"], a2), (what, h)
            assert torch.equal(w["lp"], torch.cat([lpa, lpb])) and torch.equal(w["tv"], tv2), (what, h)
            assert torch.equal(w["v"][:h + 1], va) and torch.equal(w["v"][h:], vb), (what, h)
            assert torch.equal(va[h], vb[0]), (what, h)             # row T of the first call IS row 0 of the second
            if net.kind == "gru":
                assert torch.equal(pw.hidden, ps.hidden), (what, h)
            _close(ps, cs, split)
        _close(pw, cwh, whole)


# ---- 7. terminal values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("pair", [PAIRS[1], PAIRS[2], PAIRS[3]], ids=PAIR_IDS[1:])
def test_terminal_values_are_values_dev_of_the_terminal_rows(pair, regime):
    """each env reports exactly one done in the window, so the registered terminal tensor ends up holding each env's one terminal row"""
    import torch
    spec, cw = pair
    k = PAIRS.index(pair)
    for n, layout in CASES[:2] if regime == "aligned" else CASES[2:]:
        runs = []
        for rep in range(2):                                        # twice: the order of the gathered list is free, the values are not
            env = _env(n, layout)
            scale = _obs_scale(env)
            net, cnet = _Net(spec, scale, k), _CNet(cw, scale, k)
            pol, crit = net.build(env, value=False), cnet.build(env)
            w = _window(env, pol, crit, regime)
            what = (pair, regime, n, layout, rep)
            at = _one_done_each(w["d"], what)
            if regime == "staggered":
                assert sorted(set(at.cpu().tolist())) == [10, 15], what
            _zeros_are_plus_zero(w["tv"], w["d"], what)
            assert bool(torch.isfinite(w["tt"]).all()), what        # every env's terminal row was captured
            got = w["tv"][at, torch.arange(n, device=_dev())]
            assert torch.equal(got, crit.values_dev(w["tt"])), what
            # teeth: the terminal row is not the row the rollout went on with, and its value is not the next value
            nxt = w["o"][at, torch.arange(n, device=_dev())]
            assert float(((nxt - w["tt"]).abs().max(dim=1).values > 1e-3).float().mean()) > 0.9, what
            assert float((got != w["v"][at + 1, torch.arange(n, device=_dev())]).float().mean()) > 0.9, what
            runs.append(w)
            _close(pol, crit, env)
        for key in ("o", "d", "a", "v", "lp", "tv", "tt"):
            assert torch.equal(runs[0][key], runs[1][key]), (pair, regime, n, layout, key)


# ---- 8. GAE end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [PAIRS[2], PAIRS[3]], ids=[PAIR_IDS[2], PAIR_IDS[3]])
def test_gae_with_the_critics_values_against_fp64(pair):
    import torch
    spec, cw = pair
    k = PAIRS.index(pair)
    gamma, lam = 0.99, 0.95
    env = _env(2096, "alias")
    scale = _obs_scale(env)
    net, cnet = _Net(spec, scale, k), _CNet(cw, scale, k)
    pol, crit = net.build(env, value=False), cnet.build(env)
    w = _window(env, pol, crit, "staggered")
    _one_done_each(w["d"], pair)
    adv, ret = torch.full_like(w["r"], float("nan")), torch.full_like(w["r"], float("nan"))
    env.gae_dev(w["r"], w["d"], w["v"], gamma, lam, adv, ret, term_values=w["tv"])
    torch.cuda.synchronize()
    rn, dn, vn, tn = (w[key].cpu().numpy() for key in ("r", "d", "v", "tv"))
    aref, _ = term_ref.gae_term64(rn, dn, vn, tn, gamma, lam)
    bar = term_ref.gae_term_bar(rn, dn, vn, tn, aref, gamma, lam)
    err = np.abs(adv.cpu().numpy().astype(np.float64) - aref)
    print("%s: gae worst error %.3g, worst error / bar %.3g" % (pair, float(err.max()), float((err / bar[None]).max())))
    assert (err <= bar[None]).all(), float((err / bar[None]).max())
    assert float(np.abs(aref).max()) > 100 * float(bar.max())       # teeth
    assert float(np.mean(np.abs(tn[dn != 0]) > 100 * float(bar.max()))) > 0.9        # ... and the terminal values are in it
    assert bool(torch.isfinite(ret).all())
    _close(pol, crit, env)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_everything_usable():
    import torch
    from gym_art_amd import QuadrotorEnv, _lib
    from gym_art_amd.policy import MLPCritic, MLPPolicy, _CriticDesc
    n, steps = 68, 4
    env, twin = _env(n, "alias"), _env(n, "alias")
    scale = _obs_scale(env)
    _obs_scale(twin)
    net, cnet = _Net(("mlp", [48]), scale, 0), _CNet([48], scale, 0)
    pol, pt = net.build(env, value=False), net.build(twin, value=False)
    crit, ct = cnet.build(env), cnet.build(twin)
    _reset(env, pol); _reset(twin, pt)
    o, r, d, a = _bufs(env, steps)
    v, lp = _ac_bufs(env, steps)
    tv = _tv_buf(env, steps)
    bufs2 = _bufs(twin, steps) + _ac_bufs(twin, steps) + (_tv_buf(twin, steps),)

    def usable(p=pol, ptwin=pt, logp=True):
        """a good call with the critic on the refused env and on the twin that was never refused: the same bits"""
        o2, r2, d2, a2, v2, lp2, tv2 = bufs2
        for x in (v, lp, tv, v2, lp2, tv2):
            x.fill_(float("nan"))
        env.rollout_policy_dev(p, o, r, d, a, values=v, logp=lp if logp else None, term_values=tv, critic=crit)
        twin.rollout_policy_dev(ptwin, o2, r2, d2, a2, values=v2, logp=lp2 if logp else None, term_values=tv2, critic=ct)
        torch.cuda.synchronize()
        assert torch.equal(o, o2) and torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(d, d2)
        assert bool(torch.isfinite(v).all()) and torch.equal(v, v2) and torch.equal(tv, tv2)
        if logp:
            assert bool(torch.isfinite(lp).all()) and torch.equal(lp, lp2)
        assert _same(env.state_dict(), twin.state_dict())

    usable()
    # a policy with a value head, and a critic: which of the two is meant?
    pol.set_value_head(*net.value)
    with pytest.raises(_lib.GaqError, match="value head and a critic.*remove one"):       # GAQ_ERR_STATE
        env.rollout_policy_dev(pol, o, r, d, a, values=v, critic=crit)
    with pytest.raises(_lib.GaqError, match="remove one"):
        env.rollout_policy_dev(pol, o, r, d, a, critic=crit)
    pol.set_value_head(None)
    usable()
    # engines without an actor-critic form: today's texts
    small = _mlp([48], 18, 1, scale)
    for engine in ("valu", "bf16"):
        p2 = MLPPolicy.from_arrays(env, small, "tanh", True, log_std=LOG_STD, engine=engine)
        with pytest.raises(ValueError, match=r"values and log-probabilities are not computed by the %s engine \(fp32 MFMA and GRU policies only\)"
                           % ("VALU" if engine == "valu" else "bf16")):
            env.rollout_policy_dev(p2, o, r, d, a, values=v, critic=crit)
        with pytest.raises(ValueError, match="VALU" if engine == "valu" else "bf16"):
            env.rollout_policy_dev(p2, o, r, d, a, critic=crit)
        p2.close()
    usable()
    # a critic built for another env: refused by the Python layer and by the library
    with pytest.raises(ValueError, match="critic was built for another env"):
        env.rollout_policy_dev(pol, o, r, d, a, values=v, critic=ct)
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gaq_step_policy_critic_many_dev(env._handle, pol.handle, ct.handle, steps, _lib.ptr(o), _lib.ptr(r), _lib.ptr(d), _lib.ptr(a),
                                               _lib.ptr(v), None, None, st) == -1
    assert b"critic: created for another env" in lib.gaq_last_error()
    usable()
    # logp on a deterministic policy
    pol.set_log_std(None); pt.set_log_std(None)
    with pytest.raises(_lib.GaqError, match="deterministic"):       # GAQ_ERR_STATE
        env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp, critic=crit)
    usable(logp=False)
    pol.set_log_std(LOG_STD); pt.set_log_std(LOG_STD)
    # misaligned outputs; Python-side shape checks
    off = torch.empty((steps + 1) * n + 1, device=_dev())[1:].view(steps + 1, n)      # contiguous, 4 bytes off a 16-byte boundary
    with pytest.raises(ValueError, match="aligned"):                # GAQ_ERR_INVALID
        env.rollout_policy_dev(pol, o, r, d, a, values=off, critic=crit)
    with pytest.raises(ValueError, match="values must be"):
        env.rollout_policy_dev(pol, o, r, d, a, values=v[:-1], critic=crit)
    with pytest.raises(ValueError, match="term_values must be"):
        env.rollout_policy_dev(pol, o, r, d, a, values=v, term_values=v, critic=crit)
    usable()
    # values_dev: the wrong last dimension, dtype, layout, device, a wrong `out`
    good = torch.zeros((5, 18), device=_dev())
    for bad in (torch.zeros((5, 19), device=_dev()), torch.zeros((5, 17), device=_dev()), good.double(), good.t().contiguous().t(),
                torch.zeros((), device=_dev())):
        with pytest.raises(ValueError, match=r"obs must be a contiguous float32 tensor of shape \[\.\.\., 18\], got"):
            crit.values_dev(bad)
    with pytest.raises(ValueError, match="on the critic's device"):
        crit.values_dev(good.cpu())
    with pytest.raises(ValueError, match=r"out must be .*\(5,\)"):
        crit.values_dev(good, out=torch.zeros((4,), device=_dev()))
    with pytest.raises(ValueError, match="4-byte aligned"):         # the library's own check (a byte offset no tensor can have)
        _lib.check(lib.gaq_critic_eval_dev(crit.handle, 5, C.c_void_p(good.data_ptr() + 1), _lib.ptr(torch.zeros(5, device=_dev())), st))
    with pytest.raises(ValueError, match="rows"):
        _lib.check(lib.gaq_critic_eval_dev(crit.handle, -1, _lib.ptr(good), _lib.ptr(torch.zeros(5, device=_dev())), st))
    assert crit.values_dev(good).shape == (5,)
    usable()
    # a critic whose in_dim is not the env's: nothing is created
    dsc = _CriticDesc()
    dsc.struct_size, dsc.in_dim, dsc.n_hidden, dsc.hidden_act = C.sizeof(_CriticDesc), 19, 1, 0
    dsc.width[0] = 48
    h = C.c_void_p(1)
    assert lib.gaq_critic_create(env._handle, C.byref(dsc), C.byref(h)) == -1 and h.value is None
    assert b"in_dim" in lib.gaq_last_error()
    with pytest.raises(ValueError, match="takes 19 inputs, expected 18"):
        MLPCritic.from_arrays(env, _CNet([48], np.ones(19), 0, 19).layers, "tanh")
    # set_weights: another architecture is refused, the same one replaces the weights
    with pytest.raises(ValueError, match=r"hidden widths \[64\], the critic was built with \[48\]"):
        crit.set_weights(_CNet([64], scale, 0).layers)
    other = _CNet([48], scale, 3)
    before = crit.values_dev(good + 1.0).clone()
    crit.set_weights(other.layers)
    assert not torch.equal(before, crit.values_dev(good + 1.0))
    crit.set_weights(cnet.layers)
    assert torch.equal(before, crit.values_dev(good + 1.0))
    usable()
    # term_values on a handle without auto-reset
    noreset = QuadrotorEnv(num_envs=n, ep_time=0.15, seed=7, init_random_state=True, auto_reset=False, alias_obs=True)
    _obs_scale(noreset)
    pn, cn = net.build(noreset, value=False), cnet.build(noreset)
    _reset(noreset, pn)
    o3, r3, d3, a3 = _bufs(noreset, steps)
    v3, _ = _ac_bufs(noreset, steps)
    with pytest.raises(_lib.GaqError, match=r"auto_reset = 0"):     # GAQ_ERR_STATE
        noreset.rollout_policy_dev(pn, o3, r3, d3, a3, values=v3, term_values=tv, critic=cn)
    noreset.rollout_policy_dev(pn, o3, r3, d3, a3, values=v3, critic=cn)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v3).all())
    _close(pn, cn, noreset, pol, pt, crit, ct, env, twin)
