"""Time-limit bootstrapping on the device (gaq.h gaq_step_policy_ac_term_many_dev, gaq_gae_term_dev): asking for terminal values changes
nothing else, the values against fp64 references fed the device's recorded terminal rows, a bit-level anchor against a twin without
auto-reset, splitting / repeating / a stale terminal buffer, the library's own terminal scratch, the advantages, and the refusals.
Nets, batches, layouts and helpers are those of tests/test_gpu_policy_ac.py.  ep_time=0.15 gives episodes of 16 steps (done = tick > 15).
Two regimes: "aligned" -- reset, then the T = 20 window: every env finishes in step 15; "staggered" -- 5 steps, a masked reset of a fixed
pseudo-random half (and of its hidden rows), then the window: the half that went on finishes in step 10, the other in step 15, in most
tiles side by side.  Every test asserts that EVERY env reports exactly one done inside the window."""
import numpy as np
import pytest

from tests import ac_ref, term_ref
from tests.policy_util import _bufs, _dev
from tests.test_gpu_policy_ac import BATCHES, LAYOUTS, LOG_STD, NET_IDS, NETS, T, _ac_bufs, _env, _Net, _reset, _same
from tests.test_gpu_policy_shapes import _mlp, _obs_scale

pytestmark = pytest.mark.gpu

REGIMES = ["aligned", "staggered"]


def _start(env, pol, regime, mask=None):
    """bring env and policy to the start of the window; returns a copy of the observation the first action will see.  mask: the envs
    (a bool array) the staggered regime resets instead of its pseudo-random half"""
    import torch
    _, o0 = _reset(env, pol)
    if regime == "aligned":
        return o0
    o, r, d, a = _bufs(env, 5)
    env.rollout_policy_dev(pol, o, r, d, a)
    half = torch.from_numpy(np.random.RandomState(11).rand(env.num_envs) < 0.5 if mask is None else mask).to(_dev(), torch.uint8)
    cur = o[4].clone()                                              # the rows of the envs that go on keep the current observation
    env.reset_dev(cur, half)
    if hasattr(pol, "reset_hidden"):
        pol.reset_hidden(half)
    torch.cuda.synchronize()
    assert int(d.sum()) == 0
    return cur.clone()


def _term_buf(env, fill=float("nan")):
    import torch
    return torch.full((env.num_envs, env.obs_dim), fill, device=_dev())


def _tv_buf(env, steps=T):
    import torch
    return torch.full((steps, env.num_envs), float("nan"), device=_dev())


def _one_done_each(d, what):
    """the condition every test stands on: each env reports exactly one done inside the window; returns the step of each"""
    import torch
    per_env = d.to(torch.int32).sum(dim=0)
    assert bool((per_env == 1).all()), (what, int(per_env.min()), int(per_env.max()))
    return torch.argmax(d.to(torch.int32), dim=0)


def _zeros_are_plus_zero(tv, d, what):
    """where done is clear the entry is +0.0: all 32 bits clear (the buffer was pre-filled with NaN)"""
    import torch
    bits = tv.view(torch.int32)
    assert bool((bits[d == 0] == 0).all()), what
    assert bool(torch.isfinite(tv).all()), what


def _window(env, pol, regime, term=True, tt="nan", mask=None):
    """one window with everything asked for; returns a dict of the tensors"""
    import torch
    o0 = _start(env, pol, regime, mask)
    h0 = pol.hidden.clone() if hasattr(pol, "hidden") else None
    term_rows = None
    if tt is not None:
        term_rows = _term_buf(env)
        env.set_terminal_obs(term_rows)
    o, r, d, a = _bufs(env, T)
    v, lp = _ac_bufs(env, T)
    tv = _tv_buf(env) if term else None
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp, term_values=tv)
    torch.cuda.synchronize()
    return dict(o0=o0, h0=h0, o=o, r=r, d=d, a=a, v=v, lp=lp, tv=tv, tt=term_rows)


# ---- 1. asking for terminal values changes nothing else ----------------------------------------------------------------------
@pytest.mark.parametrize("graph_safe", [False, True], ids=["eager", "graph_safe"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("spec", NETS, ids=NET_IDS)
def test_asking_for_terminal_values_changes_nothing_else(spec, layout, graph_safe):
    import torch
    k = NETS.index(spec)
    for n, regime in zip(BATCHES + BATCHES, ["aligned", "staggered", "staggered", "aligned"]):
        plain, asked = _env(n, layout, graph_safe), _env(n, layout, graph_safe)
        net = _Net(spec, _obs_scale(plain), k)
        _obs_scale(asked)                                           # the same calls on both envs
        pp, pa = net.build(plain), net.build(asked)
        w1, w2 = _window(plain, pp, regime, term=False), _window(asked, pa, regime, term=True)
        what = (spec, layout, graph_safe, n, regime)
        _one_done_each(w2["d"], what)
        for key in ("o", "r", "d", "a", "v", "lp", "tt"):
            assert torch.equal(w1[key], w2[key]), (what, key)       # (v, lp, tt: no NaN left in them, so equal means bit-equal)
        assert bool(torch.isfinite(w2["tt"]).all()), what           # every env's terminal row was captured
        _zeros_are_plus_zero(w2["tv"], w2["d"], what)
        if net.kind == "gru":
            assert torch.equal(pp.hidden, pa.hidden), what
        assert _same(plain.state_dict(), asked.state_dict()), what
        # ... and nothing later: the caller's terminal tensor is still registered (the next window refills it from NaN) and the next
        # plain call of both gives the same bits
        for w in (w1, w2):
            w["tt"].fill_(float("nan"))
        plain.rollout_policy_dev(pp, w1["o"], w1["r"], w1["d"], w1["a"])
        asked.rollout_policy_dev(pa, w2["o"], w2["r"], w2["d"], w2["a"])
        torch.cuda.synchronize()
        _one_done_each(w2["d"], what)                               # 16-step episodes: each env finishes once in the next 20 steps too
        assert bool(torch.isfinite(w2["tt"]).all()) and torch.equal(w1["tt"], w2["tt"]), what
        for key in ("o", "r", "d", "a"):
            assert torch.equal(w1[key], w2[key]), (what, key)
        for x in (pp, pa, plain, asked):
            x.close()


# ---- 2. terminal values against fp64 ------------------------------------------------------------------------------------------
_WORST = {"mlp": 0.0, "gru": 0.0}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("spec", NETS, ids=NET_IDS)
def test_terminal_values_against_fp64(spec, layout, regime):
    """term_values[t_i, i] within the engine's bar (ATOL_FP32 / ATOL_GRU, as the value tests use them) of V64 of env i's terminal row --
    for a GRU with h_t from the fp64 recurrence on the recorded observations and dones -- and exactly +0.0 everywhere else"""
    k = NETS.index(spec)
    for n in BATCHES:
        env = _env(n, layout)
        net = _Net(spec, _obs_scale(env), k)
        pol = net.build(env)
        w = _window(env, pol, regime)
        what = "%s %s %s n=%d" % (spec, layout, regime, n)
        at = _one_done_each(w["d"], what)
        if regime == "staggered":
            assert sorted(set(at.cpu().tolist())) == [10, 15], what
        _zeros_are_plus_zero(w["tv"], w["d"], what)
        rows = w["tt"].cpu().numpy()
        assert np.isfinite(rows).all(), what                        # each env's one terminal row
        atn = at.cpu().numpy()
        got = w["tv"].cpu().numpy()[atn, np.arange(n)].astype(np.float64)
        if net.kind == "mlp":
            ref = term_ref.mlp_term_values64(net, rows)
        else:
            ref = term_ref.gru_term_values64(net, w["o0"].cpu().numpy(), w["o"].cpu().numpy(), w["d"].cpu().numpy(),
                                             w["h0"].cpu().numpy().astype(np.float64), atn, rows)
        assert np.isfinite(ref).all(), what
        assert float(np.mean(np.abs(ref) > net.atol)) > 0.9, what   # teeth: the values are not all within the bar of zero
        # teeth: the terminal row is not the row the rollout went on with (the new episode's first observation)
        nxt = w["o"].cpu().numpy()[atn, np.arange(n)]
        assert float(np.mean(np.abs(nxt - rows).max(axis=1) > 1e-3)) > 0.9, what
        err = float(np.max(np.abs(got - ref)))
        _WORST[net.kind] = max(_WORST[net.kind], err)
        print("%s: worst |V_term - V_ref| %.3g (bar %.3g); %s so far: %.3g" % (what, err, net.atol, net.kind, _WORST[net.kind]))
        assert err <= net.atol, (what, err)
        pol.close(); env.close()


# ---- 3. bit-level anchor: a twin without auto-reset -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["plain"])
@pytest.mark.parametrize("spec", NETS[:3], ids=NET_IDS[:3])
def test_terminal_value_is_the_next_value_of_a_twin_without_auto_reset(spec, layout):
    """aligned regime, MLP: the twin (auto_reset=False, same seed and policy) does not start a new episode in the done step, so the
    observation it returns there IS the terminal observation and its values[t + 1] is V of it, from the full-batch kernel.
    Plain layout only.  In the alias layout the twin reproduces the trajectory too, but the row it returns is the fp64 state's fp32
    HEAD (the step kernel's heads18 split, whose residual the state keeps) while the terminal row is the packed observation (the
    state cast to fp32): the two rows are not the same bits there (measured on an MI355X: the twin's row != the captured row for all
    three nets at N = 68), so no bit-level anchor exists in that layout and test_terminal_values_against_fp64 is its anchor."""
    import torch
    from gym_art_amd import QuadrotorEnv
    k = NETS.index(spec)
    for n in BATCHES:
        env = _env(n, layout)
        twin = QuadrotorEnv(num_envs=n, ep_time=0.15, seed=7, init_random_state=True, auto_reset=False, alias_obs=layout == "alias")
        net = _Net(spec, _obs_scale(env), k)
        _obs_scale(twin)
        pol, pt = net.build(env), net.build(twin)
        w = _window(env, pol, "aligned")
        what = (spec, layout, n)
        at = _one_done_each(w["d"], what)
        t_done = int(at[0])
        assert bool((at == t_done).all()) and t_done == 15, what
        _reset(twin, pt)
        steps = t_done + 1
        o, r, d, a = _bufs(twin, steps)
        v, lp = _ac_bufs(twin, steps)
        twin.rollout_policy_dev(pt, o, r, d, a, values=v, logp=lp)
        torch.cuda.synchronize()
        # the twin reproduces the trajectory up to the done step, and the row it returns there is the captured terminal row
        assert torch.equal(o[:t_done], w["o"][:t_done]) and torch.equal(a, w["a"][:steps]) and torch.equal(d, w["d"][:steps]), what
        assert torch.equal(r, w["r"][:steps]) and torch.equal(v[:steps], w["v"][:steps]), what
        assert torch.equal(o[t_done], w["tt"]), what
        assert torch.equal(v[steps], w["tv"][t_done]), what
        assert not torch.equal(v[steps], w["v"][steps]), what       # (the first env's next value is the new episode's)
        for x in (pol, pt, env, twin):
            x.close()


# ---- 4. split, repeat, a stale buffer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("spec", NETS, ids=NET_IDS)
def test_splitting_repeating_and_a_stale_terminal_buffer_change_nothing(spec, layout):
    """staggered regime.  The window in one call, against: the same again (the order in which the gather's atomics hand out the slots is
    free, the values are not), two calls split at T / 2 = the first done step, and two split right after it -- each with a terminal
    tensor that holds NaN in every row when its first call starts."""
    import torch
    k = NETS.index(spec)
    for n in BATCHES:
        whole = _env(n, layout)
        net = _Net(spec, _obs_scale(whole), k)
        pw = net.build(whole)
        w = _window(whole, pw, "staggered")
        what = (spec, layout, n)
        at = _one_done_each(w["d"], what)
        first_done = int(at.min())
        assert first_done == T // 2 and int(at.max()) == 15, what
        _zeros_are_plus_zero(w["tv"], w["d"], what)
        for h in (None, T // 2, first_done + 1):
            other = _env(n, layout)
            _obs_scale(other)                                       # the same calls as on `whole`
            po = net.build(other)
            if h is None:
                w2 = _window(other, po, "staggered")
                tv2, v2 = w2["tv"], w2["v"]
                o2, d2 = w2["o"], w2["d"]
            else:
                _start(other, po, "staggered")
                tt = _term_buf(other)
                other.set_terminal_obs(tt)
                o2, r2, d2, a2 = _bufs(other, T)
                va, lpa = _ac_bufs(other, h)
                vb, lpb = _ac_bufs(other, T - h)
                tv2 = _tv_buf(other)
                other.rollout_policy_dev(po, o2[:h], r2[:h], d2[:h], a2[:h], values=va, logp=lpa, term_values=tv2[:h])
                other.rollout_policy_dev(po, o2[h:], r2[h:], d2[h:], a2[h:], values=vb, logp=lpb, term_values=tv2[h:])
                torch.cuda.synchronize()
                v2 = torch.cat([va[:h], vb])
            assert torch.equal(o2, w["o"]) and torch.equal(d2, w["d"]) and torch.equal(v2, w["v"]), (what, h)
            assert torch.equal(tv2, w["tv"]), (what, h)             # finite everywhere (checked above): equal means bit-equal
            if net.kind == "gru":
                assert torch.equal(pw.hidden, po.hidden), (what, h)
            po.close(); other.close()
        pw.close(); whole.close()


# ---- 5. the library's own terminal scratch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [NETS[1], NETS[4]], ids=["mlp240-80", "gru48-16-80"])
def test_without_a_registered_terminal_tensor_the_library_uses_its_own(spec):
    import torch
    k = NETS.index(spec)
    for n, layout in zip(BATCHES, LAYOUTS):
        reg, own = _env(n, layout), _env(n, layout)
        net = _Net(spec, _obs_scale(reg), k)
        _obs_scale(own)
        pr, po = net.build(reg), net.build(own)
        w1 = _window(reg, pr, "staggered")
        # `own` has had a tensor registered and unregistered: the call must neither need it nor bring it back
        old = _term_buf(own)
        own.set_terminal_obs(old)
        own.set_terminal_obs(None)
        w2 = _window(own, po, "staggered", tt=None)
        what = (spec, layout, n)
        _one_done_each(w2["d"], what)
        for key in ("o", "r", "d", "a", "v", "lp", "tv"):
            assert torch.equal(w1[key], w2[key]), (what, key)
        assert bool(torch.isnan(old).all()), what
        # a second window on the library's scratch (allocated once, reused), still equal to the registered twin's
        o, r, d, a = _bufs(reg, T)
        o2, r2, d2, a2 = _bufs(own, T)
        tv, tv2 = _tv_buf(reg), _tv_buf(own)
        reg.rollout_policy_dev(pr, o, r, d, a, term_values=tv)      # (no values, no logp: the plain policy launches + the terminal pass)
        own.rollout_policy_dev(po, o2, r2, d2, a2, term_values=tv2)
        torch.cuda.synchronize()
        _one_done_each(d2, what)
        assert torch.equal(o, o2) and torch.equal(a, a2) and torch.equal(d, d2) and torch.equal(tv, tv2), what
        _zeros_are_plus_zero(tv2, d2, what)
        assert bool(torch.isnan(old).all()), what                   # never written: the env is unregistered as before
        assert _same(reg.state_dict(), own.state_dict()), what
        for x in (pr, po, reg, own):
            x.close()


# ---- 6. advantages ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.99, 0.0), (0.99, 1.0), (1.0, 0.95), (1.0, 1.0)])
def test_gae_with_terminal_values_against_fp64(gamma, lam):
    import ctypes as C
    import torch
    from gym_art_amd import _lib
    n, steps = 2096, 64
    env = _env(n, "alias")
    net = _Net(NETS[0], _obs_scale(env), 0)
    pol = net.build(env)
    _reset(env, pol)
    o, r, d, a = _bufs(env, steps)
    v, lp = _ac_bufs(env, steps)
    tv = _tv_buf(env, steps)
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp, term_values=tv)
    adv, ret = torch.full_like(r, float("nan")), torch.full_like(r, float("nan"))
    env.gae_dev(r, d, v, gamma, lam, adv, ret, term_values=tv)
    adv_only = torch.full_like(r, float("nan"))
    env.gae_dev(r, d, v, gamma, lam, adv_only, term_values=tv)
    plain, none, null = torch.full_like(r, float("nan")), torch.full_like(r, float("nan")), torch.full_like(r, float("nan"))
    env.gae_dev(r, d, v, gamma, lam, plain)
    env.gae_dev(r, d, v, gamma, lam, none, term_values=None)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().gaq_gae_term_dev(env._handle, steps, _lib.ptr(r), _lib.ptr(d), _lib.ptr(v), None, gamma, lam, _lib.ptr(null), None, st))
    torch.cuda.synchronize()
    assert bool((d.to(torch.int32).sum(dim=0) == 4).all())          # every env: dones at steps 15, 31, 47 and 63
    assert torch.equal(adv, adv_only)
    assert torch.equal(plain, none) and torch.equal(plain, null)    # without terminal values: gaq_gae_dev's bits
    rn, dn, vn, tn = r.cpu().numpy(), d.cpu().numpy(), v.cpu().numpy(), tv.cpu().numpy()
    aref, _ = term_ref.gae_term64(rn, dn, vn, tn, gamma, lam)
    bar = term_ref.gae_term_bar(rn, dn, vn, tn, aref, gamma, lam)
    an, retn = adv.cpu().numpy(), ret.cpu().numpy()
    err = np.abs(an.astype(np.float64) - aref)
    print("gae term gamma=%g lam=%g: worst error %.3g, worst error / bar %.3g" % (gamma, lam, float(err.max()), float((err / bar[None]).max())))
    assert (err <= bar[None]).all(), float((err / bar[None]).max())
    assert float(np.abs(aref).max()) > 100 * float(bar.max())       # teeth
    # ret - adv == values[:T] within one ulp
    diff = retn.astype(np.float64) - an.astype(np.float64) - vn[:steps]
    ulp_r = np.spacing(np.maximum(np.abs(retn), np.abs(vn[:steps])).astype(np.float32)).astype(np.float64)
    assert (np.abs(diff) <= ulp_r).all()
    # the feature is live: at a done step the advantage is today's plus gamma * term_value.  Today's is fl(r - V), one rounding; the new
    # one fl(fl(gamma tv + r) - V), two; gamma itself is rounded to fp32: four roundings of quantities below |r| + |V| + |tv|
    cut = dn != 0
    pn = plain.cpu().numpy().astype(np.float64)
    g32 = float(np.float32(gamma))
    tol = 4.0 * ac_ref.U24 * (np.abs(rn) + np.abs(vn[:steps]) + np.abs(tn))
    move = an.astype(np.float64) - pn
    assert (np.abs(move - g32 * tn)[cut] <= tol[cut]).all()
    assert float(np.mean(np.abs(g32 * tn[cut]) > 100 * tol[cut])) > 0.9          # teeth: the move is far above its tolerance
    pol.close(); env.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_env_and_policy_usable():
    import torch
    from gym_art_amd import QuadrotorEnv, _lib
    from gym_art_amd.multi_device import _MultiDeviceMixin
    from gym_art_amd.policy import MLPPolicy
    n, steps = 68, 4
    env, twin = _env(n, "alias"), _env(n, "alias")
    scale = _obs_scale(env)
    _obs_scale(twin)
    net = _Net(NETS[0], scale, 0)
    pol, pt = net.build(env, value=False), net.build(twin)
    _reset(env, pol); _reset(twin, pt)
    o, r, d, a = _bufs(env, steps)
    o2, r2, d2, a2 = _bufs(twin, steps)
    v, lp = _ac_bufs(env, steps)
    tv = _tv_buf(env, steps)

    def usable(p, ptwin):
        """a plain rollout of the refused pair and of the twin that was never refused: the same bits"""
        env.rollout_policy_dev(p, o, r, d, a)
        twin.rollout_policy_dev(ptwin, o2, r2, d2, a2)
        torch.cuda.synchronize()
        assert torch.equal(o, o2) and torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(d, d2)
        assert _same(env.state_dict(), twin.state_dict())

    with pytest.raises(_lib.GaqError, match="value head"):          # GAQ_ERR_STATE
        env.rollout_policy_dev(pol, o, r, d, a, term_values=tv)
    with pytest.raises(_lib.GaqError, match="value head"):
        env.rollout_policy_dev(pol, o, r, d, a, logp=lp, term_values=tv)
    usable(pol, pt)
    pol.set_value_head(*net.value)
    # Python-side checks: shape, dtype, layout, device
    for bad in (tv[:-1], torch.empty((steps, n + 1), device=_dev()), tv.double(), tv.t().contiguous().t(), tv.cpu(), v):
        with pytest.raises(ValueError, match="term_values must be"):
            env.rollout_policy_dev(pol, o, r, d, a, values=v, term_values=bad)
    off = torch.empty(steps * n + 1, device=_dev())[1:].view(steps, n)      # contiguous, 4 bytes off a 16-byte boundary
    with pytest.raises(ValueError, match="aligned"):                # GAQ_ERR_INVALID
        env.rollout_policy_dev(pol, o, r, d, a, values=v, term_values=off)
    usable(pol, pt)
    # engines without a value head
    small = _mlp([48], 18, 1, scale)
    for engine in ("valu", "bf16"):
        p2 = MLPPolicy.from_arrays(env, small, "tanh", True, log_std=LOG_STD, engine=engine)
        p2t = MLPPolicy.from_arrays(twin, small, "tanh", True, log_std=LOG_STD, engine=engine)
        with pytest.raises(ValueError, match="VALU" if engine == "valu" else "bf16"):       # GAQ_ERR_INVALID
            env.rollout_policy_dev(p2, o, r, d, a, term_values=tv)
        usable(p2, p2t)
        p2.close(); p2t.close()
    # a handle without auto-reset
    noreset = QuadrotorEnv(num_envs=n, ep_time=0.15, seed=7, init_random_state=True, auto_reset=False, alias_obs=True)
    _obs_scale(noreset)
    pn = net.build(noreset)
    _reset(noreset, pn)
    o3, r3, d3, a3 = _bufs(noreset, steps)
    with pytest.raises(_lib.GaqError, match=r"auto_reset = 0.*value_out\[t \+ 1\] already is"):      # GAQ_ERR_STATE
        noreset.rollout_policy_dev(pn, o3, r3, d3, a3, values=v, term_values=tv)
    v3, _ = _ac_bufs(noreset, steps)
    noreset.rollout_policy_dev(pn, o3, r3, d3, a3, values=v3)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v3).all())
    pn.close(); noreset.close()
    # gae
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp, term_values=tv)
    twin.rollout_policy_dev(pt, o2, r2, d2, a2)
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    with pytest.raises(ValueError, match="overlap"):
        env.gae_dev(r, d, v, 0.99, 0.95, tv, ret, term_values=tv)
    with pytest.raises(ValueError, match="overlap"):
        env.gae_dev(r, d, v, 0.99, 0.95, adv, tv, term_values=tv)
    for bad in (tv[:-1], tv.double(), tv.cpu(), v):
        with pytest.raises(ValueError, match="term_values must be"):
            env.gae_dev(r, d, v, 0.99, 0.95, adv, ret, term_values=bad)
    with pytest.raises(ValueError, match="gamma"):
        env.gae_dev(r, d, v, 1.5, 0.95, adv, ret, term_values=tv)
    env.gae_dev(r, d, v, 0.99, 0.95, adv, ret, term_values=tv)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(adv).all()) and bool(torch.isfinite(ret).all())
    usable(pol, pt)
    # the multi-device env refuses both, as it refuses values=
    for name in ("rollout_policy_dev", "gae_dev"):
        with pytest.raises(NotImplementedError, match="term_values"):
            getattr(_MultiDeviceMixin, name)(_MultiDeviceMixin.__new__(_MultiDeviceMixin), term_values=tv)
    for x in (pol, pt, env, twin):
        x.close()
