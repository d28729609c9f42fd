"""The LSTM policy engine (gaq.h GAQ_POLICY_CELL_LSTM, gym_art_amd.policy.LSTMPolicy): policy_lstm_kernel, policy_lstm_ac_kernel and
policy_lstm_term_kernel + the ordinary step launch per step.  Every case starts from non-zero h0, c0 (set_hidden) and uses ep_time = 0.15
(episodes of 16 steps) with T = 20, so that every env reports a done inside the window; each case asserts that it did.

1. actions, final h and c, V, terminal values, log-probabilities and advantages against the fp64 reference of tests/lstm_util.py fed the
   device's recorded observations, dones and terminal rows, at the smallest shapes that reach each code path (CASES below);
2. the reset of both states, split calls, repeated runs and a captured graph, bit for bit;
3. values=, logp=, term_values= and critic= change no other output bit; values[T] of one call is values[0] of the next; the gather at
   done counts 1, 63, 64, 65 and 129;
4. refusals that launch nothing.

ERROR BARS.  The LSTM's bars are not the GRU's: c is unbounded where a GRU's h is a convex mix.  The yardstick is torch's fp32 nn.LSTMCell
on the CPU run through the same rollouts (tests/lstm_util.py torch_step32 and torch_head32: the same recorded observations, dones and terminal rows, the
head in torch fp32 too) against the same fp64 reference; the bar of a quantity is 4 x the yardstick's worst error over CASES (the matrix core's
4-wide k-steps sum in another order than the BLAS), capped at the project's ATOL_FP32 = 1.5e-5 for actions and V.  Each case prints the
yardstick's and the device's figures before it asserts.
FIGURES.  Yardstick, worst over CASES: actions 5.43e-7, h 2.14e-7, c 3.33e-7, V and terminal values 2.49e-7; bars (4 x): actions
2.17e-6, h 8.55e-7, c 1.33e-6, V 9.96e-7 (the ATOL_FP32 cap does not bind).  These yardstick figures were taken on the CPU with the
nets, shapes, initial states and done pattern (every env done in step 15) of CASES but unit-normal stand-ins for the observations and
terminal rows, because no MI355X run could be obtained while this was written: the recorded inputs, and with them the device's worst
errors, are NOT MEASURED yet.  Every case prints the yardstick on its recorded inputs beside the device's figures; whoever runs this
file on a device first writes both here and in DESIGN.md, and takes YARD from the recorded-input yardstick if it differs."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from tests import ac_ref, term_ref
from tests.gru_util import _head
from tests.lstm_util import _lstm, reference_rollout, torch_head32, torch_step32
from tests.policy_util import _bufs, _dev
from tests.test_gpu_policy_shapes import ATOL_FP32, OBS, _kw, _obs_scale

pytestmark = pytest.mark.gpu

T = 20
LOG_STD = (-1.0, -0.5, -1.5, -1.0)
GAMMA, LAM = 0.99, 0.95
# the yardstick's worst |torch fp32 on the CPU - fp64| over CASES, per quantity (a: actions, h, c: final states, v: V and terminal
# values), and the bars derived from it
YARD = dict(a=5.43e-7, h=2.14e-7, c=3.33e-7, v=2.49e-7)
BAR = dict(a=min(4 * YARD["a"], ATOL_FP32), h=4 * YARD["h"], c=4 * YARD["c"], v=min(4 * YARD["v"], ATOL_FP32))

_BY_D = {d: o for o in OBS for d in [o[2]]}
# (H, head, act, out_tanh, D, N, layout).  H: 16 one chunk, three waves idle; 48 wave 3 idle; 80 wave 0 takes two chunks; 240; 256.
# D: 18 and 19 partial last k-steps of 2 and 3; 24 a multiple of 8; 13 and 20: (D & ~3) mod 8 = 4, the 4-wide tail after the 8-wide loop
# (20: no partial step); 108 with H = 256: LDS at its limit.  N: 1, 63, 64, 65, 130, 2096 (N D a multiple of 4: T > 1).
CASES = [(16, (), "tanh", True, 18, 130, "alias"), (48, (16, 80), "relu", False, 19, 64, "plain"),
         (80, (), "tanh", False, 13, 2096, "alias"), (240, (64,), "relu", True, 24, 64, "alias"),
         (256, (), "tanh", True, 108, 64, "alias"), (48, (), "relu", True, 20, 1, "plain"),
         (80, (16, 80), "tanh", True, 20, 63, "alias"), (16, (), "relu", False, 20, 65, "plain"),
         (256, (16, 80), "tanh", False, 18, 2096, "plain"), (240, (), "relu", False, 19, 2096, "alias")]
CASE_IDS = ["h%d-%s-%s-d%d-n%d-%s" % (H, "x".join(map(str, hd)) or "nohead", act, D, n, lay) for H, hd, act, _, D, n, lay in CASES]


def _env(D, n, layout="alias", graph_safe=False):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(**dict(_kw(_BY_D[D], n), alias_obs=layout == "alias"))
    assert env.obs_dim == D
    if graph_safe:
        env.set_graph_safe(True)
    return env


class _Net:
    """an LSTM cell whose gates stay off their tails (weights ~ 1 / sqrt(inputs), the observation scaled by its RMS), a head and a
    value head; buildable on several (twin) envs"""

    def __init__(self, H, head, act, out_tanh, D, scale, seed=0):
        W_ih, W_hh, b_ih, b_hh = _lstm(H, D, 1100 + seed, scale=1.0 / np.sqrt(D + H))
        self.lstm = ((W_ih / scale[None, :]).astype(np.float32), W_hh, b_ih, b_hh)
        self.layers = _head(H, head, 1101 + seed)
        self.H, self.act, self.out_tanh = H, act, out_tanh
        self.value = ac_ref.value_head(head[-1] if head else H, 1102 + seed)

    def build(self, env, log_std=LOG_STD, value=True):
        from gym_art_amd.policy import LSTMPolicy
        return LSTMPolicy(env, self.lstm, self.layers, self.act, self.out_tanh, log_std=log_std, value=self.value if value else None)

    def state0(self, n):
        rng = np.random.RandomState(n + self.H)
        return (0.5 * rng.randn(n, self.H)).astype(np.float32), (0.8 * rng.randn(n, self.H)).astype(np.float32)


def _start(env, pol, net):
    """reset, then the non-zero state: returns (a copy of the observation the first action sees, h0, c0)"""
    import torch
    o0 = torch.empty((env.num_envs, env.obs_dim), device=_dev())
    env.reset_dev(o0)
    h0, c0 = net.state0(env.num_envs)
    pol.set_hidden(h0, c0)
    return o0.clone(), h0, c0


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), device=_dev())


def _window(env, pol, net, steps=T, values=True, logp=True, term=True, critic=None):
    """one window from _start with what is asked for; a dict of tensors"""
    import torch
    n = env.num_envs
    o0, h0, c0 = _start(env, pol, net)
    tt = _nan(n, env.obs_dim)
    env.set_terminal_obs(tt)
    o, r, d, a = _bufs(env, steps)
    v = _nan(steps + 1, n) if values else None
    lp = _nan(steps, n) if logp else None
    tv = _nan(steps, n) if term else None
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp, term_values=tv, critic=critic)
    torch.cuda.synchronize()
    return dict(o0=o0, h0=h0, c0=c0, o=o, r=r, d=d, a=a, v=v, lp=lp, tv=tv, tt=tt, h=pol.hidden.clone(), c=pol.cell.clone())


def _np(w, *keys):
    return [w[k].cpu().numpy() for k in keys]


_WORST = dict(yard=dict(a=0.0, h=0.0, c=0.0, v=0.0), dev=dict(a=0.0, h=0.0, c=0.0, v=0.0), logp=0.0, adv=0.0)


# ---- 1. against fp64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_lstm_against_fp64(case):
    import torch
    H, head, act, out_tanh, D, n, layout = case
    env, twin = _env(D, n, layout), _env(D, n, layout)
    net = _Net(H, head, act, out_tanh, D, _obs_scale(env), CASES.index(case))
    _obs_scale(twin)
    pol, pt = net.build(env), net.build(twin, log_std=None)
    w = _window(env, pol, net)
    o0, o, d, a, h, c, v, lp, tv, tt, r = _np(w, "o0", "o", "d", "a", "h", "c", "v", "lp", "tv", "tt", "r")
    per_env = d.astype(np.int64).sum(axis=0)
    assert (per_env == 1).all(), (case, per_env.min(), per_env.max())          # every env reported its done inside the window
    assert np.isfinite(tt).all() and np.isfinite(v).all() and np.isfinite(lp).all() and np.isfinite(tv).all()
    rows = np.broadcast_to(tt, (T,) + tt.shape)                                 # each env's one terminal row, read where done is set
    args = (net.lstm, net.layers, act, out_tanh, o0, o, d, w["h0"], w["c0"], net.value, rows)
    ref = reference_rollout(*args)
    yard = reference_rollout(*args, step=torch_step32(net.lstm), head=torch_head32(net.layers, act, out_tanh, net.value))
    devv = np.concatenate([v.reshape(-1), tv[d != 0]])                        # V of every step, the bootstrap row, the terminal values
    refv = np.concatenate([ref["v"].reshape(-1), ref["tv"][d != 0]])
    yardv = np.concatenate([yard["v"].reshape(-1), yard["tv"][d != 0]])
    # teeth: the states and values are not within the bars of zero, the state did move, the zeros of tv are +0.0
    assert np.mean(np.abs(ref["c"]) > 1e-3) > 0.9 and np.mean(np.abs(refv) > BAR["v"]) > 0.9, case
    assert (tv.view(np.int32)[d == 0] == 0).all(), case
    ye = dict(h=np.max(np.abs(yard["h"] - ref["h"])), c=np.max(np.abs(yard["c"] - ref["c"])), v=np.max(np.abs(yardv - refv)),
              a=np.max(np.abs(yard["a"] - ref["a"])))
    # actions: this rollout's carry the exploration term, so a deterministic twin (log_std = None) gives the actions that are held to
    # the bar -- on its own trajectory, against its own reference; its states and values count too
    wt = _window(twin, pt, net, logp=False)
    at = wt["a"].cpu().numpy()
    assert (wt["d"].cpu().numpy().astype(np.int64).sum(axis=0) == 1).all(), case
    rt = reference_rollout(net.lstm, net.layers, act, out_tanh, *_np(wt, "o0", "o", "d"), wt["h0"], wt["c0"], net.value,
                           np.broadcast_to(wt["tt"].cpu().numpy(), (T, n, D)))
    de = dict(a=np.max(np.abs(at - rt["a"])), h=max(np.max(np.abs(h - ref["h"])), np.max(np.abs(wt["h"].cpu().numpy() - rt["h"]))),
              c=max(np.max(np.abs(c - ref["c"])), np.max(np.abs(wt["c"].cpu().numpy() - rt["c"]))),
              v=max(np.max(np.abs(devv - refv)), np.max(np.abs(wt["v"].cpu().numpy() - rt["v"]))))
    lref, lbar = ac_ref.logp64(a, ref["a"], LOG_STD, mean_atol=BAR["a"])
    lfrac = float(np.max(np.abs(lp - lref) / lbar))
    # advantages, with and without time-limit bootstrapping, from the device's own values: the arithmetic of the GAE kernels alone
    adv, adv_t = _nan(T, n), _nan(T, n)
    env.gae_dev(w["r"], w["d"], w["v"], GAMMA, LAM, adv)
    env.gae_dev(w["r"], w["d"], w["v"], GAMMA, LAM, adv_t, term_values=w["tv"])
    torch.cuda.synchronize()
    a64, _ = ac_ref.gae64(r, d, v, GAMMA, LAM)
    t64, _ = term_ref.gae_term64(r, d, v, tv, GAMMA, LAM)
    afrac = max(float(np.max(np.abs(adv.cpu().numpy() - a64) / ac_ref.gae_bar(r, v, a64, GAMMA, LAM)[None])),
                float(np.max(np.abs(adv_t.cpu().numpy() - t64) / term_ref.gae_term_bar(r, d, v, tv, t64, GAMMA, LAM)[None])))
    for k in ("a", "h", "c", "v"):
        _WORST["yard"][k], _WORST["dev"][k] = max(_WORST["yard"][k], ye[k]), max(_WORST["dev"][k], de[k])
    _WORST["logp"], _WORST["adv"] = max(_WORST["logp"], lfrac), max(_WORST["adv"], afrac)
    print("lstm %s: yardstick a %.3g h %.3g c %.3g v %.3g | device a %.3g h %.3g c %.3g v %.3g | logp err/bar %.3g adv err/bar %.3g"
          % (CASE_IDS[CASES.index(case)], ye["a"], ye["h"], ye["c"], ye["v"], de["a"], de["h"], de["c"], de["v"], lfrac, afrac))
    print("lstm worst so far: yardstick %s | device %s | bars %s" % (_WORST["yard"], _WORST["dev"], BAR))
    for k in ("a", "h", "c", "v"):
        assert de[k] <= BAR[k], (case, k, de[k], BAR[k])
    assert lfrac <= 1.0 and afrac <= 1.0, (case, lfrac, afrac)
    for x in (pol, pt, env, twin):
        x.close()


# ---- 2. reset and determinism -------------------------------------------------------------------------------------------------------
def test_done_rows_of_both_states_are_zero_and_reset_hidden():
    """staggered episodes: the rows of .hidden and .cell are zero exactly where done[T - 1] is set; reset_hidden(mask) zeroes exactly the
    masked rows of both"""
    import torch
    n = 2096
    env = _env(18, n)
    net = _Net(64, (), "tanh", True, 18, _obs_scale(env))
    pol = net.build(env)
    _start(env, pol, net)
    o, r, d, a = _bufs(env, 4)
    env.rollout_policy_dev(pol, o, r, d, a)
    half = torch.from_numpy(np.random.RandomState(0).rand(n) < 0.5).to(_dev(), torch.uint8)
    cur = o[3].clone()
    env.reset_dev(cur, half)
    pol.reset_hidden(half)
    o, r, d, a = _bufs(env, T)                                      # the rest finishes at t = 11, the reset half in the last step (t = 15)
    env.rollout_policy_dev(pol, o[:16], r[:16], d[:16], a[:16])
    torch.cuda.synchronize()
    last = d[15].bool()
    assert 0 < int(last.sum()) < n and torch.equal(last, half.bool())
    assert bool((d[:16].to(torch.int32).sum(dim=0) == 1).all())     # every env reported a done
    assert torch.equal((pol.hidden == 0).all(dim=1), last) and torch.equal((pol.cell == 0).all(dim=1), last)
    assert bool((pol.hidden[~last] != 0).any(dim=1).all()) and bool((pol.cell[~last] != 0).any(dim=1).all())
    h0, c0 = torch.randn(n, 64, device=_dev()) + 3.0, torch.randn(n, 64, device=_dev()) - 3.0
    pol.set_hidden(h0, c0)
    m = torch.from_numpy(np.random.RandomState(1).rand(n) < 0.3).to(_dev())
    pol.reset_hidden(m)
    torch.cuda.synchronize()
    for s, s0 in ((pol.hidden, h0), (pol.cell, c0)):
        assert not s[m].any() and torch.equal(s[~m], s0[~m])
    pol.reset_hidden()
    torch.cuda.synchronize()
    assert not pol.hidden.any() and not pol.cell.any()
    pol.close(); env.close()


@pytest.mark.parametrize("layout", ["alias", "plain"])
def test_split_and_repeated_rollouts_give_the_same_bits(layout):
    """T = 20 in one call equals 7 + 13 (the second call's first launch meets no done mask; the done step 15 falls inside it) and 16 + 4
    (the split right after the done step: the masked zero, then a first launch without done_prev), and a second run of the whole:
    actions, observations, values, log-probabilities, terminal values, h and c"""
    import torch
    n, outs = 130, []
    for splits in ([T], [7, 13], [16, 4], [T]):
        env = _env(18, n, layout)
        net = _Net(80, (16,), "tanh", True, 18, _obs_scale(env))
        pol = net.build(env)
        _start(env, pol, net)
        o, r, d, a = _bufs(env, T)
        v, lp, tv = _nan(T + 1, n), _nan(T, n), _nan(T, n)
        t = 0
        for k in splits:
            v1, lp1, tv1 = _nan(k + 1, n), _nan(k, n), _nan(k, n)   # (of their own: row t of a [T, 130] tensor is not always aligned)
            env.rollout_policy_dev(pol, o[t:t + k], r[t:t + k], d[t:t + k], a[t:t + k], values=v1, logp=lp1, term_values=tv1)
            torch.cuda.synchronize()
            if t:
                assert torch.equal(v[t], v1[0]), (splits, t)       # values[T] of one call is values[0] of the next
            v[t:t + k + 1], lp[t:t + k], tv[t:t + k] = v1, lp1, tv1
            t += k
        assert bool((d.to(torch.int32).sum(dim=0) == 1).all())
        outs.append((o, r, d, a, v, lp, tv.view(torch.int32), pol.hidden.clone(), pol.cell.clone()))
        pol.close(); env.close()
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert bool(torch.isfinite(x.float()).all()) and torch.equal(x, y)


@pytest.mark.parametrize("layout", ["alias", "plain"])
def test_graph_captured_lstm_rollout(layout):
    """graph-safe mode: a captured 10-step rollout with everything asked for, replayed twice, equals eager calls on a twin -- every
    output, .hidden and .cell.  Episodes are 16 steps: every env finishes inside the replays."""
    import torch
    n, steps = 68, 10
    graphed, eager = _env(18, n, layout, True), _env(18, n, layout, True)
    net = _Net(48, (16, 80), "relu", True, 18, _obs_scale(graphed))
    _obs_scale(eager)
    pols = [net.build(graphed), net.build(eager)]
    bufs, kws = [], []
    for e, p in zip((graphed, eager), pols):
        _start(e, p, net)
        e.set_terminal_obs(_nan(n, 18))
        bufs.append(_bufs(e, steps))
        kws.append(dict(values=_nan(steps + 1, n), logp=_nan(steps, n), term_values=_nan(steps, n)))
    torch.cuda.synchronize()

    def same(what):
        for x, y in zip(bufs[0], bufs[1]):
            assert torch.equal(x, y), what
        for key in kws[0]:
            assert bool(torch.isfinite(kws[0][key]).all()), (what, key)
            assert torch.equal(kws[0][key].view(torch.int32), kws[1][key].view(torch.int32)), (what, key)
        assert torch.equal(pols[0].hidden, pols[1].hidden) and torch.equal(pols[0].cell, pols[1].cell), what

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up on a side stream: the lazy allocations happen here
        graphed.rollout_policy_dev(pols[0], *bufs[0], **kws[0])
    torch.cuda.current_stream().wait_stream(side)
    eager.rollout_policy_dev(pols[1], *bufs[1], **kws[1])
    torch.cuda.synchronize()
    same("warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.rollout_policy_dev(pols[0], *bufs[0], **kws[0])
    dones = torch.zeros(n, dtype=torch.int32, device=_dev())
    for rep in range(2):
        g.replay()
        eager.rollout_policy_dev(pols[1], *bufs[1], **kws[1])
        torch.cuda.synchronize()
        same("replay %d" % rep)
        dones += bufs[0][2].to(torch.int32).sum(dim=0)
    assert bool((dones >= 1).all())
    for x in pols + [graphed, eager]:
        x.close()


# ---- 3. actor-critic ----------------------------------------------------------------------------------------------------------------
def _critic(env, seed=5):
    from gym_art_amd.policy import MLPCritic
    from tests.mlp_ref import _scaled_layers
    layers = _scaled_layers([48, 16], env.obs_dim, seed)
    W, b = layers[-1]
    return MLPCritic(env, layers[:-1] + [(W[:1], b[:1])], "tanh")


@pytest.mark.parametrize("layout", ["alias", "plain"])
def test_asking_for_more_changes_no_other_bit(layout):
    """values=, logp=, term_values= and critic= (on a policy without a value head): observations, rewards, dones, actions, terminal
    rows, h and c are the bits of the plain call; the actor's own outputs do not depend on what else is asked"""
    import torch
    n = 130
    asks = [dict(values=False, logp=False, term=False), dict(values=True, logp=False, term=False),
            dict(values=False, logp=True, term=False), dict(values=True, logp=True, term=True),
            dict(values=True, logp=True, term=True, critic=True)]
    ws = []
    for ask in asks:
        env = _env(18, n, layout)
        net = _Net(48, (16,), "relu", True, 18, _obs_scale(env))
        with_critic = ask.pop("critic", False)
        pol = net.build(env, value=not with_critic)
        cr = _critic(env) if with_critic else None
        ws.append(_window(env, pol, net, critic=cr, **ask))
        assert bool((ws[-1]["d"].to(torch.int32).sum(dim=0) == 1).all())
        for x in (cr, pol, env):
            if x is not None:
                x.close()
    for w in ws[1:]:
        for key in ("o", "r", "d", "a", "tt", "h", "c"):
            assert torch.equal(ws[0][key], w[key]), key
    assert torch.equal(ws[1]["v"], ws[3]["v"]) and torch.equal(ws[2]["lp"], ws[3]["lp"]) and torch.equal(ws[2]["lp"], ws[4]["lp"])
    assert bool(torch.isfinite(ws[4]["v"]).all()) and not torch.equal(ws[4]["v"], ws[3]["v"])    # the critic's V, not the head's
    assert bool((ws[4]["tv"].view(torch.int32)[ws[4]["d"] == 0] == 0).all()) and bool((ws[4]["tv"][ws[4]["d"] != 0] != 0).all())


MASKS = {"1+129": 1, "63+67": 63, "64+66": 64, "65+65": 65}


@pytest.mark.parametrize("mask_id", list(MASKS))
def test_gather_at_done_counts_of_1_to_129(mask_id):
    """N = 130, staggered: the masked envs are reset after 5 steps and finish in window step 15, the rest in step 10 -- done counts of
    1 and 129, 63, 64, 65 per step.  Terminal values against fp64 (h and c of the fp64 recurrence), +0.0 elsewhere"""
    import torch
    n, k = 130, MASKS[mask_id]
    env = _env(18, n)
    net = _Net(48, (16, 80), "tanh", True, 18, _obs_scale(env))
    pol = net.build(env)
    _start(env, pol, net)
    o, r, d, a = _bufs(env, 5)
    env.rollout_policy_dev(pol, o, r, d, a)
    mask = np.zeros(n, bool)
    mask[np.random.RandomState(k).permutation(n)[:k]] = True
    m = torch.from_numpy(mask).to(_dev(), torch.uint8)
    cur = o[4].clone()
    env.reset_dev(cur, m)
    h0, c0 = net.state0(n)
    pol.set_hidden(h0, c0)                                          # every row non-zero again
    tt = _nan(n, 18)
    env.set_terminal_obs(tt)
    o, r, d, a = _bufs(env, T)
    v, tv = _nan(T + 1, n), _nan(T, n)
    env.rollout_policy_dev(pol, o, r, d, a, values=v, term_values=tv)
    torch.cuda.synchronize()
    counts = d.to(torch.int32).sum(dim=1).cpu().numpy()
    want = np.zeros(T, np.int64)
    want[10], want[15] = n - k, k
    assert np.array_equal(counts, want), counts
    dn, tvn, ttn = d.cpu().numpy(), tv.cpu().numpy(), tt.cpu().numpy()
    assert np.isfinite(tvn).all() and (tvn.view(np.int32)[dn == 0] == 0).all()
    ref = reference_rollout(net.lstm, net.layers, net.act, net.out_tanh, cur.cpu().numpy(), o.cpu().numpy(), dn, h0, c0, net.value,
                            np.broadcast_to(ttn, (T, n, 18)))
    assert np.mean(np.abs(ref["tv"][dn != 0]) > BAR["v"]) > 0.9
    err = float(np.max(np.abs(tvn - ref["tv"])))
    print("lstm gather %s: worst |V_term - V_ref| %.3g (bar %.3g)" % (mask_id, err, BAR["v"]))
    assert err <= BAR["v"], err
    pol.close(); env.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    import torch
    from gym_art_amd.policy import GRUPolicy, MLPPolicy
    from tests.gru_util import _gru
    n = 68
    env, twin, other = _env(18, n), _env(18, n), _env(18, n)
    lib = _lib.load()
    net = _Net(64, (), "tanh", True, 18, np.ones(18))
    pol, pol_other = net.build(env), net.build(other)
    for e in (env, twin, other):
        e.reset_dev(torch.empty((n, 18), device=_dev()))
    o, r, d, a = _bufs(env, 4)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rollout(p):
        return lib.gaq_step_policy_many_dev(env._handle, p.handle, 4, _lib.ptr(o), _lib.ptr(r), _lib.ptr(d), _lib.ptr(a), st)
    # only an LSTM policy has a cell state
    mlp = MLPPolicy.from_arrays(env, [(np.zeros((16, 18)), np.zeros(16)), (np.zeros((4, 16)), np.zeros(4))], engine="mfma")
    gru = GRUPolicy(env, _gru(64), _head(64))
    assert lib.gaq_policy_cell(pol.handle) == 3 and lib.gaq_policy_cell(gru.handle) == 1 and lib.gaq_policy_cell(mlp.handle) == 0
    assert lib.gaq_policy_set_cell_dev(mlp.handle, _lib.ptr(pol.cell)) == -1
    assert lib.gaq_policy_set_cell_dev(gru.handle, _lib.ptr(pol.cell)) == -1
    assert lib.gaq_policy_set_cell_dev(gru.handle, None) == -1
    # a misaligned buffer is refused and the registration stays
    assert lib.gaq_policy_set_cell_dev(pol.handle, C.c_void_p(pol.cell.data_ptr() + 4)) == -1
    # a policy of another env
    assert rollout(pol_other) == -1
    with pytest.raises(ValueError):
        env.rollout_policy_dev(pol_other, o, r, d, a)
    # either buffer unregistered: GAQ_ERR_STATE
    _lib.check(lib.gaq_policy_set_cell_dev(pol.handle, None))
    assert rollout(pol) == -4
    assert lib.gaq_policy_reset_hidden_dev(pol.handle, None, st) == -4
    _lib.check(lib.gaq_policy_set_cell_dev(pol.handle, _lib.ptr(pol.cell)))
    _lib.check(lib.gaq_policy_set_hidden_dev(pol.handle, None))
    assert rollout(pol) == -4
    with pytest.raises(_lib.GaqError):
        env.rollout_policy_dev(pol, o, r, d, a)
    _lib.check(lib.gaq_policy_set_hidden_dev(pol.handle, _lib.ptr(pol.hidden)))
    torch.cuda.synchronize()
    assert not pol.hidden.any() and not pol.cell.any()              # no launch wrote a state
    # nothing moved: the env and its twin step alike
    acts = torch.rand((6, n, 4), device=_dev()) * 2 - 1
    o1, r1, d1, _ = _bufs(env, 6)
    o2, r2, d2, _ = _bufs(twin, 6)
    env.step_many_dev(acts, o1, r1, d1)
    twin.step_many_dev(acts, o2, r2, d2)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    for x in (mlp, gru, pol, pol_other, env, twin, other):
        x.close()
