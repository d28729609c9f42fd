"""An encoder in front of the cell (gaq.h gaq_policy_desc_rnn_enc; GRUPolicy / LSTMPolicy.with_encoder): policy_encode_kernel and its
gathered form in front of the six unchanged cell kernels.

1. actions, final h and c, V (every step, the bootstrap row, the terminal values) and log-probabilities against the fp64 reference of
   tests/enc_util.py fed the device's recorded observations, dones and terminal rows, after one step and after twenty with auto-resets
   (episodes are 16 steps: ep_time = 0.15), at the smallest shapes at which the kernel can go wrong (CASES);
2. bits: the same rollout twice and on another stream, 20 = 7 + 13, a captured graph, the recorded actions replayed through
   step_many_dev, values= / logp= / term_values= / critic= against the plain call;
3. existing paths: a policy without an encoder is the old constructor path bit for bit, gaq_policy_encoder_width is 0 without an encoder;
4. refusals by text, which launch nothing and leave the handle's bits alone.

ERROR BARS.  The bar of a quantity in a case is 8 x the error torch fp32 on the CPU (tests/enc_util.py yardstick_parts: F.linear,
nn.GRUCell / nn.LSTMCell, the head in torch fp32) shows against the same fp64 reference on the same recorded inputs: YARD below, taken
on the recorded inputs of an MI355X run (the env is seeded, so they are the same on every run; each case prints the yardstick it
computes beside the committed one and beside the device's error before it asserts).  Keys: a actions, h and c the final states, v the
values of every step, the bootstrap row and the terminal values.
FIGURES (MI355X, worst over the 14 cases, yardstick | device): a 3.37e-7 | 5.65e-7, h 2.65e-7 | 3.32e-7, c 2.99e-7 | 4.38e-7,
v 3.63e-7 | 3.27e-7; the device's worst error is 1.94 x its case's yardstick; the worst log-probability error 0.13 of its derived bar.

SHAPES.  A call of more than one step needs N * obs_dim * 4 to be a multiple of 16 (gaq.h gaq_step_many_dev), which N = 65 is for
neither D = 18 nor D = 19 and N = 454 is not for D = 19.  At those shapes the twenty steps are twenty calls of one step into buffers of
their own -- a rollout does not depend on how it is split into calls, which section 2 asserts bit for bit -- and at the others (N = 454
with D = 18) one call, whose launches apply the done mask of the step before inside the cell's launch."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from tests import ac_ref
from tests.enc_util import _cell, _desc_enc, _encoder, reference_rollout, yardstick_parts
from tests.gru_util import _desc_rnn, _head
from tests.policy_util import _bufs, _dev, _replay, environ

pytestmark = pytest.mark.gpu

T = 20
LOG_STD = (-1.0, -0.5, -1.5, -1.0)
REPR = {18: "xyz_vxyz_R_omega", 19: "xyz_vxyz_R_omega_h"}
NORM_EPS, NORM_CLIP = 2.0 ** -20, 5.0

# (cell, encoder widths, D, H, head, act, out_tanh, N, layout, norm).  Encoder widths: 16 one chunk, three waves idle; 48 wave 3 idle;
# 80 wave 0 owns two chunks; 256 every wave four; 240-80 two layers (the first through LDS, 15 chunks).  D = 19: the partial k-step.
CASES = [("gru", (16,), 18, 16, (), "tanh", True, 65, "alias", False),
         ("gru", (48,), 19, 48, (), "relu", False, 454, "plain", False),
         ("lstm", (80,), 18, 48, (32,), "tanh", False, 454, "alias", False),
         ("lstm", (256,), 19, 16, (), "relu", True, 65, "plain", False),
         ("gru", (240, 80), 18, 48, (), "tanh", True, 454, "plain", False),
         ("lstm", (240, 80), 19, 16, (), "relu", False, 65, "alias", False),
         ("gru", (48,), 18, 16, (), "tanh", False, 454, "alias", True)]
CASE_IDS = ["%s-enc%s-d%d-h%d-%s-%s-n%d-%s%s" % (c, "x".join(map(str, e)), D, H, "x".join(map(str, hd)) or "nohead", act, n, lay,
                                                 "-norm" if nm else "") for c, e, D, H, hd, act, _, n, lay, nm in CASES]

# |torch fp32 on the CPU - fp64| on the recorded inputs, per case and window length (see ERROR BARS)
YARD = {
    "gru-enc16-d18-h16-nohead-tanh-n65-alias/1": dict(a=1.02e-07, h=1.32e-07, v=1.04e-07),
    "gru-enc16-d18-h16-nohead-tanh-n65-alias/20": dict(a=1.26e-07, h=9.09e-08, v=1.48e-07),
    "gru-enc48-d19-h48-nohead-relu-n454-plain/1": dict(a=1.73e-07, h=2.09e-07, v=1.59e-07),
    "gru-enc48-d19-h48-nohead-relu-n454-plain/20": dict(a=3.37e-07, h=1.62e-07, v=3.63e-07),
    "lstm-enc80-d18-h48-32-tanh-n454-alias/1": dict(a=1.38e-07, h=1.8e-07, c=2.9e-07, v=1.03e-07),
    "lstm-enc80-d18-h48-32-tanh-n454-alias/20": dict(a=1.75e-07, h=1.3e-07, c=2.96e-07, v=1.25e-07),
    "lstm-enc256-d19-h16-nohead-relu-n65-plain/1": dict(a=7.23e-08, h=9.15e-08, c=1.64e-07, v=7.84e-08),
    "lstm-enc256-d19-h16-nohead-relu-n65-plain/20": dict(a=1.72e-07, h=1.01e-07, c=2.99e-07, v=1.27e-07),
    "gru-enc240x80-d18-h48-nohead-tanh-n454-plain/1": dict(a=1.64e-07, h=2.53e-07, v=1.86e-07),
    "gru-enc240x80-d18-h48-nohead-tanh-n454-plain/20": dict(a=2.36e-07, h=2.4e-07, v=3.15e-07),
    "lstm-enc240x80-d19-h16-nohead-relu-n65-alias/1": dict(a=9.74e-08, h=7.74e-08, c=1.97e-07, v=6.49e-08),
    "lstm-enc240x80-d19-h16-nohead-relu-n65-alias/20": dict(a=2.1e-07, h=7.55e-08, c=1.62e-07, v=8.63e-08),
    "gru-enc48-d18-h16-nohead-tanh-n454-alias-norm/1": dict(a=2.34e-07, h=2.21e-07, v=1.79e-07),
    "gru-enc48-d18-h16-nohead-tanh-n454-alias-norm/20": dict(a=2.88e-07, h=2.65e-07, v=1.96e-07),
}


def _calls(n, D, steps):
    """how a window of `steps` steps is split into calls: one call where N * D * 4 bytes are a multiple of 16, else one call per step"""
    return [steps] if (n * D) % 4 == 0 else [1] * steps


def _env(D, n, layout="alias", graph_safe=False):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(num_envs=n, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=layout == "alias", obs_repr=REPR[D])
    assert env.obs_dim == D
    if graph_safe:
        env.set_graph_safe(True)
    return env


def _reset_obs(env):
    import torch
    o0 = torch.empty((env.num_envs, env.obs_dim), device=_dev())
    env.reset_dev(o0)
    torch.cuda.synchronize()
    return o0


def _norm_stats(x):
    """statistics whose fp32 table is exact: means on a grid of 1/4, var + eps a power of 4 (inv_std a power of 2)"""
    mean = np.round(x.mean(axis=0) * 4.0) / 4.0
    inv_std = 2.0 ** -np.round(np.log2(np.maximum(x.std(axis=0), 0.25)))
    return mean, 1.0 / inv_std ** 2 - NORM_EPS, inv_std


class _Net:
    """an encoder, a cell whose gates stay off their tails, a head and a value head; buildable on several (twin) envs.  Without a
    normaliser the observation's RMS is folded into the encoder's first layer; with one the normaliser does that."""

    def __init__(self, case, env, seed=0):
        self.cell, self.enc_w, self.D, self.H, self.head, self.act, self.out_tanh = case[:7]
        x = _reset_obs(env).double().cpu().numpy()
        self.norm = None
        scale = np.maximum(1.0, np.sqrt((x * x).mean(axis=0)))
        if case[9]:
            mean, var, inv_std = _norm_stats(x)
            self.norm, self.var, scale = (mean, inv_std, NORM_CLIP), var, None
        self.enc = _encoder(self.D, self.enc_w, 2100 + seed, scale)
        self.weights = _cell(self.cell, self.H, self.enc_w[-1], 2101 + seed)
        self.layers = _head(self.H, self.head, 2102 + seed)
        self.value = ac_ref.value_head(self.head[-1] if self.head else self.H, 2103 + seed)

    def build(self, env, log_std=LOG_STD, value=True, encoder=True):
        from gym_art_amd.policy import GRUPolicy, LSTMPolicy, ObsNorm
        norm = None
        if self.norm is not None:
            norm = ObsNorm.from_stats(env, self.norm[0], self.var, 1.0, NORM_EPS, NORM_CLIP)
        cls = GRUPolicy if self.cell == "gru" else LSTMPolicy
        value = self.value if value else None
        if not encoder:
            assert norm is None
            return cls(env, self.weights, self.layers, self.act, self.out_tanh, log_std=log_std, value=value)
        return cls.with_encoder(env, self.enc, self.weights, self.layers, self.act, self.out_tanh, log_std=log_std, value=value, obs_norm=norm)

    def state0(self, n):
        rng = np.random.RandomState(n + self.H)
        return tuple((s * rng.randn(n, self.H)).astype(np.float32) for s in ((0.5,) if self.cell == "gru" else (0.5, 0.8)))

    def args(self):
        return self.cell, self.enc, self.weights, self.layers, self.act, self.out_tanh


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), device=_dev())


def _states(pol):
    return [pol.hidden.clone()] + ([pol.cell.clone()] if hasattr(pol, "cell") else [])


def _window(env, pol, net, steps=T, values=True, logp=True, term=True, critic=None, splits=None):
    """reset, the non-zero state, then one window (in `splits` calls) with what is asked for; a dict of tensors"""
    import torch
    n = env.num_envs
    o0 = _reset_obs(env).clone()
    s0 = net.state0(n)
    pol.set_hidden(*s0)
    tt = _nan(n, env.obs_dim)
    env.set_terminal_obs(tt)
    o, r, d, a = _bufs(env, steps)
    v = _nan(steps + 1, n) if values else None
    lp = _nan(steps, n) if logp else None
    tv = _nan(steps, n) if term else None
    t = 0
    for k in splits or _calls(n, env.obs_dim, steps):
        o1, r1, d1, a1 = _bufs(env, k)                             # (of their own: row t of a [T, N, ...] tensor is not always 16-byte aligned)
        v1 = _nan(k + 1, n) if values else None
        lp1 = _nan(k, n) if logp else None
        tv1 = _nan(k, n) if term else None
        env.rollout_policy_dev(pol, o1, r1, d1, a1, values=v1, logp=lp1, term_values=tv1, critic=critic)
        torch.cuda.synchronize()
        o[t:t + k], r[t:t + k], d[t:t + k], a[t:t + k] = o1, r1, d1, a1
        if values:
            if t:
                assert torch.equal(v[t], v1[0]), (splits, t)       # values[T] of one call is values[0] of the next
            v[t:t + k + 1] = v1
        if logp:
            lp[t:t + k] = lp1
        if term:
            tv[t:t + k] = tv1
        t += k
    out = dict(o0=o0, s0=s0, o=o, r=r, d=d, a=a, v=v, lp=lp, tv=tv, tt=tt)
    out["s"] = _states(pol)
    return out


def _np(w, *keys):
    return [w[k].cpu().numpy() for k in keys]


def _errors(net, w, parts=None):
    """max |x - fp64 reference| of a window's actions, states and values, x = the window's own (parts None) or the yardstick's"""
    o0, o, d, tt = _np(w, "o0", "o", "d", "tt")
    steps = o.shape[0]
    rows = np.broadcast_to(tt, (steps,) + tt.shape)               # every env ends at most one episode in a window: its one terminal row
    ref = reference_rollout(*net.args(), o0, o, d, w["s0"], net.value, rows, net.norm)
    if parts is not None:
        x = reference_rollout(*net.args(), o0, o, d, w["s0"], net.value, rows, net.norm, parts=parts)
        xa, xs, xv, xtv = x["a"], [x["h"]] + ([x["c"]] if "c" in x else []), x["v"], x["tv"]
    else:
        xa, xs, xv, xtv = w["a"].cpu().numpy(), [s.cpu().numpy() for s in w["s"]], w["v"].cpu().numpy(), w["tv"].cpu().numpy()
        assert np.isfinite(xv).all() and np.isfinite(xtv).all()
        assert (xtv.view(np.int32)[d == 0] == 0).all()           # +0.0 wherever no episode ended
    e = dict(a=np.max(np.abs(xa - ref["a"])), h=np.max(np.abs(xs[0] - ref["h"])),
             v=max(np.max(np.abs(xv - ref["v"])), np.max(np.abs(xtv - ref["tv"])[d != 0], initial=0.0)))
    if "c" in ref:
        e["c"] = np.max(np.abs(xs[1] - ref["c"]))
    return e, ref


def _measure(case, steps):
    """one case at one window length: (the yardstick's errors, the device's, the worst log-probability error / its bar)"""
    cell, enc_w, D, H, head, act, out_tanh, n, layout, norm = case
    env, twin = _env(D, n, layout), _env(D, n, layout)
    net = _Net(case, env, CASES.index(case))
    det, exp = net.build(env, log_std=None), net.build(twin)
    if norm:                                                       # the table is exact in fp32: normalize_dev is the fp32 formula's bits
        x = _reset_obs(env)
        z = det.obs_norm.normalize_dev(x).cpu().numpy()
        x32, (mean, inv_std, clip) = x.cpu().numpy(), net.norm
        assert np.array_equal(z, np.clip((x32 - mean.astype(np.float32)) * inv_std.astype(np.float32), -clip, clip).astype(np.float32))
    w = _window(env, det, net, steps, logp=False)
    d = w["d"].cpu().numpy()
    if steps == T:
        assert 0 < int(d[:-1].sum()) and d[15].any(), case         # auto-resets inside the window, episodes ended by the time limit
        assert (d.astype(np.int64).sum(axis=0) <= 1).all()
    dev, ref = _errors(net, w)
    yard, _ = _errors(net, w, yardstick_parts(*net.args(), net.value, net.norm))
    # teeth: the states moved and the values are not within the bars of zero
    assert np.mean(np.abs(ref["h"]) > 1e-3) > 0.5 and np.mean(np.abs(ref["v"]) > 1e-3) > 0.9, case
    # log-probabilities: the exploring twin on its own trajectory, against the reference's means on that trajectory
    we = _window(twin, exp, net, steps)
    _, refe = _errors(net, we)
    lref, lbar = ac_ref.logp64(we["a"].cpu().numpy(), refe["a"], LOG_STD, mean_atol=8 * yard["a"])
    lfrac = float(np.max(np.abs(we["lp"].cpu().numpy() - lref) / lbar))
    for x in (det, exp, env, twin):
        x.close()
    return yard, dev, lfrac


@pytest.mark.parametrize("steps", [1, T], ids=["one-step", "twenty-steps"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_encoder_against_fp64(case, steps):
    name = "%s/%d" % (CASE_IDS[CASES.index(case)], steps)
    yard, dev, lfrac = _measure(case, steps)
    fmt = lambda e: " ".join("%s %.3g" % (k, e[k]) for k in sorted(e))
    print("enc %s: yardstick now %s | committed %s | device %s | logp err/bar %.3g" % (name, fmt(yard), fmt(YARD.get(name, {})), fmt(dev), lfrac))
    for k in dev:
        assert dev[k] <= 8 * YARD[name][k], (name, k, dev[k], 8 * YARD[name][k])
    assert lfrac <= 1.0, (name, lfrac)


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------
BITS = {"gru": CASES[4], "lstm": CASES[2]}                       # two layers into a GRU; one layer into an LSTM with a head
KEYS = ("o", "r", "d", "a", "v", "lp", "tv", "tt")


def _same(w1, w2, what, keys=KEYS):
    import torch
    for k in keys:
        assert bool(torch.isfinite(w1[k].float()).all()) or k == "tt", (what, k)
        assert torch.equal(w1[k].view(torch.int32) if w1[k].dtype == torch.float32 else w1[k],
                           w2[k].view(torch.int32) if w2[k].dtype == torch.float32 else w2[k]), (what, k)
    for s1, s2 in zip(w1["s"], w2["s"]):
        assert torch.equal(s1, s2), (what, "state")


def _fresh(cell, layout, n=132, **build):
    case = BITS[cell]
    env = _env(case[2], n, layout)
    net = _Net(case, env)
    return env, net, net.build(env, **build)


@pytest.mark.parametrize("layout", ["alias", "plain"])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_repeats_streams_and_splits_give_the_same_bits(cell, layout):
    """the same window twice, on another stream, and as 7 + 13: obs, rew, done, actions, values, logp, terminal values, h and c"""
    import torch
    ws = []
    for how in ("one call", "again", "side stream", "7 + 13"):
        env, net, pol = _fresh(cell, layout)
        if how == "side stream":
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ws.append(_window(env, pol, net))
            torch.cuda.current_stream().wait_stream(side)
        else:
            ws.append(_window(env, pol, net, splits=[7, 13] if how == "7 + 13" else None))
        assert bool((ws[-1]["d"].to(torch.int32).sum(dim=0) == 1).all())
        pol.close(); env.close()
    for w, how in zip(ws[1:], ("again", "side stream", "7 + 13")):
        _same(ws[0], w, how)


@pytest.mark.parametrize("cell,layout", [("gru", "alias"), ("lstm", "plain")])
def test_graph_captured_rollout(cell, layout):
    """graph-safe mode: a captured 10-step rollout with everything asked for, replayed twice, equals eager calls on a twin"""
    import torch
    case, n, steps = BITS[cell], 68, 10
    graphed, eager = _env(case[2], n, layout, True), _env(case[2], n, layout, True)
    net = _Net(case, graphed)
    _reset_obs(eager)
    pols = [net.build(graphed), net.build(eager)]
    bufs, kws = [], []
    for e, p in zip((graphed, eager), pols):
        _reset_obs(e)
        p.set_hidden(*net.state0(n))
        e.set_terminal_obs(_nan(n, case[2]))
        bufs.append(_bufs(e, steps))
        kws.append(dict(values=_nan(steps + 1, n), logp=_nan(steps, n), term_values=_nan(steps, n)))
    torch.cuda.synchronize()

    def same(what):
        for x, y in zip(bufs[0], bufs[1]):
            assert torch.equal(x, y), what
        for key in kws[0]:
            assert bool(torch.isfinite(kws[0][key]).all()), (what, key)
            assert torch.equal(kws[0][key].view(torch.int32), kws[1][key].view(torch.int32)), (what, key)
        for s1, s2 in zip(_states(pols[0]), _states(pols[1])):
            assert torch.equal(s1, s2), what

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


@pytest.mark.parametrize("cell,layout", [("gru", "plain"), ("lstm", "alias")])
def test_recorded_actions_replay_bit_for_bit(cell, layout):
    """the recorded actions through step_many_dev on a twin reproduce obs, reward and done"""
    import torch
    env, net, pol = _fresh(cell, layout)
    with environ(GAQ_NO_FUSED="1"):                                 # the replay steps with the per-step launch too
        twin = _env(BITS[cell][2], env.num_envs, layout)
    w = _window(env, pol, net)
    assert int(w["d"].sum()) > 0
    _reset_obs(twin)                                                # (the env has been reset twice: by _Net and by _window)
    o2, r2, d2 = _replay(twin, w["a"])
    assert torch.equal(w["o"], o2) and torch.equal(w["r"], r2) and torch.equal(w["d"], d2)
    for x in (pol, env, twin):
        x.close()


def _critic(env, seed=5):
    from gym_art_amd.policy import MLPCritic
    from tests.mlp_ref import _scaled_layers
    layers = _scaled_layers([48, 16], env.obs_dim, seed)
    W, b = layers[-1]
    return MLPCritic(env, layers[:-1] + [(W[:1], b[:1])], "tanh")


@pytest.mark.parametrize("layout", ["alias", "plain"])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_every_form_and_asking_for_more_changes_no_other_bit(cell, layout):
    """plain, values=, logp=, everything, and critic= (on a policy without a value head): observations, rewards, dones, actions,
    terminal rows, h and c are the plain call's bits; the critic's values are the critic's own on the raw observations"""
    import torch
    asks = [dict(values=False, logp=False, term=False), dict(values=True, logp=False, term=False),
            dict(values=False, logp=True, term=False), dict(values=True, logp=True, term=True),
            dict(values=True, logp=True, term=True, critic=True)]
    ws = []
    for ask in asks:
        with_critic = ask.pop("critic", False)
        env, net, pol = _fresh(cell, layout, value=not with_critic)
        cr = _critic(env) if with_critic else None
        ws.append(_window(env, pol, net, critic=cr, **ask))
        d = ws[-1]["d"]
        assert bool((d.to(torch.int32).sum(dim=0) == 1).all()) and bool(d[15].any())     # every env ended by the time limit
        if cr is not None:
            w = ws[-1]
            seen = torch.cat([w["o0"][None], w["o"]])                # the raw observations, not the features
            assert torch.equal(cr.values_dev(seen.reshape(-1, seen.shape[-1])).reshape(T + 1, -1).view(torch.int32), w["v"].view(torch.int32))
            assert torch.equal(cr.values_dev(w["tt"])[d[15] != 0].view(torch.int32), w["tv"][15][d[15] != 0].view(torch.int32))
        for x in (cr, pol, env):
            if x is not None:
                x.close()
    for w in ws[1:]:
        _same(ws[0], w, "ask", keys=("o", "r", "d", "a", "tt"))
    assert torch.equal(ws[1]["v"], ws[3]["v"]) and torch.equal(ws[2]["lp"], ws[3]["lp"]) and torch.equal(ws[2]["lp"], ws[4]["lp"])
    assert bool(torch.isfinite(ws[4]["v"]).all()) and not torch.equal(ws[4]["v"], ws[3]["v"])    # the critic's V, not the head's
    for w in ws[3:]:
        assert bool((w["tv"].view(torch.int32)[w["d"] == 0] == 0).all()) and bool((w["tv"][w["d"] != 0] != 0).all())


# ---- 3. existing paths --------------------------------------------------------------------------------------------------------------
class _RawPolicy:
    """a handle made with the entry points a policy without an encoder always used, for rollout_policy_dev"""

    def __init__(self, env, net, create="gaq_policy_create_rnn", desc=None):
        import torch
        from gym_art_amd.policy import pack_gru_weights
        self.lib = _lib.load()
        widths = [net.H] + list(net.head)
        cell_id = 1 if net.cell == "gru" else 3
        d = desc if desc is not None else _desc_rnn(widths, cell=cell_id, in_dim=net.weights[0].shape[1])
        d.hidden_act, d.out_tanh = (0 if net.act == "tanh" else 1), int(net.out_tanh)
        h = C.c_void_p()
        _lib.check(getattr(self.lib, create)(env._handle, C.byref(d), C.byref(h)))
        self.handle, self.env_handle = h, _lib.handle_value(env._handle)
        packed = pack_gru_weights(net.weights, net.layers)          # (named: _lib.ptr keeps no reference to its array)
        _lib.check(self.lib.gaq_policy_set_weights(h, _lib.ptr(packed)))
        self.hidden = torch.zeros((env.num_envs, net.H), device=_dev())
        _lib.check(self.lib.gaq_policy_set_hidden_dev(h, _lib.ptr(self.hidden)))
        if net.cell == "lstm":
            self.cell = torch.zeros((env.num_envs, net.H), device=_dev())
            _lib.check(self.lib.gaq_policy_set_cell_dev(h, _lib.ptr(self.cell)))
        ls = np.asarray(LOG_STD, np.float32)
        _lib.check(self.lib.gaq_policy_set_explore(h, _lib.ptr(ls)))
        wb = np.concatenate([net.value[0], [net.value[1]]]).astype(np.float32)
        _lib.check(self.lib.gaq_policy_set_value_head(h, _lib.ptr(wb)))

    def set_hidden(self, *states):
        import torch
        for t, s in zip([self.hidden] + ([self.cell] if hasattr(self, "cell") else []), states):
            t.copy_(torch.as_tensor(s))

    def close(self):
        self.lib.gaq_policy_destroy(self.handle)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_without_an_encoder_it_is_the_old_path_bit_for_bit(cell):
    """GRUPolicy / LSTMPolicy(...) by keywords, the same call by position, and a handle made with gaq_policy_create_rnn by hand: the
    same bytes on the same seed"""
    case = ("gru", (16,), 18, 48, (32,), "relu", True, 132, "alias", False) if cell == "gru" else \
        ("lstm", (16,), 18, 48, (32,), "tanh", False, 132, "alias", False)
    ws = []
    for how in ("keywords", "positional", "by hand"):
        env = _env(18, 132)
        net = _Net(case, env)
        net.weights = _cell(cell, net.H, 18, 7)                    # the cell on the observation
        if how == "keywords":
            pol = net.build(env, encoder=False)
        elif how == "positional":
            from gym_art_amd.policy import GRUPolicy, LSTMPolicy
            pol = (GRUPolicy if cell == "gru" else LSTMPolicy)(env, net.weights, net.layers, net.act, net.out_tanh, LOG_STD, net.value)
        else:
            pol = _RawPolicy(env, net)
        assert _lib.load().gaq_policy_encoder_width(pol.handle) == 0
        ws.append(_window(env, pol, net))
        pol.close(); env.close()
    _same(ws[0], ws[1], "positional")
    _same(ws[0], ws[2], "by hand")


def test_encoder_width_is_zero_without_an_encoder():
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPPolicy
    from tests.policy_util import _layers
    lib = _lib.load()
    env = _env(18, 64)
    pols = [MLPPolicy.from_arrays(env, _layers([16]), engine=e) for e in ("valu", "mfma", "bf16")]
    pols += [GRUPolicy(env, _cell("gru", 16, 18), _head(16)), LSTMPolicy(env, _cell("lstm", 16, 18), _head(16))]
    for p in pols:
        assert lib.gaq_policy_encoder_width(p.handle) == 0
    with_enc = GRUPolicy.with_encoder(env, _encoder(18, (32, 48)), _cell("gru", 16, 48), _head(16))
    assert lib.gaq_policy_encoder_width(with_enc.handle) == 48 and with_enc.encoder_widths == (32, 48)
    got = with_enc.get_encoder_weights()
    for (W, b), (W2, b2) in zip(_encoder(18, (32, 48)), got):
        assert np.array_equal(W, W2) and np.array_equal(b, b2)
    for p in pols + [with_enc]:
        p.close()
    env.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def _err():
    return _lib.load().gaq_last_error().decode()


def test_create_refusals_on_the_device():
    lib = _lib.load()
    env = _env(18, 64)
    h = C.c_void_p()
    assert lib.gaq_policy_create_rnn_enc(env._handle, C.byref(_desc_enc([16], (48,), enc_in=19)), C.byref(h)) == -1
    assert "encoder" in _err() and "obs_dim" in _err() and not h.value
    for d, word in ((_desc_enc([16], (24,)), "enc_width"), (_desc_enc([16], (48, 48, )), None), (_desc_enc([16], (48,), in_dim=18), "last width")):
        if word is None:
            d.enc_layers = 3
            word = "enc_layers"
        assert lib.gaq_policy_create_rnn_enc(env._handle, C.byref(d), C.byref(h)) == -1 and "encoder" in _err() and word in _err()
    d = _desc_enc([16], (48,))
    d.struct_size -= 4
    assert lib.gaq_policy_create_rnn_enc(env._handle, C.byref(d), C.byref(h)) == -1 and "encoder" in _err()
    env.close()


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_refusals_launch_nothing_and_leave_the_bits(cell):
    import torch
    from gym_art_amd.policy import AdamDev, GRUPolicy
    lib = _lib.load()
    case = BITS[cell]
    D, n = case[2], 132
    # (a) encoder weights never set: the rollout is refused and launches nothing
    env, twin = _env(D, n), _env(D, n)
    net = _Net(case, env)
    _reset_obs(twin)
    raw = _RawPolicy(env, net, "gaq_policy_create_rnn_enc", _desc_enc([net.H] + list(net.head), net.enc_w, D, 1 if cell == "gru" else 3))
    raw.set_hidden(*net.state0(n))
    before = [s.clone() for s in _states(raw)]
    o, r, d, a = _bufs(env, 4)
    a.fill_(float("nan"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gaq_step_policy_many_dev(env._handle, raw.handle, 4, _lib.ptr(o), _lib.ptr(r), _lib.ptr(d), _lib.ptr(a), st) == -1
    assert "encoder weights not set" in _err()
    with pytest.raises(ValueError, match="encoder weights not set"):
        env.rollout_policy_dev(raw, o, r, d, a, values=_nan(5, n))
    host = np.empty(lib.gaq_policy_encoder_weight_count(C.byref(_desc_enc([net.H] + list(net.head), net.enc_w, D))), np.float32)
    assert lib.gaq_policy_get_encoder_weights(raw.handle, _lib.ptr(host)) == -1 and "encoder weights not set" in _err()
    torch.cuda.synchronize()
    assert bool(torch.isnan(a).all()) and all(torch.equal(x, y) for x, y in zip(before, _states(raw)))
    acts = torch.rand((4, n, 4), device=_dev()) * 2 - 1             # nothing moved: the env and its twin step alike
    o1, r1, d1, _ = _bufs(env, 4)
    o2, r2, d2, _ = _bufs(twin, 4)
    env.step_many_dev(acts, o1, r1, d1)
    twin.step_many_dev(acts, o2, r2, d2)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    # ... and once they are set it is the policy the Python constructor builds
    from gym_art_amd.policy import pack_encoder_weights
    packed = pack_encoder_weights(net.enc)
    _lib.check(lib.gaq_policy_set_encoder_weights(raw.handle, _lib.ptr(packed)))
    raw.close(); env.close(); twin.close()
    # (b) what is out of scope is refused by name, and the handle computes the bits of a handle that was never asked
    ws = []
    for ask in (False, True):
        env, net, pol = _fresh(cell, "alias")
        if ask:
            S, H = 8, net.H
            obs, acts = torch.zeros((3, S, D), device=_dev()), torch.zeros((3, S, 4), device=_dev())
            dn = torch.zeros((3, S), dtype=torch.uint8, device=_dev())
            s0 = [torch.zeros((S, H), device=_dev()) for _ in _states(pol)]
            z = torch.zeros((3, S), device=_dev())
            idx = torch.arange(S, dtype=torch.int32, device=_dev())
            grads = (pol.ppo_seq_grad_dev, pol.ppo_seq_grad_idx_dev) if cell == "gru" else (pol.ppo_bptt_grad_dev, pol.ppo_bptt_grad_idx_dev)
            with pytest.raises(ValueError, match="encoder"):
                pol.evaluate_seq_dev(obs, acts, dn, *s0)
            with pytest.raises(ValueError, match="encoder"):
                grads[0](obs, acts, dn, *s0, z, z, z)
            with pytest.raises(ValueError, match="encoder"):
                grads[1](idx, obs, acts, dn, *s0, z, z, z)
            with pytest.raises(ValueError, match="encoder"):
                AdamDev(pol)
            with pytest.raises(ValueError, match="encoder"):
                pol.set_encoder_weights(_encoder(D, (16,)))         # other widths
            plain = GRUPolicy(env, _cell("gru", 16, D), _head(16))
            with pytest.raises(ValueError, match="no encoder"):
                plain.set_encoder_weights(net.enc)
            four = np.zeros(4, np.float32)
            assert lib.gaq_policy_set_encoder_weights(plain.handle, _lib.ptr(four)) == -1 and "no encoder" in _err()
            plain.close()
        ws.append(_window(env, pol, net))
        pol.close(); env.close()
    _same(ws[0], ws[1], "after the refusals")
