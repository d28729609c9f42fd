"""The four copied actor-critic kernels (policy_mfma_ac_kernel, policy_gru_ac_kernel, policy_mfma_term_kernel, policy_gru_term_kernel) and
term_gather_kernel at the shapes tests/test_gpu_policy_shapes.py pins the plain engines at: every observation width the env offers (0 to
3 padded rows, an odd number of k-steps, swarm widths up to 108), a single partial tile, one full tile, a tile plus a sliver and 32 tiles
plus a tail, last layers of 16 to 256 units (per-wave value chains of 4, 12, 20, 36 and 64 units; waves that own no chunk), and the GRU
engine's largest footprint plus the value parts.  Then the gather at done counts of 1, 2, 64, 65, 66, 128 and 129 per step, and a
captured actor-critic rollout replayed against an eager twin.

Values, log-probabilities and terminal values are held to the fp64 references of tests/ac_ref.py and tests/term_ref.py on the device's
recorded observations, dones and terminal rows, at the bars of tests/test_gpu_policy_shapes.py (ATOL_FP32 = 1.5e-5 for the MLP engine,
ATOL_GRU = 4e-6 for the GRU engine: a value is one more output sum) and the derived log-probability bar of ac_ref.logp64.  Every case
asserts that it has teeth and leaves no element out.

Each case prints the worst |V - V_ref|, log-probability error / bar and |V_term - V_ref| of its observation width so far.
FIGURES: not yet measured on an MI355X; the bars above are the project's own."""
import numpy as np
import pytest

from tests import ac_ref, term_ref
from tests.mlp_ref import assert_not_saturated
from tests.policy_util import _bufs, _dev
from tests.test_gpu_policy_ac import LOG_STD, T, _ac_bufs, _Net
from tests.test_gpu_policy_shapes import OBS, _batches, _kw, _obs_scale
from tests.test_gpu_policy_term import _one_done_each, _start, _term_buf, _tv_buf, _window, _zeros_are_plus_zero

pytestmark = pytest.mark.gpu

MLP_NETS = [[16], [80, 48], [144], [240, 80], [48, 256, 16], [256, 256, 256]]
GRU_H, GRU_HEADS = [48, 80, 240], [(), (48,), (16, 80)]
# alias layout at every width; the plain layout at D = 18 and D = 19
CASES = [(obs, "alias") for obs in OBS] + [(obs, "plain") for obs in OBS if obs[2] in (18, 19)]

_WORST = {}                                      # (kind, D) -> [values, logp / bar, terminal values]


def _env(obs, n, layout="alias", graph_safe=False):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(**dict(_kw(obs, n), alias_obs=layout == "alias"))
    assert env.obs_dim == obs[2], (obs, env.obs_dim)
    if graph_safe:
        env.set_graph_safe(True)
    return env


def _specs(kind, D):
    """[(spec, k)] of the nets of one kind at observation width D: _Net takes its activation and output tanh from _style(k)"""
    if kind == "mlp":
        return [(("mlp", widths), k + D) for k, widths in enumerate(MLP_NETS)]
    return [(("gru", H, GRU_HEADS[(j + D) % 3]), j + D) for j, H in enumerate(GRU_H)]


def _term_check(net, w, n, what, at=None):
    """the terminal values of a window against fp64 on the captured rows, +0.0 everywhere else; returns the worst error"""
    at = _one_done_each(w["d"], what) if at is None else at
    _zeros_are_plus_zero(w["tv"], w["d"], what)
    rows = w["tt"].cpu().numpy()
    assert np.isfinite(rows).all(), what                            # each env's one terminal row
    atn = at.cpu().numpy()
    got = w["tv"].cpu().numpy()[atn, np.arange(n)].astype(np.float64)
    if net.kind == "mlp":
        ref = term_ref.mlp_term_values64(net, rows)
    else:
        ref = term_ref.gru_term_values64(net, w["o0"].cpu().numpy(), w["o"].cpu().numpy(), w["d"].cpu().numpy(),
                                         w["h0"].cpu().numpy().astype(np.float64), atn, rows)
    assert np.isfinite(ref).all(), what
    assert float(np.mean(np.abs(ref) > net.atol)) > 0.9, what       # teeth: the values are not all within the bar of zero
    nxt = w["o"].cpu().numpy()[atn, np.arange(n)]                   # teeth: the terminal row is not the new episode's first row
    assert float(np.mean(np.abs(nxt - rows).max(axis=1) > 1e-3)) > 0.9, what
    err = float(np.max(np.abs(got - ref)))
    assert err <= net.atol, (what, "terminal values", err)
    return err


def _check(net, w, n, what):
    """values, log-probabilities and terminal values of an aligned window against fp64; returns the three worst figures"""
    assert int(w["d"][:-1].sum()) > 0, what
    hidden = []
    means, vref, z = net.reference(w["o0"], w["o"], w["d"], hidden)
    assert_not_saturated(z, hidden, net.act, what)
    assert vref.shape == (T + 1, n) and float(np.mean(np.abs(vref) > net.atol)) > 0.9, what
    verr = float(np.max(np.abs(w["v"].cpu().numpy().astype(np.float64) - vref)))
    ref, bar = ac_ref.logp64(w["a"].cpu().numpy(), means, LOG_STD, mean_atol=net.atol)
    lerr = np.abs(w["lp"].cpu().numpy().astype(np.float64) - ref)
    assert lerr.shape == (T, n) and np.isfinite(lerr).all(), what
    frac = float((lerr / bar).max())
    assert verr <= net.atol, (what, "values", verr)
    assert (lerr <= bar).all(), (what, "logp error / bar", frac)
    return verr, frac, _term_check(net, w, n, what)


def _plain_twin_check(obs, layout, n, net, w, what):
    """asking changed nothing else: a twin with the same seed and the same calls, its rollout a plain one"""
    import torch
    twin = _env(obs, n, layout)
    _obs_scale(twin)
    pt = net.build(twin)
    _start(twin, pt, "aligned")
    tt = _term_buf(twin)
    twin.set_terminal_obs(tt)
    o, r, d, a = _bufs(twin, T)
    twin.rollout_policy_dev(pt, o, r, d, a)
    torch.cuda.synchronize()
    for key, x in (("o", o), ("r", r), ("d", d), ("a", a), ("tt", tt)):
        assert torch.equal(w[key], x), (what, key)
    if net.kind == "gru":
        assert torch.equal(pt.hidden, w["hidden"]), what
    pt.close(); twin.close()


def _run_case(obs, layout, n, kind, specs):
    """each net on an env of its own (so that a twin with the same calls exists): one aligned window with everything asked for"""
    D = obs[2]
    worst = _WORST.setdefault((kind, D), [0.0, 0.0, 0.0])
    for spec, k in specs:
        env = _env(obs, n, layout)
        net = _Net(spec, _obs_scale(env), k, D)
        pol = net.build(env)
        what = "%s %s %d d=%d %s n=%d" % (spec, net.act, net.out_tanh, D, layout, n)
        w = _window(env, pol, "aligned")
        if net.kind == "gru":
            w["hidden"] = pol.hidden.clone()
        figures = _check(net, w, n, what)
        for j in range(3):
            worst[j] = max(worst[j], figures[j])
        if n <= 64:                                                 # a single partial tile and one full tile
            _plain_twin_check(obs, layout, n, net, w, what)
        pol.close(); env.close()
    print("%s d=%d %s n=%d: worst so far at this width |V - V_ref| %.3g, logp error / bar %.3g, |V_term - V_ref| %.3g (bar %.3g)"
          % (kind, D, layout, n, worst[0], worst[1], worst[2], net.atol))


# ---- 1. the four copied kernels at the plain engines' edge shapes ---------------------------------------------------------------
_CB = [(case, j) for case in CASES for j in range(4)]
_CB_IDS = ["d%d-%s-b%d" % (obs[2], layout, j) for (obs, layout), j in _CB]


@pytest.mark.parametrize("case,j", _CB, ids=_CB_IDS)
def test_mlp_values_logp_and_terminal_values_against_fp64(case, j):
    """policy_mfma_ac_kernel and policy_mfma_term_kernel: batch j of _batches (q, 64, 64 + q, 2096), the six nets"""
    obs, layout = case
    _run_case(obs, layout, _batches(obs[1])[j], "mlp", _specs("mlp", obs[2]))


@pytest.mark.parametrize("case,j", _CB, ids=_CB_IDS)
def test_gru_values_logp_and_terminal_values_against_fp64(case, j):
    """policy_gru_ac_kernel and policy_gru_term_kernel: batch j of _batches, H of 3, 5 and 15 chunks, the heads in turn"""
    obs, layout = case
    _run_case(obs, layout, _batches(obs[1])[j], "gru", _specs("gru", obs[2]))


@pytest.mark.parametrize("n", [16, 2096])
def test_gru_largest_actor_critic_footprint(n):
    """H = 256 on a 16-agent swarm's 108 inputs: the GRU engine's 156 KiB of LDS and the 1 KiB of value parts, 157 KiB of the 160 KiB"""
    _run_case(OBS[-1], "alias", n, "gru256", [(("gru", 256, (48,)), 3 + 108)])


# ---- 2. done counts the gather has not seen ---------------------------------------------------------------------------------------
N_GATHER = 130                                   # three gather waves, three policy tiles, the last of 2 envs
GATHER_NETS = [("mlp", [240, 80]), ("gru", 48, (16, 80))]
MASKS = {"first": [0], "last": [129], "lane63": [63, 127], "first64": list(range(64)), "first65": list(range(65)),
         "all-but-first": list(range(1, 130))}


@pytest.mark.parametrize("mask_id", list(MASKS))
@pytest.mark.parametrize("spec", GATHER_NETS, ids=["mlp240-80", "gru48-16-80"])
def test_gather_at_done_counts_of_1_to_129(spec, mask_id):
    """staggered regime with a chosen mask: the unmasked envs finish in window step 10, the masked ones in step 15.  The terminal
    values against fp64, and the window as twenty T = 1 calls (each re-zeroes the two counters and uses counter 0 only) bit-equal"""
    import torch
    n, k = N_GATHER, GATHER_NETS.index(spec)
    mask = np.zeros(n, bool)
    mask[MASKS[mask_id]] = True
    env, twin = _env(OBS[2], n), _env(OBS[2], n)
    net = _Net(spec, _obs_scale(env), k)
    _obs_scale(twin)
    pol, pt = net.build(env), net.build(twin)
    what = "%s %s n=%d" % (spec, mask_id, n)
    w = _window(env, pol, "staggered", mask=mask)
    at = _one_done_each(w["d"], what)
    counts = w["d"].to(torch.int32).sum(dim=1).cpu().numpy()
    want = np.zeros(T, np.int64)
    want[10], want[15] = n - int(mask.sum()), int(mask.sum())
    assert np.array_equal(counts, want), (what, counts)
    assert np.array_equal(at.cpu().numpy(), np.where(mask, 15, 10)), what
    err = _term_check(net, w, n, what, at)
    print("%s: dones per step %d and %d, worst |V_term - V_ref| %.3g (bar %.3g)" % (what, want[10], want[15], err, net.atol))
    # the same window in twenty calls of one step
    _start(twin, pt, "staggered", mask)
    tt = _term_buf(twin)
    twin.set_terminal_obs(tt)
    o, r, d, a = _bufs(twin, T)
    lp = torch.full((T, n), float("nan"), device=_dev())
    tv = _tv_buf(twin)
    v = torch.full((T + 1, n), float("nan"), device=_dev())
    for t in range(T):
        v1, lp1 = _ac_bufs(twin, 1)                                 # (of their own: row t of a [T, 130] tensor is 16-byte aligned
        tv1 = _tv_buf(twin, 1)                                      # for even t only, and the call asks that of what it is given)
        twin.rollout_policy_dev(pt, o[t:t + 1], r[t:t + 1], d[t:t + 1], a[t:t + 1], values=v1, logp=lp1, term_values=tv1)
        if t:
            assert torch.equal(v[t], v1[0]), (what, t)              # the bootstrap row IS the next call's row 0
        v[t:t + 2], lp[t], tv[t] = v1, lp1[0], tv1[0]
    torch.cuda.synchronize()
    for key, x in (("o", o), ("r", r), ("d", d), ("a", a), ("v", v), ("lp", lp), ("tt", tt)):
        assert torch.equal(w[key], x), (what, key)                  # (no NaN left in them: equal means bit-equal)
    assert torch.equal(w["tv"].view(torch.int32), tv.view(torch.int32)), what
    if net.kind == "gru":
        assert torch.equal(pol.hidden, pt.hidden), what
    for x in (pol, pt, env, twin):
        x.close()


# ---- 3. a captured actor-critic rollout ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["alias", "plain"])
@pytest.mark.parametrize("spec", GATHER_NETS, ids=["mlp240-80", "gru48-16-80"])
def test_graph_captured_actor_critic_rollout(spec, layout):
    """graph-safe mode: one captured 8-step rollout with values, log-probabilities and terminal values, replayed three times, equals
    three eager calls on a twin bit for bit -- every output, and .hidden for the GRU.  Episodes are 16 steps: each env finishes in
    the replays, and every done is seen."""
    import torch
    n, steps, k = 68, 8, GATHER_NETS.index(spec)
    graphed, eager = _env(OBS[2], n, layout, True), _env(OBS[2], n, layout, True)
    net = _Net(spec, _obs_scale(graphed), k)
    _obs_scale(eager)
    pols = [net.build(graphed), net.build(eager)]
    bufs, kws = [], []
    for e, p in zip((graphed, eager), pols):
        o0 = torch.empty((n, 18), device=_dev())
        e.reset_dev(o0)
        if net.kind == "gru":
            p.reset_hidden()
        e.set_terminal_obs(_term_buf(e))
        bufs.append(_bufs(e, steps))
        v, lp = _ac_bufs(e, steps)
        kws.append(dict(values=v, logp=lp, term_values=_tv_buf(e, steps)))
    torch.cuda.synchronize()

    def same(what):
        for x, y in zip(bufs[0], bufs[1]):
            assert torch.equal(x, y), what
        for key in ("values", "logp", "term_values"):               # finite everywhere once written: bit-equal
            assert bool(torch.isfinite(kws[0][key]).all()), (what, key)
            assert torch.equal(kws[0][key].view(torch.int32), kws[1][key].view(torch.int32)), (what, key)
        if net.kind == "gru":
            assert torch.equal(pols[0].hidden, pols[1].hidden), what

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
    for rep in range(3):
        for kw in kws:
            for key in ("values", "logp", "term_values"):
                kw[key].fill_(float("nan"))
        g.replay()
        eager.rollout_policy_dev(pols[1], *bufs[1], **kws[1])
        torch.cuda.synchronize()
        same("replay %d" % rep)
        d, tv = bufs[0][2], kws[0]["term_values"]
        assert bool((tv.view(torch.int32)[d == 0] == 0).all()), rep
        if int(d.sum()):
            assert float((tv[d != 0].abs() > net.atol).double().mean()) > 0.9, rep          # every done has its terminal value
        dones += d.to(torch.int32).sum(dim=0)
    assert bool((dones >= 1).all()), dones.cpu().tolist()           # every env finished inside the replays
    for x in pols + [graphed, eager]:
        x.close()
