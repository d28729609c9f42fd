"""The three separate-critic kernels (critic_mfma_kernel, critic_mfma_term_kernel and the fused policy_mfma_critic_kernel) and the critic's
branch of the host's policy_rollout at the shapes they branch on -- the shapes tests/test_gpu_policy_shapes.py and
tests/test_gpu_policy_ac_shapes.py pin the other engines at:
 a. values_dev at every observation width the env offers (0 to 3 padded rows, an odd number of k-steps, in_dim sizing the LDS at 108),
    M = 1, 63, 64, 65, 130 rows, last widths of 16 to 256, narrow after wide, both activations; a 4-byte-aligned input bit-equal;
 b. rollouts with an MLP actor (the fused kernel) and with a GRU actor (the batch kernel after every step) at every width, a single
    partial tile, one full tile, a tile plus a sliver and 32 tiles plus a tail, the (actor, critic) pairs rotated with the width;
 c. actor and critic with different activations, all four mixes with the output tanh on and off, fused and in two launches, with
    the fused launch's LDS sized by in_dim, by the actor, by the critic and by both (MIX);
 d. the GRU engine's largest footprint (H = 256 on 108 inputs) followed by critic launches;
 e. the gather at done counts of 1, 2, 64, 65, 66, 128 and 129 per step with a critic reading the list (one of them above 64 KiB);
 f. a captured rollout with a critic (two or three launches per step) replayed against an eager twin;
 g. every subset of the outputs the host branches on, bit-equal to the call that asks for everything, nothing else written.
tests/test_policy_critic_shapes_cpu.py asserts from the LDS formulas that the tables below contain what this text claims.

V and terminal values are held to _CNet.ref64 (float64 on the recorded rows) at ATOL_FP32 = 1.5e-5, log-probabilities to
ac_ref.logp64's derived bar with the actor's fp64 means (known to ATOL_FP32 for an MLP actor, ATOL_GRU for a GRU): the project's own
bars, none new.  |V_ref| is held to the range tests/test_gpu_policy_critic.py sees by construction: ac_ref.value_head for the last layer,
_obs_scale folded into the first.  Every case asserts that it has teeth (more than 0.9 of |V_ref| above the bar, hidden units not
saturated), leaves no element out, and that every env finishes inside the window (T = 20 at ep_time=0.15).

Each case prints the worst |V - V_ref|, log-probability error / bar and |V_term - V_ref| of its observation width so far.
FIGURES (MI355X): 146 passed in 24.9 s, the slowest case 0.79 s.  Worst per observation width over every case of the width (bar for
V and V_term: 1.5e-5; the log-probability error as a fraction of its bar):
  D     values_dev   MLP actor: |V-V_ref|  logp/bar  |V_term-V_ref|   GRU actor: |V-V_ref|  logp/bar  |V_term-V_ref|
  13    5.7e-07      9.28e-07              0.128     9.01e-07         1.02e-06              0.136     1.04e-06
  14    4.4e-07      9.1e-07               0.045     8.86e-07         1.1e-06               0.080     1.3e-06
  18    4.8e-07      1.14e-06              0.063     1.14e-06         6.69e-07              0.129     6.04e-07
  19    6.3e-07      7.84e-07              0.044     6.45e-07         1.02e-06              0.096     1.03e-06
  20    5.4e-07      8.76e-07              0.037     7.5e-07          9.94e-07              0.079     9.27e-07
  22    4.8e-07      1.65e-06              0.083     1.15e-06         6.05e-07              0.074     6.91e-07
  25    4.6e-07      1.53e-06              0.034     1.54e-06         8.64e-07              0.091     1.06e-06
  24    5.5e-07      1.44e-06              0.077     1.51e-06         6.22e-07              0.115     4.9e-07
  36    5e-07        9.12e-07              0.052     9.68e-07         7.68e-07              0.093     8.1e-07
  60    4.5e-07      7.16e-07              0.054     9.35e-07         7.09e-07              0.108     8.5e-07
  108   5.2e-07      2.47e-06              0.047     1.87e-06         7.72e-07              0.093     1e-06
(D = 18 and 108 include the mixed-activation cases, D = 108 the H = 256 GRU.)  The captured rollout with the 256-wide critic captures
and replays: raising the LDS attribute before every launch is accepted during capture.
MUTANTS (wrong arithmetic only, built apart, run on an MI355X):
 1. policy_mfma_critic_kernel hands the critic's mfma_hidden a copy of cr.trunk with the actor's hidden_act: this file fails in 66 of
    146 cases (all 52 of the MLP rollouts, all 8 of c, the 6 MLP cases of e); tests/test_gpu_policy_critic.py passes all 29 -- its
    pairs never mix activations.
 2. critic_ac points wv one float into the value layer, the bias read from the old last weight: this file fails in 140 of 146 cases
    (all but the captured rollouts, which compare two runs of the same library); tests/test_gpu_policy_critic.py fails in 11 of 29."""
import numpy as np
import pytest

from tests import ac_ref
from tests.mlp_ref import assert_not_saturated
from tests.policy_util import _bufs, _dev
from tests.test_gpu_policy_ac import LOG_STD, T, _ac_bufs, _Net, _same, _style
from tests.test_gpu_policy_ac_shapes import CASES, GATHER_NETS, MASKS, N_GATHER, _env, _plain_twin_check, _specs
from tests.test_gpu_policy_critic import ACTS, _close, _CNet, _window
from tests.test_gpu_policy_shapes import ATOL_FP32, ATOL_GRU, OBS, OBS_IDS, _batches, _obs_scale
from tests.test_gpu_policy_term import _one_done_each, _start, _term_buf, _tv_buf, _zeros_are_plus_zero

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 130)
# (a): last widths of 1, 9, 5, 1 and 16 chunks (per-wave value chains of 4, 36, 20, 4 and 64 units), narrow after wide
VALUE_TRUNKS = [[16], [144], [240, 80], [48, 256, 16], [256, 256, 256]]
# (b): the critics the pairs rotate through: last widths 16, 144, 80, 16, 256, 48, 240, 256
CRITICS = [[16], [144], [240, 80], [48, 256, 16], [256, 256, 256], [48], [80, 240], [256, 256]]
# (c): (which term sizes the fused launch's LDS, observation, actor widths, critic widths); each with the actor styles MIX_STYLES
# (_style: tanh / relu, output tanh on / off) and both critic activations
MIX = [("in_dim", OBS[-1], [16], [48]), ("actor", OBS[2], [256, 256, 256], [16]), ("critic", OBS[2], [16], [256, 256]),
       ("both", OBS[-1], [256], [256])]
MIX_STYLES = [0, 1, 2, 3]
# (d)
BIG_GRU, BIG_GRU_CRITICS = ("gru", 256, (48,)), [[256, 256, 256], [16]]
# (e): the actors are GATHER_NETS of tests/test_gpu_policy_ac_shapes.py (an MLP: the fused kernel; a GRU)
GATHER_CRITICS = [[240, 80], [256, 256]]
# (f), (g): (actor, critic widths, fused)
GRAPH_PAIRS = [(("mlp", [240, 80]), [240, 80], True), (("mlp", [240, 80]), [240, 80], False), (("gru", 48, (16, 80)), [256, 256], True)]
GRAPH_IDS = ["mlp240-80+c240-80-fused", "mlp240-80+c240-80-two", "gru48-16-80+c256x2"]
SUBSET_PAIRS = [(("mlp", [240, 80]), [256, 256], True), (("mlp", [240, 80]), [256, 256], False), (("gru", 80, (48,)), [144], True)]
SUBSET_IDS = ["mlp240-80+c256x2-fused", "mlp240-80+c256x2-two", "gru80-48+c144"]
SUBSETS = [("lp",), ("tv",), ("lp", "tv"), ("v",), ("v", "tv")]

_WORST = {}                                      # (kind, D) -> [values, logp / bar, terminal values]


def _pairs(kind, D):
    """[(actor spec, its k, critic widths, its k)] of the rollouts at observation width D: four of the six MLP nets of
    tests/test_gpu_policy_ac_shapes.py, or its three GRU nets, and the critics, rotated with the position i of D in OBS (so that no two
    widths share a table).  The activations come from the k's (_style, ACTS[k % 2]): the critic's parity is D + (j >> 1) against the
    actor's D + i + j (MLP) or D + j (GRU), so at every width some pairs share an activation and some do not"""
    i = [obs[2] for obs in OBS].index(D)
    specs = _specs(kind, D)
    if kind == "mlp":
        specs = [specs[(i + j) % len(specs)] for j in range(4)]
    shift = 0 if kind == "mlp" else 4
    return [(spec, k, CRITICS[(3 * i + shift + j) % len(CRITICS)], 200 + 2 * (D + j) + ((D + (j >> 1)) & 1)) for j, (spec, k) in enumerate(specs)]


def _term_check(cnet, crit, w, n, what, at=None):
    """the terminal values of a window: values_dev of the captured rows bit for bit, within the bar of fp64, +0.0 everywhere else;
    returns the worst error"""
    import torch
    at = _one_done_each(w["d"], what) if at is None else at
    _zeros_are_plus_zero(w["tv"], w["d"], what)
    assert bool(torch.isfinite(w["tt"]).all()), what                # each env's one terminal row
    idx = torch.arange(n, device=_dev())
    got = w["tv"][at, idx]
    assert torch.equal(got, crit.values_dev(w["tt"])), (what, "terminal values != values_dev")
    ref = cnet.ref64(w["tt"].cpu().numpy(), what + " terminal rows")
    assert ref.shape == (n,) and float(np.mean(np.abs(ref) > ATOL_FP32)) > 0.9, what       # teeth
    nxt = w["o"][at, idx]                                           # teeth: the terminal row is not the new episode's first row
    assert float(((nxt - w["tt"]).abs().max(dim=1).values > 1e-3).float().mean()) > 0.9, what
    err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - ref)))
    assert err <= ATOL_FP32, (what, "terminal values", err)
    return err


def _check(net, cnet, crit, w, n, what):
    """values, log-probabilities and terminal values of an aligned window; returns the three worst figures"""
    import torch
    rows = torch.cat([w["o0"][None], w["o"]])                       # row t: what action t (and value t) saw; row T: where the call ends
    alone = crit.values_dev(rows)
    torch.cuda.synchronize()
    assert w["v"].shape == (T + 1, n) and bool(torch.isfinite(w["v"]).all()), what
    assert torch.equal(w["v"], alone), (what, "values != values_dev")
    vref = cnet.ref64(rows.cpu().numpy(), what)                     # (asserts that the critic's hidden units are not saturated)
    assert vref.shape == (T + 1, n) and float(np.mean(np.abs(vref) > ATOL_FP32)) > 0.9, what
    verr = float(np.max(np.abs(w["v"].cpu().numpy().astype(np.float64) - vref)))
    hidden = []
    means, _, z = net.reference(w["o0"], w["o"], w["d"], hidden)    # the actor's fp64 means (its value head is not on the device)
    assert_not_saturated(z, hidden, net.act, what)
    ref, bar = ac_ref.logp64(w["a"].cpu().numpy(), means, LOG_STD, mean_atol=net.atol)
    lerr = np.abs(w["lp"].cpu().numpy().astype(np.float64) - ref)
    assert lerr.shape == (T, n) and np.isfinite(lerr).all(), what
    frac = float((lerr / bar).max())
    assert verr <= ATOL_FP32, (what, "values", verr)
    assert (lerr <= bar).all(), (what, "logp error / bar", frac)
    return verr, frac, _term_check(cnet, crit, w, n, what)


def _rollout_case(obs, layout, n, spec, k, cw, kc, cact=None, fused=True, twin=False):
    """one (actor, critic) pair on an env of its own: an aligned window with values, logp and term_values from the critic, checked;
    returns the window"""
    D = obs[2]
    env = _env(obs, n, layout)
    scale = _obs_scale(env)
    net, cnet = _Net(spec, scale, k, D), _CNet(cw, scale, kc, D, cact)
    assert net.atol == (ATOL_FP32 if net.kind == "mlp" else ATOL_GRU)
    pol, crit = net.build(env, value=False), cnet.build(env, fused)
    what = "%s %s %d + critic %s %s%s d=%d %s n=%d" % (spec, net.act, net.out_tanh, cw, cnet.act, "" if fused else " (two launches)", D, layout, n)
    w = _window(env, pol, crit)
    if net.kind == "gru":
        w["hidden"] = pol.hidden.clone()
    figures = _check(net, cnet, crit, w, n, what)
    worst = _WORST.setdefault((net.kind, D), [0.0, 0.0, 0.0])
    for j in range(3):
        worst[j] = max(worst[j], figures[j])
    if twin:                                                        # a plain rollout on a twin: asking changed nothing else
        _plain_twin_check(obs, layout, n, net, w, what)
    _close(pol, crit, env)
    return w


def _masked_window(env, pol, crit, mask):
    """_window in the staggered regime with a chosen mask (which _window does not take): the same calls in the same order"""
    import torch
    o0 = _start(env, pol, "staggered", mask)
    tt = _term_buf(env)
    env.set_terminal_obs(tt)
    o, r, d, a = _bufs(env, T)
    v, lp = _ac_bufs(env, T)
    tv = _tv_buf(env)
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp, term_values=tv, critic=crit)
    torch.cuda.synchronize()
    return dict(o0=o0, o=o, r=r, d=d, a=a, v=v, lp=lp, tv=tv, tt=tt)


def _report(kind, D, what):
    worst = _WORST[(kind, D)]
    print("%s actor + critic d=%d %s: worst so far at this width |V - V_ref| %.3g (bar %.3g), logp error / bar %.3g, |V_term - V_ref| %.3g"
          % (kind, D, what, worst[0], ATOL_FP32, worst[1], worst[2]))


# ---- a. values_dev at every width -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_values_dev_at_every_width(obs):
    """critic_mfma_kernel alone: unit-variance rows (what _obs_scale makes of the env's), every trunk with both activations"""
    import torch
    D, worst = obs[2], 0.0
    env = _env(obs, max(8, obs[1]))
    rng = np.random.RandomState(1000 + D)
    xs = {M: rng.randn(M, D).astype(np.float32) for M in ROWS}
    nets = [(widths, act) for widths in VALUE_TRUNKS for act in ACTS]
    for i, (widths, act) in enumerate(nets):
        net = _CNet(widths, np.ones(D), i + D, D, act)
        crit = net.build(env)
        for M in ROWS:
            xd = torch.from_numpy(xs[M]).to(_dev())
            got = crit.values_dev(xd)
            torch.cuda.synchronize()
            what = "critic %s %s D=%d M=%d" % (widths, act, D, M)
            ref = net.ref64(xs[M], what)
            assert got.shape == (M,) and got.dtype == torch.float32 and bool(torch.isfinite(got).all()), what
            assert float(np.mean(np.abs(ref) > ATOL_FP32)) > 0.9, what                  # teeth
            err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - ref)))
            worst = max(worst, err)
            assert err <= ATOL_FP32, (what, err)
            if i == D % len(nets) and M in (1, 65):
                # gaq_critic_eval_dev promises 4-byte alignment only: the same rows 4 bytes off a 16-byte boundary ...
                flat = torch.empty(M * D + 1, device=_dev())
                off = flat[1:].view(M, D)
                off.copy_(xd)
                assert off.is_contiguous() and off.data_ptr() % 16 == 4, what
                assert torch.equal(crit.values_dev(off), got), (what, "4 bytes off")
                if D % 2:                                           # ... and as the rows 1: of an [M + 1, D] tensor (odd D: 4 D % 16 != 0)
                    tall = torch.zeros((M + 1, D), device=_dev())
                    tall[1:] = xd
                    assert tall[1:].is_contiguous() and tall[1:].data_ptr() % 16 != 0 and tall[1:].data_ptr() % 4 == 0, what
                    assert torch.equal(crit.values_dev(tall[1:]), got), (what, "rows 1:")
        crit.close()
    print("values_dev d=%d: worst |V - V_ref| %.3g (bar %.3g)" % (D, worst, ATOL_FP32))
    env.close()


# ---- b. rollouts at every width and batch ---------------------------------------------------------------------------------------
_CB = [(case, j) for case in CASES for j in range(4)]
_CB_IDS = ["d%d-%s-b%d" % (obs[2], layout, j) for (obs, layout), j in _CB]


def _run_pairs(case, j, kind):
    obs, layout = case
    n = _batches(obs[1])[j]
    for spec, k, cw, kc in _pairs(kind, obs[2]):
        _rollout_case(obs, layout, n, spec, k, cw, kc, twin=n <= 64)
    _report(kind, obs[2], "%s n=%d" % (layout, n))


@pytest.mark.parametrize("case,j", _CB, ids=_CB_IDS)
def test_mlp_actor_with_a_critic_against_fp64(case, j):
    """policy_mfma_critic_kernel, critic_mfma_kernel (the bootstrap row) and critic_mfma_term_kernel: batch j of _batches"""
    _run_pairs(case, j, "mlp")


@pytest.mark.parametrize("case,j", _CB, ids=_CB_IDS)
def test_gru_actor_with_a_critic_against_fp64(case, j):
    """policy_gru_ac_kernel with no V of its own, then critic_mfma_kernel after every step, and critic_mfma_term_kernel"""
    _run_pairs(case, j, "gru")


# ---- c. mixed activations, and which term sizes the LDS ---------------------------------------------------------------------------
@pytest.mark.parametrize("cact", ACTS)
@pytest.mark.parametrize("mix", MIX, ids=[m[0] for m in MIX])
def test_mixed_activations_fused_and_in_two_launches(mix, cact):
    """each trunk with its own activation: a fused kernel that took hidden_act from the actor for both would miss fp64 by far more
    than the bar in half of these (tests/test_policy_critic_shapes_cpu.py)"""
    import torch
    _, obs, aw, cw = mix
    n = _batches(obs[1])[2]                                         # a tile plus a sliver
    for k in MIX_STYLES:
        assert _style(k) == (ACTS[k % 2], k < 2)
        runs = [_rollout_case(obs, "alias", n, ("mlp", aw), k, cw, 40 + k, cact, fused) for fused in (True, False)]
        for key in ("o", "r", "d", "a", "v", "lp", "tt"):
            assert torch.equal(runs[0][key], runs[1][key]), (mix, cact, k, key)
        assert torch.equal(runs[0]["tv"].view(torch.int32), runs[1]["tv"].view(torch.int32)), (mix, cact, k)
    _report("mlp", obs[2], "%s-sized, critic %s, n=%d" % (mix[0], cact, n))


# ---- d. the GRU engine's largest footprint, then the critic ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 2096])
def test_gru_largest_footprint_with_a_critic(n):
    """H = 256 on a 16-agent swarm's 108 inputs (157 KiB of LDS in the actor's launch), each step followed by a critic launch of
    65 KiB (256-256-256) or 28 KiB (16: in_dim sizes it)"""
    for j, cw in enumerate(BIG_GRU_CRITICS):
        _rollout_case(OBS[-1], "alias", n, BIG_GRU, 3 + 108, cw, 108 + j, twin=n <= 64)
    _report("gru", 108, "H=256 n=%d" % n)


# ---- e. done counts the critic's gathered kernel has not seen ---------------------------------------------------------------------
@pytest.mark.parametrize("mask_id", list(MASKS))
@pytest.mark.parametrize("spec", GATHER_NETS, ids=["mlp240-80", "gru48-16-80"])
def test_gather_with_a_critic_at_done_counts_of_1_to_129(spec, mask_id):
    """staggered regime with a chosen mask, as tests/test_gpu_policy_ac_shapes.py runs it: the unmasked envs finish in window step 10,
    the masked ones in step 15.  The terminal values against values_dev and fp64, and the window as twenty T = 1 calls bit-equal"""
    import torch
    n, k = N_GATHER, GATHER_NETS.index(spec)
    mask = np.zeros(n, bool)
    mask[MASKS[mask_id]] = True
    for j, cw in enumerate(GATHER_CRITICS):
        env, twin = _env(OBS[2], n), _env(OBS[2], n)
        scale = _obs_scale(env)
        _obs_scale(twin)
        net, cnet = _Net(spec, scale, k), _CNet(cw, scale, 60 + 2 * k + j)
        pol, pt = net.build(env, value=False), net.build(twin, value=False)
        crit, ct = cnet.build(env), cnet.build(twin)
        what = "%s + critic %s %s n=%d" % (spec, cw, mask_id, n)
        w = _masked_window(env, pol, crit, mask)
        at = _one_done_each(w["d"], what)
        counts = w["d"].to(torch.int32).sum(dim=1).cpu().numpy()
        want = np.zeros(T, np.int64)
        want[10], want[15] = n - int(mask.sum()), int(mask.sum())
        assert np.array_equal(counts, want), (what, counts)
        assert np.array_equal(at.cpu().numpy(), np.where(mask, 15, 10)), what
        err = _term_check(cnet, crit, w, n, what, at)
        assert torch.equal(w["v"], crit.values_dev(torch.cat([w["o0"][None], w["o"]]))), what
        print("%s: dones per step %d and %d, worst |V_term - V_ref| %.3g (bar %.3g)" % (what, want[10], want[15], err, ATOL_FP32))
        # the same window in twenty calls of one step
        _start(twin, pt, "staggered", mask)
        tt = _term_buf(twin)
        twin.set_terminal_obs(tt)
        o, r, d, a = _bufs(twin, T)
        lp = torch.full((T, n), float("nan"), device=_dev())
        tv = _tv_buf(twin)
        v = torch.full((T + 1, n), float("nan"), device=_dev())
        for t in range(T):
            v1, lp1 = _ac_bufs(twin, 1)                             # (of their own: row t of a [T, 130] tensor is 16-byte aligned
            tv1 = _tv_buf(twin, 1)                                  # for even t only, and the call asks that of what it is given)
            twin.rollout_policy_dev(pt, o[t:t + 1], r[t:t + 1], d[t:t + 1], a[t:t + 1], values=v1, logp=lp1, term_values=tv1, critic=ct)
            if t:
                assert torch.equal(v[t], v1[0]), (what, t)          # the bootstrap row IS the next call's row 0
            v[t:t + 2], lp[t], tv[t] = v1, lp1[0], tv1[0]
        torch.cuda.synchronize()
        for key, x in (("o", o), ("r", r), ("d", d), ("a", a), ("v", v), ("lp", lp), ("tt", tt)):
            assert torch.equal(w[key], x), (what, key)              # (no NaN left in them: equal means bit-equal)
        assert torch.equal(w["tv"].view(torch.int32), tv.view(torch.int32)), what
        if net.kind == "gru":
            assert torch.equal(pol.hidden, pt.hidden), what
        _close(pol, pt, crit, ct, env, twin)


# ---- f. a captured rollout with a critic ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["alias", "plain"])
@pytest.mark.parametrize("pair", GRAPH_PAIRS, ids=GRAPH_IDS)
def test_graph_captured_rollout_with_a_critic(pair, layout):
    """graph-safe mode: one captured 8-step rollout with values, log-probabilities and terminal values from the critic -- two launches
    per step fused, three otherwise, on one stream -- replayed three times, equals three eager calls on a twin bit for bit: every
    output, and .hidden for the GRU.  Episodes are 16 steps: each env finishes in the replays, and every done is seen."""
    import torch
    spec, cw, fused = pair
    n, steps, k = 68, 8, GRAPH_PAIRS.index(pair)
    graphed, eager = _env(OBS[2], n, layout, True), _env(OBS[2], n, layout, True)
    scale = _obs_scale(graphed)
    _obs_scale(eager)
    net, cnet = _Net(spec, scale, k), _CNet(cw, scale, 70 + k)
    pols = [net.build(graphed, value=False), net.build(eager, value=False)]
    crits = [cnet.build(graphed, fused), cnet.build(eager, fused)]
    bufs, kws = [], []
    for e, p, c in zip((graphed, eager), pols, crits):
        o0 = torch.empty((n, 18), device=_dev())
        e.reset_dev(o0)
        if net.kind == "gru":
            p.reset_hidden()
        e.set_terminal_obs(_term_buf(e))
        bufs.append(_bufs(e, steps))
        v, lp = _ac_bufs(e, steps)
        kws.append(dict(values=v, logp=lp, term_values=_tv_buf(e, steps), critic=c))
    torch.cuda.synchronize()
    outs = ("values", "logp", "term_values")

    def same(what):
        for x, y in zip(bufs[0], bufs[1]):
            assert torch.equal(x, y), what
        for key in outs:                                            # finite everywhere once written: bit-equal
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
            for key in outs:
                kw[key].fill_(float("nan"))
        g.replay()
        eager.rollout_policy_dev(pols[1], *bufs[1], **kws[1])
        torch.cuda.synchronize()
        same("replay %d" % rep)
        d, tv = bufs[0][2], kws[0]["term_values"]
        assert bool((tv.view(torch.int32)[d == 0] == 0).all()), rep
        if int(d.sum()):
            assert float((tv[d != 0].abs() > ATOL_FP32).double().mean()) > 0.9, rep         # every done has its terminal value
        # the bootstrap row is V of the observation the replay ended on
        assert torch.equal(kws[0]["values"][steps], crits[0].values_dev(bufs[0][0][steps - 1])), rep
        dones += d.to(torch.int32).sum(dim=0)
    assert bool((dones >= 1).all()), dones.cpu().tolist()           # every env finished inside the replays
    _close(*(pols + crits + [graphed, eager]))


# ---- g. which outputs are asked for -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", SUBSET_PAIRS, ids=SUBSET_IDS)
def test_every_subset_of_the_outputs_is_the_full_calls(pair):
    """with a critic, logp alone (the actor-critic kernel with no value layer), term_values alone (the gathered kernel with no batch
    launch), both, values alone and values + term_values: what was asked for is the full call's bits, and so are the rollout, the
    env's state and .hidden; the buffers that were not passed stay NaN"""
    import torch
    spec, cw, fused = pair
    n, k, obs = 64 + 4, SUBSET_PAIRS.index(pair), OBS[2]

    def build():
        env = _env(obs, n)
        scale = _obs_scale(env)
        net, cnet = _Net(spec, scale, k), _CNet(cw, scale, 80 + k)
        return env, net, cnet, net.build(env, value=False), cnet.build(env, fused)

    env, net, cnet, pol, crit = build()
    what = "%s + critic %s%s" % (spec, cw, "" if fused else " (two launches)")
    full = _window(env, pol, crit)
    _check(net, cnet, crit, full, n, what)
    state = env.state_dict()
    hidden = pol.hidden.clone() if net.kind == "gru" else None
    for subset in SUBSETS:
        twin, _, _, pt, ct = build()
        _start(twin, pt, "aligned")
        tt = _term_buf(twin)
        twin.set_terminal_obs(tt)
        o, r, d, a = _bufs(twin, T)
        v, lp = _ac_bufs(twin, T)
        got = dict(v=v, lp=lp, tv=_tv_buf(twin))
        names = dict(v="values", lp="logp", tv="term_values")
        twin.rollout_policy_dev(pt, o, r, d, a, critic=ct, **{names[key]: got[key] for key in subset})
        torch.cuda.synchronize()
        for key, x in (("o", o), ("r", r), ("d", d), ("a", a), ("tt", tt)):
            assert torch.equal(full[key], x), (what, subset, key)
        for key, x in got.items():
            if key in subset:
                assert torch.equal(full[key].view(torch.int32), x.view(torch.int32)), (what, subset, key)
            else:
                assert bool(torch.isnan(x).all()), (what, subset, key, "written without being asked for")
        assert _same(state, twin.state_dict()), (what, subset)
        if hidden is not None:
            assert torch.equal(hidden, pt.hidden), (what, subset)
        _close(pt, ct, twin)
    _close(pol, crit, env)
