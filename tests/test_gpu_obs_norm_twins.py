"""The thirteen *_norm_kernel twins of gym_art_amd/csrc/gaq_policy.hip at every observation width the env offers.
(X_norm_kernel labels the <PolObsNorm> instantiation of the kernel template X_kernel; its plain original is X_kernel<>.)

A. Every twin against its plain original, BIT FOR BIT, under a table that differs in every column (tests/obs_norm_twins_plan.py has the
   argument, tests/test_obs_norm_twins_cpu.py checks it without a GPU): mean 0, eps 0, clip +inf and var[k] = s[k]^-2 with
   s[k] = 2^((3 k mod 5) - 2), so that the published inv_std is exactly s and the staged value exactly x s[k].  The twin run attaches that
   table to a net with first-layer weights W; the plain run, on a twin env built with the same arguments, attaches nothing and uses
   W s[None, :] (W_ih of a recurrent cell; a critic's first layer too).  Observations, rewards, dones, actions, terminal rows, h and c
   must be torch.equal, values, log-probabilities and terminal values equal as int32.  No tolerance anywhere.  Teeth of every case: a
   third run with the unscaled W and no table differs in its first actions (and values); every env reports a done inside the window
   (T = 20, ep_time = 0.15); terminal values are non-zero exactly where done is set; the table is read back through normalize_dev
   (a row of ones gives s, a row of zeros +0); no recorded observation is a non-zero value below 2^-100 (nothing near the denormals).
   The sweep: nine families (obs_norm_twins_plan.FAMILIES, which names the twins each reaches) x eleven widths x the batches q, 64,
   64 + q (and 2096 for the MLP and LSTM actor-critic families), then D = 20 at N = 1, 63 and 65, the 157 KiB LDS case (D = 108,
   H = 256), D = 108 under a 256 x 3 actor and a 256 x 2 critic, a staggered window per family at D = 19, N = 130 (gathered passes of 67
   and 63 rows; 130 x 19 floats is no multiple of 16 bytes, which a T > 1 call needs, so the window runs as calls of one step each),
   and both layouts at D = 13 and 108.
B. The clamp and a non-zero mean, which A cannot exercise: deterministic actors with the case table of tests/obs_norm_ref.py (clip 5)
   at every width against the fp64 references on the device's recorded observations normalised in fp64 with the published table -- what
   tests/test_gpu_obs_norm.py does at D = 18, at its bar: MARGIN (8) x the torch-fp32 yardstick on the same inputs; the bf16 engine
   against tests/policy_bf16_ref.py at ATOL_ALL / ATOL_MOST / FRAC_MOST of tests/test_gpu_policy_bf16.py.  Every case asserts the clip
   census (elements at +clip, at -clip and inside) and prints device error, yardstick and error / bar.

FIGURES (MI355X): 171 passed in 6.3 s, the slowest case 0.51 s (the first, which loads the library), every other below 0.13 s.  Part A: 127
cases (99 of the sweep, 28 beside it), no mismatch.  Part B, the worst error / bar over the eleven widths: MFMA 48 0.195 (D = 13; device 4.93e-7, yardstick 3.15e-7),
GRU 16 0.153 (D = 36), LSTM 16 0.163 (D = 20); bf16 48-48 worst action error 6.9e-4 = 0.138 of ATOL_ALL (D = 25), at least 0.99890 of
the actions within ATOL_MOST at every width.
MUTANTS (wrong staging only, each built apart as a library of its own, run on an MI355X; all reads stay inside the table):
 1. pol_stage_obs takes the mean from column k + 1;  2. it takes inv_std from column (k + 1) mod D;  3. it reads the table with
    dim = D - 1: each fails 148 of the 171 cases -- everything but the 23 bf16 cases, whose kernel does not call pol_stage_obs.
 4. policy_mfma_bf16_norm_kernel's own staging loop takes inv_std from column (k + 1) mod D: exactly those 23 cases fail.
 tests/test_gpu_obs_norm.py fails 58, 55, 58 and 4 of its 93 cases under them: it sees such a mutant where it changes D = 18 (or the
 critic's twin); this file sees it in every twin at every width."""
import numpy as np
import pytest

from tests import ac_ref
from tests import obs_norm_ref as R
from tests import obs_norm_twins_plan as P
from tests.gru_util import _gru, _head
from tests.gru_util import reference_rollout as gru_reference
from tests.lstm_util import _lstm, torch_head32, torch_step32
from tests.lstm_util import reference_rollout as lstm_reference
from tests.mlp_ref import forward64
from tests.policy_util import _bufs, _dev
from tests.test_gpu_obs_norm import MARGIN, T5, _Actor, _bf16_forward32, _case_norm, _gru_rollout32, _rollout, _table, _torch_mlp32
from tests.test_gpu_obs_norm import _env as _norm_env
from tests.test_gpu_policy_ac import LOG_STD
from tests.test_gpu_policy_ac_shapes import _env
from tests.test_gpu_policy_bf16 import ATOL_ALL, ATOL_MOST, FRAC_MOST
from tests.test_gpu_policy_shapes import OBS, OBS_IDS, RELU_BF16_SCALE, _batches, _mlp, _obs_scale, _style

pytestmark = pytest.mark.gpu

T = P.T
TINY = 2.0 ** -100
ACTS = ["tanh", "relu"]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _times(layer, s):
    """(W s[None, :], b) in float32: exact, a power-of-two scaling of values far from the ends of the range"""
    W, b = layer
    nz = np.abs(W[W != 0])
    assert nz.min() > TINY and nz.max() < 1.0 / TINY
    Ws = (W * s[None, :]).astype(np.float32)
    assert np.array_equal(Ws.astype(np.float64), W.astype(np.float64) * s[None, :].astype(np.float64))
    return Ws, b


class _Net:
    """the net of one case, buildable on several (twin) envs with its first layer(s) as drawn or scaled per input.  The observation
    scale of tests/test_gpu_policy_shapes.py (_obs_scale) is folded into the first layers as drawn."""

    def __init__(self, case, scale):
        fam, spec, D = P.FAMILIES[case.family], case.net, case.D
        self.kind, self.fam = fam.kind, fam
        self.act, self.out_tanh = _style(spec.k)
        seed = 1100 + 7 * spec.k + D
        if self.kind in ("mlp", "bf16"):
            layers = _mlp(spec.widths, D, seed, scale)
            if self.kind == "bf16" and self.act == "relu":          # (as tests/test_gpu_policy_shapes.py conditions its relu bf16 nets)
                W, b = layers[0]
                layers[0] = ((RELU_BF16_SCALE * W).astype(np.float32), (RELU_BF16_SCALE * b).astype(np.float32))
            self.first, self.rest, last = layers[0], layers[1:], spec.widths[-1]
        else:
            H = self.H = spec.H
            W_ih, W_hh, b_ih, b_hh = (_gru if self.kind == "gru" else _lstm)(H, D, seed, 1.0 / np.sqrt(D + H))
            self.first, self.hh = ((W_ih / scale[None, :]).astype(np.float32), b_ih), (W_hh, b_hh)
            self.rest, last = _head(H, spec.head, seed + 1), (spec.head[-1] if spec.head else H)
        self.value = ac_ref.value_head(last, seed + 2) if "v" in fam.ask and not fam.critic else None
        if fam.critic:
            trunk = _mlp(spec.critic, D, seed + 3, scale)
            w, b = ac_ref.value_head(spec.critic[-1], seed + 4)
            self.cfirst, self.crest = trunk[0], trunk[1:-1] + [(w.reshape(1, -1), np.asarray([b], np.float32))]
            self.cact = ACTS[(spec.k // 2) % 2]

    def build(self, env, s=None, norm=None):
        """(policy, critic or None) on env; s: the per-input scales multiplied into the first layers; norm: attached to both"""
        from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPCritic, MLPPolicy
        first = self.first if s is None else _times(self.first, s)
        if self.kind in ("mlp", "bf16"):
            pol = MLPPolicy.from_arrays(env, [first] + self.rest, self.act, self.out_tanh, LOG_STD, "bf16" if self.kind == "bf16" else "mfma",
                                        self.value, norm)
        else:
            cell = (first[0], self.hh[0], first[1], self.hh[1])
            pol = (GRUPolicy if self.kind == "gru" else LSTMPolicy)(env, cell, self.rest, self.act, self.out_tanh, LOG_STD, self.value)
            if norm is not None:
                pol.set_obs_norm(norm)
        assert pol.obs_norm is norm
        crit = None
        if self.fam.critic:
            crit = MLPCritic.from_arrays(env, [self.cfirst if s is None else _times(self.cfirst, s)] + self.crest, self.cact)
            if norm is not None:
                crit.set_obs_norm(norm)
            assert crit.obs_norm is norm
        return pol, crit


def _scale_norm(env):
    """the normaliser of part A on env, its published table read back and required to be exact; returns (norm, s)"""
    import torch
    from gym_art_amd.policy import ObsNorm
    D = env.obs_dim
    s = P.scales(D)
    assert set(s.tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0} and np.all(s[1:] != s[:-1]) and (s[D - 1] != s[0] or s[D - 1] != s[1])
    norm = ObsNorm.from_stats(env, np.zeros(D), s.astype(np.float64) ** -2, 1.0, 0.0, float("inf"))
    ones = norm.normalize_dev(torch.ones((1, D), device=_dev()))
    zeros = norm.normalize_dev(torch.zeros((1, D), device=_dev()))
    assert torch.equal(ones[0], _t(s)), "the published inv_std is not s"
    assert not bool(zeros.view(torch.int32).any()), "a zero row does not normalise to +0"
    return norm, s


def _window(case, env, pol, crit):
    """reset (an LSTM from non-zero h0, c0), the staggered regime's prelude where the case has one, then the window with everything the
    family asks for; a dict of tensors"""
    import torch
    fam = P.FAMILIES[case.family]
    n, D, dev = env.num_envs, env.obs_dim, _dev()
    nan = float("nan")

    def call(steps, ask):
        o, r, d, a = _bufs(env, steps)
        kw = {}
        if "v" in ask:
            kw["values"] = torch.full((steps + 1, n), nan, device=dev)
        if "lp" in ask:
            kw["logp"] = torch.full((steps, n), nan, device=dev)
        if "tv" in ask:
            kw["term_values"] = torch.full((steps, n), nan, device=dev)
        if crit is not None and ask:
            kw["critic"] = crit
        env.rollout_policy_dev(pol, o, r, d, a, **kw)
        return dict(o=o, r=r, d=d, a=a, v=kw.get("values"), lp=kw.get("logp"), tv=kw.get("term_values"))

    def run(steps, ask):
        """one call, or (case.single) calls of one step each, joined"""
        if not case.single:
            return call(steps, ask)
        parts = [call(1, ask) for _ in range(steps)]
        out = {k: (torch.cat([p[k] for p in parts]) if parts[0][k] is not None else None) for k in ("o", "r", "d", "a", "lp", "tv")}
        out["v"] = None
        if parts[0]["v"] is not None:
            for p, q in zip(parts, parts[1:]):                      # the bootstrap row IS the next call's row 0
                assert torch.equal(p["v"][1].view(torch.int32), q["v"][0].view(torch.int32))
            out["v"] = torch.cat([p["v"][:1] for p in parts] + [parts[-1]["v"][1:]])
        return out

    o0 = torch.empty((n, D), device=dev)
    env.reset_dev(o0)
    if fam.kind == "lstm":
        rng = np.random.RandomState(n + pol.hidden_size)
        pol.set_hidden((0.5 * rng.randn(n, pol.hidden_size)).astype(np.float32), (0.5 * rng.randn(n, pol.hidden_size)).astype(np.float32))
    elif fam.kind == "gru":
        pol.reset_hidden()
    cur = o0.clone()
    if case.stagger:
        pre = run(P.STAGGER_AFTER, ())
        mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        mask[:P.STAGGER_MASKED] = 1
        cur = pre["o"][P.STAGGER_AFTER - 1].clone()                 # the rows of the envs that go on keep the current observation
        env.reset_dev(cur, mask)
        if hasattr(pol, "reset_hidden"):
            pol.reset_hidden(mask)
        torch.cuda.synchronize()
        assert int(pre["d"].sum()) == 0
        start = cur.clone()
    else:
        start = cur
    tt = torch.full((n, D), nan, device=dev)
    env.set_terminal_obs(tt)
    w = run(T, fam.ask)
    torch.cuda.synchronize()
    w.update(o0=start, tt=tt)
    for name in ("hidden", "cell"):
        w[name] = getattr(pol, name).clone() if hasattr(pol, name) else None
    return w


def _assert_bit_equal(a, b, what):
    import torch
    assert a.keys() == b.keys()
    for k in ("o0", "o", "r", "d", "a", "tt", "hidden", "cell"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert bool(torch.isfinite(a[k].float()).all()), (what, k)
            assert torch.equal(a[k], b[k]), (what, k, "the twin with the table != the plain kernel on W s")
    for k in ("v", "lp", "tv"):                                     # as int32: +0.0 is checked
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert bool(torch.isfinite(a[k]).all()), (what, k)
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k, "the twin with the table != the plain kernel on W s")


def _run_case(case):
    """the three runs of one case -- "twin": the table and W; "plain": no table, W s; "raw": no table, W -- and every assertion"""
    import torch
    fam = P.FAMILIES[case.family]
    obs = OBS[P.WIDTHS.index(case.D)]
    what = tuple(case)
    runs, net, scale0 = {}, None, None
    for mode in ("twin", "plain", "raw"):
        env = _env(obs, case.N, case.layout)
        scale = _obs_scale(env)                                     # (the same calls on the three envs: the same resets)
        if net is None:
            net, scale0 = _Net(case, scale), scale
        assert np.array_equal(scale, scale0), what
        norm, s = _scale_norm(env) if mode == "twin" else (None, P.scales(case.D))
        pol, crit = net.build(env, s if mode == "plain" else None, norm)
        runs[mode] = _window(case, env, pol, crit)
        for x in (pol, crit, norm, env):
            if x is not None:
                x.close()
    twin, plain, raw = runs["twin"], runs["plain"], runs["raw"]
    # teeth first: they say whether the comparison below means anything
    d = twin["d"]
    assert bool((d.to(torch.int32).sum(dim=0) >= 1).all()), (what, "an env reported no done inside the window")
    if case.stagger:
        counts = d.to(torch.int32).sum(dim=1).cpu().numpy()
        assert counts[10] == case.N - P.STAGGER_MASKED and counts[15] == P.STAGGER_MASKED and counts.sum() == case.N, (what, counts)
    for k in ("o0", "o", "tt"):
        x = twin[k]
        assert bool(torch.isfinite(x).all()), (what, k)
        assert not bool(((x != 0) & (x.abs() < TINY)).any()), (what, k, "a recorded observation is non-zero below 2^-100")
    if "tv" in fam.ask:
        assert torch.equal(twin["tv"].view(torch.int32) != 0, d != 0), (what, "terminal values are not non-zero exactly where done is set")
    # (the first step sees the same observation in both runs, except after a staggered prelude, whose five steps already differ)
    first = slice(None) if case.stagger else 0
    assert case.stagger or torch.equal(twin["o0"], raw["o0"]), what
    assert not torch.equal(twin["a"][first], raw["a"][first]), (what, "the table changed nothing")
    if "v" in fam.ask:
        assert not torch.equal(twin["v"][first], raw["v"][first]), (what, "the table changed no value")
    _assert_bit_equal(twin, plain, what)


# ---- A. the sweep ---------------------------------------------------------------------------------------------------------------------
_SWEEP = [(obs, family) for obs in OBS for family in P.FAMILIES]
_SWEEP_IDS = ["d%d-%s" % (obs[2], family) for obs, family in _SWEEP]


@pytest.mark.parametrize("obs,family", _SWEEP, ids=_SWEEP_IDS)
def test_twin_equals_plain_kernel_on_scaled_weights(obs, family):
    """one family at one observation width: q, 64 and 64 + q envs (2096 too for the MLP and LSTM actor-critic families)"""
    cases = dict(P.sweep(obs))[family]
    assert [c.N for c in cases] == _batches(obs[1])[:len(cases)]
    for case in cases:
        _run_case(case)


_EXTRAS = P.extras()


@pytest.mark.parametrize("case", [c for _, c in _EXTRAS], ids=[i for i, _ in _EXTRAS])
def test_twin_equals_plain_kernel_at_the_edges(case):
    """single rows and tile edges at D = 20, the 157 KiB LDS case, 256-wide nets on 108 inputs, the staggered windows (gathered passes of
    67 and 63 rows at a partial k-step of 3), both layouts"""
    _run_case(case)


# ---- B. the clamp and the mean against fp64 -------------------------------------------------------------------------------------------
B_NETS = [("mfma", [48]), ("gru", [16]), ("lstm", [16])]
_WORST = {}                                      # kind -> the worst error / bar so far


@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
@pytest.mark.parametrize("kind,widths", B_NETS, ids=["mfma48", "gru16", "lstm16"])
def test_actors_against_fp64_under_the_case_table(kind, widths, obs):
    """tests/test_gpu_obs_norm.py test_actors_against_fp64_on_normalised_inputs at this observation width, N = 64 + q: action[t] (and a
    recurrent state) against the fp64 references fed the recorded observations normalised in fp64 with the published fp32 table.
    Bar: MARGIN (8) x the worst error of torch fp32 on the CPU on the same normalised inputs, as there."""
    D, n = obs[2], _batches(obs[1])[2]
    env = _norm_env(obs, n)
    norm = _case_norm(env)
    mean32, inv32 = _table(norm)
    net = _Actor(kind, widths, D=D, value=False)
    pol = net.build(env, norm, log_std=None)
    run = {k: v.cpu().numpy() for k, v in _rollout(env, pol, T5).items()}
    assert int(run["done"][:-1].sum()) >= n
    z0, z = (R.normalize(run[k], mean32, inv32, R.CLIP, np.float64) for k in ("obs0", "obs"))
    hi, lo, inside = R.clip_census(np.concatenate([z0[None], z]))
    assert hi > 0 and lo > 0 and inside > 0, (D, hi, lo, inside)
    z0_32, z_32 = z0.astype(np.float32), z.astype(np.float32)
    if kind == "mfma":
        prev64, prev32 = np.concatenate([z0[None], z[:-1]]), np.concatenate([z0_32[None], z_32[:-1]])
        ref, _ = forward64(net.layers, net.act, net.out_tanh, prev64)
        ref = np.asarray(ref, np.float64)
        yard = np.abs(_torch_mlp32(net.layers, net.act, net.out_tanh, prev32) - ref).max()
        err = np.abs(run["actions"] - ref).max()
    elif kind == "gru":
        ra, rh = gru_reference(net.cell, net.layers, net.act, net.out_tanh, z0, z, run["done"], np.zeros((n, widths[0])))
        ya, yh = _gru_rollout32(net, z0_32, z_32, run["done"])
        yard = max(np.abs(ya - ra).max(), np.abs(yh - rh).max())
        err = max(np.abs(run["actions"] - ra).max(), np.abs(run["hidden"] - rh).max())
    else:
        zeros = np.zeros((n, widths[0]))
        ref = lstm_reference(net.cell, net.layers, net.act, net.out_tanh, z0, z, run["done"], zeros, zeros)
        y = lstm_reference(net.cell, net.layers, net.act, net.out_tanh, z0_32, z_32, run["done"], zeros, zeros, step=torch_step32(net.cell),
                           head=torch_head32(net.layers, net.act, net.out_tanh))
        yard = max(np.abs(y[k] - ref[k]).max() for k in ("a", "h", "c"))
        err = max(np.abs(run["actions"] - ref["a"]).max(), np.abs(run["hidden"] - ref["h"]).max(), np.abs(run["cell"] - ref["c"]).max())
    bar = MARGIN * yard
    _WORST[kind] = max(_WORST.get(kind, 0.0), err / bar)
    print("%s %s d=%d n=%d: clip census +%d -%d inside %d; device error %.3g, torch fp32 yardstick %.3g, error / bar %.3g (worst %s so far %.3g)"
          % (kind, widths, D, n, hi, lo, inside, err, yard, err / bar, kind, _WORST[kind]))
    assert yard > 0 and err <= bar, (kind, widths, D, n, err, yard)
    pol.close(); norm.close(); env.close()


@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_bf16_actor_against_its_reference_under_the_case_table(obs):
    """bf16 D-48-48-4 with the case table attached, N = 64 + q: action[t] against tests/policy_bf16_ref.py forward on the recorded
    observations normalised in fp32 with the published table (the contract: the element expression runs in fp32 and its result is what
    is rounded to bf16), at the tolerances of tests/test_gpu_policy_bf16.py: every action within ATOL_ALL, FRAC_MOST of them within
    ATOL_MOST.  The yardstick printed beside them is the same contract with torch fp32 sums on the CPU."""
    import torch
    from tests.policy_bf16_ref import forward as bf16_forward
    D, n = obs[2], _batches(obs[1])[2]
    env = _norm_env(obs, n)
    norm = _case_norm(env)
    mean32, inv32 = _table(norm)
    net = _Actor("bf16", [48, 48], D=D)
    pol = net.build(env, norm, log_std=None)
    run = {k: v.cpu().numpy() for k, v in _rollout(env, pol, T5).items()}
    assert int(run["done"][:-1].sum()) >= n
    prev = np.concatenate([run["obs0"][None], run["obs"][:-1]]).reshape(-1, D)
    z = R.normalize(prev, mean32, inv32, R.CLIP)
    hi, lo, inside = R.clip_census(z)
    assert z.dtype == np.float32 and hi > 0 and lo > 0 and inside > 0, (D, hi, lo, inside)
    zt = torch.from_numpy(np.ascontiguousarray(z))
    ref = bf16_forward(net.layers, net.act, net.out_tanh, zt).numpy()
    yard = np.abs(_bf16_forward32(net.layers, net.act, net.out_tanh, zt).numpy() - ref).max()
    err = np.abs(run["actions"].reshape(-1, 4) - ref)
    frac = float((err <= ATOL_MOST).mean())
    _WORST["bf16"] = max(_WORST.get("bf16", 0.0), float(err.max()) / ATOL_ALL)
    print("bf16 [48, 48] d=%d n=%d: clip census +%d -%d inside %d; device error %.3g, torch fp32 yardstick %.3g, error / bar %.3g, within %.0e: "
          "%.5f of %d (worst bf16 so far %.3g)" % (D, n, hi, lo, inside, err.max(), yard, err.max() / ATOL_ALL, ATOL_MOST, frac, err.size, _WORST["bf16"]))
    assert err.max() <= ATOL_ALL, (D, n, float(err.max()))
    assert frac >= FRAC_MOST, (D, n, frac)
    pol.close(); norm.close(); env.close()
