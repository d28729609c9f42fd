"""Actor-critic rollouts on the device (gaq.h gaq_step_policy_ac_many_dev, gaq_gae_dev): asking for values and log-probabilities changes
nothing else, splitting a rollout changes nothing, values and log-probabilities against fp64 references fed the device's recorded
observations, advantages against fp64, and the refusals.  ep_time=0.15 and T = 20: every env auto-resets inside the window."""
import numpy as np
import pytest

from tests import ac_ref
from tests.gru_util import _gru, _head
from tests.mlp_ref import assert_not_saturated
from tests.policy_util import _bufs, _dev
from tests.test_gpu_policy_shapes import ATOL_FP32, ATOL_GRU, _mlp, _obs_scale

pytestmark = pytest.mark.gpu

T = 20
BATCHES = [64 + 4, 2096]                 # a tile plus a sliver; 32 tiles plus a tail
LAYOUTS = ["alias", "plain"]
# ("mlp", widths) / ("gru", H, head widths)
NETS = [("mlp", [48]), ("mlp", [240, 80]), ("mlp", [256, 256, 256]), ("gru", 48, ()), ("gru", 48, (16, 80)), ("gru", 240, ())]
NET_IDS = ["mlp48", "mlp240-80", "mlp256x3", "gru48", "gru48-16-80", "gru240"]
LOG_STD = (-1.0, -0.5, -1.5, -1.0)


def _env(n, layout, graph_safe=False):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(num_envs=n, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=layout == "alias")
    if graph_safe:
        env.set_graph_safe(True)
    return env


def _style(k):
    return ("tanh", "relu")[k % 2], (k // 2) % 2 == 0


class _Net:
    """one net of NETS with a value head, buildable on several (twin) envs"""

    def __init__(self, spec, scale, k, D=18):
        self.kind = spec[0]
        self.act, self.out_tanh = _style(k)
        if self.kind == "mlp":
            self.layers = _mlp(spec[1], D, 700 + k, scale)
            self.last = spec[1][-1]
        else:
            H, head = spec[1], spec[2]
            W_ih, W_hh, b_ih, b_hh = _gru(H, D, 700 + k, scale=1.0 / np.sqrt(D + H))
            self.gru = ((W_ih / scale[None, :]).astype(np.float32), W_hh, b_ih, b_hh)
            self.layers = _head(H, head, 701 + k)
            self.H, self.last = H, (head[-1] if head else H)
        self.value = ac_ref.value_head(self.last, 900 + k)
        self.atol = ATOL_FP32 if self.kind == "mlp" else ATOL_GRU

    def build(self, env, log_std=LOG_STD, value=True):
        from gym_art_amd.policy import GRUPolicy, MLPPolicy
        v = self.value if value else None
        if self.kind == "mlp":
            return MLPPolicy.from_arrays(env, self.layers, self.act, self.out_tanh, log_std=log_std, engine="mfma", value=v)
        return GRUPolicy(env, self.gru, self.layers, self.act, self.out_tanh, log_std=log_std, value=v)

    def reference(self, o0, o, d, hidden=None):
        """(means [T, N, 4], values [T + 1, N], output sums) in fp64 on the recorded observations and dones, h from 0"""
        o0, o, d = (x.cpu().numpy() for x in (o0, o, d))
        if self.kind == "mlp":
            x = np.concatenate([o0[None], o])                       # [T + 1, N, D]: row t is what action t (and value t) saw
            means, values, z = ac_ref.mlp_means_values64(self.layers, self.act, self.out_tanh, self.value, x.astype(np.float64), hidden)
            return means[:-1], values, z[:-1]
        return ac_ref.gru_means_values64(self.gru, self.layers, self.act, self.out_tanh, self.value, o0, o, d,
                                         np.zeros((o0.shape[0], self.H)), hidden)


def _reset(env, pol):
    import torch
    o0 = torch.empty((env.num_envs, env.obs_dim), device=_dev())
    env.reset_dev(o0)
    if hasattr(pol, "reset_hidden"):
        pol.reset_hidden()
    return o0, o0.clone()


def _ac_bufs(env, steps):
    import torch
    n = env.num_envs
    return torch.full((steps + 1, n), float("nan"), device=_dev()), torch.full((steps, n), float("nan"), device=_dev())


def _same(a, b):
    """state_dict values: arrays, tuples / lists of them, dicts, plain values"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    return a == b


# ---- 4. asking for more changes nothing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph_safe", [False, True], ids=["eager", "graph_safe"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("spec", NETS, ids=NET_IDS)
def test_asking_for_values_and_logp_changes_nothing_else(spec, layout, graph_safe):
    import torch
    k = NETS.index(spec)
    for n in BATCHES:
        plain, asked = _env(n, layout, graph_safe), _env(n, layout, graph_safe)
        net = _Net(spec, _obs_scale(plain), k)
        _obs_scale(asked)                                           # the same calls on both envs
        pp, pa = net.build(plain), net.build(asked)
        _reset(plain, pp); _reset(asked, pa)
        o, r, d, a = _bufs(plain, T)
        o2, r2, d2, a2 = _bufs(asked, T)
        v, lp = _ac_bufs(asked, T)
        plain.rollout_policy_dev(pp, o, r, d, a)
        asked.rollout_policy_dev(pa, o2, r2, d2, a2, values=v, logp=lp)
        torch.cuda.synchronize()
        assert int(d.sum()) >= n                                    # every env finished an episode
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2) and torch.equal(a, a2), (spec, n)
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(lp).all())
        if net.kind == "gru":
            assert torch.equal(pp.hidden, pa.hidden), (spec, n)     # the value-only launch wrote no h'
        assert _same(plain.state_dict(), asked.state_dict()), (spec, n)
        # ... and nothing later either: the next plain call of both gives the same bits
        plain.rollout_policy_dev(pp, o, r, d, a)
        asked.rollout_policy_dev(pa, o2, r2, d2, a2)
        torch.cuda.synchronize()
        assert torch.equal(o, o2) and torch.equal(a, a2) and torch.equal(d, d2), (spec, n)
        for x in (pp, pa, plain, asked):
            x.close()


# ---- 5. splitting changes nothing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("spec", NETS, ids=NET_IDS)
def test_splitting_the_rollout_changes_nothing(spec, layout):
    """one call of T = 20 against two of 10, and against two that split right after the first step that reports dones (so that the
    bootstrap launch, and for a GRU the next call's first launch, meet a done mask)"""
    import torch
    k = NETS.index(spec)
    for n in BATCHES:
        whole = _env(n, layout)
        net = _Net(spec, _obs_scale(whole), k)
        pw = net.build(whole)
        _reset(whole, pw)
        o, r, d, a = _bufs(whole, T)
        v, lp = _ac_bufs(whole, T)
        whole.rollout_policy_dev(pw, o, r, d, a, values=v, logp=lp)
        torch.cuda.synchronize()
        assert int(d.sum()) >= n                                    # every env auto-reset inside the window
        first_done = int(torch.nonzero(d.sum(dim=1))[0])
        assert first_done + 1 < T
        for h in (T // 2, first_done + 1):
            split = _env(n, layout)
            _obs_scale(split)                                       # the same calls as on `whole`
            ps = net.build(split)
            _reset(split, ps)
            o2, r2, d2, a2 = _bufs(split, T)
            va, lpa = _ac_bufs(split, h)
            vb, lpb = _ac_bufs(split, T - h)
            split.rollout_policy_dev(ps, o2[:h], r2[:h], d2[:h], a2[:h], values=va, logp=lpa)
            split.rollout_policy_dev(ps, o2[h:], r2[h:], d2[h:], a2[h:], values=vb, logp=lpb)
            torch.cuda.synchronize()
            what = (spec, n, h)
            assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2) and torch.equal(a, a2), what
            assert torch.equal(lp, torch.cat([lpa, lpb])), what
            assert torch.equal(v[:h + 1], va) and torch.equal(v[h:], vb), what
            assert torch.equal(va[h], vb[0]), what                  # the bootstrap row IS the next call's row 0
            if net.kind == "gru":
                assert torch.equal(pw.hidden, ps.hidden), what
            ps.close(); split.close()
        assert int(d[first_done].sum()) > 0
        pw.close(); whole.close()


# ---- 6. values against fp64, 8. log-probs of a whole rollout ------------------------------------------------------------------
_WORST = {"mlp": [0.0, 0.0], "gru": [0.0, 0.0]}                    # [values, logp / bar]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("spec", NETS, ids=NET_IDS)
def test_values_and_logp_against_fp64(spec, layout):
    """value[t] within the engine's bar of the fp64 forward pass on the recorded observations (the bars of tests/test_gpu_policy_shapes.py
    for an output sum of these nets: a value is one more), and logp[t] within sum_k |z'_k| ATOL / std_k + the one-step bar of the same
    formula with the reference's mean.  The worst figures are printed per case."""
    import torch
    k = NETS.index(spec)
    for n in BATCHES:
        env = _env(n, layout)
        net = _Net(spec, _obs_scale(env), k)
        pol = net.build(env)
        _, o0 = _reset(env, pol)
        o, r, d, a = _bufs(env, T)
        v, lp = _ac_bufs(env, T)
        env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp)
        torch.cuda.synchronize()
        assert int(d[:-1].sum()) > 0
        hidden = []
        means, vref, z = net.reference(o0, o, d, hidden)
        what = "%s %s n=%d" % (spec, layout, n)
        assert_not_saturated(z, hidden, net.act, what)
        assert float(np.mean(np.abs(vref) > net.atol)) > 0.9, what  # teeth: the values are not all within the bar of zero
        verr = float(np.max(np.abs(v.cpu().numpy().astype(np.float64) - vref)))
        ref, bar = ac_ref.logp64(a.cpu().numpy(), means, LOG_STD, mean_atol=net.atol)
        lerr = np.abs(lp.cpu().numpy().astype(np.float64) - ref)
        frac = float((lerr / bar).max())
        w = _WORST[net.kind]
        w[0], w[1] = max(w[0], verr), max(w[1], frac)
        print("%s: worst |V - V_ref| %.3g (bar %.3g), worst logp error / bar %.3g; %s so far: %.3g, %.3g"
              % (what, verr, net.atol, frac, net.kind, w[0], w[1]))
        assert verr <= net.atol, (what, verr)
        assert (lerr <= bar).all(), (what, frac)
        assert float(ref.std()) > 0.5, what                         # teeth: the log-probs vary with the draws
        pol.close(); env.close()


def test_mlp_and_gru_policies_give_bit_equal_logp():
    """the log-probability depends only on the draws (keyed by seed, env and step) and on log_std"""
    import torch
    n = 2096
    em, eg = _env(n, "alias"), _env(n, "alias")
    scale = _obs_scale(em)
    _obs_scale(eg)
    nm, ng = _Net(NETS[1], scale, 1), _Net(NETS[4], scale, 4)
    pm, pg = nm.build(em), ng.build(eg)
    out = []
    for env, pol in ((em, pm), (eg, pg)):
        _reset(env, pol)
        o, r, d, a = _bufs(env, T)
        v, lp = _ac_bufs(env, T)
        env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp)
        torch.cuda.synchronize()
        out.append((lp, a))
    assert torch.equal(out[0][0], out[1][0])
    assert not torch.equal(out[0][1], out[1][1])                    # (different nets: different actions)
    for x in (pm, pg, em, eg):
        x.close()


# ---- 7. log-probs, one step, tight --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_std", [(-2, -2, -2, -2), (-1, -1, -1, -1), (0, 0, 0, 0), (-2, 0, -1, -0.5)],
                         ids=["m2", "m1", "0", "mixed"])
@pytest.mark.parametrize("spec", [NETS[1], NETS[4]], ids=["mlp240-80", "gru48-16-80"])
def test_one_step_logp_against_the_deterministic_twin(spec, log_std):
    """T = 1 from the same reset: the deterministic twin's action is the exploring twin's mean bit for bit, so z' = (a - m) / std recovers
    the draw to half an ulp of a, and the bar is derived (tests/ac_ref.py logp64), not measured.  No element is excluded."""
    import torch
    n, k = 2096, NETS.index(spec)
    det, exp = _env(n, "alias"), _env(n, "alias")
    net = _Net(spec, _obs_scale(det), k)
    _obs_scale(exp)
    pd, pe = net.build(det, log_std=None), net.build(exp, log_std=log_std)
    _reset(det, pd); _reset(exp, pe)
    o, r, d, m = _bufs(det, 1)
    o2, r2, d2, a = _bufs(exp, 1)
    v, lp = _ac_bufs(exp, 1)
    vd, _ = _ac_bufs(det, 1)
    det.rollout_policy_dev(pd, o, r, d, m, values=vd)
    exp.rollout_policy_dev(pe, o2, r2, d2, a, values=v, logp=lp)
    torch.cuda.synchronize()
    assert torch.equal(vd[0], v[0])                                 # the same observation, the same value
    assert not torch.equal(m, a)
    ref, bar = ac_ref.logp64(a[0].cpu().numpy(), m[0].cpu().numpy(), log_std)
    err = np.abs(lp[0].cpu().numpy().astype(np.float64) - ref)
    print("one-step logp %s log_std=%s: worst error / bar %.3g, worst error %.3g" % (spec, log_std, float((err / bar).max()), float(err.max())))
    assert (err <= bar).all(), float((err / bar).max())
    z = (a[0].cpu().numpy().astype(np.float64) - m[0].cpu().numpy()) / ac_ref.std_of(log_std)
    assert 0.9 < float(z.std()) < 1.1 and abs(float(z.mean())) < 0.1        # teeth: standard normal draws
    for x in (pd, pe, det, exp):
        x.close()


# ---- 9. GAE against fp64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.99, 0.0), (0.99, 1.0), (1.0, 0.95), (1.0, 1.0)])
def test_gae_against_fp64(gamma, lam):
    import torch
    n, steps = 2096, 64
    env = _env(n, "alias")
    net = _Net(NETS[0], _obs_scale(env), 0)
    pol = net.build(env)
    _reset(env, pol)
    o, r, d, a = _bufs(env, steps)
    v, lp = _ac_bufs(env, steps)
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp)
    adv, ret = torch.full_like(r, float("nan")), torch.full_like(r, float("nan"))
    env.gae_dev(r, d, v, gamma, lam, adv, ret)
    adv_only = torch.full_like(r, float("nan"))
    env.gae_dev(r, d, v, gamma, lam, adv_only)
    torch.cuda.synchronize()
    assert int(d.sum()) > n                                         # dones occur
    assert torch.equal(adv, adv_only)
    rn, dn, vn = r.cpu().numpy(), d.cpu().numpy(), v.cpu().numpy()
    aref, _ = ac_ref.gae64(rn, dn, vn, gamma, lam)
    bar = ac_ref.gae_bar(rn, vn, aref, gamma, lam)
    an, retn = adv.cpu().numpy(), ret.cpu().numpy()
    err = np.abs(an.astype(np.float64) - aref)
    print("gae gamma=%g lam=%g: worst error %.3g, worst error / bar %.3g" % (gamma, lam, float(err.max()), float((err / bar[None]).max())))
    assert (err <= bar[None]).all(), float((err / bar[None]).max())
    # a done row cuts: adv = r - V within one fp32 ulp of it
    cut = dn != 0
    want = rn.astype(np.float64) - vn[:steps]
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(an.astype(np.float64) - want)[cut] <= ulp[cut]).all()
    # ret - adv == values[:T] within one ulp
    diff = retn.astype(np.float64) - an.astype(np.float64) - vn[:steps]
    ulp_r = np.spacing(np.maximum(np.abs(retn), np.abs(vn[:steps])).astype(np.float32)).astype(np.float64)
    assert (np.abs(diff) <= ulp_r).all()
    assert float(np.abs(aref).max()) > 100 * float(bar.max())       # teeth
    pol.close(); env.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_env_and_policy_usable():
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import MLPPolicy
    n = 68
    env = _env(n, "alias")
    scale = _obs_scale(env)
    net = _Net(NETS[0], scale, 0)
    pol = net.build(env, value=False)
    _reset(env, pol)
    o, r, d, a = _bufs(env, 4)
    v, lp = _ac_bufs(env, 4)

    def usable(p):
        env.rollout_policy_dev(p, o, r, d, a)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all())

    with pytest.raises(_lib.GaqError, match="value head"):          # GAQ_ERR_STATE
        env.rollout_policy_dev(pol, o, r, d, a, values=v)
    usable(pol)
    env.rollout_policy_dev(pol, o, r, d, a, logp=lp)                 # log-probs need no head
    pol.set_value_head(*net.value)
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp)
    pol.set_value_head(None)
    with pytest.raises(_lib.GaqError, match="value head"):
        env.rollout_policy_dev(pol, o, r, d, a, values=v)
    pol.set_value_head(*net.value)
    pol.set_log_std(None)
    with pytest.raises(_lib.GaqError, match="deterministic"):       # GAQ_ERR_STATE
        env.rollout_policy_dev(pol, o, r, d, a, logp=lp)
    env.rollout_policy_dev(pol, o, r, d, a, values=v)                # values need no exploration
    usable(pol)
    pol.set_log_std(LOG_STD)
    for bad_v, bad_lp in ((v[:-1], None), (v.double(), None), (v.t().contiguous().t(), None), (v.cpu(), None), (None, lp[:-1]),
                          (None, torch.empty((4, n + 1), device=_dev())), (None, v)):
        with pytest.raises(ValueError, match="must be"):
            env.rollout_policy_dev(pol, o, r, d, a, values=bad_v, logp=bad_lp)
    usable(pol)
    # engines without an actor-critic form
    small = _mlp([48], 18, 1, scale)
    for engine in ("valu", "bf16"):
        p2 = MLPPolicy.from_arrays(env, small, "tanh", True, log_std=LOG_STD, engine=engine)
        with pytest.raises(ValueError, match=engine):
            p2.set_value_head(*net.value)
        with pytest.raises(ValueError, match="VALU" if engine == "valu" else "bf16"):       # GAQ_ERR_INVALID from the library itself
            _lib.check(_lib.load().gaq_policy_set_value_head(p2.handle, _lib.ptr(np.zeros(49, np.float32))))
        with pytest.raises(ValueError, match="VALU" if engine == "valu" else "bf16"):
            env.rollout_policy_dev(p2, o, r, d, a, logp=lp)
        with pytest.raises(ValueError, match="VALU" if engine == "valu" else "bf16"):
            env.rollout_policy_dev(p2, o, r, d, a, values=v)
        with pytest.raises(ValueError):
            MLPPolicy.from_arrays(env, small, "tanh", True, engine=engine, value=net.value)
        usable(p2)
        p2.close()
    p3 = MLPPolicy.from_arrays(env, small, "tanh", True, value=ac_ref.value_head(48, 3))
    assert p3.engine == "mfma"                                      # "auto" with a value head
    p4 = MLPPolicy.from_arrays(env, small, "tanh", True)
    assert p4.engine == "valu"                                      # ... and without one, what it always was
    p3.close(); p4.close()
    # gae
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp)
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    for g, l in ((1.5, 0.9), (0.9, 1.5), (-0.1, 0.9), (float("nan"), 0.9)):
        with pytest.raises(ValueError, match="gamma"):
            env.gae_dev(r, d, v, g, l, adv, ret)
    with pytest.raises(ValueError, match="overlap"):
        env.gae_dev(r, d, v, 0.99, 0.95, r, ret)
    with pytest.raises(ValueError, match="overlap"):
        env.gae_dev(r, d, v, 0.99, 0.95, adv, v[:4])
    with pytest.raises(ValueError, match="overlap"):
        env.gae_dev(r, d, v, 0.99, 0.95, adv, adv)
    with pytest.raises(ValueError, match="must be"):
        env.gae_dev(r, d, v[:-1], 0.99, 0.95, adv, ret)
    with pytest.raises(ValueError, match="must be"):
        env.gae_dev(r, d.float(), v, 0.99, 0.95, adv, ret)
    env.gae_dev(r, d, v, 0.99, 0.95, adv, ret)
    usable(pol)
    assert bool(torch.isfinite(adv).all()) and bool(torch.isfinite(ret).all())
    pol.close(); env.close()


def test_from_torch_with_a_value_module():
    import torch
    from gym_art_amd.policy import GRUPolicy, MLPPolicy
    nn = torch.nn
    torch.manual_seed(0)
    n = 68
    env = _env(n, "plain")
    trunk = nn.Sequential(nn.Linear(18, 64), nn.Tanh(), nn.Linear(64, 4), nn.Tanh())
    critic = nn.Linear(64, 1)
    pol = MLPPolicy.from_torch(trunk, env, log_std=LOG_STD, value=critic)
    assert pol.engine == "mfma"
    _, o0 = _reset(env, pol)
    o, r, d, a = _bufs(env, 3)
    v, lp = _ac_bufs(env, 3)
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp)
    torch.cuda.synchronize()
    with torch.no_grad():
        x = torch.cat([o0[None], o]).cpu()
        want = critic(trunk[1](trunk[0](x)))[..., 0]
    assert float((v.cpu() - want).abs().max()) < 1e-5
    with pytest.raises(ValueError, match=r"Linear\(W, 1\)"):
        MLPPolicy.from_torch(trunk, env, value=nn.Linear(64, 2))
    with pytest.raises(ValueError, match="weights"):
        MLPPolicy.from_torch(trunk, env, value=nn.Linear(32, 1))
    pol.close()
    cell, head, gcritic = nn.GRUCell(18, 32), nn.Linear(32, 4), nn.Linear(32, 1)
    pg = GRUPolicy.from_torch(cell, head, env, log_std=LOG_STD, value=gcritic)
    _, o0 = _reset(env, pg)
    env.rollout_policy_dev(pg, o, r, d, a, values=v, logp=lp)
    torch.cuda.synchronize()
    with torch.no_grad():
        want0 = gcritic(cell(o0.cpu(), torch.zeros(n, 32)))[..., 0]
    assert float((v[0].cpu() - want0).abs().max()) < 1e-5
    pg.close(); env.close()
