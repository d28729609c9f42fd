"""The wide learner on the device (gaq.h "the wide learner": gaq_policy_eval_wide_dev, gaq_policy_grad_ppo_wide_dev,
gaq_critic_grad_mse_wide_dev) over the case list of tests/policy_grad_wide.py: the case matrix under the bound 8 x torch fp32's error,
the narrow calls' bits on nets they take, the rollout's bits, the index-gathered form, determinism and a captured epoch with AdamDev, a
closed Adam loop, and the refusals.  Every figure a test bounds is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_grad_wide as W
from tests.policy_util import _bufs, _dev, environ

G, A = W.G, W.A
pytestmark = pytest.mark.gpu

REPR = {18: "xyz_vxyz_R_omega", 19: "xyz_vxyz_R_omega_h"}
AC_KEYS = ("obs", "actions", "logp_old", "adv", "ret", "v_old")
NAN = float("nan")


def _make_env(D=18, n=64):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(num_envs=n, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True, obs_repr=REPR[D])
    assert env.obs_dim == D
    return env


@pytest.fixture(scope="module")
def envs():
    made = {}

    def get(D=18):
        if D not in made:
            made[D] = _make_env(D)
        return made[D]
    yield get
    for e in made.values():
        e.close()


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=_dev())


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64),
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64))


def _net(env, case, inp, log_std=G.LOG_STD, value=None):
    """the case's handle on the device -- a critic, or a policy with the value head an AcCase has (value: override) -- and the
    normaliser it keeps alive"""
    from gym_art_amd.policy import MLPCritic, MLPPolicy, ObsNorm
    norm = None
    if case.norm:
        mean, var, eps, clip = G.norm_stats(case.D)
        norm = ObsNorm.from_stats(env, mean, var, 1.0, eps, clip)
    if not W.is_ac(case) and case.n_out == 1:
        crit = MLPCritic.from_arrays(env, inp["layers"], case.act)
        if norm is not None:
            crit.set_obs_norm(norm)
        return crit, norm
    head = W.is_ac(case) if value is None else value
    return MLPPolicy.from_arrays(env, inp["layers"], case.act, case.out_tanh, log_std=log_std, engine="mfma",
                                 value=(inp["wv"], inp["bv"]) if head else None, obs_norm=norm), norm


def _dev_inputs(inp):
    return {k: _t(v) for k, v in inp.items() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == W.R and k != "x"}


def _close(*handles):
    for h in handles:
        if h is not None:
            h.close()


def _ppo(pol, case, d, rows=None, lo=0, idx=None, **kw):
    """ppo_wide_grad_dev on the rows [lo, lo + rows) (idx: on the rows it names) with the case's coefficients"""
    head = pol.value_head is not None
    sl = slice(None) if idx is not None else slice(lo, d["obs"].shape[0] if rows is None else lo + rows)
    vclip = kw.pop("vclip", getattr(case, "vclip", 0.0)) if head else 0.0
    kw.setdefault("vf_coef", W.VF_COEF)
    kw.setdefault("ent_coef", W.ENT_COEF)
    return pol.ppo_wide_grad_dev(d["obs"][sl], d["actions"][sl], d["logp_old"][sl], d["adv"][sl], d["ret"][sl] if head else None,
                                 d["v_old"][sl] if head and vclip > 0 else None, idx=idx, clip=G.CLIP, vclip=vclip if vclip > 0 else None, **kw)


def _mse(crit, d, rows=None, lo=0, idx=None, **kw):
    sl = slice(None) if idx is not None else slice(lo, d["obs"].shape[0] if rows is None else lo + rows)
    return crit.mse_wide_grad_dev(d["obs"][sl], d["target"][sl], idx=idx, **kw)


def _check(name, d, net, rows, what):
    """one gradient call and one forward call of the case at `rows` against the shared reference; returns the worst error / bound"""
    case = W.CASES[name]
    ref, b = W.case_ref(name, rows), W.bounds(name, rows)
    if not W.is_ac(case) and case.n_out == 1:
        g, st = _mse(net, d, rows)
        st = _np(st)
        figs = [("grad", max(G.grad_errors(net.unpack(_np(g)), None, ref)), b[0]), ("V", G.rel(_np(net.values_dev(d["obs"][:rows])), ref["value"]), b[1]),
                ("loss", G.rel(st[0], ref["stats"][0]), b[2])]
        assert st[1] == rows, st
    else:
        g, gv, gls, st = _ppo(net, case, d, rows)
        lp, v = net.evaluate_wide_dev(d["obs"][:rows], d["actions"][:rows])
        st = _np(st)
        if W.is_ac(case):
            errs = A.grad_errors(net.unpack(_np(g)), _np(gv), _np(gls), ref)
            figs = [("grad", max(errs), b[0]), ("logp", G.rel(_np(lp), ref["logp"]), b[1]), ("V", G.rel(_np(v), ref["value"]), b[2]),
                    ("loss", G.rel(st[0], ref["stats"][0]), b[3]), ("kl", G.rel(st[2], ref["stats"][2]), b[4]),
                    ("L_V", G.rel(st[3], ref["stats"][3]), b[5])]
            assert st[4] == ref["stats"][4], (st, ref["stats"])     # the rows the value clip cut: exact
        else:
            assert gv is None and v is None
            errs = G.grad_errors(net.unpack(_np(g)), _np(gls), ref)
            figs = [("grad", max(errs), b[0]), ("logp", G.rel(_np(lp), ref["logp"]), b[1]), ("loss", G.rel(st[0], ref["stats"][0]), b[2]),
                    ("kl", G.rel(st[2], ref["stats"][2]), b[3])]
            assert st[3] == 0.0 and st[4] == 0.0, st                # no value loss without a head
        assert st[1] == ref["stats"][1] and st[5] == rows, (st, ref["stats"])     # the clipped rows and the row count: exact
    print("%s %s rows=%d: %s" % (name, what, rows, ", ".join("%s %.3g (bound %.3g)" % f for f in figs)))
    for what_, e, bound in figs:
        assert e <= bound, (name, what, rows, what_, e, bound)
    return max(e / bound for _, e, bound in figs), st


ALL = W.AC_CASES + W.POLICY_CASES + W.CRITIC_CASES


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_matrix(case, envs):
    """every net as actor-critic (with and without vclip), head-less policy and critic at 1, 63, 64, 65 and 453 rows, and 453 rows over 3
    workgroups: each parameter tensor, grad_value, grad_log_std, logp, V and the sums within 8 x torch fp32's error; the counts exact"""
    _, inp = W.case_inputs(case.name)
    net, norm = _net(envs(case.D), case, inp)
    d = _dev_inputs(inp)
    worst = 0.0
    for rows in W.ROWS:
        worst = max(worst, _check(case.name, d, net, rows, "default")[0])
    with environ(GAQ_GRAD_GROUPS="3"):
        e, st = _check(case.name, d, net, W.R, "3 groups")
    if W.is_ac(case):
        assert (0.1 * W.R <= st[4] <= 0.7 * W.R) if case.vclip > 0 else st[4] == 0
    print("%s: worst device error over its bound %.3f" % (case.name, max(worst, e)))
    _close(net, norm)


# ---- 2. on a net the narrow calls take, their bits ---------------------------------------------------------------------------------
NARROW = [([128, 128], "tanh", True), ([128, 128], "relu", False), ([48, 80, 32], "tanh", True), ([48, 80, 32], "relu", False)]


@pytest.mark.parametrize("widths,act,out_tanh", NARROW, ids=["%s-%s" % ("x".join(map(str, w)), a) for w, a, _ in NARROW])
def test_narrow_parity(widths, act, out_tanh, envs):
    import torch
    from gym_art_amd.policy import perm_dev
    env = envs()
    case = A.AcCase(widths, act, out_tanh, vclip=W.VCLIP)
    inp = A.inputs(case, 3)
    d = _dev_inputs(inp)
    idx = perm_dev(W.R, 11, device=_dev())[:300].contiguous()
    coef = dict(clip=G.CLIP, vclip=W.VCLIP, vf_coef=W.VF_COEF, ent_coef=W.ENT_COEF)
    pol, _ = _net(env, case, inp)
    for rows in (65, W.R):
        o, a, lo, adv, ret, vo = (d[k][:rows] for k in AC_KEYS)
        m1, m2 = (torch.full((rows, 4), NAN, device=_dev()) for _ in range(2))
        for x, y in zip(pol.evaluate_wide_dev(o, a, mean=m1) + (m1,), pol.evaluate_dev(o, a, mean=m2) + (m2,)):
            assert _bits(x, y), (rows, "evaluate")
        for x, y in zip(pol.ppo_wide_grad_dev(o, a, lo, adv, ret, vo, **coef), pol.ppo_ac_grad_dev(o, a, lo, adv, ret, vo, **coef)):
            assert _bits(x, y), (rows, "ppo")
    full = tuple(d[k] for k in AC_KEYS)
    for x, y in zip(pol.ppo_wide_grad_dev(*full, idx=idx, **coef), pol.ppo_ac_grad_idx_dev(idx, *full, **coef)):
        assert _bits(x, y), "ppo idx"
    pol.close()
    # without a head, and without the entropy term: ppo_grad_dev's grad and grad_log_std
    pol, _ = _net(env, case, inp, value=False)
    for rows in (65, W.R):
        o, a, lo, adv = (d[k][:rows] for k in AC_KEYS[:4])
        g, gv, gls, st = pol.ppo_wide_grad_dev(o, a, lo, adv, clip=G.CLIP, ent_coef=0.0)
        g0, gls0, st0 = pol.ppo_grad_dev(o, a, lo, adv, clip=G.CLIP)
        assert gv is None and _bits(g, g0) and _bits(gls, gls0) and torch.equal(st[:3], st0[:3]) and float(st[5]) == rows
        lp, v = pol.evaluate_wide_dev(o, a)
        assert v is None and _bits(lp, pol.logp_dev(o, a))
    pol.close()
    ccase = G.Case(widths, act, False, n_out=1)
    cinp = G.inputs(ccase, 3)
    cd = _dev_inputs(cinp)
    crit, _ = _net(env, ccase, cinp)
    for rows in (65, W.R):
        for x, y in zip(_mse(crit, cd, rows), crit.mse_grad_dev(cd["obs"][:rows], cd["target"][:rows])):
            assert _bits(x, y), (rows, "mse")
    for x, y in zip(_mse(crit, cd, idx=idx), crit.mse_grad_idx_dev(idx, cd["obs"], cd["target"])):
        assert _bits(x, y), "mse idx"
    torch.cuda.synchronize()
    crit.close()


# ---- 3. the rollout's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 453])
def test_rollouts_bits(n):
    """T = 4 steps (as calls of one step: a call of T > 1 needs N * obs_dim * 4 bytes to be a multiple of 16): from a deterministic
    rollout mean == the recorded actions and value == the recorded values; from an exploring one |logp - recorded| <= 1e-4 (the means
    are bit-equal, so only z is recomputed from the rounded action: log_std >= -1, |a| <= 8, as tests/test_gpu_policy_grad.py states)"""
    import torch
    T = 4
    env = _make_env(18, n)
    assert float(G.LOG_STD.min()) >= -1.0
    for name in ("ac-256x256-tanh", "ac-144-tanh"):
        case, inp = W.case_inputs(name)
        for explore in (False, True):
            pol, _ = _net(env, case, inp, log_std=G.LOG_STD if explore else None)
            o0 = torch.empty((n, 18), device=_dev())
            env.reset_dev(o0)
            prev = o0.clone()
            worst = 0.0
            for t in range(T):
                o, r, dn, a = _bufs(env, 1)
                v = torch.full((2, n), NAN, device=_dev())
                lp = torch.empty((1, n), device=_dev())
                env.rollout_policy_dev(pol, o, r, dn, a, values=v, logp=lp if explore else None)
                if not explore:
                    pol.set_log_std(G.LOG_STD)
                mean = torch.full((n, 4), NAN, device=_dev())
                got_lp, got_v = pol.evaluate_wide_dev(prev, a[0], mean=mean)
                torch.cuda.synchronize()
                assert _bits(got_v, v[0]), (name, explore, t)
                if explore:
                    assert float(a.abs().max()) <= 8.0
                    worst = max(worst, float((got_lp - lp[0]).abs().max()))
                else:
                    assert _bits(mean, a[0]), (name, t)
                    pol.set_log_std(None)
                prev = o[0].clone()
            if explore:
                print("%s n=%d: max |logp - recorded| = %.3g" % (name, n, worst))
                assert worst <= 1e-4, worst
            pol.close()
    env.close()


# ---- 4. the idx form ---------------------------------------------------------------------------------------------------------------
def _idx_vectors(src):
    import torch
    from gym_art_amd.policy import perm_dev
    perm = perm_dev(src, 5, device=_dev())
    rep = torch.cat([perm[:100], perm[:100], torch.full((7,), 64, dtype=torch.int32, device=_dev())]).contiguous()
    more = torch.cat([perm, perm[:70]]).contiguous()                # rows > src_rows
    return {"prefix": perm[:130].contiguous(), "repeats": rep, "rows > src": more}


@pytest.mark.parametrize("name", ["ac-256x256-relu-vclip", "policy-144-tanh", "critic-192x256x64-tanh"])
def test_idx_is_the_contiguous_call_on_gathered_rows(name, envs):
    """bit for bit, repeated indices and rows > src_rows included; three indices out of range are counted and contribute exactly 0; NaN in
    the rows no index names changes no output bit"""
    import torch
    case, inp = W.case_inputs(name)
    net, norm = _net(envs(case.D), case, inp)
    src = 200
    d = {k: v[:src].contiguous() for k, v in _dev_inputs(inp).items()}
    critic = not W.is_ac(case) and case.n_out == 1
    call = (lambda dd, *ar, **kw: _mse(net, dd, *ar, **kw)) if critic else (lambda dd, *ar, **kw: _ppo(net, case, dd, *ar, **kw))
    for what, idx in _idx_vectors(src).items():
        got = [x for x in call(d, idx=idx) if x is not None]
        gathered = {k: v[idx.long()].contiguous() for k, v in d.items()}
        want = [x for x in call(gathered) if x is not None]
        for x, y in zip(got[:-1], want[:-1]):
            assert _bits(x, y), (name, what)
        assert torch.equal(got[-1][:-1], want[-1]) and float(got[-1][-1]) == 0.0, (name, what)
    # out of range: counted, exactly 0 -- behind the good indices they move no row to another tile, so the call with them is the call
    # without them at the same scale, bit for bit (ent_coef = 0: the entropy term counts the call's rows, skipped or not)
    extra = {} if critic else {"ent_coef": 0.0}
    good = _idx_vectors(src)["prefix"]
    bad = torch.cat([good, _t([-1, src, 2 ** 31 - 1], torch.int32)]).contiguous()
    a = [x for x in call(d, idx=bad, scale=1.0 / 130, **extra) if x is not None]
    b = [x for x in call(d, idx=good, scale=1.0 / 130, **extra) if x is not None]
    for x, y in zip(a[:-1], b[:-1]):
        assert _bits(x, y), name
    sa, sb = _np(a[-1]), _np(b[-1])
    assert sa[-1] == 3.0 and sb[-1] == 0.0 and sa[-2] == 133.0 and sb[-2] == 130.0 and np.array_equal(sa[:-2], sb[:-2])
    only = _t([-1, src, -7], torch.int32)
    z = [x for x in call(d, idx=only, scale=1.0, **extra) if x is not None]
    assert all(not bool(x.any()) for x in z[:-1]) and float(z[-1][-1]) == 3.0 and not bool(z[-1][:-2].any())   # exactly 0
    # NaN outside the named rows (and past `rows` of a contiguous call) changes no bit
    named = torch.zeros(src, dtype=torch.bool, device=_dev())
    named[good.long()] = True
    nan = {k: v.clone() for k, v in d.items()}
    for v in nan.values():
        v[~named] = NAN
    for x, y in zip([t for t in call(nan, idx=good) if t is not None], [t for t in call(d, idx=good) if t is not None]):
        assert _bits(x, y) and not torch.isnan(x).any(), name
    nan = {k: v.clone() for k, v in d.items()}
    for v in nan.values():
        v[65:] = NAN
    for x, y in zip([t for t in call(nan, 65) if t is not None], [t for t in call(d, 65) if t is not None]):
        assert _bits(x, y) and not torch.isnan(x).any(), name
    torch.cuda.synchronize()
    _close(net, norm)


@pytest.mark.parametrize("name", ["ac-256x256-tanh-vclip", "policy-256-relu", "critic-256x128x128-relu"])
def test_partial_tile_adds_up(name, envs):
    """65 rows = the references of rows 0-63 and of row 64, added"""
    case, inp = W.case_inputs(name)
    net, norm = _net(envs(case.D), case, inp)
    d = _dev_inputs(inp)
    lo, hi = W.reference(case, inp, 64), W.reference(case, inp, 1, lo=64)
    want = dict(grads=[((a * 64 + c) / 65, (b * 64 + e) / 65) for (a, b), (c, e) in zip(lo["grads"], hi["grads"])])
    for k in ("gvalue", "glogstd"):
        if k in lo:
            want[k] = (lo[k] * 64 + hi[k]) / 65
    if W.is_ac(case):
        g, gv, gls, _ = _ppo(net, case, d, 65)
        errs = A.grad_errors(net.unpack(_np(g)), _np(gv), _np(gls), want)
    elif case.n_out == 4:
        g, _, gls, _ = _ppo(net, case, d, 65)
        errs = G.grad_errors(net.unpack(_np(g)), _np(gls), want)
    else:
        errs = G.grad_errors(net.unpack(_np(_mse(net, d, 65)[0])), None, want)
    print("%s partial tile: %.3g (bound %.3g)" % (name, max(errs), W.bounds(name, 65)[0]))
    assert max(errs) <= W.bounds(name, 65)[0]
    _close(net, norm)


# ---- 5. determinism and graphs -------------------------------------------------------------------------------------------------------
def test_determinism(envs):
    import torch
    case, inp = W.case_inputs("ac-256x256-tanh-vclip")
    pol, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    idx = _idx_vectors(W.R)["repeats"]
    for kw in ({}, {"idx": idx}):
        first = [x.clone() for x in _ppo(pol, case, d, **kw)]
        again = [x.clone() for x in _ppo(pol, case, d, **kw)]
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=_dev())
        with torch.cuda.stream(side):
            other = [x.clone() for x in _ppo(pol, case, d, **kw)]
        side.synchronize()
        for a, b, c in zip(first, again, other):
            assert _bits(a, b) and _bits(a, c)
    pol.close()


def test_a_captured_epoch_with_adam_replays_with_the_eager_bits(envs):
    """perm_dev(epoch_dev=) -> ppo_wide_grad_dev(idx=) -> AdamDev.step, log_std in device mode and learnt, captured after one warm-up
    call: three replays leave the weights, the value head, the log_std table, the moments and the step count bit-equal to three eager
    iterations from the same start.  AdamDev takes the wide gradients as they are."""
    import torch
    from gym_art_amd.policy import AdamDev, perm_dev
    case, inp = W.case_inputs("ac-256x256-relu-vclip")
    env = envs()
    src, mb, seed = W.R, 200, 77

    def read(pol, opt):
        sd = opt.state_dict()
        w, b = pol.get_value_head()
        return [pol.get_packed(), w, np.float32(b), pol.get_log_std(), sd["m"], sd["v"]], (sd["step"], sd["skipped"])

    def it(pol, opt, d, perm, word, outs):
        perm_dev(src, seed, epoch_dev=word, out=perm)
        _ppo(pol, case, d, idx=perm[:mb], grad=outs[0], grad_value=outs[1], grad_log_std=outs[2], stats=outs[3])
        opt.step(outs[0], outs[1], outs[2])
        word.add_(1)

    def make():
        pol, _ = _net(env, case, inp)
        pol.log_std_to_device()
        d = _dev_inputs(inp)
        perm = torch.empty((src,), dtype=torch.int32, device=_dev())
        word = torch.full((1,), 3, dtype=torch.int64, device=_dev())
        outs = [torch.empty_like(x) for x in _ppo(pol, case, d, idx=perm_dev(src, 1, device=_dev())[:mb])]     # the warm-up call
        return pol, AdamDev(pol, lr=1e-3, max_grad_norm=0.5), d, perm, word, outs

    eager = make()
    assert [g[0] for g in eager[1].groups] == ["weights", "value_head", "log_std"]      # AdamDev as it is: the packed layouts are the parents'
    perms = []
    for _ in range(3):
        it(*eager)
        perms.append(eager[3].clone())
    torch.cuda.synchronize()
    want = read(eager[0], eager[1])
    assert want[1] == (3, 0) and not torch.equal(perms[0], perms[1])
    cap = make()
    start = read(cap[0], cap[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        it(*cap)
    assert cap[1].step_count == 0
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap[3], perms[k]), k
    got = read(cap[0], cap[1])
    assert got[1] == (3, 0)
    for x, y in zip(got[0], want[0]):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert not np.array_equal(got[0][0], start[0][0]) and not np.array_equal(got[0][3], start[0][3])
    for x in (cap[1], cap[0], eager[1], eager[0]):
        x.close()


# ---- 6. a closed loop ------------------------------------------------------------------------------------------------------------------
def test_closed_loop_of_ten_adam_steps():
    """Ten AdamDev steps (lr 3e-4) on the 453 rows of 18-256-256 beside torch fp32 Adam on the twin module.  The parents' rule: each
    parameter tensor ends within 100 x the single-step bound, and the loss trajectories agree -- both fall, and at every step they
    differ by no more than the forward bound on the two loss sums plus, to first order, what the allowed parameter difference can move
    the loss by.  The stepped handle then rolls out as a fresh handle built from get_weights() does (_rolls_out_as_a_fresh_handle).

    The inputs are policy_grad_wide.loop_inputs(): the case at the first seed that keeps every row off the loss's branch edges before
    each of the ten steps of the fp64 reference trajectory (loop_conditions(): conditions()'s margins, held along the loop).  With the
    matrix's own seed of that case a ratio comes within 1.5e-5 of the clip range's edge before steps 8 and 9; two fp32 trajectories
    about 1e-4 apart (Adam's first step is lr * sign(g)) then take different branches, and on an MI355X the parameters ended 1.05e-3
    apart against 9.76e-4, with losses equal to 1e-6 through step 8 and 1.3e-4 apart at step 9, while the device gradient at the
    device's own parameters stayed as close to torch fp64 autograd as torch fp32 at every step: that comparison measured the edge,
    not the gradient call.  The bound is the rule's, from torch's single-step error on these inputs (LOOP_BASELINE)."""
    import torch
    from gym_art_amd.policy import AdamDev
    case, inp = W.loop_inputs()
    n = 64
    env = _make_env(18, n)
    pol, _ = _net(env, case, inp)
    d = _dev_inputs(inp)
    lr, steps = W.LOOP_LR, W.LOOP_STEPS
    ent_const = float(W.ENT_COEF * 2.0 * (1.0 + np.log(2.0 * np.pi)))
    opt = AdamDev(pol, lr=lr)
    loss_dev = []
    for _ in range(steps):
        ls = pol.get_log_std()
        g, gv, gls, st = _ppo(pol, case, d)
        loss_dev.append((float(st[0]) + W.VF_COEF * float(st[3])) / W.R - W.ENT_COEF * float(ls.astype(np.float64).sum()) - ent_const)
        opt.step(g, gv, gls)
    model = A.torch_model(case, inp, torch.float32)
    trunk, actor, critic, ls = model
    topt = torch.optim.Adam(list(trunk.parameters()) + list(actor.parameters()) + list(critic.parameters()) + [ls], lr=lr)
    loss_ref = []
    for _ in range(steps):
        topt.zero_grad()
        loss = A.torch_loss(case, inp, W.R, torch.float32, model)[0]
        loss.backward()
        loss_ref.append(float(loss.detach()))
        topt.step()
    print("closed loop: loss %s on the device, %s in torch" % (["%.6f" % x for x in loss_dev], ["%.6f" % x for x in loss_ref]))
    assert not np.array_equal(pol.get_weights()[0][0], inp["layers"][0][0])
    ls_end = pol.get_log_std()
    _rolls_out_as_a_fresh_handle(env, pol, case)                  # after the ten steps; it leaves pol exploring again
    pol.set_log_std(ls_end)
    bounds = W.loop_bounds()
    bound = 100.0 * bounds[0]
    layers = pol.get_weights()
    wv, bv = pol.get_value_head()
    got = [x for Wb in layers for x in Wb] + [np.concatenate([wv, [bv]]), pol.get_log_std()]
    lins = [m for m in trunk if hasattr(m, "weight")] + [actor]
    want = [_np(p) for m in lins for p in (m.weight, m.bias)] + [np.concatenate([_np(critic.weight).reshape(-1), _np(critic.bias).reshape(-1)]), _np(ls)]
    errs = [G.rel(a, b) for a, b in zip(got, want)]
    print("closed loop: parameters after %d steps differ by %.3g at most (bound %.3g)" % (steps, max(errs), bound))
    ref = W.reference(case, inp, W.R)
    g0 = [x for Wb in ref["grads"] for x in Wb] + [ref["gvalue"], ref["glogstd"]]
    th0 = [x for Wb in inp["layers"] for x in Wb] + [np.concatenate([inp["wv"], [inp["bv"]]]), G.LOG_STD]
    tol = (bounds[3] * abs(ref["stats"][0]) + W.VF_COEF * bounds[5] * ref["stats"][3]) / W.R \
        + sum(float(np.abs(g).sum()) * bound * float(np.abs(th).max()) for g, th in zip(g0, th0))
    diff = max(abs(a - b) for a, b in zip(loss_dev, loss_ref))
    print("closed loop: the trajectories differ by %.3g at most (tolerance %.3g)" % (diff, tol))
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    assert diff <= tol, (loss_dev, loss_ref, tol)
    assert max(errs) <= bound, (errs, bound)
    _close(opt, pol)
    env.close()


def _rolls_out_as_a_fresh_handle(env, pol, case):
    """a deterministic one-step rollout's actions and values are evaluate_wide_dev's mean and value on `pol` and on a fresh handle built
    from its get_weights() and get_value_head(), and the two handles agree bit for bit on the same observations"""
    import torch
    from gym_art_amd.policy import MLPPolicy
    n = env.num_envs
    layers = pol.get_weights()
    wv, bv = pol.get_value_head()
    # the stepped handle rolls out as a fresh one with its weights does
    fresh = MLPPolicy.from_arrays(env, layers, case.act, case.out_tanh, log_std=None, engine="mfma", value=(wv, bv))
    pol.set_log_std(None)
    outs = []
    for p in (pol, fresh):
        o0 = torch.empty((n, 18), device=_dev())
        env.reset_dev(o0)
        o, r, dn, a = _bufs(env, 1)
        v = torch.full((2, n), NAN, device=_dev())
        mean = torch.full((n, 4), NAN, device=_dev())
        obs0 = o0.clone()                                         # (the env may alias o0 as its current observation)
        env.rollout_policy_dev(p, o, r, dn, a, values=v)
        p.set_log_std(G.LOG_STD)
        _, val = p.evaluate_wide_dev(obs0, a[0], mean=mean)
        p.set_log_std(None)
        torch.cuda.synchronize()
        assert _bits(mean, a[0]) and _bits(val, v[0])
        outs.append((obs0, mean, val))
    # (the two resets need not draw the same states: compare the two handles on the SAME observations)
    pol.set_log_std(G.LOG_STD)
    fresh.set_log_std(G.LOG_STD)
    for x, y in zip(pol.evaluate_wide_dev(outs[1][0], outs[1][1]), fresh.evaluate_wide_dev(outs[1][0], outs[1][1])):
        assert _bits(x, y)
    pol.set_log_std(G.LOG_STD)
    fresh.close()


def test_rows_zero_gives_zeros(envs):
    import torch
    case, inp = W.case_inputs("ac-144-tanh-vclip")
    pol, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    out = [torch.full_like(x, 7.0) for x in _ppo(pol, case, d)]
    _ppo(pol, case, d, 0, grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])
    lp, v = pol.evaluate_wide_dev(d["obs"][:0], d["actions"][:0])
    torch.cuda.synchronize()
    assert lp.shape == (0,) and v.shape == (0,) and not any(bool(x.any()) for x in out)
    pol.close()


# ---- 7. the refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(envs):
    """each returns the stated code with its own text, launches nothing and leaves the NaN-filled outputs untouched; the first call
    repeated afterwards gives its bits"""
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPCritic, MLPPolicy
    from tests.enc_util import _cell, _encoder
    from tests.gru_util import _gru, _head
    from tests.policy_util import _layers
    env = envs()
    lib = _lib.load()
    case, inp = W.case_inputs("ac-144-tanh-vclip")
    d = {k: v[:65].contiguous() for k, v in _dev_inputs(inp).items()}
    o, a, lo, adv, ret, vo = (d[k] for k in AC_KEYS)
    cs = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    pol, _ = _net(env, case, inp)
    first = [x.clone() for x in _ppo(pol, case, d)]
    g, gv, gls, st = (torch.full_like(x, NAN) for x in first)
    lp_out, v_out = torch.full((65,), NAN, device=_dev()), torch.full((65,), NAN, device=_dev())
    idx = torch.arange(65, dtype=torch.int32, device=_dev())
    st7 = torch.full((7,), NAN, dtype=torch.float64, device=_dev())

    def raw(rows=65, idx=None, src=65, obs=o, ret=ret, v_old=vo, clip=0.2, vclip=0.2, vf=0.5, ent=0.01, scale=1.0, grad=g, grad_value=gv, grad_ls=gls,
            stats=st, handle=None):
        return lib.gaq_policy_grad_ppo_wide_dev(pol.handle if handle is None else handle, rows, _lib.ptr(idx), src, _lib.ptr(obs), _lib.ptr(a),
                                                _lib.ptr(lo), _lib.ptr(adv), _lib.ptr(ret), _lib.ptr(v_old), clip, vclip, vf, ent, scale,
                                                _lib.ptr(grad), _lib.ptr(grad_value), _lib.ptr(grad_ls), _lib.ptr(stats), cs)

    def ev(handle, value=v_out):
        return lib.gaq_policy_eval_wide_dev(handle, 65, _lib.ptr(o), _lib.ptr(a), _lib.ptr(lp_out), _lib.ptr(value), None, cs)

    def err():
        return lib.gaq_last_error()
    # the one limit: LDS and the sum, never "width"; the same text from all three calls
    for widths in ([256, 256, 32], [256, 256, 256]):
        big = MLPPolicy.from_arrays(env, _layers(widths), "tanh", True, log_std=G.LOG_STD, engine="mfma")
        assert raw(handle=big.handle, ret=None, v_old=None, grad_value=None) == -1 and b"LDS" in err() and b"sum" in err() and b"width" not in err()
        assert ev(big.handle, None) == -1 and b"LDS" in err() and b"width" not in err()
        big.close()
        lay = _layers(widths)
        crit = MLPCritic.from_arrays(env, lay[:-1] + [(lay[-1][0][:1], lay[-1][1][:1])], "tanh")
        assert lib.gaq_critic_grad_mse_wide_dev(crit.handle, 65, None, 65, _lib.ptr(o), _lib.ptr(lo), 1.0, _lib.ptr(g), _lib.ptr(st), cs) == -1
        assert b"LDS" in err() and b"sum" in err() and b"width" not in err()
        with pytest.raises(ValueError, match="LDS"):                # (GAQ_ERR_INVALID surfaces as ValueError)
            crit.mse_wide_grad_dev(o, lo)
        crit.close()
    # the engines
    for engine, text in (("bf16", b"bf16 engine"), ("valu", b"VALU engine")):
        other = MLPPolicy.from_arrays(env, _layers([64, 64]), "tanh", True, log_std=G.LOG_STD, engine=engine)
        assert raw(handle=other.handle, ret=None, v_old=None, grad_value=None) == -1 and text in err(), err()
        assert ev(other.handle, None) == -1 and text in err()
        other.close()
    gru = GRUPolicy(env, _gru(16, 18, 3), _head(16), "tanh", True, log_std=G.LOG_STD)
    assert raw(handle=gru.handle, ret=None, v_old=None, grad_value=None) == -1 and b"GRU" in err()
    assert ev(gru.handle, None) == -1 and b"GRU" in err()
    gru.close()
    # an encoder in front of the cell (gaq_policy_create_rnn_enc), either cell, with and without a value head: the cell's engine
    for cls, cell, text in ((GRUPolicy, "gru", b"GRU engine"), (LSTMPolicy, "lstm", b"LSTM engine")):
        for value in (None, (np.zeros(16, np.float32), 0.0)):
            enc = cls.with_encoder(env, _encoder(18, (32, 48)), _cell(cell, 16, 48), _head(16), log_std=G.LOG_STD, value=value)
            assert raw(handle=enc.handle, ret=None, v_old=None, grad_value=None) == -1 and text in err(), err()
            assert raw(handle=enc.handle) == -1 and text in err()
            assert ev(enc.handle, None) == -1 and text in err()
            assert ev(enc.handle) == -1 and text in err()
            enc.close()
    torch.cuda.synchronize()
    for x in (g, gv, gls, st, lp_out, v_out):                     # nothing above was launched
        assert bool(torch.isnan(x).all()), "a refused call wrote an output"
    # the value head and its arguments
    assert raw(ret=None) == -1 and b"needs ret" in err()
    assert raw(grad_value=None) == -1 and b"null" in err()
    assert ev(pol.handle, None) == -1 and b"null" in err()
    nohead, _ = _net(env, case, inp, value=False)
    for kw in (dict(v_old=None, grad_value=None), dict(ret=None, grad_value=None), dict(ret=None, v_old=None)):
        assert raw(handle=nohead.handle, **kw) == -1 and b"no value head" in err()
    assert ev(nohead.handle) == -1 and b"no value head" in err()
    with pytest.raises(ValueError, match="no value head"):
        nohead.ppo_wide_grad_dev(o, a, lo, adv, ret)
    with pytest.raises(ValueError, match="needs ret"):
        pol.ppo_wide_grad_dev(o, a, lo, adv)
    assert raw(handle=nohead.handle, ret=None, v_old=None, grad_value=None, vclip=0.2) == 0    # (vclip is checked and unused)
    torch.cuda.synchronize()
    assert not torch.isnan(g).any()
    g.fill_(NAN), gls.fill_(NAN), st.fill_(NAN)
    nohead.close()
    # the shared checks
    pol.set_log_std(None)
    assert raw() == -4 and b"no log_std set" in err()
    assert ev(pol.handle) == -4 and b"no log_std set" in err()
    pol.set_log_std(G.LOG_STD)
    for clip in (0.0, 1.0, NAN):
        assert raw(clip=clip) == -1 and b"clip_eps" in err()
    for vclip in (-0.1, NAN):
        assert raw(vclip=vclip) == -1 and b"vclip" in err()
    assert raw(vf=NAN) == -1 and b"NaN" in err()
    assert raw(ent=NAN) == -1 and b"NaN" in err()
    assert raw(scale=NAN) == -1 and b"NaN" in err()
    assert raw(v_old=None) == -1 and b"v_old" in err()
    with pytest.raises(ValueError, match="v_old"):
        pol.ppo_wide_grad_dev(o, a, lo, adv, ret, None, vclip=0.2)
    assert raw(rows=-1) == -1 and b"rows" in err()
    assert raw(obs=None) == -1 and b"null" in err()
    assert raw(idx=idx, src=0, stats=st7) == -1 and b"src_rows" in err()
    assert raw(grad=o.view(-1)[:g.numel()]) == -1 and b"overlap" in err()
    assert raw(grad_ls=g[4:8]) == -1 and b"overlap" in err()
    assert raw(grad_value=g[:gv.numel()]) == -1 and b"overlap" in err()
    assert raw(idx=lo.view(torch.int32), stats=st7, grad_value=lo[:gv.numel()]) == -1 and b"overlap" in err()
    assert raw(ret=ret.data_ptr() + 2) == -1 and b"aligned" in err()
    assert raw(stats=st.data_ptr() + 4) == -1 and b"aligned" in err()
    torch.cuda.synchronize()
    for x in (g, gv, gls, st, st7, lp_out, v_out):
        assert bool(torch.isnan(x).all()), "a refused call wrote an output"
    again = _ppo(pol, case, d)
    torch.cuda.synchronize()
    for x, y in zip(first, again):
        assert _bits(x, y)
    pol.close()
