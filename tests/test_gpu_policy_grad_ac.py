"""Shared-trunk actor-critic gradients on the device (gaq.h gaq_policy_eval_ac_dev, gaq_policy_grad_ppo_ac_dev) against the fp64
reference of tests/policy_grad_ac_ref.py: the case matrix under the bound 8 x torch fp32's error, the forward pass's bits against
logp_dev's and the rollout's recorded values, the policy-only limit against ppo_grad_dev bit for bit, partial tiles, determinism,
graphs and the scratch rule, a closed Adam loop, and the refusals.  Every figure a test bounds is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_grad_ac_ref as A
from tests.policy_util import _bufs, _dev, environ

G = A.G
pytestmark = pytest.mark.gpu

REPR = {18: "xyz_vxyz_R_omega", 19: "xyz_vxyz_R_omega_h"}
KEYS = ("obs", "actions", "logp_old", "adv", "ret", "v_old")


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


def _policy(env, case, inp, log_std=G.LOG_STD, value=True):
    """the case's policy with its value head on the device, and the normaliser it keeps alive"""
    from gym_art_amd.policy import MLPPolicy, ObsNorm
    norm = None
    if case.norm:
        mean, var, eps, clip = G.norm_stats(case.D)
        norm = ObsNorm.from_stats(env, mean, var, 1.0, eps, clip)
    return MLPPolicy.from_arrays(env, inp["layers"], case.act, case.out_tanh, log_std=log_std, engine="mfma",
                                 value=(inp["wv"], inp["bv"]) if value else None, obs_norm=norm), norm


def _dev_inputs(inp):
    return {k: _t(inp[k]) for k in KEYS}


def _call(pol, case, d, rows=None, lo=0, **kw):
    """ppo_ac_grad_dev on the rows [lo, lo + rows) with the case's coefficients"""
    rows = d["obs"].shape[0] - lo if rows is None else rows
    o, a, lp, adv, ret, vo = (d[k][lo:lo + rows] for k in KEYS)
    kw.setdefault("vf_coef", A.VF_COEF)
    kw.setdefault("ent_coef", A.ENT_COEF)
    vclip = kw.pop("vclip", case.vclip)
    return pol.ppo_ac_grad_dev(o, a, lp, adv, ret, vo if vclip > 0 else None, clip=A.CLIP, vclip=vclip if vclip > 0 else None, **kw)


def _check(case, inp, d, pol, rows, what):
    ref = A.ppo_ac(case, inp, rows)
    bg, blp, bv, bloss, bkl, blv = A.bounds(case.name, rows)
    g, gv, gls, st = _call(pol, case, d, rows)
    lp, v = pol.evaluate_dev(d["obs"][:rows], d["actions"][:rows])
    errs = A.grad_errors(pol.unpack(_np(g)), _np(gv), _np(gls), ref)
    st = _np(st)
    e_lp, e_v = G.rel(_np(lp), ref["logp"]), G.rel(_np(v), ref["value"])
    e_loss, e_kl, e_lv = G.rel(st[0], ref["stats"][0]), G.rel(st[2], ref["stats"][2]), G.rel(st[3], ref["stats"][3])
    print("%s %s rows=%d: grad %.3g (bound %.3g) [value head %.3g, log_std %.3g] logp %.3g (%.3g) V %.3g (%.3g) loss %.3g (%.3g) "
          "kl %.3g (%.3g) L_V %.3g (%.3g) cut %d" % (case.name, what, rows, max(errs), bg, errs[-2], errs[-1], e_lp, blp, e_v, bv, e_loss,
                                                   bloss, e_kl, bkl, e_lv, blv, st[4]))
    assert max(errs) <= bg, (case.name, what, rows, errs, bg)
    assert e_lp <= blp and e_v <= bv and e_loss <= bloss and e_kl <= bkl and e_lv <= blv, (case.name, what, rows)
    assert st[1] == ref["stats"][1] and st[4] == ref["stats"][4] and st[5] == rows, (st, ref["stats"])     # the counts are exact
    return max(errs), st[4]


@pytest.mark.parametrize("case", A.AC_CASES, ids=[c.name for c in A.AC_CASES])
def test_case_matrix(case, envs):
    """every net x style x observation form x value clip at 1, 63, 64, 65 and 453 rows, and 453 rows over 3 workgroups: each parameter
    tensor, grad_value, grad_log_std, logp, V and the sums within 8 x torch fp32's error; the clipped and cut row counts exact"""
    _, inp = A.case_inputs(case.name)
    assert A.conditions(case, inp) is None
    pol, norm = _policy(envs(case.D), case, inp)
    d = _dev_inputs(inp)
    worst = 0.0
    for rows in A.ROWS:
        worst = max(worst, _check(case, inp, d, pol, rows, "default")[0])
    with environ(GAQ_GRAD_GROUPS="3"):
        e, cut = _check(case, inp, d, pol, A.R, "3 groups")
    assert (0.1 * A.R <= cut <= 0.7 * A.R) if case.vclip > 0 else cut == 0       # a case cannot pass by having no clipped rows
    print("%s: worst gradient error %.3g" % (case.name, max(worst, e)))
    pol.close()
    if norm is not None:
        norm.close()


def test_evaluate_is_logp_dev_bit_for_bit(envs):
    import torch
    for name in ("ac-128x128x128-tanh", "ac-48x80x32-relu", "ac-64x64-relu-norm"):
        case, inp = A.case_inputs(name)
        pol, norm = _policy(envs(case.D), case, inp)
        d = _dev_inputs(inp)
        m1, m2 = (torch.full((A.R, 4), float("nan"), device=_dev()) for _ in range(2))
        lp1 = pol.logp_dev(d["obs"], d["actions"], mean=m1)
        lp2, _ = pol.evaluate_dev(d["obs"], d["actions"], mean=m2)
        torch.cuda.synchronize()
        assert torch.equal(lp1.view(torch.int32), lp2.view(torch.int32)) and torch.equal(m1.view(torch.int32), m2.view(torch.int32)), name
        pol.close()
        if norm is not None:
            norm.close()


@pytest.mark.parametrize("n", [65, 453])
def test_value_is_the_rollouts_recorded_value_bit_for_bit(n):
    """evaluate_dev's value on the observation each action was computed from == the values rollout_policy_dev(values=, logp=) recorded,
    over T = 3 steps on two nets.  (The three steps run as calls of one step each: a call of T > 1 needs N * obs_dim * 4 bytes to be a
    multiple of 16, which 18 floats give at neither 65 nor 453 envs.)"""
    import torch
    T = 3
    env = _make_env(18, n)
    for name in ("ac-128x128x128-tanh", "ac-48x80x32-relu"):
        case, inp = A.case_inputs(name)
        pol, _ = _policy(env, case, inp)
        o0 = torch.empty((n, 18), device=_dev())
        env.reset_dev(o0)
        prev = o0.clone()
        for t in range(T):
            o, r, dn, a = _bufs(env, 1)
            v = torch.full((2, n), float("nan"), device=_dev())
            lp = torch.empty((1, n), device=_dev())
            env.rollout_policy_dev(pol, o, r, dn, a, values=v, logp=lp)
            _, got_v = pol.evaluate_dev(prev, a[0])
            _, boot = pol.evaluate_dev(o[0], a[0])
            torch.cuda.synchronize()
            assert torch.equal(got_v.view(torch.int32), v[0].view(torch.int32)), (name, t)
            assert torch.equal(boot.view(torch.int32), v[1].view(torch.int32)) or bool(dn.any()), (name, t)
            prev = o[0].clone()
        pol.close()
    env.close()


def test_without_the_value_terms_it_is_ppo_grad_dev_bit_for_bit(envs):
    """vf_coef = 0, ent_coef = 0: grad, grad_log_std and the first three statistics are ppo_grad_dev's bits, grad_value exactly zero"""
    import torch
    for name in ("ac-128x128x128-relu-vclip", "ac-16-tanh", "ac-64x64-tanh-d19-vclip"):
        case, inp = A.case_inputs(name)
        pol, _ = _policy(envs(case.D), case, inp)
        d = _dev_inputs(inp)
        for rows in (65, A.R):
            g, gv, gls, st = _call(pol, case, d, rows, vf_coef=0.0, ent_coef=0.0)
            g0, gls0, st0 = pol.ppo_grad_dev(d["obs"][:rows], d["actions"][:rows], d["logp_old"][:rows], d["adv"][:rows], clip=A.CLIP)
            torch.cuda.synchronize()
            assert torch.equal(g.view(torch.int32), g0.view(torch.int32)) and torch.equal(gls.view(torch.int32), gls0.view(torch.int32)), name
            assert torch.equal(st[:3], st0[:3]) and float(st[5]) == rows == float(st0[3])
            assert not gv.any(), name
        pol.close()


def test_partial_tiles(envs):
    """65 rows = the references of rows 0-63 and of row 64 added up; NaN in every input past `rows`, ret and v_old included, changes no
    output bit"""
    import torch
    case, inp = A.case_inputs("ac-48x80x32-relu-vclip")
    pol, _ = _policy(envs(), case, inp)
    d = _dev_inputs(inp)
    sc = 1.0 / 65
    lo, hi = A.ppo_ac(case, inp, 64, scale=sc), A.ppo_ac(case, inp, 1, scale=sc, lo=64)
    want = dict(grads=[(a + c, b + e) for (a, b), (c, e) in zip(lo["grads"], hi["grads"])], gvalue=lo["gvalue"] + hi["gvalue"],
                glogstd=lo["glogstd"] + hi["glogstd"])
    out = _call(pol, case, d, 65)
    errs = A.grad_errors(pol.unpack(_np(out[0])), _np(out[1]), _np(out[2]), want)
    print("partial tile: %.3g (bound %.3g)" % (max(errs), A.bounds(case.name, 65)[0]))
    assert max(errs) <= A.bounds(case.name, 65)[0]
    assert hi["dv"][0] != 0.0                                     # the partial tile's only row has a value delta
    ev = pol.evaluate_dev(d["obs"][:65], d["actions"][:65])
    nan = {k: v.clone() for k, v in d.items()}
    for v in nan.values():
        v[65:] = float("nan")
    out2 = _call(pol, case, nan, 65)
    ev2 = pol.evaluate_dev(nan["obs"][:65], nan["actions"][:65])
    torch.cuda.synchronize()
    for a, b in zip(tuple(out) + tuple(ev), tuple(out2) + tuple(ev2)):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    pol.close()


def test_determinism(envs):
    """the same call twice, and once on another stream: equal bits"""
    import torch
    case, inp = A.case_inputs("ac-128x128x128-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    d = _dev_inputs(inp)
    first = [x.clone() for x in _call(pol, case, d)]
    again = [x.clone() for x in _call(pol, case, d)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        other = [x.clone() for x in _call(pol, case, d)]
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    pol.close()


def test_captured_in_a_graph(envs):
    """ppo_ac_grad_dev captured after one warm-up call replays with the eager call's bits, also on new contents of the same buffers"""
    import torch
    case, inp = A.case_inputs("ac-128x128x128-tanh-vclip")       # (more than 64 KiB of LDS: the launch raises the kernel's limit)
    pol, _ = _policy(envs(), case, inp)
    d = _dev_inputs(inp)
    eager = [x.clone() for x in _call(pol, case, d)]
    _call(pol, case, d, 65)                                       # the warm-up may be of any size
    out = [torch.empty_like(x) for x in eager]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call(pol, case, d, grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])
    for x in out:
        x.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    flipped = [x.clone() for x in _call(pol, case, dict(d, adv=-d["adv"], ret=d["ret"] + 0.5))]
    d["adv"].neg_()
    d["ret"].add_(0.5)                                            # new contents, the same buffers
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, flipped):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], eager[0]) and not torch.equal(out[1], eager[1])
    pol.close()


def test_a_graph_of_ppo_grad_dev_survives_an_actor_critic_call(envs):
    """the scratch is sized for the actor-critic form from the handle's first gradient call of any form: a graph captured around
    ppo_grad_dev on a fresh handle replays with the same bits after an eager ppo_ac_grad_dev on that handle"""
    import torch
    case, inp = A.case_inputs("ac-128x128x128-relu-vclip")
    pol, _ = _policy(envs(), case, inp)                           # a fresh handle: its first gradient call is ppo_grad_dev's warm-up
    d = _dev_inputs(inp)
    args = (d["obs"], d["actions"], d["logp_old"], d["adv"])
    eager = [x.clone() for x in pol.ppo_grad_dev(*args, clip=A.CLIP)]
    out = [torch.empty_like(x) for x in eager]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pol.ppo_grad_dev(*args, clip=A.CLIP, grad=out[0], grad_log_std=out[1], stats=out[2])
    ac = [x.clone() for x in _call(pol, case, d)]                 # an eager actor-critic call in between
    for x in out:
        x.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    again = _call(pol, case, d)
    torch.cuda.synchronize()
    for a, b in zip(ac, again):
        assert torch.equal(a, b)
    pol.close()


def _pack_torch(layers):
    import torch
    out = []
    for W, b in layers[:-1]:
        o, i = W.shape
        out += [W.reshape(o // 16, 16, i).permute(0, 2, 1).reshape(-1), b]
    out += [layers[-1][0].T.reshape(-1), layers[-1][1]]
    return torch.cat(out).contiguous()


def test_closed_loop_of_ten_adam_steps(envs):
    """Ten Adam steps (lr 3e-4) on the 453 rows: device gradients -> unpack / grad_value -> param.grad -> set_weights_dev /
    set_value_head_dev, beside the same ten steps of torch fp32 autograd on the twin module (a shared trunk with two Linear heads).
    Each parameter tensor ends within 100 x the single-step bound, as tests/test_gpu_policy_grad.py's loop holds it.  The loss
    trajectories agree: both fall, and at every step they differ by no more than the forward bound on the two loss sums plus, to first
    order, what the allowed parameter difference can move the loss by: sum over the tensors of |g|_1 x 100 x bound x max|theta|, g the
    reference's gradient at the start (ten steps of 3e-4 do not move it far)."""
    import torch
    case, inp = A.case_inputs("ac-64x64-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    d = _dev_inputs(inp)
    lr, steps = 3e-4, 10
    ent_const = float(A.ENT_COEF * 2.0 * (1.0 + np.log(2.0 * np.pi)))

    params = [(_t(W).clone().requires_grad_(True), _t(b).clone().requires_grad_(True)) for W, b in inp["layers"]]
    head = _t(np.concatenate([inp["wv"], [inp["bv"]]]).astype(np.float32)).clone().requires_grad_(True)
    log_std = _t(G.LOG_STD).clone().requires_grad_(True)
    leaves = [p for Wb in params for p in Wb] + [head, log_std]
    opt = torch.optim.Adam(leaves, lr=lr)
    loss_dev = []
    for _ in range(steps):
        with torch.no_grad():
            pol.set_weights_dev(_pack_torch(params))
            pol.set_value_head_dev(head.detach())
        pol.set_log_std(_np(log_std))
        g, gv, gls, st = _call(pol, case, d)
        for (W, b), (gW, gb) in zip(params, pol.unpack(g)):
            W.grad, b.grad = gW.contiguous(), gb.contiguous()
        head.grad, log_std.grad = gv.clone(), gls.clone()
        loss_dev.append((float(st[0]) + A.VF_COEF * float(st[3])) / A.R - A.ENT_COEF * float(log_std.detach().double().sum()) - ent_const)
        opt.step()
    model = A.torch_model(case, inp, torch.float32)
    trunk, actor, critic, ls = model
    opt = torch.optim.Adam(list(trunk.parameters()) + list(actor.parameters()) + list(critic.parameters()) + [ls], lr=lr)
    loss_ref = []
    for _ in range(steps):
        opt.zero_grad()
        loss = A.torch_loss(case, inp, A.R, torch.float32, model)[0]
        loss.backward()
        loss_ref.append(float(loss.detach()))
        opt.step()
    print("closed loop: loss %s on the device, %s in torch" % (["%.6f" % x for x in loss_dev], ["%.6f" % x for x in loss_ref]))
    bounds = A.bounds(case.name, A.R)
    bound = 100.0 * bounds[0]
    lins = [m for m in trunk if hasattr(m, "weight")] + [actor]
    got = [p for Wb in params for p in Wb] + [head, log_std]
    want = [p for m in lins for p in (m.weight, m.bias)] + [torch.cat([critic.weight.reshape(-1), critic.bias.reshape(-1)]), ls]
    errs = [G.rel(_np(a), _np(b)) for a, b in zip(got, want)]
    print("closed loop: parameters after %d steps differ by %.3g at most (bound %.3g)" % (steps, max(errs), bound))
    assert max(errs) <= bound, (errs, bound)
    ref = A.ppo_ac(case, inp, A.R)
    g0 = [x for Wb in ref["grads"] for x in Wb] + [ref["gvalue"], ref["glogstd"]]
    th0 = [x for Wb in inp["layers"] for x in Wb] + [np.concatenate([inp["wv"], [inp["bv"]]]), G.LOG_STD]
    tol = (bounds[3] * abs(ref["stats"][0]) + A.VF_COEF * bounds[5] * ref["stats"][3]) / A.R \
        + sum(float(np.abs(g).sum()) * bound * float(np.abs(th).max()) for g, th in zip(g0, th0))
    diff = max(abs(a - b) for a, b in zip(loss_dev, loss_ref))
    print("closed loop: the trajectories differ by %.3g at most (tolerance %.3g)" % (diff, tol))
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    assert diff <= tol, (loss_dev, loss_ref, tol)
    pol.close()


def test_rows_zero_gives_zeros(envs):
    import torch
    case, inp = A.case_inputs("ac-16-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    d = _dev_inputs(inp)
    out = [torch.full_like(x, 7.0) for x in _call(pol, case, d)]
    _call(pol, case, d, 0, grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])
    lp, v = pol.evaluate_dev(d["obs"][:0], d["actions"][:0])
    torch.cuda.synchronize()
    assert lp.shape == (0,) and v.shape == (0,) and not any(bool(x.any()) for x in out)
    pol.close()


def test_refusals(envs):
    """each returns the stated code with the named text, launches nothing, and the first call repeated afterwards gives its bits"""
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import GRUPolicy
    from tests.gru_util import _gru, _head
    env = envs()
    lib = _lib.load()
    case, inp = A.case_inputs("ac-16-tanh-vclip")
    d = {k: v[:65].contiguous() for k, v in _dev_inputs(inp).items()}
    o, a, lo, adv, ret, vo = (d[k] for k in KEYS)
    cs = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)

    pol, _ = _policy(env, case, inp)
    first = [x.clone() for x in _call(pol, case, d)]
    ev = [x.clone() for x in pol.evaluate_dev(o, a)]
    g, gv, gls, st = (x.clone() for x in first)

    def raw(rows=65, obs=o, ret=ret, v_old=vo, clip=0.2, vclip=0.2, vf=0.5, ent=0.01, scale=1.0, grad=g, grad_value=gv, grad_ls=gls, stats=st,
            handle=None):
        return lib.gaq_policy_grad_ppo_ac_dev(pol.handle if handle is None else handle, rows, _lib.ptr(obs), _lib.ptr(a), _lib.ptr(lo),
                                              _lib.ptr(adv), _lib.ptr(ret), _lib.ptr(v_old), clip, vclip, vf, ent, scale, _lib.ptr(grad),
                                              _lib.ptr(grad_value), _lib.ptr(grad_ls), _lib.ptr(stats), cs)

    def err():
        return lib.gaq_last_error()
    # no value head: GAQ_ERR_STATE, the text names the value head; no log_std: GAQ_ERR_STATE, the existing text
    pol.set_value_head(None)
    assert raw() == -4 and b"value head" in err()
    assert lib.gaq_policy_eval_ac_dev(pol.handle, 65, _lib.ptr(o), _lib.ptr(a), _lib.ptr(lo.clone()), _lib.ptr(adv.clone()), None, cs) == -4
    assert b"value head" in err()
    with pytest.raises(_lib.GaqError, match="value head"):
        _call(pol, case, d)
    pol.set_value_head(inp["wv"], inp["bv"])
    pol.set_log_std(None)
    assert raw() == -4 and b"no log_std set" in err()
    with pytest.raises(_lib.GaqError, match="log_std"):
        pol.evaluate_dev(o, a)
    pol.set_log_std(G.LOG_STD)
    for clip in (0.0, 1.0, float("nan")):
        assert raw(clip=clip) == -1 and b"clip_eps" in err()
    for vclip in (-0.1, float("nan")):
        assert raw(vclip=vclip) == -1 and b"vclip" in err()
    assert raw(vf=float("nan")) == -1 and b"NaN" in err()
    assert raw(ent=float("nan")) == -1 and b"NaN" in err()
    assert raw(scale=float("nan")) == -1 and b"NaN" in err()
    assert raw(v_old=None) == -1 and b"v_old" in err()
    assert raw(v_old=None, vclip=0.0) == 0                         # (v_old may be null without the clip)
    with pytest.raises(ValueError, match="v_old"):
        pol.ppo_ac_grad_dev(o, a, lo, adv, ret, None, vclip=0.2)
    assert raw(rows=-1) == -1 and b"rows" in err()
    assert raw(obs=None) == -1 and b"null" in err()
    assert raw(ret=None) == -1 and b"null" in err()
    assert raw(grad_value=None) == -1 and b"null" in err()
    assert raw(grad=o.view(-1)[:g.numel()]) == -1 and b"overlap" in err()          # an output over an input
    assert raw(grad_value=ret[:gv.numel()]) == -1 and b"overlap" in err()
    assert raw(grad_ls=g[4:8]) == -1 and b"overlap" in err()                        # two outputs
    assert raw(grad_value=g[:gv.numel()]) == -1 and b"overlap" in err()
    assert raw(ret=ret.data_ptr() + 2) == -1 and b"aligned" in err()
    assert raw(stats=st.data_ptr() + 4) == -1 and b"aligned" in err()
    # the engine and width refusals are policy_grad_view's: a GRU policy with a value head is refused with the "GRU" text
    gru = GRUPolicy(env, _gru(16, 18, 3), _head(16), "tanh", True, log_std=G.LOG_STD)
    W = lib.gaq_policy_value_width(gru.handle)
    gru.set_value_head(np.zeros(W, np.float32), 0.0)
    assert raw(handle=gru.handle) == -1 and b"GRU" in err()
    assert lib.gaq_policy_eval_ac_dev(gru.handle, 65, _lib.ptr(o), _lib.ptr(a), _lib.ptr(lo.clone()), _lib.ptr(adv.clone()), None, cs) == -1
    assert b"GRU" in err()
    gru.close()
    # the handle is as usable as before: the first call's bits
    again = _call(pol, case, d)
    ev2 = pol.evaluate_dev(o, a)
    torch.cuda.synchronize()
    for x, y in zip(first + ev, list(again) + list(ev2)):
        assert torch.equal(x, y)
    pol.close()
