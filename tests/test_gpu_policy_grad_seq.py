"""The recurrent learner on the device (gaq.h gaq_policy_eval_seq_dev, gaq_policy_grad_ppo_seq_dev) against the fp64 reference of
tests/policy_grad_seq_ref.py: the case matrix under the bound 8 x torch fp32's error, the forward pass's bits against a GRUPolicy
rollout's recorded actions, values and hidden state, splitting in time, cuts at dones, independent sequences, the limits of the loss,
determinism and graphs, a closed Adam loop, and the refusals.  Every figure a test bounds is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_grad_seq_ref as R
from tests.policy_util import _bufs, _dev, environ

G = R.G
pytestmark = pytest.mark.gpu

REPR = {18: "xyz_vxyz_R_omega", 19: "xyz_vxyz_R_omega_h"}
KEYS = ("obs", "actions", "done", "h0", "logp_old", "adv", "ret", "v_old")


def _make_env(D=18, n=64, ep_time=0.15):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(num_envs=n, ep_time=ep_time, seed=7, init_random_state=True, auto_reset=True, alias_obs=True, obs_repr=REPR[D])
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
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _policy(env, case, inp, log_std=R.LOG_STD, value=None):
    """the case's GRU policy (with its value head unless the case has none) and the normaliser it keeps alive"""
    from gym_art_amd.policy import GRUPolicy, ObsNorm
    value = case.value if value is None else value
    pol = GRUPolicy(env, inp["gru"], inp["head"], case.act, case.out_tanh, log_std=log_std, value=(inp["wv"], inp["bv"]) if value else None)
    norm = None
    if case.norm:
        mean, var, eps, clip = G.norm_stats(case.D)
        norm = ObsNorm.from_stats(env, mean, var, 1.0, eps, clip)
        pol.set_obs_norm(norm)
    return pol, norm


def _dev_inputs(inp, T, S, t_lo=0, s_lo=0, done=None):
    """the steps [t_lo, t_lo + T) of the sequences [s_lo, s_lo + S) as contiguous device tensors"""
    src = dict(inp, done=inp["done"] if done is None else done)
    d = {k: _t(src[k][t_lo:t_lo + T, s_lo:s_lo + S]) for k in KEYS if k != "h0"}
    d["h0"] = _t(inp["h0"][s_lo:s_lo + S])
    return d


def _call(pol, case, d, **kw):
    """ppo_seq_grad_dev with the case's coefficients"""
    kw.setdefault("vf_coef", R.VF_COEF)
    kw.setdefault("ent_coef", R.ENT_COEF)
    vclip = kw.pop("vclip", case.vclip)
    head = pol.value_head is not None
    return pol.ppo_seq_grad_dev(d["obs"], d["actions"], d["done"], d["h0"], d["logp_old"], d["adv"], d["ret"] if head else None,
                                d["v_old"] if head and vclip > 0 else None, clip=R.CLIP, vclip=vclip if vclip > 0 else None, **kw)


def _errors(pol, out, ref):
    gru, head = pol.unpack(_np(out[0]))
    return R.grad_errors(gru, head, None if out[1] is None else _np(out[1]), _np(out[2]), ref)


def _check(case, inp, pol, T, S, what):
    ref = R.case_ref(case.name, T, S)
    bg, blp, bv, bloss, bkl, blv = R.bounds(case.name, T, S)
    d = _dev_inputs(inp, T, S)
    out = _call(pol, case, d)
    lp, v = pol.evaluate_seq_dev(d["obs"], d["actions"], d["done"], d["h0"])
    errs = _errors(pol, out, ref)
    st = _np(out[3])
    e_lp = G.rel(_np(lp), ref["logp"])
    e_v = G.rel(_np(v), ref["value"]) if case.value else 0.0
    e_loss, e_kl = G.rel(st[0], ref["stats"][0]), G.rel(st[2], ref["stats"][2])
    e_lv = G.rel(st[3], ref["stats"][3]) if case.value else float(st[3])
    names = ["W_ih", "b_ih", "W_hh", "b_hh"]
    print("%s %s (T, S) = (%d, %d): grad %.3g (bound %.3g) [%s | rest %.3g] logp %.3g (%.3g) V %.3g (%.3g) loss %.3g (%.3g) kl %.3g (%.3g) "
          "L_V %.3g (%.3g) clipped %d cut %d" % (case.name, what, T, S, max(errs), bg, " ".join("%s %.3g" % x for x in zip(names, errs)),
                                                max(errs[4:]), e_lp, blp, e_v, bv, e_loss, bloss, e_kl, bkl, e_lv, blv, st[1], st[4]))
    assert max(errs) <= bg, (case.name, what, T, S, errs, bg)
    assert e_lp <= blp and e_v <= bv and e_loss <= bloss and e_kl <= bkl and e_lv <= blv, (case.name, what, T, S)
    assert st[1] == ref["stats"][1] and st[4] == ref["stats"][4] and st[5] == T * S, (st, ref["stats"])     # the counts are exact
    if not case.value:
        assert v is None and out[1] is None and st[3] == 0.0 and st[4] == 0.0
    return max(errs)


@pytest.mark.parametrize("case", R.SEQ_CASES, ids=[c.name for c in R.SEQ_CASES])
def test_case_matrix(case, envs):
    """every (H, head) x style x observation form x value clip (and two nets without a value head) at every (T, S), and (6, 130) over 2
    workgroups: each parameter tensor -- W_ih, b_ih, W_hh, b_hh separately -- grad_value, grad_log_std, logp, V and the sums within
    8 x torch fp32's error; the clipped and cut counts and T S exact"""
    _, inp = R.case_inputs(case.name)
    assert R.conditions(case, inp) is None
    pol, norm = _policy(envs(case.D), case, inp)
    worst = 0.0
    for T, S in R.CONFIGS:
        worst = max(worst, _check(case, inp, pol, T, S, "default"))
    with environ(GAQ_GRAD_GROUPS="2"):
        worst = max(worst, _check(case, inp, pol, R.TMAX, R.SMAX, "2 groups"))
    print("%s: worst gradient error %.3g" % (case.name, worst))
    pol.close()
    if norm is not None:
        norm.close()


@pytest.mark.parametrize("n", [66, 130])
def test_the_rollouts_bits(n):
    """a deterministic GRUPolicy rollout of T = 6 with values=: evaluate_seq_dev on (obs0, obs[:-1]), done and the hidden state copied
    before the call gives the recorded actions as mean, values[:T] as value and policy.hidden as h_out, bit for bit; with exploration
    logp is within 1e-4 of the recorded one (gaq_policy_logp_dev's bound for the same recomputation).  ep_time = 0.025 (episodes of 3 steps): episodes end
    inside the window, at more than one t."""
    import torch
    T = 6
    env = _make_env(18, n, ep_time=0.025)
    for name in ("gru64x64x64-tanh", "gru48x32-relu"):
        case, inp = R.case_inputs(name)
        pol, _ = _policy(env, case, inp, log_std=None)
        o0 = torch.empty((n, 18), device=_dev())
        env.reset_dev(o0)
        prev = o0.clone()
        for explore in (False, True):
            pol.set_log_std(R.LOG_STD if explore else None)
            h0 = pol.hidden.clone()
            o, r, dn, a = _bufs(env, T)
            v = torch.full((T + 1, n), float("nan"), device=_dev())
            lp = torch.full((T, n), float("nan"), device=_dev()) if explore else None
            env.rollout_policy_dev(pol, o, r, dn, a, values=v, logp=lp)
            seq = torch.cat([prev[None], o[:-1]]).contiguous()
            mean = torch.full((T, n, 4), float("nan"), device=_dev())
            h_out = torch.full_like(h0, float("nan"))
            got_lp, got_v = pol.evaluate_seq_dev(seq, a if explore else None, dn, h0, mean=mean, h_out=h_out)
            torch.cuda.synchronize()
            assert int((dn.sum(dim=1) > 0).sum()) > 1, "dones at one t only"
            assert _bits(got_v, v[:T]), (name, explore)
            assert _bits(h_out, pol.hidden), (name, explore)
            if explore:
                e = float((got_lp - lp).abs().max())
                print("%s n=%d: |logp - recorded| %.3g (bound 1e-4)" % (name, n, e))
                assert e <= 1e-4
            else:
                assert got_lp is None and _bits(mean, a), name
            prev = o[-1].clone()
        pol.close()
    env.close()


def test_splitting_in_time(envs):
    """T = 5 in one call == T = 2 then T = 3 chained through h_out: logp, value, mean and h_out bit for bit"""
    import torch
    for name in ("gru64x16x48-relu-vclip", "gru16-tanh"):
        case, inp = R.case_inputs(name)
        pol, _ = _policy(envs(), case, inp)
        S = 65
        d, a, b = _dev_inputs(inp, 5, S), _dev_inputs(inp, 2, S), _dev_inputs(inp, 3, S, t_lo=2)
        outs = []
        for x, h0 in ((d, d["h0"]), (a, a["h0"]), (b, None)):
            mean, h_out = torch.empty(x["obs"].shape[:2] + (4,), device=_dev()), torch.empty_like(d["h0"])
            lp, v = pol.evaluate_seq_dev(x["obs"], x["actions"], x["done"], outs[-1][3] if h0 is None else h0, mean=mean, h_out=h_out)
            outs.append((lp, v, mean, h_out))
        torch.cuda.synchronize()
        whole, first, second = outs
        for k in range(3):
            assert _bits(whole[k], torch.cat([first[k], second[k]])), (name, k)
        assert _bits(whole[3], second[3]) and not torch.isnan(whole[3]).any()
        pol.close()


def test_a_cut_is_a_cut(envs):
    """done[1, :] all set: logp and value of t >= 2 are, bit for bit, those of a call on the steps 2 .. 4 with h0 = 0, and the gradient is
    grad(steps 0 .. 1 from h0) + grad(steps 2 .. 4 from 0) within the case's bound"""
    import torch
    case, inp = R.case_inputs("gru48x32-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S = 5, 65
    done = inp["done"].copy()
    done[1, :] = 1
    d, tail = _dev_inputs(inp, T, S, done=done), _dev_inputs(inp, 3, S, t_lo=2, done=done)
    tail["h0"].zero_()
    lp, v = pol.evaluate_seq_dev(d["obs"], d["actions"], d["done"], d["h0"])
    lp2, v2 = pol.evaluate_seq_dev(tail["obs"], tail["actions"], tail["done"], tail["h0"])
    torch.cuda.synchronize()
    assert _bits(lp[2:], lp2) and _bits(v[2:], v2)
    sc = 1.0 / (T * S)
    one = R.ppo_seq(case, inp, 2, S, scale=sc, done=done)
    two = R.ppo_seq(case, inp, 3, S, scale=sc, done=done, t_lo=2, h0=np.zeros((S, case.H)))
    want = dict(g_gru=[x + y for x, y in zip(one["g_gru"], two["g_gru"])],
                g_head=[(a + c, b + e) for (a, b), (c, e) in zip(one["g_head"], two["g_head"])],
                gvalue=one["gvalue"] + two["gvalue"], glogstd=one["glogstd"] + two["glogstd"])
    # (each part's entropy term is -ent_coef * scale * its rows: together the whole call's)
    errs = _errors(pol, _call(pol, case, d), want)
    bound = R.bounds(case.name, T, S)[0]
    print("cut at t = 1: %.3g (bound %.3g)" % (max(errs), bound))
    assert max(errs) <= bound, errs
    pol.close()


def test_sequences_are_independent(envs):
    """S = 65 == the references of the sequences 0-63 and of sequence 64 added up; NaN (and set done bytes) behind every input past S,
    h0, ret and v_old included, changes no output bit"""
    import torch
    case, inp = R.case_inputs("gru64x16x48-relu-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S = 5, 65
    sc = 1.0 / (T * S)
    lo, hi = R.ppo_seq(case, inp, T, 64, scale=sc), R.ppo_seq(case, inp, T, 1, scale=sc, s_lo=64)
    want = dict(g_gru=[x + y for x, y in zip(lo["g_gru"], hi["g_gru"])], g_head=[(a + c, b + e) for (a, b), (c, e) in zip(lo["g_head"], hi["g_head"])],
                gvalue=lo["gvalue"] + hi["gvalue"], glogstd=lo["glogstd"] + hi["glogstd"])
    assert all(np.abs(g).max() > 0 for g in hi["g_gru"])          # the partial tile's only sequence has a gradient through time
    d = _dev_inputs(inp, T, S)
    out = _call(pol, case, d)
    errs = _errors(pol, out, want)
    print("partial tile: %.3g (bound %.3g)" % (max(errs), R.bounds(case.name, T, S)[0]))
    assert max(errs) <= R.bounds(case.name, T, S)[0]
    ev = pol.evaluate_seq_dev(d["obs"], d["actions"], d["done"], d["h0"])
    nan = {}
    for k, v in d.items():                                        # the same values at the head of a buffer whose tail is poisoned
        big = torch.full((v.numel() + 4096,), 255 if v.dtype == torch.uint8 else float("nan"), dtype=v.dtype, device=_dev())
        big[:v.numel()] = v.reshape(-1)
        nan[k] = big[:v.numel()].view(v.shape)
    out2 = _call(pol, case, nan)
    ev2 = pol.evaluate_seq_dev(nan["obs"], nan["actions"], nan["done"], nan["h0"])
    torch.cuda.synchronize()
    for a, b in zip(tuple(out) + tuple(ev), tuple(out2) + tuple(ev2)):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    pol.close()


def test_limits_of_the_loss(envs):
    """vf_coef = 0, ent_coef = 0 with a value head: grad, grad_log_std and the first three statistics are the no-head call's bits and
    grad_value is exactly 0.  T = 1 from h0 = 0: the W_hh gradient is exactly 0, b_hh's r and z words are b_ih's bits, and its n words
    (da_n r against b_ih's da_n) meet the reference within the bound"""
    import torch
    for name in ("gru64x64x64-relu-vclip", "gru16-tanh"):
        case, inp = R.case_inputs(name)
        pol, _ = _policy(envs(), case, inp)
        d = _dev_inputs(inp, 5, 65)
        g, gv, gls, st = (x.clone() for x in _call(pol, case, d, vf_coef=0.0, ent_coef=0.0))
        pol.set_value_head(None)
        g0, gv0, gls0, st0 = _call(pol, case, d, ent_coef=0.0)
        torch.cuda.synchronize()
        assert gv0 is None and _bits(g, g0) and _bits(gls, gls0) and torch.equal(st[:3], st0[:3]), name
        assert not gv.any() and float(st0[3]) == 0.0 and float(st0[4]) == 0.0 and float(st0[5]) == 5 * 65
        pol.close()
    case, inp = R.case_inputs("gru48x32-tanh")
    pol, _ = _policy(envs(), case, inp)
    S, H = 65, case.H
    d = _dev_inputs(inp, 1, S)
    d["h0"].zero_()
    out = _call(pol, case, d)
    ref = R.ppo_seq(case, inp, 1, S, h0=np.zeros((S, H)))
    (W_ih, W_hh, b_ih, b_hh), _ = pol.unpack(out[0])
    torch.cuda.synchronize()
    assert not W_hh.any() and not ref["g_gru"][1].any()
    assert _bits(b_hh[:2 * H], b_ih[:2 * H]) and not _bits(b_hh[2 * H:], b_ih[2 * H:])
    e = G.rel(_np(b_hh[2 * H:]), ref["g_gru"][3][2 * H:])
    bound = R.bounds(case.name, 1, 65)[0]
    errs = _errors(pol, out, ref)
    print("T = 1, h0 = 0: b_hh's n words %.3g, every tensor %.3g (bound %.3g)" % (e, max(errs), bound))
    assert e <= bound and max(errs) <= bound
    pol.close()


def test_determinism(envs):
    """the same call twice, and once on another stream: equal bits"""
    import torch
    case, inp = R.case_inputs("gru64x64x64-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    d = _dev_inputs(inp, R.TMAX, R.SMAX)
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
    """ppo_seq_grad_dev captured after one warm-up call replays with the eager call's bits, also on new contents of the same buffers and
    after an eager call of smaller T in between (the tape grows only when a call needs more)"""
    import torch
    case, inp = R.case_inputs("gru64x64x64-tanh-vclip")          # (more than 64 KiB of LDS: the launch raises the kernel's limit)
    pol, _ = _policy(envs(), case, inp)
    d, small = _dev_inputs(inp, R.TMAX, R.SMAX), _dev_inputs(inp, 2, 63)
    eager = [x.clone() for x in _call(pol, case, d)]              # the warm-up: the largest T and S
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
    _call(pol, case, small)                                       # an eager call of smaller T in between
    flipped = [x.clone() for x in _call(pol, case, dict(d, adv=-d["adv"], ret=d["ret"] + 0.5))]
    d["adv"].neg_()
    d["ret"].add_(0.5)                                            # new contents, the same buffers
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, flipped):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], eager[0]) and not torch.equal(out[1], eager[1])
    pol.close()


def _pack_gru_torch(gru, head):
    """pack_gru_weights on torch tensors: gru = (W_ih, W_hh, b_ih, b_hh)"""
    import torch
    out = []
    for W, b in ((gru[0], gru[2]), (gru[1], gru[3])):
        o, i = W.shape
        out += [W.reshape(o // 16, 16, i).permute(0, 2, 1).reshape(-1), b]
    for W, b in head[:-1]:
        o, i = W.shape
        out += [W.reshape(o // 16, 16, i).permute(0, 2, 1).reshape(-1), b]
    out += [head[-1][0].T.reshape(-1), head[-1][1]]
    return torch.cat(out).contiguous()


def test_closed_loop_of_ten_adam_steps(envs):
    """Ten Adam steps (lr 3e-4) at (T, S) = (6, 130): device gradients -> unpack_gru_weights / grad_value -> param.grad ->
    set_weights_dev / set_value_head_dev, beside the same ten steps of torch fp32 autograd on the twin module (GRUCell loop with
    torch.where resets, Linear head, value Linear).  Each parameter tensor ends within 100 x the single-step bound.  The loss
    trajectories agree: both fall, and at every step they differ by no more than the forward bound on the two loss sums plus, to first
    order, what the allowed parameter difference can move the loss by (tests/test_gpu_policy_grad_ac.py's tolerance)."""
    import torch
    case, inp = R.case_inputs("gru64x16x48-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S = R.TMAX, R.SMAX
    d = _dev_inputs(inp, T, S)
    lr, steps = 3e-4, 10
    ent_const = float(R.ENT_COEF * 2.0 * (1.0 + np.log(2.0 * np.pi)))
    leaf = lambda a: _t(a).clone().requires_grad_(True)
    gru = [leaf(a) for a in inp["gru"]]
    head = [(leaf(W), leaf(b)) for W, b in inp["head"]]
    vhead = leaf(np.concatenate([inp["wv"], [inp["bv"]]]).astype(np.float32))
    log_std = leaf(R.LOG_STD)
    opt = torch.optim.Adam(gru + [p for Wb in head for p in Wb] + [vhead, log_std], lr=lr)
    loss_dev = []
    for _ in range(steps):
        with torch.no_grad():
            pol.set_weights_dev(_pack_gru_torch(gru, head))
            pol.set_value_head_dev(vhead.detach())
        pol.set_log_std(_np(log_std))
        g, gv, gls, st = _call(pol, case, d)
        ggru, ghead = pol.unpack(g)
        for p, gp in zip(gru, ggru):
            p.grad = gp.contiguous()
        for (W, b), (gW, gb) in zip(head, ghead):
            W.grad, b.grad = gW.contiguous(), gb.contiguous()
        vhead.grad, log_std.grad = gv.clone(), gls.clone()
        loss_dev.append((float(st[0]) + R.VF_COEF * float(st[3])) / (T * S) - R.ENT_COEF * float(log_std.detach().double().sum()) - ent_const)
        opt.step()
    model = R.torch_model(case, inp, torch.float32)
    cell, lins, critic, ls = model
    tens = R.torch_tensors(inp, T, S, torch.float32)
    opt = torch.optim.Adam(list(cell.parameters()) + [p for l in lins for p in l.parameters()] + list(critic.parameters()) + [ls], lr=lr)
    loss_ref = []
    for _ in range(steps):
        opt.zero_grad()
        loss = R.torch_loss(case, tens, T, S, model)[0]
        loss.backward()
        loss_ref.append(float(loss.detach()))
        opt.step()
    print("closed loop: loss %s on the device, %s in torch" % (["%.6f" % x for x in loss_dev], ["%.6f" % x for x in loss_ref]))
    bounds = R.bounds(case.name, T, S)
    bound = 100.0 * bounds[0]
    got = [gru[0], gru[2], gru[1], gru[3]] + [p for Wb in head for p in Wb] + [vhead, log_std]
    want = [cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh] + [p for l in lins for p in (l.weight, l.bias)] + \
           [torch.cat([critic.weight.reshape(-1), critic.bias.reshape(-1)]), ls]
    errs = [G.rel(_np(a), _np(b)) for a, b in zip(got, want)]
    print("closed loop: parameters after %d steps differ by %.3g at most (bound %.3g)" % (steps, max(errs), bound))
    assert max(errs) <= bound, (errs, bound)
    ref = R.case_ref(case.name, T, S)
    g0 = R.tensors(ref) + [ref["gvalue"], ref["glogstd"]]
    th0 = [inp["gru"][0], inp["gru"][2], inp["gru"][1], inp["gru"][3]] + [x for Wb in inp["head"] for x in Wb] + \
          [np.concatenate([inp["wv"], [inp["bv"]]]), R.LOG_STD]
    tol = (bounds[3] * abs(ref["stats"][0]) + R.VF_COEF * bounds[5] * ref["stats"][3]) / (T * S) \
        + sum(float(np.abs(g).sum()) * bound * float(np.abs(th).max()) for g, th in zip(g0, th0))
    diff = max(abs(a - b) for a, b in zip(loss_dev, loss_ref))
    print("closed loop: the trajectories differ by %.3g at most (tolerance %.3g)" % (diff, tol))
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    assert diff <= tol, (loss_dev, loss_ref, tol)
    pol.close()


def test_no_sequences_gives_zeros(envs):
    import torch
    case, inp = R.case_inputs("gru16-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    out = [torch.full_like(x, 7.0) for x in _call(pol, case, _dev_inputs(inp, 2, 63))]
    d = _dev_inputs(inp, 2, 0)
    _call(pol, case, d, grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])
    lp, v = pol.evaluate_seq_dev(d["obs"], d["actions"], d["done"], d["h0"])
    torch.cuda.synchronize()
    assert lp.shape == (2, 0) and v.shape == (2, 0) and not any(bool(x.any()) for x in out)
    pol.close()


def test_refusals(envs):
    """each returns the stated code with the named text, launches nothing, and the first call repeated afterwards gives its bits"""
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPPolicy
    from tests.gru_util import _gru, _head
    from tests.policy_util import _layers
    env = envs()
    lib = _lib.load()
    case, inp = R.case_inputs("gru16-tanh-vclip")
    T, S, H = 5, 65, case.H
    d = _dev_inputs(inp, T, S)
    o, a, dn, h0, lo, adv, ret, vo = (d[k] for k in KEYS)
    cs = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)

    pol, _ = _policy(env, case, inp)
    first = [x.clone() for x in _call(pol, case, d)]
    ev = [x.clone() for x in pol.evaluate_seq_dev(o, a, dn, h0)]
    g, gv, gls, st = (x.clone() for x in first)
    lp_out, v_out = (x.clone() for x in ev)

    def raw(T=T, S=S, obs=o, h0=h0, ret=ret, v_old=vo, clip=0.2, vclip=0.2, vf=0.5, ent=0.01, scale=1.0, grad=g, grad_value=gv, grad_ls=gls,
            stats=st, handle=None):
        return lib.gaq_policy_grad_ppo_seq_dev(pol.handle if handle is None else handle, T, S, _lib.ptr(obs), _lib.ptr(a), _lib.ptr(dn),
                                               _lib.ptr(h0), _lib.ptr(lo), _lib.ptr(adv), _lib.ptr(ret), _lib.ptr(v_old), clip, vclip, vf, ent,
                                               scale, _lib.ptr(grad), _lib.ptr(grad_value), _lib.ptr(grad_ls), _lib.ptr(stats), cs)

    def raw_eval(T=T, S=S, handle=None, logp=lp_out, value=v_out, h_out=None, actions=a):
        return lib.gaq_policy_eval_seq_dev(pol.handle if handle is None else handle, T, S, _lib.ptr(o), _lib.ptr(actions), _lib.ptr(dn),
                                           _lib.ptr(h0), _lib.ptr(logp), _lib.ptr(value), None, _lib.ptr(h_out), cs)

    def err():
        return lib.gaq_last_error()
    for f in (raw, raw_eval):
        assert f(T=0) == -1 and b"T must" in err()
        assert f(S=-1) == -1 and b"S must" in err()
    # the value head: GAQ_ERR_STATE either way round; no log_std: GAQ_ERR_STATE, the existing text
    pol.set_value_head(None)
    assert raw() == -4 and b"value head" in err()
    assert raw(v_old=None, grad_value=None) == -4 and b"value head" in err()          # ret alone is refused too
    assert raw_eval() == -4 and b"value head" in err()
    assert raw(ret=None, v_old=None, grad_value=None) == 0
    assert raw_eval(value=None) == 0
    pol.set_value_head(inp["wv"], inp["bv"])
    assert raw(ret=None) == -1 and b"null" in err()
    assert raw(grad_value=None) == -1 and b"null" in err()
    pol.set_log_std(None)
    assert raw() == -4 and b"no log_std set" in err()
    assert raw_eval() == -4 and b"no log_std set" in err()
    assert raw_eval(logp=None, actions=None) == 0                   # (without logp the actions may be null)
    pol.set_log_std(R.LOG_STD)
    assert raw_eval(actions=None) == -1 and b"null" in err()
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
        pol.ppo_seq_grad_dev(o, a, dn, h0, lo, adv, ret, None, vclip=0.2)
    assert raw(obs=None) == -1 and b"null" in err()
    assert raw(h0=None) == -1 and b"null" in err()
    assert raw(stats=None) == -1 and b"null" in err()
    assert raw(grad=o.view(-1)[:g.numel()]) == -1 and b"overlap" in err()          # an output over an input
    assert raw(grad_ls=g[4:8]) == -1 and b"overlap" in err()                        # two outputs
    assert raw(grad_value=g[:gv.numel()]) == -1 and b"overlap" in err()
    assert raw_eval(h_out=h0) == -1 and b"overlap" in err()
    assert raw(ret=ret.data_ptr() + 2) == -1 and b"aligned" in err()
    assert raw(h0=h0.data_ptr() + 4) == -1 and b"aligned" in err()                 # h0: 16 bytes
    assert raw_eval(h_out=torch.empty(S * H + 4, device=_dev()).data_ptr() + 8) == -1 and b"aligned" in err()
    assert raw(stats=st.data_ptr() + 4) == -1 and b"aligned" in err()
    # what the handle is: a feed-forward policy, an LSTM, a cell over the width limit (the first refused width), weights never set
    mlp = MLPPolicy.from_arrays(env, _layers([16]), "tanh", True, log_std=R.LOG_STD, engine="mfma")
    for f in (raw, raw_eval):
        assert f(handle=mlp.handle) == -1 and b"recurrent cell" in err()
    mlp.close()
    lstm = LSTMPolicy(env, tuple(np.zeros(s, np.float32) for s in ((64, 18), (64, 16), (64,), (64,))), _head(16), "tanh", True, log_std=R.LOG_STD)
    for f in (raw, raw_eval):
        assert f(handle=lstm.handle) == -1 and b"LSTM" in err()
    lstm.close()
    wide = GRUPolicy(env, _gru(80, 18, 3), _head(80), "tanh", True, log_std=R.LOG_STD)
    for f in (raw, raw_eval):
        assert f(handle=wide.handle) == -1 and b"width" in err()
    wide.close()
    from gym_art_amd.policy import _DescRnn, _fill_desc, ENGINES, CELL_GRU
    desc = _fill_desc(_DescRnn(), 18, [16], "tanh", out_tanh=1, engine=ENGINES["mfma"], cell=CELL_GRU)
    bare = C.c_void_p()
    assert lib.gaq_policy_create_rnn(env._handle, C.byref(desc), C.byref(bare)) == 0
    for f in (raw, raw_eval):
        assert f(handle=bare) == -1 and b"weights not set" in err()
    lib.gaq_policy_destroy(bare)
    # the feed-forward entry points keep their refusal of a GRU handle
    assert lib.gaq_policy_logp_dev(pol.handle, 65, _lib.ptr(o), _lib.ptr(a), _lib.ptr(lo.clone()), None, cs) == -1 and b"GRU" in err()
    # the handle is as usable as before: the first call's bits
    again = _call(pol, case, d)
    ev2 = pol.evaluate_seq_dev(o, a, dn, h0)
    torch.cuda.synchronize()
    for x, y in zip(first + ev, list(again) + list(ev2)):
        assert torch.equal(x, y)
    pol.close()
