"""The wide recurrent learner on the device (gaq.h "the wide recurrent learner": gaq_policy_eval_seq_wide_dev,
gaq_policy_grad_ppo_seq_wide_dev) against the fp64 reference of tests/policy_grad_seq_ref.py on the cases of
tests/policy_grad_seq_wide.py: the case matrix under the bound 8 x torch fp32's error, the forward pass's bits against a GRUPolicy
rollout at H = 80 and 128, the narrow calls' bits at H <= 64, splitting in time, cuts at dones, the idx form, determinism and a captured
chain with AdamDev, a closed Adam loop, and the refusals.  S <= 130 and T <= 6 throughout.  Every figure a test bounds is printed
before it is asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_grad_seq_wide as W
from tests.policy_util import _bufs, _dev, environ

R = W.R
G = R.G
pytestmark = pytest.mark.gpu

REPR = {18: "xyz_vxyz_R_omega", 19: "xyz_vxyz_R_omega_h"}
KEYS = ("obs", "actions", "done", "h0", "logp_old", "adv", "ret", "v_old")
NAN = float("nan")


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


def _gather(d, idx):
    """the columns idx of every input as contiguous tensors"""
    return {k: (v[idx.long()] if k == "h0" else v[:, idx.long()]).contiguous() for k, v in d.items()}


def _args(pol, case, d, kw):
    kw.setdefault("vf_coef", R.VF_COEF)
    kw.setdefault("ent_coef", R.ENT_COEF)
    vclip = kw.pop("vclip", case.vclip)
    head = pol.value_head is not None
    return (d["obs"], d["actions"], d["done"], d["h0"], d["logp_old"], d["adv"], d["ret"] if head else None,
            d["v_old"] if head and vclip > 0 else None), dict(kw, clip=R.CLIP, vclip=vclip if vclip > 0 else None)


def _call(pol, case, d, **kw):
    """ppo_seq_wide_grad_dev with the case's coefficients"""
    a, kw = _args(pol, case, d, kw)
    return pol.ppo_seq_wide_grad_dev(*a, **kw)


def _narrow(pol, case, d, idx=None, **kw):
    """the narrow calls with the case's coefficients"""
    a, kw = _args(pol, case, d, kw)
    return pol.ppo_seq_grad_dev(*a, **kw) if idx is None else pol.ppo_seq_grad_idx_dev(idx, *a, **kw)


def _errors(pol, out, ref):
    gru, head = pol.unpack(_np(out[0]))
    return R.grad_errors(gru, head, None if out[1] is None else _np(out[1]), _np(out[2]), ref)


def _check(case, inp, pol, T, S, what):
    ref = W.case_ref(case.name, T, S)
    bg, blp, bv, bloss, bkl, blv = W.bounds(case.name, T, S)
    d = _dev_inputs(inp, T, S)
    out = _call(pol, case, d)
    lp, v = pol.evaluate_seq_wide_dev(d["obs"], d["actions"], d["done"], d["h0"])
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
    assert st.shape == (6,)
    assert max(errs) <= bg, (case.name, what, T, S, errs, bg)     # every tensor, W_ih, b_ih, W_hh and b_hh each, under the one bound
    assert e_lp <= blp and e_v <= bv and e_loss <= bloss and e_kl <= bkl and e_lv <= blv, (case.name, what, T, S)
    assert st[1] == ref["stats"][1] and st[4] == ref["stats"][4] and st[5] == T * S, (st, ref["stats"])     # the counts are exact
    if not case.value:
        assert v is None and out[1] is None and st[3] == 0.0 and st[4] == 0.0
    return max(errs) / bg


# ---- 1. the case matrix --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.SEQ_CASES, ids=[c.name for c in W.SEQ_CASES])
def test_case_matrix(case, envs):
    """every net x value clip (and two nets without a value head) at every (T, S), and (6, 130) over 2 workgroups: each parameter tensor
    -- W_ih, b_ih, W_hh, b_hh separately -- grad_value, grad_log_std, logp, V and the sums within 8 x torch fp32's error; the clipped
    and cut counts and T S exact"""
    _, inp = W.case_inputs(case.name)
    pol, norm = _policy(envs(case.D), case, inp)
    worst = 0.0
    for T, S in R.CONFIGS:
        worst = max(worst, _check(case, inp, pol, T, S, "default"))
    with environ(GAQ_GRAD_GROUPS="2"):
        worst = max(worst, _check(case, inp, pol, R.TMAX, R.SMAX, "2 groups"))
    print("%s: worst gradient error / bound %.3f" % (case.name, worst))
    pol.close()
    if norm is not None:
        norm.close()


# ---- 2. the rollout's bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [66, 130])
def test_the_rollouts_bits(n):
    """a deterministic GRUPolicy rollout of T = 6 with values= at H = 80 and 128: evaluate_seq_wide_dev on (obs0, obs[:-1]), done and the
    hidden state copied before the call gives the recorded actions as mean, values[:T] as value and policy.hidden as h_out, bit for
    bit; with exploration logp is within 1e-4 of the recorded one (the project's bound for that recomputation).  ep_time = 0.025
    (episodes of 3 steps): episodes end inside the window, at more than one t."""
    import torch
    T = 6
    env = _make_env(18, n, ep_time=0.025)
    for name in ("gru80-tanh", "gru128x64x64-relu"):
        case, inp = W.case_inputs(name)
        pol, _ = _policy(env, case, inp, log_std=None)
        o0 = torch.empty((n, 18), device=_dev())
        env.reset_dev(o0)
        prev = o0.clone()
        for explore in (False, True):
            pol.set_log_std(R.LOG_STD if explore else None)
            h0 = pol.hidden.clone()
            o, r, dn, a = _bufs(env, T)
            v = torch.full((T + 1, n), NAN, device=_dev())
            lp = torch.full((T, n), NAN, device=_dev()) if explore else None
            env.rollout_policy_dev(pol, o, r, dn, a, values=v, logp=lp)
            seq = torch.cat([prev[None], o[:-1]]).contiguous()
            mean = torch.full((T, n, 4), NAN, device=_dev())
            h_out = torch.full_like(h0, NAN)
            got_lp, got_v = pol.evaluate_seq_wide_dev(seq, a if explore else None, dn, h0, mean=mean, h_out=h_out)
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


# ---- 3. one group: the narrow calls' bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gru16-tanh", "gru16-relu-vclip", "gru48x32-tanh-vclip", "gru48x32-relu", "gru64x64x64-tanh-vclip",
                                  "gru64x64x64-relu"])
def test_narrow_parity(name, envs):
    """at H <= 64 there is one group: both wide calls return the narrow calls' bits, contiguous and under a perm_dev index"""
    import torch
    from gym_art_amd.policy import perm_dev
    case, inp = R.case_inputs(name)
    pol, _ = _policy(envs(), case, inp)
    d = _dev_inputs(inp, R.TMAX, R.SMAX)
    mean, h_out = (torch.full((R.TMAX, R.SMAX, 4), NAN, device=_dev()) for _ in range(2)), (torch.full_like(d["h0"], NAN) for _ in range(2))
    mean, h_out = list(mean), list(h_out)
    a = pol.evaluate_seq_wide_dev(d["obs"], d["actions"], d["done"], d["h0"], mean=mean[0], h_out=h_out[0])
    b = pol.evaluate_seq_dev(d["obs"], d["actions"], d["done"], d["h0"], mean=mean[1], h_out=h_out[1])
    for x, y in zip(list(a) + [mean[0], h_out[0]], list(b) + [mean[1], h_out[1]]):
        assert _bits(x, y) and not torch.isnan(x).any(), name
    for x, y in zip(_call(pol, case, d), _narrow(pol, case, d)):
        assert _bits(x, y), name
    idx = perm_dev(R.SMAX, 5, device=_dev())[:100].contiguous()
    for x, y in zip(_call(pol, case, d, idx=idx), _narrow(pol, case, d, idx=idx)):
        assert _bits(x, y), name
    torch.cuda.synchronize()
    pol.close()


# ---- 4. time and dones ---------------------------------------------------------------------------------------------------------------------
def test_splitting_in_time(envs):
    """at H = 128, T = 5 in one call == T = 2 then T = 3 chained through h_out: logp, value, mean and h_out bit for bit"""
    import torch
    case, inp = W.case_inputs("gru128x64x64-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    S = 65
    d, a, b = _dev_inputs(inp, 5, S), _dev_inputs(inp, 2, S), _dev_inputs(inp, 3, S, t_lo=2)
    outs = []
    for x, h0 in ((d, d["h0"]), (a, a["h0"]), (b, None)):
        mean, h_out = torch.empty(x["obs"].shape[:2] + (4,), device=_dev()), torch.empty_like(d["h0"])
        lp, v = pol.evaluate_seq_wide_dev(x["obs"], x["actions"], x["done"], outs[-1][3] if h0 is None else h0, mean=mean, h_out=h_out)
        outs.append((lp, v, mean, h_out))
    torch.cuda.synchronize()
    whole, first, second = outs
    for k in range(3):
        assert _bits(whole[k], torch.cat([first[k], second[k]])), k
    assert _bits(whole[3], second[3]) and not torch.isnan(whole[3]).any()
    pol.close()


def test_a_cut_is_a_cut(envs):
    """at H = 128 with done[1, :] all set: logp and value of t >= 2 are, bit for bit, those of a call on the steps 2 .. 4 with h0 = 0, and
    the gradient is grad(steps 0 .. 1 from h0) + grad(steps 2 .. 4 from 0) within the case's bound; T = 1 from h0 = 0: the W_hh gradient
    is exactly 0"""
    import torch
    case, inp = W.case_inputs("gru128-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S = 5, 65
    done = inp["done"].copy()
    done[1, :] = 1
    d, tail = _dev_inputs(inp, T, S, done=done), _dev_inputs(inp, 3, S, t_lo=2, done=done)
    tail["h0"].zero_()
    lp, v = pol.evaluate_seq_wide_dev(d["obs"], d["actions"], d["done"], d["h0"])
    lp2, v2 = pol.evaluate_seq_wide_dev(tail["obs"], tail["actions"], tail["done"], tail["h0"])
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
    bound = W.bounds(case.name, T, S)[0]
    print("cut at t = 1: %.3g (bound %.3g)" % (max(errs), bound))
    assert max(errs) <= bound, errs
    d1 = _dev_inputs(inp, 1, S)
    d1["h0"].zero_()
    out = _call(pol, case, d1)
    ref = R.ppo_seq(case, inp, 1, S, h0=np.zeros((S, case.H)))
    (W_ih, W_hh, b_ih, b_hh), _ = pol.unpack(out[0])
    torch.cuda.synchronize()
    assert not W_hh.any() and not ref["g_gru"][1].any() and W_ih.any()
    errs = _errors(pol, out, ref)
    print("T = 1, h0 = 0: every tensor %.3g (bound %.3g)" % (max(errs), W.bounds(case.name, 1, 65)[0]))
    assert max(errs) <= W.bounds(case.name, 1, 65)[0]
    pol.close()


# ---- 5. the idx form -------------------------------------------------------------------------------------------------------------------
def _idx_vectors(src):
    import torch
    rng = np.random.RandomState(11)
    return {"prefix": _t(rng.permutation(src)[:70], torch.int32),                       # a permutation's first 70: two tiles, one ragged
            "repeats": _t(rng.randint(0, src, size=src + 37), torch.int32)}            # S > S_src, repeated indices, three tiles


@pytest.mark.parametrize("name", ["gru80-tanh-vclip", "gru128x64x64-relu-vclip", "gru80-tanh-nohead"])
def test_idx_is_the_contiguous_call_on_gathered_columns(name, envs):
    """bit for bit, repeated indices and S > S_src included; three indices out of range are counted and contribute exactly 0; NaN in the
    columns no index names changes no output bit"""
    import torch
    case, inp = W.case_inputs(name)
    pol, _ = _policy(envs(), case, inp)
    T, src = 5, 100
    d = _dev_inputs(inp, T, src)
    live = lambda out: [x for x in out if x is not None]
    for what, idx in _idx_vectors(src).items():
        got, want = live(_call(pol, case, d, idx=idx)), live(_call(pol, case, _gather(d, idx)))
        for x, y in zip(got[:-1], want[:-1]):
            assert _bits(x, y), (name, what)
        assert got[-1].shape == (7,) and want[-1].shape == (6,)
        assert torch.equal(got[-1][:-1], want[-1]) and float(got[-1][-1]) == 0.0, (name, what)
    # out of range: counted, exactly 0 -- behind the good indices they move no sequence to another tile, so the call with them is the
    # call without them at the same scale, bit for bit (ent_coef = 0: the entropy term counts the call's rows, skipped or not)
    good = _idx_vectors(src)["prefix"]
    bad = torch.cat([good, _t([-1, src, 2 ** 31 - 1], torch.int32)]).contiguous()
    a = live(_call(pol, case, d, idx=bad, scale=1.0 / 350, ent_coef=0.0))
    b = live(_call(pol, case, d, idx=good, scale=1.0 / 350, ent_coef=0.0))
    for x, y in zip(a[:-1], b[:-1]):
        assert _bits(x, y), name
    sa, sb = _np(a[-1]), _np(b[-1])
    assert sa[-1] == 3.0 and sb[-1] == 0.0 and sa[-2] == T * 73.0 and sb[-2] == T * 70.0 and np.array_equal(sa[:-2], sb[:-2])
    only = _t([-1, src, -7], torch.int32)
    z = live(_call(pol, case, d, idx=only, scale=1.0, ent_coef=0.0))
    assert all(not bool(x.any()) for x in z[:-1]) and float(z[-1][-1]) == 3.0 and not bool(z[-1][:-2].any())   # exactly 0
    # NaN (and set done bytes) in the columns no index names changes no bit
    named = torch.zeros(src, dtype=torch.bool, device=_dev())
    named[good.long()] = True
    nan = {k: v.clone() for k, v in d.items()}
    for k, v in nan.items():
        if k == "h0":
            v[~named] = NAN
        else:
            v[:, ~named] = 255 if v.dtype == torch.uint8 else NAN
    for x, y in zip(live(_call(pol, case, nan, idx=good)), live(_call(pol, case, d, idx=good))):
        assert _bits(x, y) and not torch.isnan(x).any(), name
    torch.cuda.synchronize()
    pol.close()


# ---- 6. determinism and graphs -----------------------------------------------------------------------------------------------------------
def test_determinism(envs):
    """the same call twice, and once on another stream: equal bits, contiguous and with an index vector"""
    import torch
    case, inp = W.case_inputs("gru128x64x64-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    d = _dev_inputs(inp, R.TMAX, R.SMAX)
    for kw in ({}, {"idx": _idx_vectors(R.SMAX)["repeats"]}):
        first = [x.clone() for x in _call(pol, case, d, **kw)]
        again = [x.clone() for x in _call(pol, case, d, **kw)]
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=_dev())
        with torch.cuda.stream(side):
            other = [x.clone() for x in _call(pol, case, d, **kw)]
        side.synchronize()
        for a, b, c in zip(first, again, other):
            assert _bits(a, b) and _bits(a, c)
    pol.close()


def test_a_captured_epoch_with_adam_replays_with_the_eager_bits(envs):
    """perm_dev(epoch_dev=) -> ppo_seq_wide_grad_dev(idx=) -> AdamDev.step at 18-GRU128-64-64, log_std in device mode and learnt, captured
    after one warm-up call at the largest T and S: three replays leave the weights, the value head, the log_std table, the moments and
    the step count bit-equal to three eager iterations from the same start.  AdamDev takes the wide gradients as they are."""
    import torch
    from gym_art_amd.policy import AdamDev, perm_dev
    case, inp = W.case_inputs("gru128x64x64-relu-vclip")
    env = envs()
    T, src, mb, seed = R.TMAX, R.SMAX, 100, 77

    def read(pol, opt):
        sd = opt.state_dict()
        w, b = pol.get_value_head()
        return [pol.get_packed(), w, np.float32(b), pol.get_log_std(), sd["m"], sd["v"]], (sd["step"], sd["skipped"])

    def it(pol, opt, d, perm, word, outs):
        perm_dev(src, seed, epoch_dev=word, out=perm)
        _call(pol, case, d, idx=perm[:mb], grad=outs[0], grad_value=outs[1], grad_log_std=outs[2], stats=outs[3])
        opt.step(outs[0], outs[1], outs[2])
        word.add_(1)

    def make():
        pol, _ = _policy(env, case, inp)
        pol.log_std_to_device()
        d = _dev_inputs(inp, T, src)
        perm = torch.empty((src,), dtype=torch.int32, device=_dev())
        word = torch.full((1,), 3, dtype=torch.int64, device=_dev())
        outs = [torch.empty_like(x) for x in _call(pol, case, d, idx=perm_dev(src, 1, device=_dev())[:mb])]     # the warm-up call
        return pol, AdamDev(pol, lr=1e-3, max_grad_norm=0.5), d, perm, word, outs

    eager = make()
    assert [g[0] for g in eager[1].groups] == ["weights", "value_head", "log_std"]
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


# ---- 7. a closed loop ------------------------------------------------------------------------------------------------------------------
def test_closed_loop_of_ten_adam_steps(envs):
    """Ten AdamDev steps (lr 3e-4) at (T, S) = (6, 130) on gru128 tanh with vclip, beside the same ten steps of torch fp32 Adam on the
    twin module (GRUCell loop with torch.where resets, value Linear).  The parents' rule: each parameter tensor ends within 100 x the
    single-step bound, and the loss trajectories agree -- both fall, and at every step they differ by no more than the forward bound on
    the two loss sums plus, to first order, what the allowed parameter difference can move the loss by."""
    import torch
    from gym_art_amd.policy import AdamDev
    case, inp = W.case_inputs("gru128-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S = R.TMAX, R.SMAX
    d = _dev_inputs(inp, T, S)
    lr, steps = 3e-4, 10
    ent_const = float(R.ENT_COEF * 2.0 * (1.0 + np.log(2.0 * np.pi)))
    opt = AdamDev(pol, lr=lr)
    loss_dev = []
    for _ in range(steps):
        ls = pol.get_log_std()
        g, gv, gls, st = _call(pol, case, d)
        loss_dev.append((float(st[0]) + R.VF_COEF * float(st[3])) / (T * S) - R.ENT_COEF * float(ls.astype(np.float64).sum()) - ent_const)
        opt.step(g, gv, gls)
    model = R.torch_model(case, inp, torch.float32)
    cell, lins, critic, ls = model
    tens = R.torch_tensors(inp, T, S, torch.float32)
    topt = torch.optim.Adam(list(cell.parameters()) + [p for l in lins for p in l.parameters()] + list(critic.parameters()) + [ls], lr=lr)
    loss_ref = []
    for _ in range(steps):
        topt.zero_grad()
        loss = R.torch_loss(case, tens, T, S, model)[0]
        loss.backward()
        loss_ref.append(float(loss.detach()))
        topt.step()
    print("closed loop: loss %s on the device, %s in torch" % (["%.6f" % x for x in loss_dev], ["%.6f" % x for x in loss_ref]))
    bounds = W.bounds(case.name, T, S)
    bound = 100.0 * bounds[0]
    gru, head = pol.unpack(pol.get_packed())
    wv, bv = pol.get_value_head()
    got = [gru[0], gru[2], gru[1], gru[3]] + [x for Wb in head for x in Wb] + [np.concatenate([wv, [bv]]), pol.get_log_std()]
    want = [cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh] + [p for l in lins for p in (l.weight, l.bias)] + \
           [torch.cat([critic.weight.reshape(-1), critic.bias.reshape(-1)]), ls]
    assert not np.array_equal(np.asarray(got[0]), inp["gru"][0])
    errs = [G.rel(np.asarray(a), _np(b)) for a, b in zip(got, want)]
    print("closed loop: parameters after %d steps differ by %.3g at most (bound %.3g)" % (steps, max(errs), bound))
    ref = W.case_ref(case.name, T, S)
    g0 = R.tensors(ref) + [ref["gvalue"], ref["glogstd"]]
    th0 = [inp["gru"][0], inp["gru"][2], inp["gru"][1], inp["gru"][3]] + [x for Wb in inp["head"] for x in Wb] + \
          [np.concatenate([inp["wv"], [inp["bv"]]]), R.LOG_STD]
    tol = (bounds[3] * abs(ref["stats"][0]) + R.VF_COEF * bounds[5] * ref["stats"][3]) / (T * S) \
        + sum(float(np.abs(g).sum()) * bound * float(np.abs(th).max()) for g, th in zip(g0, th0))
    diff = max(abs(a - b) for a, b in zip(loss_dev, loss_ref))
    print("closed loop: the trajectories differ by %.3g at most (tolerance %.3g)" % (diff, tol))
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    assert diff <= tol, (loss_dev, loss_ref, tol)
    assert max(errs) <= bound, (errs, bound)
    opt.close()
    pol.close()


def test_no_sequences_gives_zeros(envs):
    import torch
    case, inp = W.case_inputs("gru80-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    out = [torch.full_like(x, 7.0) for x in _call(pol, case, _dev_inputs(inp, 2, 63))]
    d = _dev_inputs(inp, 2, 0)
    _call(pol, case, d, grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])
    lp, v = pol.evaluate_seq_wide_dev(d["obs"], d["actions"], d["done"], d["h0"])
    torch.cuda.synchronize()
    assert lp.shape == (2, 0) and v.shape == (2, 0) and not any(bool(x.any()) for x in out)
    pol.close()


# ---- 8. the LDS edge on a wide observation -----------------------------------------------------------------------------------------------
def test_the_lds_edge_on_a_swarm():
    """An 8-agent swarm observes 60 words (kx = 64).  60-GRU112 is the top of LDS (544 rows: 156 416 B, 156 672 B with an index vector)
    and runs: at (5, 65) every tensor, logp, V and the sums within the bounds, the idx form the gathered call's bits.  60-GRU128 is the
    first shape past the figure (576 rows, 165 120 B): the gradient call refuses it, contiguous and with an index vector, by a text
    that names LDS and the call, launches nothing, and both handles stay usable.  The forward call keeps no carried dh and no planes
    (8.25 KiB + 272 B x 320 rows at 60-GRU128), so it takes that handle."""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import GRUPolicy
    from tests.gru_util import _gru, _head
    env = QuadrotorEnv(num_envs=64, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True, obs_repr=REPR[18],
                       swarm=dict(agents=8))
    assert env.obs_dim == 60
    case, inp = W.edge_inputs()
    T, S = W.EDGE_SIZE
    assert W.lds_bytes(60, case.H, case.head, idx=True) == 156672 <= W.LDS_MAX < W.lds_bytes(60, 128, ()) == 165120
    pol, _ = _policy(env, case, inp)
    d = _dev_inputs(inp, T, S)
    ref = R.ppo_seq(case, inp, T, S)
    bg, blp, bv, bloss, bkl, blv = W.edge_bounds()
    out = [x.clone() for x in _call(pol, case, d)]
    lp, v = pol.evaluate_seq_wide_dev(d["obs"], d["actions"], d["done"], d["h0"])
    errs, st = _errors(pol, out, ref), _np(out[3])
    e_lp, e_v = G.rel(_np(lp), ref["logp"]), G.rel(_np(v), ref["value"])
    e_loss, e_kl, e_lv = G.rel(st[0], ref["stats"][0]), G.rel(st[2], ref["stats"][2]), G.rel(st[3], ref["stats"][3])
    print("%s (T, S) = (%d, %d): grad %.3g (bound %.3g) logp %.3g (%.3g) V %.3g (%.3g) loss %.3g (%.3g) kl %.3g (%.3g) L_V %.3g (%.3g)"
          % (case.name, T, S, max(errs), bg, e_lp, blp, e_v, bv, e_loss, bloss, e_kl, bkl, e_lv, blv))
    assert max(errs) <= bg, errs
    assert e_lp <= blp and e_v <= bv and e_loss <= bloss and e_kl <= bkl and e_lv <= blv
    assert st[1] == ref["stats"][1] and st[4] == ref["stats"][4] and st[5] == T * S
    idx = _t(np.random.RandomState(3).permutation(S), torch.int32)
    got, want = _call(pol, case, d, idx=idx), _call(pol, case, _gather(d, idx))
    for x, y in zip(got[:3], want[:3]):
        assert _bits(x, y)
    assert torch.equal(got[3][:-1], want[3]) and float(got[3][-1]) == 0.0
    # one chunk more: refused, nothing written
    big = GRUPolicy(env, _gru(128, 60, 3), _head(128), "tanh", False, log_std=R.LOG_STD)
    h0 = torch.zeros((S, 128), device=_dev())
    a = (d["obs"], d["actions"], d["done"], h0, d["logp_old"], d["adv"])
    g = torch.full((big._count,), NAN, device=_dev())
    for kw in ({}, {"idx": idx}):
        with pytest.raises(ValueError, match="gaq_policy_grad_ppo_seq_wide_dev: in_dim too large for the sequence kernel's LDS"):
            big.ppo_seq_wide_grad_dev(*a, grad=g, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(g).all())
    lp2, v2 = big.evaluate_seq_wide_dev(d["obs"], d["actions"], d["done"], h0)
    torch.cuda.synchronize()
    assert v2 is None and bool(torch.isfinite(lp2).all())
    for x, y in zip(out, _call(pol, case, d)):
        assert _bits(x, y)
    big.close()
    pol.close()
    env.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(envs):
    """each returns the stated code with the named text, launches nothing, and the first call repeated afterwards gives its bits.  (The
    refusal of an in_dim past the LDS figure needs a wider observation than this env's: test_the_lds_edge_on_a_swarm.)"""
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPPolicy
    from tests.gru_util import _gru, _head
    from tests.policy_util import _layers
    env = envs()
    lib = _lib.load()
    case, inp = W.case_inputs("gru80-tanh-vclip")
    T, S, H = 5, 65, case.H
    d = _dev_inputs(inp, T, S)
    o, a, dn, h0, lo, adv, ret, vo = (d[k] for k in KEYS)
    cs = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    idx = _t(np.arange(S), torch.int32)

    pol, _ = _policy(env, case, inp)
    first = [x.clone() for x in _call(pol, case, d)]
    ev = [x.clone() for x in pol.evaluate_seq_wide_dev(o, a, dn, h0)]
    g, gv, gls, st = (x.clone() for x in first)
    st7 = torch.zeros(7, dtype=torch.float64, device=_dev())
    lp_out, v_out = (x.clone() for x in ev)

    def raw(T=T, S=S, idx=None, S_src=S, obs=o, h0=h0, ret=ret, v_old=vo, clip=0.2, vclip=0.2, vf=0.5, ent=0.01, scale=1.0, grad=g,
            grad_value=gv, grad_ls=gls, stats=st, handle=None):
        return lib.gaq_policy_grad_ppo_seq_wide_dev(pol.handle if handle is None else handle, T, S, _lib.ptr(idx), S_src, _lib.ptr(obs),
                                                    _lib.ptr(a), _lib.ptr(dn), _lib.ptr(h0), _lib.ptr(lo), _lib.ptr(adv), _lib.ptr(ret),
                                                    _lib.ptr(v_old), clip, vclip, vf, ent, scale, _lib.ptr(grad), _lib.ptr(grad_value),
                                                    _lib.ptr(grad_ls), _lib.ptr(stats), cs)

    def raw_eval(T=T, S=S, handle=None, logp=lp_out, value=v_out, h_out=None, actions=a):
        return lib.gaq_policy_eval_seq_wide_dev(pol.handle if handle is None else handle, T, S, _lib.ptr(o), _lib.ptr(actions), _lib.ptr(dn),
                                                _lib.ptr(h0), _lib.ptr(logp), _lib.ptr(value), None, _lib.ptr(h_out), cs)

    def err():
        return lib.gaq_last_error()
    for f, who in ((raw, b"gaq_policy_grad_ppo_seq_wide_dev"), (raw_eval, b"gaq_policy_eval_seq_wide_dev")):
        assert f(T=0) == -1 and b"T must" in err() and who in err()
        assert f(S=-1) == -1 and b"S must" in err()
    # the parents' argument refusals under the new names: the value head and log_std (GAQ_ERR_STATE), the hyper-parameters, nulls,
    # overlaps, alignment, the index vector's
    pol.set_value_head(None)
    assert raw() == -4 and b"value head" in err()
    assert raw(v_old=None, grad_value=None) == -4 and b"value head" in err()
    assert raw_eval() == -4 and b"value head" in err()
    assert raw(ret=None, v_old=None, grad_value=None) == 0
    assert raw_eval(value=None) == 0
    pol.set_value_head(inp["wv"], inp["bv"])
    assert raw(ret=None) == -1 and b"null" in err()
    assert raw(grad_value=None) == -1 and b"null" in err()
    pol.set_log_std(None)
    assert raw() == -4 and b"no log_std set" in err()
    assert raw_eval() == -4 and b"no log_std set" in err()
    assert raw_eval(logp=None, actions=None) == 0
    pol.set_log_std(R.LOG_STD)
    assert raw_eval(actions=None) == -1 and b"null" in err()
    for clip in (0.0, 1.0, NAN):
        assert raw(clip=clip) == -1 and b"clip_eps" in err()
    for vclip in (-0.1, NAN):
        assert raw(vclip=vclip) == -1 and b"vclip" in err()
    assert raw(vf=NAN) == -1 and b"NaN" in err()
    assert raw(ent=NAN) == -1 and b"NaN" in err()
    assert raw(scale=NAN) == -1 and b"NaN" in err()
    assert raw(v_old=None) == -1 and b"v_old" in err()
    assert raw(v_old=None, vclip=0.0) == 0
    with pytest.raises(ValueError, match="v_old"):
        pol.ppo_seq_wide_grad_dev(o, a, dn, h0, lo, adv, ret, None, vclip=0.2)
    assert raw(obs=None) == -1 and b"null" in err()
    assert raw(h0=None) == -1 and b"null" in err()
    assert raw(stats=None) == -1 and b"null" in err()
    assert raw(grad=o.view(-1)[:g.numel()]) == -1 and b"overlap" in err()
    assert raw(grad_ls=g[4:8]) == -1 and b"overlap" in err()
    assert raw_eval(h_out=h0) == -1 and b"overlap" in err()
    assert raw(ret=ret.data_ptr() + 2) == -1 and b"aligned" in err()
    assert raw(h0=h0.data_ptr() + 4) == -1 and b"aligned" in err()
    assert raw(stats=st.data_ptr() + 4) == -1 and b"aligned" in err()
    assert raw(idx=idx, stats=st7, S_src=0) == -1 and b"S_src must be at least 1" in err()
    assert raw(idx=idx, stats=st7, S_src=2 ** 31) == -1 and b"S_src must not exceed" in err()
    assert raw(idx=g.view(torch.int32)[:S], stats=st7) == -1 and b"overlap" in err()
    assert raw(idx=idx, stats=st7) == 0 and raw(S_src=-5) == 0      # (without idx S_src is ignored)
    # what the handle is: H = 144, a head layer of 80, an LSTM, a policy with an encoder, a feed-forward policy, weights never set
    big = GRUPolicy(env, _gru(144, 18, 3), _head(144), "tanh", True, log_std=R.LOG_STD)
    for f in (raw, raw_eval):
        assert f(handle=big.handle) == -1 and b"width[0] is 144" in err() and b"up to 128" in err()
    big.close()
    big = GRUPolicy(env, _gru(96, 18, 3), _head(96, (80,), 4), "tanh", True, log_std=R.LOG_STD)
    for f in (raw, raw_eval):
        assert f(handle=big.handle) == -1 and b"width[1] is 80" in err() and b"up to 64" in err()
    big.close()
    lstm = LSTMPolicy(env, tuple(np.zeros(s, np.float32) for s in ((64, 18), (64, 16), (64,), (64,))), _head(16), "tanh", True, log_std=R.LOG_STD)
    for f in (raw, raw_eval):
        assert f(handle=lstm.handle) == -1 and b"LSTM" in err()
    lstm.close()
    enc = GRUPolicy.with_encoder(env, _layers([32])[:1], _gru(16, 32, 3), _head(16), "tanh", True, log_std=R.LOG_STD)
    for f in (raw, raw_eval):
        assert f(handle=enc.handle) == -1 and b"encoder" in err()
    enc.close()
    mlp = MLPPolicy.from_arrays(env, _layers([16]), "tanh", True, log_std=R.LOG_STD, engine="mfma")
    for f in (raw, raw_eval):
        assert f(handle=mlp.handle) == -1 and b"feed-forward" in err()
    mlp.close()
    from gym_art_amd.policy import _DescRnn, _fill_desc, ENGINES, CELL_GRU
    desc = _fill_desc(_DescRnn(), 18, [128], "tanh", out_tanh=1, engine=ENGINES["mfma"], cell=CELL_GRU)
    bare = C.c_void_p()
    assert lib.gaq_policy_create_rnn(env._handle, C.byref(desc), C.byref(bare)) == 0
    for f in (raw, raw_eval):
        assert f(handle=bare) == -1 and b"weights not set" in err()
    lib.gaq_policy_destroy(bare)
    # the narrow calls keep their refusal of H = 80, word for word
    with pytest.raises(ValueError, match="policy: the sequence passes take a GRU and head layers of width up to 64, width\\[0\\] is 80"):
        _narrow(pol, case, d)
    with pytest.raises(ValueError, match="policy: the sequence passes take a GRU and head layers of width up to 64, width\\[0\\] is 80"):
        pol.evaluate_seq_dev(o, a, dn, h0)
    # the handle is as usable as before: the first call's bits
    again = _call(pol, case, d)
    ev2 = pol.evaluate_seq_wide_dev(o, a, dn, h0)
    torch.cuda.synchronize()
    for x, y in zip(first + ev, list(again) + list(ev2)):
        assert torch.equal(x, y)
    pol.close()
