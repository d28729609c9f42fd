"""The recurrent learner for an LSTM policy on the device (gaq.h gaq_policy_eval_lstm_seq_dev, gaq_policy_grad_ppo_lstm_seq_dev and its idx
form) against the fp64 reference of tests/policy_grad_lstm_ref.py: the case matrix under the bound 8 x torch fp32's error, the forward
pass's bits against an LSTMPolicy rollout's recorded actions, values and both states, chaining in time, cuts at dones, the exact zeros
of the f gate, the limits of the loss, determinism, poisoned tails, the idx form, graphs, a closed AdamDev loop, and the refusals.
Every figure a test bounds is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_grad_lstm_ref as R
from tests.policy_util import _bufs, _dev, environ

G = R.G
pytestmark = pytest.mark.gpu

REPR = {18: "xyz_vxyz_R_omega", 19: "xyz_vxyz_R_omega_h"}
KEYS = ("obs", "actions", "done", "h0", "c0", "logp_old", "adv", "ret", "v_old")
STATES = ("h0", "c0")


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
    """the case's LSTM policy (with its value head unless the case has none) and the normaliser it keeps alive"""
    from gym_art_amd.policy import LSTMPolicy, ObsNorm
    value = case.value if value is None else value
    pol = LSTMPolicy(env, inp["lstm"], inp["head"], case.act, case.out_tanh, log_std=log_std, value=(inp["wv"], inp["bv"]) if value else None)
    norm = None
    if case.norm:
        mean, var, eps, clip = G.norm_stats(case.D)
        norm = ObsNorm.from_stats(env, mean, var, 1.0, eps, clip)
        pol.set_obs_norm(norm)
    return pol, norm


def _dev_inputs(inp, T, S, t_lo=0, s_lo=0, done=None):
    """the steps [t_lo, t_lo + T) of the sequences [s_lo, s_lo + S) as contiguous device tensors"""
    src = dict(inp, done=inp["done"] if done is None else done)
    d = {k: _t(src[k][t_lo:t_lo + T, s_lo:s_lo + S]) for k in KEYS if k not in STATES}
    for k in STATES:
        d[k] = _t(inp[k][s_lo:s_lo + S])
    return d


def _args(pol, case, d, kw):
    kw.setdefault("vf_coef", R.VF_COEF)
    kw.setdefault("ent_coef", R.ENT_COEF)
    vclip = kw.pop("vclip", case.vclip)
    head = pol.value_head is not None
    return (d["obs"], d["actions"], d["done"], d["h0"], d["c0"], d["logp_old"], d["adv"], d["ret"] if head else None,
            d["v_old"] if head and vclip > 0 else None), dict(kw, clip=R.CLIP, vclip=vclip if vclip > 0 else None)


def _call(pol, case, d, **kw):
    """ppo_bptt_grad_dev with the case's coefficients"""
    a, kw = _args(pol, case, d, kw)
    return pol.ppo_bptt_grad_dev(*a, **kw)


def _call_idx(pol, case, idx, d, **kw):
    a, kw = _args(pol, case, d, kw)
    return pol.ppo_bptt_grad_idx_dev(idx, *a, **kw)


def _eval(pol, d, **kw):
    return pol.evaluate_seq_dev(d["obs"], d["actions"], d["done"], d["h0"], d["c0"], **kw)


def _errors(pol, out, ref):
    lstm, head = pol.unpack(_np(out[0]))
    return R.grad_errors(lstm, head, None if out[1] is None else _np(out[1]), _np(out[2]), ref)


def _bias_halves_equal(pol, grad):
    (_, _, b_ih, b_hh), _ = pol.unpack(grad)
    return _bits(b_ih, b_hh)


def _check(case, inp, pol, T, S, what):
    ref = R.case_ref(case.name, T, S)
    bg, blp, bv, bloss, bkl, blv = R.bounds(case.name, T, S)
    d = _dev_inputs(inp, T, S)
    out = _call(pol, case, d)
    lp, v = _eval(pol, d)
    errs = _errors(pol, out, ref)
    st = _np(out[3])
    e_lp = G.rel(_np(lp), ref["logp"])
    e_v = G.rel(_np(v), ref["value"]) if case.value else 0.0
    e_loss, e_kl = G.rel(st[0], ref["stats"][0]), G.rel(st[2], ref["stats"][2])
    e_lv = G.rel(st[3], ref["stats"][3]) if case.value else float(st[3])
    print("%s %s (T, S) = (%d, %d): grad %.3g (bound %.3g) [%s | rest %.3g] logp %.3g (%.3g) V %.3g (%.3g) loss %.3g (%.3g) kl %.3g (%.3g) "
          "L_V %.3g (%.3g) clipped %d cut %d" % (case.name, what, T, S, max(errs), bg, " ".join("%s %.3g" % x for x in zip(R.TENSOR_NAMES, errs)),
                                                max(errs[4:]), e_lp, blp, e_v, bv, e_loss, bloss, e_kl, bkl, e_lv, blv, st[1], st[4]))
    assert max(errs) <= bg, (case.name, what, T, S, errs, bg)
    assert e_lp <= blp and e_v <= bv and e_loss <= bloss and e_kl <= bkl and e_lv <= blv, (case.name, what, T, S)
    assert st[1] == ref["stats"][1] and st[4] == ref["stats"][4] and st[5] == T * S, (st, ref["stats"])     # the counts are exact
    assert _bias_halves_equal(pol, out[0]), (case.name, what, T, S)
    if not case.value:
        assert v is None and out[1] is None and st[3] == 0.0 and st[4] == 0.0
    return max(errs)


@pytest.mark.parametrize("case", R.LSTM_CASES, ids=[c.name for c in R.LSTM_CASES])
def test_case_matrix(case, envs):
    """every (H, head) x style x observation form x value clip (and two nets without a value head) at every (T, S), and (6, 130) over 2
    workgroups: each parameter tensor -- weight_ih, bias_ih, weight_hh, bias_hh separately -- grad_value, grad_log_std, logp, V and the
    sums within 8 x torch fp32's error; the clipped and cut counts and T S exact; the b_ih and b_hh halves of the gradient bit-equal"""
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
    """a deterministic LSTMPolicy rollout of T = 6 with values=: evaluate_seq_dev on (obs0, obs[:-1]), done and the two states copied
    before the call gives the recorded actions as mean, values[:T] as value, policy.hidden as h_out and policy.cell as c_out, bit for
    bit; with exploration logp is within 1e-4 of the recorded one (only z is recomputed).  ep_time = 0.025 (episodes of 3 steps):
    episodes end inside the window, at more than one t."""
    import torch
    T = 6
    env = _make_env(18, n, ep_time=0.025)
    for name in ("lstm64x64x64-tanh", "lstm48x32-relu"):
        case, inp = R.case_inputs(name)
        pol, _ = _policy(env, case, inp, log_std=None)
        o0 = torch.empty((n, 18), device=_dev())
        env.reset_dev(o0)
        prev = o0.clone()
        for explore in (False, True):
            pol.set_log_std(R.LOG_STD if explore else None)
            h0, c0 = pol.hidden.clone(), pol.cell.clone()
            o, r, dn, a = _bufs(env, T)
            v = torch.full((T + 1, n), float("nan"), device=_dev())
            lp = torch.full((T, n), float("nan"), device=_dev()) if explore else None
            env.rollout_policy_dev(pol, o, r, dn, a, values=v, logp=lp)
            seq = torch.cat([prev[None], o[:-1]]).contiguous()
            mean = torch.full((T, n, 4), float("nan"), device=_dev())
            h_out, c_out = torch.full_like(h0, float("nan")), torch.full_like(c0, float("nan"))
            got_lp, got_v = pol.evaluate_seq_dev(seq, a if explore else None, dn, h0, c0, mean=mean, h_out=h_out, c_out=c_out)
            torch.cuda.synchronize()
            assert int((dn.sum(dim=1) > 0).sum()) > 1, "dones at one t only"
            assert _bits(got_v, v[:T]), (name, explore)
            assert _bits(h_out, pol.hidden) and _bits(c_out, pol.cell), (name, explore)
            print("%s n=%d: %d of %d rows of c_out carry a state, the others were zeroed by done[T-1]"
                  % (name, n, int(c_out.any(dim=1).sum()), n))
            if explore:
                e = float((got_lp - lp).abs().max())
                print("%s n=%d: |logp - recorded| %.3g (bound 1e-4)" % (name, n, e))
                assert e <= 1e-4
            else:
                assert got_lp is None and _bits(mean, a), name
            prev = o[-1].clone()
        pol.close()
    env.close()


def test_the_rollouts_states_mid_episode():
    """the same rollout cut at T = 5, where the 3-step episodes leave step 4 inside an episode (at T = 6 every row ends on a done and
    both states are zeros): h_out and c_out are .hidden and .cell bit for bit with a state in rows of both, and so are value and mean"""
    import torch
    T, n = 5, 66
    env = _make_env(18, n, ep_time=0.025)
    case, inp = R.case_inputs("lstm64x16x48-relu")
    pol, _ = _policy(env, case, inp, log_std=None)
    o0 = torch.empty((n, 18), device=_dev())
    env.reset_dev(o0)
    h0, c0 = pol.hidden.clone(), pol.cell.clone()
    o, r, dn, a = _bufs(env, T)
    v = torch.full((T + 1, n), float("nan"), device=_dev())
    env.rollout_policy_dev(pol, o, r, dn, a, values=v)
    seq = torch.cat([o0[None], o[:-1]]).contiguous()
    mean = torch.full((T, n, 4), float("nan"), device=_dev())
    h_out, c_out = torch.full_like(h0, float("nan")), torch.full_like(c0, float("nan"))
    _, got_v = pol.evaluate_seq_dev(seq, None, dn, h0, c0, mean=mean, h_out=h_out, c_out=c_out)
    torch.cuda.synchronize()
    carried = int(c_out.any(dim=1).sum())
    print("T = 5: %d of %d rows carry a state, %d dones inside the window" % (carried, n, int(dn[:-1].sum())))
    assert int(dn[:-1].sum()) > 0 and carried > 0 and int(h_out.any(dim=1).sum()) == carried
    assert _bits(h_out, pol.hidden) and _bits(c_out, pol.cell) and _bits(got_v, v[:T]) and _bits(mean, a)
    pol.close()
    env.close()


def test_chaining_in_time(envs):
    """T = 5 in one call == T = 2 then T = 3 chained through h_out and c_out: logp, value, mean, h_out and c_out bit for bit"""
    import torch
    for name in ("lstm64x16x48-relu-vclip", "lstm16-tanh"):
        case, inp = R.case_inputs(name)
        pol, _ = _policy(envs(), case, inp)
        S = 65
        d, a, b = _dev_inputs(inp, 5, S), _dev_inputs(inp, 2, S), _dev_inputs(inp, 3, S, t_lo=2)
        outs = []
        for x, first in ((d, True), (a, True), (b, False)):
            mean = torch.empty(x["obs"].shape[:2] + (4,), device=_dev())
            h_out, c_out = torch.empty_like(d["h0"]), torch.empty_like(d["c0"])
            h0, c0 = (x["h0"], x["c0"]) if first else outs[-1][3:5]
            lp, v = pol.evaluate_seq_dev(x["obs"], x["actions"], x["done"], h0, c0, mean=mean, h_out=h_out, c_out=c_out)
            outs.append((lp, v, mean, h_out, c_out))
        torch.cuda.synchronize()
        whole, first, second = outs
        for k in range(3):
            assert _bits(whole[k], torch.cat([first[k], second[k]])), (name, k)
        for k in (3, 4):
            assert _bits(whole[k], second[k]) and not torch.isnan(whole[k]).any() and bool(whole[k].any())
        pol.close()


def test_a_cut_is_a_cut(envs):
    """done[1, :] all set: logp and value of t >= 2 are, bit for bit, those of a call on the steps 2 .. 4 with h0 = c0 = 0, and the
    gradient is grad(steps 0 .. 1 from (h0, c0)) + grad(steps 2 .. 4 from (0, 0)) within the case's bound"""
    import torch
    case, inp = R.case_inputs("lstm48x32-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S = 5, 65
    done = inp["done"].copy()
    done[1, :] = 1
    d, tail = _dev_inputs(inp, T, S, done=done), _dev_inputs(inp, 3, S, t_lo=2, done=done)
    tail["h0"].zero_()
    tail["c0"].zero_()
    lp, v = _eval(pol, d)
    lp2, v2 = _eval(pol, tail)
    torch.cuda.synchronize()
    assert _bits(lp[2:], lp2) and _bits(v[2:], v2)
    sc = 1.0 / (T * S)
    zero = np.zeros((S, case.H))
    one = R.ppo_seq(case, inp, 2, S, scale=sc, done=done)
    two = R.ppo_seq(case, inp, 3, S, scale=sc, done=done, t_lo=2, h0=zero, c0=zero)
    want = dict(g_lstm=[x + y for x, y in zip(one["g_lstm"], two["g_lstm"])],
                g_head=[(a + c, b + e) for (a, b), (c, e) in zip(one["g_head"], two["g_head"])],
                gvalue=one["gvalue"] + two["gvalue"], glogstd=one["glogstd"] + two["glogstd"])
    # (each part's entropy term is -ent_coef * scale * its rows: together the whole call's)
    errs = _errors(pol, _call(pol, case, d), want)
    bound = R.bounds(case.name, T, S)[0]
    print("cut at t = 1: %.3g (bound %.3g)" % (max(errs), bound))
    assert max(errs) <= bound, errs
    pol.close()


def test_exact_zeros_of_one_step_from_zero(envs):
    """T = 1 from h0 = c0 = 0: the W_hh gradient is exactly 0, and so are the f-gate rows of dW_ih and of both biases (da_f = dc cin
    f (1 - f) with cin = 0), while every tensor meets the reference within the bound; with c0 != 0 the f-gate rows are non-zero"""
    import torch
    case, inp = R.case_inputs("lstm48x32-tanh")
    pol, _ = _policy(envs(), case, inp)
    S, H = 65, case.H
    d = _dev_inputs(inp, 1, S)
    d["h0"].zero_()
    d["c0"].zero_()
    out = _call(pol, case, d)
    zero = np.zeros((S, H))
    ref = R.ppo_seq(case, inp, 1, S, h0=zero, c0=zero)
    (W_ih, W_hh, b_ih, b_hh), _ = pol.unpack(out[0])
    torch.cuda.synchronize()
    assert not W_hh.any() and not ref["g_lstm"][1].any()
    f = slice(H, 2 * H)
    assert not W_ih[f].any() and not b_ih[f].any() and not b_hh[f].any()
    assert bool(W_ih[:H].any()) and bool(W_ih[2 * H:].any()) and bool(b_ih[:H].any())
    errs = _errors(pol, out, ref)
    bound = R.bounds(case.name, 1, 65)[0]
    print("T = 1, h0 = c0 = 0: every tensor %.3g (bound %.3g)" % (max(errs), bound))
    assert max(errs) <= bound
    d2 = _dev_inputs(inp, 1, S)
    d2["h0"].zero_()
    (W2, Whh2, b2, bh2), _ = pol.unpack(_call(pol, case, d2)[0])
    torch.cuda.synchronize()
    assert bool(W2[f].any()) and bool(b2[f].any()) and bool(bh2[f].any()) and not Whh2.any()
    pol.close()


def test_limits_of_the_loss(envs):
    """vf_coef = 0, ent_coef = 0 with a value head: grad, grad_log_std and the first three statistics are the no-head call's bits and
    grad_value is exactly 0"""
    import torch
    for name in ("lstm64x64x64-relu-vclip", "lstm16-tanh"):
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


def test_determinism(envs):
    """the same call twice, and once on another stream: equal bits"""
    import torch
    case, inp = R.case_inputs("lstm64x64x64-tanh-vclip")
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


def test_nan_past_s_changes_no_output_bit(envs):
    """NaN (and set done bytes) behind every input past S, h0, c0, ret and v_old included, changes no output bit of the gradient call
    and of the forward call at S = 65 (a tile with one live sequence)"""
    import torch
    case, inp = R.case_inputs("lstm64x16x48-relu-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S = 5, 65
    d = _dev_inputs(inp, T, S)
    out = _call(pol, case, d)
    h_out, c_out = torch.empty_like(d["h0"]), torch.empty_like(d["c0"])
    ev = tuple(_eval(pol, d, h_out=h_out, c_out=c_out)) + (h_out, c_out)
    nan = {}
    for k, v in d.items():                                        # the same values at the head of a buffer whose tail is poisoned
        big = torch.full((v.numel() + 4096,), 255 if v.dtype == torch.uint8 else float("nan"), dtype=v.dtype, device=_dev())
        big[:v.numel()] = v.reshape(-1)
        nan[k] = big[:v.numel()].view(v.shape)
    out2 = _call(pol, case, nan)
    h2, c2 = torch.empty_like(d["h0"]), torch.empty_like(d["c0"])
    ev2 = tuple(_eval(pol, nan, h_out=h2, c_out=c2)) + (h2, c2)
    torch.cuda.synchronize()
    for a, b in zip(tuple(out) + ev, tuple(out2) + ev2):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    pol.close()


def _gathered(d, idx):
    g = {k: d[k][:, idx.long()].contiguous() for k in KEYS if k not in STATES}
    for k in STATES:
        g[k] = d[k][idx.long()].contiguous()
    return g


def test_idx_form_is_the_contiguous_call_on_gathered_columns(envs):
    """torch.equal with the contiguous call on x[:, idx], h0[idx], c0[idx] for a permutation of all 130 columns, for duplicates and for
    S = 1, 63, 65 drawn from the 130; the seventh statistic is 0"""
    import torch
    case, inp = R.case_inputs("lstm64x16x48-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S_src = 5, R.SMAX
    d = _dev_inputs(inp, T, S_src)
    gen = torch.Generator().manual_seed(11)
    perm = torch.randperm(S_src, generator=gen)
    lists = {"permutation": perm, "duplicates": torch.tensor([5, 5, 129, 0, 5, 64, 64, 129] * 9), "S=1": perm[:1], "S=63": perm[3:66],
             "S=65": perm[60:125]}
    for what, ix in lists.items():
        idx = ix.to(device=_dev(), dtype=torch.int32).contiguous()
        want = [x.clone() for x in _call(pol, case, _gathered(d, idx))]
        got = _call_idx(pol, case, idx, d)
        torch.cuda.synchronize()
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a, b), what
        assert torch.equal(got[3][:6], want[3]) and float(got[3][6]) == 0.0, what
    pol.close()


def test_idx_form_skips_and_counts_indices_out_of_range(envs):
    """60 indices in range followed by S_src, -1 and 2^31 - 1 in the same tile: with ent_coef = 0 and the same scale every gradient
    equals the call on the 60 alone (dead lanes add exact zeros), the first five statistics too, T S is the count given and the
    seventh statistic is exactly 3; nothing is read through the three"""
    import torch
    case, inp = R.case_inputs("lstm48x32-relu-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S_src = 5, 65
    d = _dev_inputs(inp, T, S_src)
    good = torch.arange(60, dtype=torch.int32, device=_dev()).flip(0).contiguous()
    bad = torch.cat([good, torch.tensor([S_src, -1, 2 ** 31 - 1], dtype=torch.int32, device=_dev())]).contiguous()
    sc = 1.0 / (T * 60)
    want = [x.clone() for x in _call_idx(pol, case, good, d, scale=sc, ent_coef=0.0)]
    got = _call_idx(pol, case, bad, d, scale=sc, ent_coef=0.0)
    torch.cuda.synchronize()
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(got[3][:5], want[3][:5]) and float(got[3][5]) == T * 63 and float(got[3][6]) == 3.0 and float(want[3][6]) == 0.0
    pol.close()


def test_captured_in_a_graph(envs):
    """ppo_bptt_grad_dev captured after one warm-up call replays with the eager call's bits, also on new contents of the same buffers
    and after an eager call of another size in between (the tape grows only when a call needs more)"""
    import torch
    case, inp = R.case_inputs("lstm64x64x64-tanh-vclip")         # (more than 64 KiB of LDS: the launch raises the kernel's limit)
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
    _call(pol, case, small)                                       # an eager call of another size in between
    flipped = [x.clone() for x in _call(pol, case, dict(d, adv=-d["adv"], ret=d["ret"] + 0.5))]
    d["adv"].neg_()
    d["ret"].add_(0.5)                                            # new contents, the same buffers
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, flipped):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], eager[0]) and not torch.equal(out[1], eager[1])
    pol.close()


def test_closed_loop_of_ten_adam_steps(envs):
    """Ten AdamDev steps (lr 3e-4, log_std stepped too) at (T, S) = (6, 130), device gradients into the device optimiser, beside the
    same ten steps of torch fp32 Adam and autograd on the twin module (LSTMCell loop with torch.where resets, Linear head, value
    Linear).  The loss falls in both, and each parameter tensor ends within 100 x the single-step bound."""
    import torch
    from gym_art_amd.policy import AdamDev
    case, inp = R.case_inputs("lstm64x16x48-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, S = R.TMAX, R.SMAX
    d = _dev_inputs(inp, T, S)
    lr, steps = 3e-4, 10
    ent_const = float(R.ENT_COEF * 2.0 * (1.0 + np.log(2.0 * np.pi)))
    opt = AdamDev(pol, lr=lr)
    loss_dev = []
    for _ in range(steps):
        ls = float(np.asarray(pol.log_std, np.float64).sum())
        g, gv, gls, st = _call(pol, case, d)
        opt.step(g, gv, gls)
        loss_dev.append((float(st[0]) + R.VF_COEF * float(st[3])) / (T * S) - R.ENT_COEF * ls - ent_const)
    (W_ih, W_hh, b_ih, b_hh), head = pol.get_weights()
    wv, bv = pol.get_value_head()
    got = [W_ih, b_ih, W_hh, b_hh] + [a for Wb in head for a in Wb] + [np.concatenate([wv, [bv]]), np.asarray(pol.log_std)]
    opt.close()
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
    bound = 100.0 * R.bounds(case.name, T, S)[0]
    want = [cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh] + [p for l in lins for p in (l.weight, l.bias)] + \
           [torch.cat([critic.weight.reshape(-1), critic.bias.reshape(-1)]), ls]
    errs = [G.rel(np.asarray(a), _np(b)) for a, b in zip(got, want)]
    print("closed loop: parameters after %d steps differ by %.3g at most (bound %.3g)" % (steps, max(errs), bound))
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    assert max(errs) <= bound, (errs, bound)
    pol.close()


def test_no_sequences_gives_zeros(envs):
    import torch
    case, inp = R.case_inputs("lstm16-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    out = [torch.full_like(x, 7.0) for x in _call(pol, case, _dev_inputs(inp, 2, 63))]
    d = _dev_inputs(inp, 2, 0)
    _call(pol, case, d, grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])
    lp, v = _eval(pol, d)
    idx = torch.empty(0, dtype=torch.int32, device=_dev())
    out7 = _call_idx(pol, case, idx, _dev_inputs(inp, 2, 63), stats=torch.full((7,), 7.0, dtype=torch.float64, device=_dev()))
    torch.cuda.synchronize()
    assert lp.shape == (2, 0) and v.shape == (2, 0) and not any(bool(x.any()) for x in out) and not any(bool(x.any()) for x in out7)
    pol.close()


def test_refusals(envs):
    """each returns the stated code with the named text, launches nothing, and the first call repeated afterwards gives its bits"""
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPPolicy
    from tests.gru_util import _gru, _head
    from tests.lstm_util import _lstm
    from tests.policy_util import _layers
    env = envs()
    lib = _lib.load()
    case, inp = R.case_inputs("lstm16-tanh-vclip")
    T, S, H = 5, 65, case.H
    d = _dev_inputs(inp, T, S)
    o, a, dn, h0, c0, lo, adv, ret, vo = (d[k] for k in KEYS)
    cs = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    idx = torch.arange(S, dtype=torch.int32, device=_dev())

    pol, _ = _policy(env, case, inp)
    first = [x.clone() for x in _call(pol, case, d)]
    ev = [x.clone() for x in _eval(pol, d)]
    g, gv, gls, st = (x.clone() for x in first)
    st7 = torch.zeros(7, dtype=torch.float64, device=_dev())
    lp_out, v_out = (x.clone() for x in ev)

    def raw(T=T, S=S, obs=o, h0=h0, c0=c0, ret=ret, v_old=vo, clip=0.2, vclip=0.2, vf=0.5, ent=0.01, scale=1.0, grad=g, grad_value=gv,
            grad_ls=gls, stats=st, handle=None):
        return lib.gaq_policy_grad_ppo_lstm_seq_dev(pol.handle if handle is None else handle, T, S, _lib.ptr(obs), _lib.ptr(a), _lib.ptr(dn),
                                                    _lib.ptr(h0), _lib.ptr(c0), _lib.ptr(lo), _lib.ptr(adv), _lib.ptr(ret), _lib.ptr(v_old), clip,
                                                    vclip, vf, ent, scale, _lib.ptr(grad), _lib.ptr(grad_value), _lib.ptr(grad_ls),
                                                    _lib.ptr(stats), cs)

    def raw_idx(T=T, S=S, idx=idx, S_src=S, c0=c0, stats=st7, handle=None):
        return lib.gaq_policy_grad_ppo_lstm_seq_idx_dev(pol.handle if handle is None else handle, T, S, _lib.ptr(idx), S_src, _lib.ptr(o),
                                                        _lib.ptr(a), _lib.ptr(dn), _lib.ptr(h0), _lib.ptr(c0), _lib.ptr(lo), _lib.ptr(adv),
                                                        _lib.ptr(ret), _lib.ptr(vo), 0.2, 0.2, 0.5, 0.01, 1.0, _lib.ptr(g), _lib.ptr(gv),
                                                        _lib.ptr(gls), _lib.ptr(stats), cs)

    def raw_eval(T=T, S=S, handle=None, logp=lp_out, value=v_out, h_out=None, c_out=None, actions=a, c0=c0):
        return lib.gaq_policy_eval_lstm_seq_dev(pol.handle if handle is None else handle, T, S, _lib.ptr(o), _lib.ptr(actions), _lib.ptr(dn),
                                                _lib.ptr(h0), _lib.ptr(c0), _lib.ptr(logp), _lib.ptr(value), None, _lib.ptr(h_out),
                                                _lib.ptr(c_out), cs)

    def err():
        return lib.gaq_last_error()
    names = {raw: b"gaq_policy_grad_ppo_lstm_seq_dev: ", raw_idx: b"gaq_policy_grad_ppo_lstm_seq_idx_dev: ", raw_eval: b"gaq_policy_eval_lstm_seq_dev: "}
    for f, nm in names.items():
        assert f(T=0) == -1 and nm + b"T must be at least 1" in err()
        assert f(S=-1) == -1 and nm + b"S must not be negative" in err()
        assert f(c0=None) == -1 and b"null" in err()
        assert f(c0=c0.data_ptr() + 4) == -1 and nm + b"pointers must be 4-byte aligned (h0, c0" in err()       # c0: 16 bytes
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
        pol.ppo_bptt_grad_dev(o, a, dn, h0, c0, lo, adv, ret, None, vclip=0.2)
    assert raw(obs=None) == -1 and b"null" in err()
    assert raw(h0=None) == -1 and b"null" in err()
    assert raw(stats=None) == -1 and b"null" in err()
    assert raw(grad=o.view(-1)[:g.numel()]) == -1 and b"overlap" in err()          # an output over an input
    assert raw(grad=c0.view(-1)[:g.numel()]) == -1 and b"overlap" in err()         # ... over c0
    assert raw(grad_ls=g[4:8]) == -1 and b"overlap" in err()                        # two outputs
    assert raw(grad_value=g[:gv.numel()]) == -1 and b"overlap" in err()
    assert raw_eval(h_out=h0) == -1 and b"overlap" in err()
    assert raw_eval(c_out=c0) == -1 and b"overlap" in err()                         # c_out over c0
    both = torch.empty(S * H, device=_dev())
    assert raw_eval(h_out=both, c_out=both) == -1 and b"two outputs overlap" in err()
    assert raw(ret=ret.data_ptr() + 2) == -1 and b"aligned" in err()
    assert raw(h0=h0.data_ptr() + 4) == -1 and b"aligned" in err()                 # h0: 16 bytes
    spare = torch.empty(S * H + 4, device=_dev())
    assert raw_eval(h_out=spare.data_ptr() + 8) == -1 and b"h_out, c_out: 16" in err()
    assert raw_eval(c_out=spare.data_ptr() + 8) == -1 and b"h_out, c_out: 16" in err()       # c_out: 16 bytes
    assert raw(stats=st.data_ptr() + 4) == -1 and b"stats_out: 8" in err()
    assert raw_idx(idx=None) == -1 and b"null" in err()
    assert raw_idx(S_src=0) == -1 and b"S_src must be at least 1" in err()
    # what the handle is: a GRU (by name), a feed-forward policy, a cell over the width limit (the first refused width), weights never set
    gru = GRUPolicy(env, _gru(16, 18, 3), _head(16), "tanh", True, log_std=R.LOG_STD)
    mlp = MLPPolicy.from_arrays(env, _layers([16]), "tanh", True, log_std=R.LOG_STD, engine="mfma")
    wide = LSTMPolicy(env, _lstm(80, 18, 3), _head(80), "tanh", True, log_std=R.LOG_STD)
    from gym_art_amd.policy import _DescRnn, _fill_desc, ENGINES
    from tests.lstm_util import CELL_LSTM
    desc = _fill_desc(_DescRnn(), 18, [16], "tanh", out_tanh=1, engine=ENGINES["mfma"], cell=CELL_LSTM)
    bare = C.c_void_p()
    assert lib.gaq_policy_create_rnn(env._handle, C.byref(desc), C.byref(bare)) == 0
    for f in (raw, raw_idx, raw_eval):
        assert f(handle=gru.handle) == -1 and b"GRU" in err()
        assert f(handle=mlp.handle) == -1 and b"recurrent cell" in err()
        assert f(handle=wide.handle) == -1 and b"width" in err() and b"80" in err()
        assert f(handle=bare) == -1 and b"weights not set" in err()
    lib.gaq_policy_destroy(bare)
    for p in (gru, mlp, wide):
        p.close()
    # the GRU entry points keep their refusal of an LSTM handle
    assert lib.gaq_policy_eval_seq_dev(pol.handle, T, S, _lib.ptr(o), _lib.ptr(a), _lib.ptr(dn), _lib.ptr(h0), None, None, None, None, cs) == -1
    assert b"LSTM" in err()
    # the handle is as usable as before: the first call's bits
    again = _call(pol, case, d)
    ev2 = _eval(pol, d)
    torch.cuda.synchronize()
    for x, y in zip(first + ev, list(again) + list(ev2)):
        assert torch.equal(x, y)
    pol.close()
