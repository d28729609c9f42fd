"""The learner's gradient for a recurrent policy with an encoder at its edge shapes (tests/policy_grad_enc_edges.py): the largest LDS
the backward sequence kernel is launched with (enc112-LSTM64-64-64, 160 768 B; 161 024 B in the idx form), the encoder's backward above
64 KiB of LDS ((128, 128): 78 336 B, the hipFuncSetAttribute branch of both instantiations), narrowing and smallest two-layer encoders,
H = 48 behind an encoder -- each against the fp64 reference under 8 x torch fp32's committed error, by the rule and with the helpers of
tests/test_gpu_policy_grad_enc.py; the refusal of E = 128 in front of LSTM64-64-64; and the idx form with REPEATED indices, where two
columns of a tile, or of two workgroups, name the same source row of feat and dfeat: bit for bit the contiguous call on the gathered
inputs, and with indices out of range the gradient of the valid ones.  Every figure a test bounds is printed before it is asserted."""
import numpy as np
import pytest

from tests import policy_grad_enc_edges as E
from tests import policy_grad_enc_ref as R
from tests.policy_util import _dev, environ
from tests.test_gpu_policy_grad_enc import (SEQ_KEYS, _bits, _call, _call_idx, _dev_inputs, _errors, _np, _policy, _states, _t,  # noqa: F401
                                            envs)  # (envs: the module's fixture)

G = R.G
pytestmark = pytest.mark.gpu


def _check(case, inp, pol, T, S, what):
    """test_gpu_policy_grad_enc._check on this list's references and bounds: every tensor of the cell, the head and the value head,
    log_std, every tensor of the encoder, logp and V of evaluate_enc_seq_dev and the sums under their bounds, the counts exact ->
    the worst error / bound of (the gradient, the encoder's gradient, logp, V and the sums)"""
    ref = E.case_ref(case.name, T, S)
    bg, be, blp, bv, bloss, bkl, blv = E.bounds(case.name, T, S)
    d = _dev_inputs(case, inp, T, S)
    out = _call(pol, case, d)
    lp, v = pol.evaluate_enc_seq_dev(d["obs"], d["actions"], d["done"], *[d[k] for k in _states(case)])
    errs, eerrs = _errors(pol, case, out, ref)
    st = _np(out[4])
    e_lp = G.rel(_np(lp), ref["logp"])
    e_v = G.rel(_np(v), ref["value"]) if case.value else 0.0
    e_loss, e_kl = G.rel(st[0], ref["stats"][0]), G.rel(st[2], ref["stats"][2])
    e_lv = G.rel(st[3], ref["stats"][3]) if case.value else float(st[3])
    print("%s %s (T, S) = (%d, %d): grad %.3g (bound %.3g) [%s] encoder %.3g (bound %.3g) [%s] logp %.3g (%.3g) V %.3g (%.3g) loss %.3g (%.3g) "
          "kl %.3g (%.3g) L_V %.3g (%.3g) clipped %d cut %d" % (case.name, what, T, S, max(errs), bg, " ".join("%.3g" % e for e in errs),
                                                                max(eerrs), be, " ".join("%.3g" % e for e in eerrs), e_lp, blp, e_v, bv,
                                                                e_loss, bloss, e_kl, bkl, e_lv, blv, st[1], st[4]))
    assert len(errs) == 4 + 2 * (len(case.head) + 1) + (1 if case.value else 0) + 1 and len(eerrs) == 2 * len(case.enc)
    assert max(errs) <= bg, (case.name, what, T, S, errs, bg)
    assert max(eerrs) <= be, (case.name, what, T, S, eerrs, be)
    assert e_lp <= blp and e_v <= bv and e_loss <= bloss and e_kl <= bkl and e_lv <= blv, (case.name, what, T, S)
    assert st[1] == ref["stats"][1] and st[4] == ref["stats"][4] and st[5] == T * S, (st, ref["stats"])     # the counts are exact
    if not case.value:
        assert v is None and out[2] is None and st[3] == 0.0 and st[4] == 0.0
    rest = [e_lp / blp, e_v / bv, e_loss / bloss, e_kl / bkl] + ([e_lv / blv] if case.value else [])
    return max(errs) / bg, max(eerrs) / be, max(rest)


@pytest.mark.parametrize("case", E.EDGE_CASES, ids=[c.name for c in E.EDGE_CASES])
def test_case_matrix(case, envs):
    """every edge case at every (T, S) of CONFIGS, then (6, 130) over 1 and over 3 workgroups"""
    _, inp = E.case_inputs(case.name)
    assert R.conditions(case, inp) is None
    pol, norm = _policy(envs(case.D), case, inp)
    worst = (0.0, 0.0, 0.0)
    for T, S in E.CONFIGS:
        worst = tuple(map(max, worst, _check(case, inp, pol, T, S, "default")))
    for groups in ("1", "3"):
        with environ(GAQ_GRAD_GROUPS=groups):
            worst = tuple(map(max, worst, _check(case, inp, pol, E.TMAX, E.SMAX, groups + " group(s)")))
    print("%s: worst error / bound: gradient %.3f, encoder gradient %.3f, logp, V and the sums %.3f; LDS asked for: sequence kernel %d B, "
          "encoder backward %d B"
          % (case.name, *worst, *E.case_lds(case)))
    pol.close()
    if norm is not None:
        norm.close()


def _slack(d):
    """the same tensors in the middle of allocations three times their size whose rest is NaN (done: 1)"""
    import torch
    out = {}
    for k, x in d.items():
        n = x.numel()
        big = torch.full((3 * n,), 1 if x.dtype == torch.uint8 else float("nan"), dtype=x.dtype, device=x.device)
        big[n:2 * n] = x.reshape(-1)
        out[k] = big[n:2 * n].view(x.shape)
    return out


def _gathered(case, full, idx):
    """the columns idx names, contiguous, between NaN slack"""
    li, states = idx.long(), _states(case)
    return _slack({k: (full[k][li] if k in states else full[k][:, li]).contiguous() for k in full})


def _poisoned(case, full, idx):
    """the source tensors with NaN (done: 1) in every column no index names"""
    import torch
    S_src = full["done"].shape[1]
    ok = (idx >= 0) & (idx < S_src)
    named = torch.zeros(S_src, dtype=torch.bool, device=_dev())
    named[idx[ok].long()] = True
    out, states = {}, _states(case)
    for k, x in full.items():
        x = x.clone()
        if k in states:
            x[~named] = float("nan")
        else:
            x[:, ~named] = 1 if x.dtype == torch.uint8 else float("nan")
        out[k] = x
    return out


def _clone(out):
    return [x.clone() if x is not None else None for x in out]


def _same_as_contiguous(got, want, what):
    for k, (x, y) in enumerate(zip(got, want)):
        assert _bits(x[:6], y) if k == 4 else _bits(x, y), (what, k)


TOP = ["enc112-lstm64x64x64-tanh-vclip", "enc128x128-gru64x64-relu"]


@pytest.mark.parametrize("name", TOP)
def test_the_idx_form_at_the_largest_lds(name, envs):
    """the LDS maximum (+ 256 B: 161 024 B) and grad_feat_kernel<true> above 64 KiB (78 592 B): a permutation's 65 of the 130 columns is
    the contiguous call on the gathered inputs bit for bit; the same call repeated gives the same bits; a captured graph of the idx
    call replays to the eager bits after its outputs were poisoned"""
    import torch
    from gym_art_amd.policy import perm_dev
    case, inp = E.case_inputs(name)
    pol, norm = _policy(envs(case.D), case, inp)
    T, S_src, S = E.TMAX, E.SMAX, 65
    print("%s idx form: sequence kernel %d B, encoder backward %d B" % (name, *E.case_lds(case, idx=True)))
    full = _dev_inputs(case, inp, T, S_src)
    idx = perm_dev(S_src, seed=23, device=_dev())[:S].contiguous()
    assert len(set(_np(idx).tolist())) == S
    want = _clone(_call(pol, case, _gathered(case, full, idx)))
    src = _poisoned(case, full, idx)
    got = _clone(_call_idx(pol, case, idx, src))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in got if x is not None)
    _same_as_contiguous(got, want, name)
    assert float(got[4][5]) == T * S and float(got[4][6]) == 0.0
    again = _call_idx(pol, case, idx, src)
    assert all(_bits(x, y) for x, y in zip(again, got))
    # captured (the calls above have sized the handle's scratch)
    outs = [torch.empty_like(x) for x in got]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _call_idx(pol, case, idx, src, grad=outs[0], grad_encoder=outs[1], grad_value=outs[2], grad_log_std=outs[3], stats=outs[4])
    for x in outs:
        x.fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(_bits(x, y) for x, y in zip(outs, got))
    del graph
    pol.close()
    if norm is not None:
        norm.close()


def test_e128_before_lstm64x64x64_is_refused_by_the_gradient_calls_only(envs):
    """gaq.h: the forward call takes enc128-LSTM64-64-64 (8448 + 272 x (128 + 128 + 192) = 130 304 B), the backward needs 165 120 B and is
    refused with "in_dim too large ..." by both entry points, which leave NaN-filled outputs untouched; the evaluation repeated
    afterwards gives its earlier bits"""
    import torch
    from gym_art_amd.policy import LSTMPolicy
    from tests.enc_util import _encoder
    from tests.gru_util import _head
    from tests.lstm_util import _lstm
    assert E.seq_lds(128, True, 64, (64, 64)) == 165120 > E.LDS_MAX >= E.seq_lds(128, True, 64, (64, 64), bwd=False)
    rng = np.random.RandomState(41)
    T, S, D, H = 2, 8, 18, 64
    wv, bv = (rng.randn(64) / 8.0).astype(np.float32), np.float32(0.1)
    pol = LSTMPolicy.with_encoder(envs(D), _encoder(D, (128,), 1), _lstm(H, 128, 2), _head(H, (64, 64), 3), "tanh", True, log_std=R.LOG_STD,
                                  value=(wv, bv))
    f = lambda *shape: _t(rng.randn(*shape).astype(np.float32))
    obs, act, h0, c0 = f(T, S, D), f(T, S, 4), f(S, H), f(S, H)
    done = torch.zeros((T, S), dtype=torch.uint8, device=_dev())
    logp_old, adv, ret, v_old = f(T, S), f(T, S), f(T, S), f(T, S)
    lp, v = (x.clone() for x in pol.evaluate_enc_seq_dev(obs, act, done, h0, c0))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(v).all())
    nan = lambda n, dtype=torch.float32: torch.full((n,), float("nan"), dtype=dtype, device=_dev())
    outs = dict(grad=nan(pol._count), grad_encoder=nan(pol._enc_count), grad_value=nan(65), grad_log_std=nan(4))
    kw = dict(clip=R.CLIP, vclip=R.VCLIP, vf_coef=R.VF_COEF, ent_coef=R.ENT_COEF)
    with pytest.raises(ValueError, match="gaq_policy_grad_ppo_enc_seq_dev: in_dim too large for the sequence kernel's LDS"):
        pol.ppo_enc_seq_grad_dev(obs, act, done, h0, c0, logp_old, adv, ret, v_old, stats=nan(6, torch.float64), **outs, **kw)
    idx = torch.arange(S - 1, -1, -1, dtype=torch.int32, device=_dev())
    stats7 = nan(7, torch.float64)
    with pytest.raises(ValueError, match="gaq_policy_grad_ppo_enc_seq_idx_dev: in_dim too large for the sequence kernel's LDS"):
        pol.ppo_enc_seq_grad_idx_dev(idx, obs, act, done, h0, c0, logp_old, adv, ret, v_old, stats=stats7, **outs, **kw)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(x).all()) for x in outs.values()) and bool(torch.isnan(stats7).all())
    lp2, v2 = pol.evaluate_enc_seq_dev(obs, act, done, h0, c0)
    assert _bits(lp2, lp) and _bits(v2, v)
    pol.close()


# ---- repeated indices -------------------------------------------------------------------------------------------------------------
REPEAT = ["enc128x16-gru48-relu-norm", "enc64x32-lstm48x32-tanh-vclip-d19"]       # a GRU and an LSTM, each behind two encoder layers
BAD = (-1, None, 2 ** 31 - 1)                                                      # (None: S_src itself)


def _vectors():
    """{kind: (S_src, the index vector)}: 65 drawn with replacement -- columns recur inside the first tile and across the two tiles --,
    192 > S_src with every column at least once, 65 times one column, and 2 of S_src = 1"""
    rng = np.random.RandomState(5)
    drawn = rng.randint(0, 130, 65)
    drawn[64] = drawn[3]                                            # tile 1's only column is one of tile 0's
    assert len(set(drawn[:64].tolist())) < 60
    cover = np.concatenate([rng.permutation(130), rng.randint(0, 130, 62)])
    cover = cover[rng.permutation(192)]
    assert len(set(cover.tolist())) == 130
    return {"drawn": (130, drawn), "cover": (130, cover), "one": (130, np.full(65, 77)), "src1": (1, np.zeros(2, np.int64))}


def _with_bad(S_src, vec):
    """three entries replaced by -1, S_src and 2^31 - 1, in the first tile, in the middle and at the end (the vector of 2: the three
    are put in, before, between and after its entries, so that the valid ones are still the vector)"""
    bad = [S_src if b is None else b for b in BAD]
    if vec.size < 4:
        return np.array([bad[0], vec[0], bad[1], vec[1], bad[2]], np.int64)
    out = vec.astype(np.int64).copy()
    out[1], out[vec.size // 2], out[-1] = bad
    return out


@pytest.mark.parametrize("name", REPEAT)
def test_repeated_indices_are_the_contiguous_call_on_the_gathered_columns(name, envs):
    """two columns of a tile, or of two workgroups, that name one source column store the same feat and dfeat row and the encoder's
    backward reads it once per naming: every output is bit for bit the contiguous call's on the gathered inputs (between NaN slack),
    with NaN in every source column no index names; stats[5] = T S, stats[6] = 0"""
    import torch
    case, inp = E.case_inputs(name)
    pol, norm = _policy(envs(case.D), case, inp)
    T = E.TMAX
    for kind, (S_src, vec) in _vectors().items():
        S = vec.size
        full = _dev_inputs(case, inp, T, S_src)
        idx = _t(vec, torch.int32)
        want = _clone(_call(pol, case, _gathered(case, full, idx)))
        got = _call_idx(pol, case, idx, _poisoned(case, full, idx))
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(x).all()) for x in got if x is not None), kind
        _same_as_contiguous(got, want, (name, kind))
        st = _np(got[4])
        print("%s %s: S %d of S_src %d, rows %g skipped %g clipped %g" % (name, kind, S, S_src, st[5], st[6], st[1]))
        assert st[5] == T * S and st[6] == 0.0
        assert float(got[1].abs().max()) > 0.0
    pol.close()
    if norm is not None:
        norm.close()


@pytest.mark.parametrize("name", REPEAT)
def test_repeated_indices_with_three_out_of_range(name, envs):
    """the same vectors with -1, S_src and 2^31 - 1 in three places: stats[6] = 3, stats[5] = T S, the clipped count the reference's,
    and the gradients those of the valid entries at the call's scale -- against the fp64 reference on those columns (repeats
    included), under 8 x torch fp32's error on the same sub-problem (computed here), as
    test_an_index_out_of_range_contributes_nothing_and_is_counted bounds it.  (The entropy bonus's term of grad_log_std is
    -ent_coef scale T S with the call's S, the three included.)"""
    import torch
    case, inp = E.case_inputs(name)
    pol, norm = _policy(envs(case.D), case, inp)
    T = E.TMAX
    for kind, (S_src, vec) in _vectors().items():
        vec = _with_bad(S_src, vec)
        S = vec.size
        ok = (vec >= 0) & (vec < S_src)
        keep = vec[ok]
        assert int((~ok).sum()) == 3 and keep.size == S - 3
        scale = 1.0 / (T * keep.size)
        full = _dev_inputs(case, inp, T, S_src)
        idx = _t(vec, torch.int32)
        got = _call_idx(pol, case, idx, _poisoned(case, full, idx), scale=scale)
        sub = dict(inp)
        for k in SEQ_KEYS + ("x",):
            sub[k] = inp[k][:, keep]
        for k in _states(case):
            sub[k] = inp[k][keep]
        ref = R.ppo_enc_seq(case, sub, T, keep.size, scale=scale)
        ref = dict(ref, glogstd=ref["glogstd"] - R.ENT_COEF * scale * T * 3)
        errs, eerrs = _errors(pol, case, got, ref)
        base = R.torch_errors(case, sub, T, keep.size, torch.float32)
        bg, be = R.FACTOR * base[0], R.FACTOR * base[1]
        st = _np(got[4])
        print("%s %s with three out of range: grad %.3g (bound %.3g) encoder %.3g (bound %.3g) skipped %g rows %g"
              % (name, kind, max(errs), bg, max(eerrs), be, st[6], st[5]))
        assert max(errs) <= bg and max(eerrs) <= be, (name, kind, errs, bg, eerrs, be)
        assert st[6] == 3.0 and st[5] == T * S and st[1] == ref["stats"][1]
    pol.close()
    if norm is not None:
        norm.close()
