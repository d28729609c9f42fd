"""The learner's forward pass for a recurrent policy with an encoder (gaq.h "sequences through an encoder";
GRUPolicy / LSTMPolicy.evaluate_enc_seq_dev): the rollout's encoder kernel over the stored rows, then the cell's forward sequence kernel on
the features.

1. on a rollout's recorded observations, dones and pre-rollout states it gives the rollout's bits: the deterministic actions as mean,
   values[:T], the final h (and c); with exploration V and the states still bit for bit and logp within 1e-4 of the recorded one (the
   bound of the encoder-less calls' tests: only z = (a - mean) / std is recomputed, from a mean that is the rollout's bits);
2. a window split in time chains through h_out / c_out to the same bits;
3. the same call twice gives the same bits, a smaller call after the largest one leaves the scratch where it was, and a graph
   captured after the largest call replays to the eager bits;
4. S = 0 is accepted and writes nothing; refusals by text launch nothing, and a handle without an encoder keeps the bits of the calls
   it always had.

SHAPES.  N = 130 sequences: two whole 64-column tiles and one of 2.  T = 20 with episodes of 16 steps (ep_time = 0.15), so every sequence
meets a done inside the window and carries a state out of it.  D = 18 is one rollout call; at D = 19, N x D x 4 bytes is no multiple
of 16 and the rollout is twenty calls of one step (tests/test_gpu_policy_encoder.py SHAPES) -- the evaluation is one call either way.
Encoders: 64 (the flagship 18-enc64-GRU64-64), 80 behind the exact-table normaliser (wave 0 owns two chunks), two layers 32-64 at
D = 19 (the partial k-step), 128 (the width limit) into LSTM64-64-64, the largest forward LDS of the family (110.25 KiB)."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from tests.enc_util import _cell, _desc_enc, _encoder
from tests.gru_util import _head
from tests.policy_util import _dev
from tests.test_gpu_policy_encoder import LOG_STD, _env, _nan, _Net, _RawPolicy, _states, _window

pytestmark = pytest.mark.gpu

T = 20
# (cell, encoder widths, D, H, head, act, out_tanh, N, layout, norm) -- tests/test_gpu_policy_encoder.py's case record
CASES = [("gru", (64,), 18, 64, (64,), "tanh", True, 130, "alias", False),
         ("lstm", (80,), 18, 48, (32,), "tanh", False, 130, "plain", True),
         ("gru", (32, 64), 19, 16, (), "relu", False, 130, "plain", False),
         ("lstm", (128,), 19, 64, (64, 64), "relu", True, 130, "alias", False)]
IDS = ["%s-enc%s-d%d-h%d%s" % (c[0], "x".join(map(str, c[1])), c[2], c[3], "-norm" if c[9] else "") for c in CASES]


def _bits(x, y):
    import torch
    return x.shape == y.shape and bool(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)))


def _recorded(case, log_std=None):
    """one recorded window of the case: (env, pol, net, window, what evaluate_enc_seq_dev takes of it)"""
    import torch
    env = _env(case[2], case[7], case[8])
    net = _Net(case, env, CASES.index(case))
    pol = net.build(env, log_std=log_std)
    w = _window(env, pol, net, T, logp=log_std is not None, term=False)
    seq = torch.cat([w["o0"][None], w["o"][:-1]]).contiguous()
    s0 = [torch.as_tensor(s, device=_dev()).contiguous() for s in w["s0"]]
    return env, pol, net, w, (seq, w["a"], w["d"], s0)


def _evaluate(pol, seq, a, dn, s0, **kw):
    """-> (logp, value, mean, [h_out, c_out]) into NaN-filled tensors of their own"""
    mean = _nan(*seq.shape[:2], 4)
    outs = [_nan(*s.shape) for s in s0]
    names = ("h_out", "c_out")[:len(s0)]
    lp, v = pol.evaluate_enc_seq_dev(seq, a, dn, *s0, mean=mean, **dict(zip(names, outs)), **kw)
    return lp, v, mean, outs


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_rollouts_bits(case):
    import torch
    for explore in (False, True):
        env, pol, net, w, (seq, a, dn, s0) = _recorded(case, LOG_STD if explore else None)
        lp, v, mean, outs = _evaluate(pol, seq, a if explore else None, dn, s0)
        torch.cuda.synchronize()
        carried = int(outs[0].any(dim=1).sum())
        print("%s explore=%d: %d dones inside the window, %d of %d rows carry a state out" % (IDS[CASES.index(case)], explore,
                                                                                              int(dn[:-1].sum()), carried, case[7]))
        assert int(dn[:-1].sum()) > 0 and carried > 0                  # the done select is taken, and not every state is a zero
        assert _bits(v, w["v"][:T]), (case, explore)
        for got, want in zip(outs, _states(pol)):
            assert _bits(got, want), (case, explore)
        if explore:
            err = float((lp - w["lp"]).abs().max())
            print("%s: |logp - recorded| %.3g (bound 1e-4)" % (IDS[CASES.index(case)], err))
            assert err <= 1e-4
            assert not _bits(mean, a)
        else:
            assert lp is None and _bits(mean, a), case
        pol.close(); env.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_chaining_in_time(case):
    """T = 20 in one call == 7 then 13 chained through h_out (and c_out): logp, value, mean and the final states bit for bit"""
    import torch
    env, pol, net, w, (seq, a, dn, s0) = _recorded(case, LOG_STD)
    whole = _evaluate(pol, seq, a, dn, s0)
    first = _evaluate(pol, seq[:7].contiguous(), a[:7].contiguous(), dn[:7].contiguous(), s0)
    second = _evaluate(pol, seq[7:].contiguous(), a[7:].contiguous(), dn[7:].contiguous(), first[3])
    torch.cuda.synchronize()
    for k in range(3):
        assert bool(torch.isfinite(whole[k]).all()) and _bits(whole[k], torch.cat([first[k], second[k]])), (case, k)
    for x, y in zip(whole[3], second[3]):
        assert _bits(x, y) and bool(x.any())
    pol.close(); env.close()


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_repeats_the_scratch_and_a_captured_graph(case):
    """the largest call, a smaller one (one step of 65 sequences: the scratch does not move), the largest again, then a graph captured
    of it and replayed twice after the outputs were poisoned: the same bits every time"""
    import torch
    env, pol, net, w, (seq, a, dn, s0) = _recorded(case, LOG_STD)
    ref = _evaluate(pol, seq, a, dn, s0)
    small = _evaluate(pol, seq[:1, :65].contiguous(), a[:1, :65].contiguous(), dn[:1, :65].contiguous(), [s[:65].contiguous() for s in s0])
    again = _evaluate(pol, seq, a, dn, s0)
    torch.cuda.synchronize()
    assert _bits(small[1], ref[1][:1, :65]) and _bits(small[2], ref[2][:1, :65])
    flat = lambda r: [r[0], r[1], r[2]] + r[3]
    for x, y in zip(flat(ref), flat(again)):
        assert bool(torch.isfinite(x).all()) and _bits(x, y)
    lp, v, mean = _nan(T, case[7]), _nan(T, case[7]), _nan(T, case[7], 4)
    outs = [_nan(*s.shape) for s in s0]
    kw = dict(zip(("h_out", "c_out"), outs))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up on a side stream, as a capture wants it
        pol.evaluate_enc_seq_dev(seq, a, dn, *s0, logp=lp, value=v, mean=mean, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pol.evaluate_enc_seq_dev(seq, a, dn, *s0, logp=lp, value=v, mean=mean, **kw)
    for rep in range(2):
        for x in [lp, v, mean] + outs:
            x.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(flat(ref), [lp, v, mean] + outs):
            assert _bits(x, y), rep
    pol.close(); env.close()


def _err():
    return _lib.load().gaq_last_error().decode()


def test_refusals_launch_nothing_and_an_empty_call_is_accepted():
    import torch
    from gym_art_amd.policy import GRUPolicy
    lib = _lib.load()
    D, n, S, H = 18, 66, 8, 16
    env = _env(D, n)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    obs, acts = torch.zeros((3, S, D), device=_dev()), torch.zeros((3, S, 4), device=_dev())
    dn = torch.zeros((3, S), dtype=torch.uint8, device=_dev())
    h0, c0 = torch.zeros((S, H), device=_dev()), torch.zeros((S, H), device=_dev())
    out = {k: _nan(3, S) for k in ("logp", "value")}
    mean, h_out = _nan(3, S, 4), _nan(S, H)

    def raw(handle, h0_=h0, c0_=None, c_out=None):
        return lib.gaq_policy_eval_enc_seq_dev(handle, 3, S, _lib.ptr(obs), _lib.ptr(acts), _lib.ptr(dn), _lib.ptr(h0_), _lib.ptr(c0_),
                                               _lib.ptr(out["logp"]), _lib.ptr(out["value"]), _lib.ptr(mean), _lib.ptr(h_out),
                                               _lib.ptr(c_out), st)

    def untouched():
        torch.cuda.synchronize()
        return all(bool(torch.isnan(x).all()) for x in (out["logp"], out["value"], mean, h_out))

    value = (np.zeros(H, np.float32), 0.0)
    # (a) a handle without an encoder: refused by the method and by the library, and the calls it always had keep their bits
    plain = GRUPolicy(env, _cell("gru", H, D), _head(H), log_std=LOG_STD, value=value)
    before = [x.clone() for x in plain.evaluate_seq_dev(obs, acts, dn, h0)]
    with pytest.raises(ValueError, match="encoder"):
        plain.evaluate_enc_seq_dev(obs, acts, dn, h0)
    assert raw(plain.handle) == -1 and "encoder" in _err() and "has none" in _err()
    after = plain.evaluate_seq_dev(obs, acts, dn, h0)
    assert all(_bits(x, y) for x, y in zip(before, after)) and untouched()
    plain.close()
    # (b) a GRU behind an encoder: c0 or c_out is an LSTM's; a null h0; the parent call keeps refusing it
    pol = GRUPolicy.with_encoder(env, _encoder(D, (32,)), _cell("gru", H, 32), _head(H), log_std=LOG_STD, value=value)
    assert raw(pol.handle, c0_=c0) == -1 and "must be NULL" in _err() and "GRU" in _err()
    assert raw(pol.handle, c_out=c0) == -1 and "must be NULL" in _err()
    assert raw(pol.handle, h0_=None) == -1 and "null" in _err()
    with pytest.raises(ValueError, match="encoder"):
        pol.evaluate_seq_dev(obs, acts, dn, h0)
    with pytest.raises(ValueError, match="h0"):
        pol.evaluate_enc_seq_dev(obs, acts, dn, h0[:4])
    assert untouched()
    # ... and it is accepted as it should be: S = 0 launches nothing, S = 8 fills every output
    e = lambda *shape: torch.empty(shape, device=_dev())
    lp0, v0 = pol.evaluate_enc_seq_dev(e(3, 0, D), e(3, 0, 4), torch.empty((3, 0), dtype=torch.uint8, device=_dev()), e(0, H))
    assert lp0.shape == (3, 0) and v0.shape == (3, 0) and untouched()
    assert raw(pol.handle) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in (out["logp"], out["value"], mean, h_out))
    pol.close()
    for x in (out["logp"], out["value"], mean, h_out):
        x.fill_(float("nan"))
    # (c) an encoder wider than the gradient family takes: the text names the width
    wide = GRUPolicy.with_encoder(env, _encoder(D, (144,)), _cell("gru", H, 144), _head(H), log_std=LOG_STD, value=value)
    with pytest.raises(ValueError, match="width"):
        wide.evaluate_enc_seq_dev(obs, acts, dn, h0)
    assert "128" in _err() and "144" in _err() and untouched()
    wide.close()
    # (d) encoder weights never set
    case = ("gru", (32,), D, H, (), "tanh", True, n, "alias", False)
    net = _Net(case, env)
    unset = _RawPolicy(env, net, "gaq_policy_create_rnn_enc", _desc_enc([H], (32,), D, 1))
    assert raw(unset.handle) == -1 and "encoder weights not set" in _err() and untouched()
    unset.close()
    env.close()
