"""Shuffled minibatches on the device (gaq.h "shuffled minibatches"): the four index-gathered gradient calls against their oracle -- the
existing contiguous call on torch-gathered inputs, bit for bit (torch.equal, no tolerance) -- at every tile edge, with duplicates, under
two workgroups, with an ObsNorm; indices out of range (skipped, counted, never read: the sources lie between NaN slack); gaq_perm_dev
against tests/perm_ref.py bit for bit; a captured epoch of shuffled minibatches against the eager one; the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_grad_seq_ref as R
from tests.perm_ref import perm_ref
from tests.policy_util import _dev, _layers, environ

pytestmark = pytest.mark.gpu

REPR = {18: "xyz_vxyz_R_omega", 19: "xyz_vxyz_R_omega_h"}
LOG_STD = R.LOG_STD
NETS = {"18-16-tanh": (18, [16], "tanh", True, False), "19-48x80x32-relu-norm": (19, [48, 80, 32], "relu", False, True)}
ROW_CONFIGS = [(1, 1, None), (1, 200, None), (63, 65, None), (64, 65, None), (65, 65, None), (130, 200, None), (130, 200, 2)]   # rows, src, groups
SEQ_CONFIGS = [(1, 1, 3, None), (2, 63, 65, None), (5, 65, 130, None), (6, 130, 200, 2)]                                      # T, S, S_src, groups
SRC = 200
COEF = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)


@pytest.fixture(scope="module")
def envs():
    from gym_art_amd import QuadrotorEnv
    made = {}

    def get(D=18):
        if D not in made:
            made[D] = QuadrotorEnv(num_envs=64, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True, obs_repr=REPR[D])
            assert made[D].obs_dim == D
        return made[D]
    yield get
    for e in made.values():
        e.close()


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=_dev())


def _groups(g):
    return environ(GAQ_GRAD_GROUPS=str(g)) if g else environ()


def _same(got, want, what):
    """every tensor of `got` equals its twin in `want` (None matches None) and is finite"""
    import torch
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, (what, k)
            continue
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (what, k)


def _clones(out):
    return [None if x is None else x.clone() for x in out]


def _idx_kinds(rows, src, seed):
    """the index vectors of a config: a perm_dev prefix, the identity, the reverse, all the same row"""
    import torch
    from gym_art_amd.policy import perm_dev
    ar = torch.arange(rows, dtype=torch.int32, device=_dev())
    return {"perm": perm_dev(src, seed, epoch=rows, device=_dev())[:rows], "identity": ar, "reverse": (src - 1 - ar).contiguous(),
            "same": torch.full((rows,), src // 2, dtype=torch.int32, device=_dev())}


def _nets(env, name):
    """(policy with a value head, critic, normaliser or None) of NETS[name]"""
    from gym_art_amd.policy import MLPCritic, MLPPolicy, ObsNorm
    D, widths, act, out_tanh, normed = NETS[name]
    norm = None
    if normed:                                                     # every column with a mean and a scale of its own
        norm = ObsNorm.from_stats(env, 0.05 * np.arange(D) - 0.4, 0.5 + 0.1 * np.arange(D), 1.0, 1e-5, 4.0)
    rng = np.random.RandomState(5)
    layers = [(0.5 * W, 0.5 * b) for W, b in _layers(widths, D, seed=11)]
    wv, bv = (rng.randn(widths[-1]) / np.sqrt(widths[-1])).astype(np.float32), np.float32(0.1)
    pol = MLPPolicy.from_arrays(env, layers, act, out_tanh, log_std=LOG_STD, engine="mfma", value=(wv, bv), obs_norm=norm)
    cl = [(0.5 * W, 0.5 * b) for W, b in _layers(widths, D, seed=12)]
    cri = MLPCritic.from_arrays(env, cl[:-1] + [(cl[-1][0][:1], cl[-1][1][:1])], act)
    if norm is not None:
        cri.set_obs_norm(norm)
    return pol, cri, norm


def _slack(flat_shape, pad, dtype=None, fill=float("nan")):
    """a contiguous tensor of `flat_shape` that is a view into a larger allocation with `pad` elements of `fill` before and after it"""
    import torch
    n = int(np.prod(flat_shape))
    big = torch.full((n + 2 * pad,), fill, dtype=dtype or torch.float32, device=_dev())
    return big, big[pad:pad + n].view(flat_shape)


def _row_data(pol, D, src=SRC):
    """the source arrays of the row forms, each between one slack row of NaN: obs, actions, logp_old, adv, ret, v_old, target"""
    import torch
    rng = np.random.RandomState(21)
    keep, d = [], {}
    for key, shape, pad in (("obs", (src, D), D), ("actions", (src, 4), 4), ("logp_old", (src,), 1), ("adv", (src,), 1), ("ret", (src,), 1),
                            ("v_old", (src,), 1), ("target", (src,), 1)):
        big, d[key] = _slack(shape, pad)
        keep.append(big)
    d["obs"].copy_(_t(rng.randn(src, D).astype(np.float32)))
    d["actions"].copy_(_t((0.8 * rng.randn(src, 4)).astype(np.float32)))
    lp, v = pol.evaluate_dev(d["obs"], d["actions"])
    d["logp_old"].copy_(lp + _t((0.15 * rng.randn(src)).astype(np.float32)))
    d["adv"].copy_(_t(rng.randn(src).astype(np.float32)))
    d["ret"].copy_(v + _t((0.5 * rng.randn(src)).astype(np.float32)))
    d["v_old"].copy_(v + _t((0.25 * rng.randn(src)).astype(np.float32)))
    d["target"].copy_(_t(rng.randn(src).astype(np.float32)))
    torch.cuda.synchronize()
    d["_keep"] = keep
    return d


ROW_FORMS = ("ppo", "ac", "ac-vclip", "mse")


def _row_call(form, pol, cri, d, idx=None, n=None, **kw):
    """the contiguous call on the first n rows of d (idx None) or the idx call on d's first n source rows"""
    s = slice(0, n)
    if form == "mse":
        return cri.mse_grad_dev(d["obs"][s], d["target"][s], **kw) if idx is None else cri.mse_grad_idx_dev(idx, d["obs"][s], d["target"][s], **kw)
    if form == "ppo":
        a = (d["obs"][s], d["actions"][s], d["logp_old"][s], d["adv"][s])
        return pol.ppo_grad_dev(*a, clip=0.2, **kw) if idx is None else pol.ppo_grad_idx_dev(idx, *a, clip=0.2, **kw)
    vclip = 0.2 if form == "ac-vclip" else None
    a = (d["obs"][s], d["actions"][s], d["logp_old"][s], d["adv"][s], d["ret"][s], d["v_old"][s] if vclip else None)
    if idx is None:
        return pol.ppo_ac_grad_dev(*a, vclip=vclip, **COEF, **kw)
    return pol.ppo_ac_grad_idx_dev(idx, *a, vclip=vclip, **COEF, **kw)


def _gathered(d, idx):
    j = idx.long()
    return {k: v[j].contiguous() for k, v in d.items() if k != "_keep"}


def _split(out):
    """(the tensors before stats, stats)"""
    return list(out[:-1]), out[-1]


@pytest.mark.parametrize("net", list(NETS))
def test_row_forms_are_the_contiguous_call_on_gathered_rows(net, envs):
    """every form x (rows, src_rows) x kind of idx: every gradient and the parent's statistics are the parent call's bits on x[idx], the
    trailing statistic is 0; the identity at rows == src_rows is also the contiguous call on the buffers themselves; and the parent
    call repeated after the idx call gives the bits it gave before (they share the handle's scratch)"""
    import torch
    D = NETS[net][0]
    pol, cri, norm = _nets(envs(D), net)
    d = _row_data(pol, D)
    n_checked = 0
    for form in ROW_FORMS:
        for rows, src, groups in ROW_CONFIGS:
            for kind, idx in _idx_kinds(rows, src, seed=rows + src).items():
                what = (net, form, rows, src, groups, kind)
                with _groups(groups):
                    want = _clones(_row_call(form, pol, cri, _gathered(d, idx), n=rows))      # the parent first: its outputs are cloned
                    got = _row_call(form, pol, cri, d, idx=idx, n=src)
                    again = _row_call(form, pol, cri, _gathered(d, idx), n=rows)
                    torch.cuda.synchronize()
                    (g, st), (wg, wst) = _split(got), _split(want)
                    _same(g, wg, what)
                    # (equal because computed alike, not because both are zero; one row, alone or repeated, may be a clipped one,
                    #  whose gradient is 0)
                    assert rows < 63 or kind == "same" or float(wg[0].abs().max()) > 0.0, what
                    assert st.shape[0] == wst.shape[0] + 1 and torch.equal(st[:-1], wst) and float(st[-1]) == 0.0, (what, st, wst)
                    assert float(st[-2]) == rows, what
                    _same(again, want, what)
                    if kind == "identity" and rows == src:
                        own = _row_call(form, pol, cri, d, n=rows)
                        torch.cuda.synchronize()
                        _same(_split(own)[0], g, what)
                n_checked += 1
    assert n_checked == len(ROW_FORMS) * len(ROW_CONFIGS) * 4
    # rows == 0: zeros to every output, statistics included
    empty = torch.empty((0,), dtype=torch.int32, device=_dev())
    for form in ROW_FORMS:
        out = _row_call(form, pol, cri, d, idx=empty, n=SRC)
        torch.cuda.synchronize()
        assert all(float(x.abs().sum()) == 0.0 for x in out), form
    for x in (pol, cri):
        x.close()
    if norm is not None:
        norm.close()


@pytest.mark.parametrize("net", list(NETS))
def test_row_forms_skip_and_count_indices_out_of_range(net, envs):
    """rows = 130 of src_rows = 160 with -1 and src_rows at the tile positions 0, 63 and 64 (the sources lie between slack rows of
    NaN, so a read through such an index would show): the trailing statistic is exactly 3, every output is finite, and every gradient
    equals (torch.equal) the idx call with those entries replaced by a valid row that is arranged to be a ZERO ROW -- adv = 0, and
    ret = v_old = V (evaluate_dev's bits) for the value loss; for the critic target = V, V read as the output bias's gradient of a
    one-row call with target 0 and scale 1.  The zero row is checked to be one: alone, it gives all-zero gradients."""
    import torch
    D = NETS[net][0]
    pol, cri, norm = _nets(envs(D), net)
    rows, src, z = 130, 160, 77                                    # z: the source row made a zero row (not otherwise in idx)
    d = _row_data(pol, D, src)
    base = torch.arange(rows, dtype=torch.int32, device=_dev()) * 7 % src
    base[base == z] = z + 1
    _, v = pol.evaluate_dev(d["obs"], d["actions"])
    d["adv"][z] = 0.0
    d["ret"][z] = v[z]
    d["v_old"][z] = v[z]
    one = torch.tensor([z], dtype=torch.int32, device=_dev())
    probe, _ = cri.mse_grad_idx_dev(one, d["obs"], torch.zeros_like(d["target"]), scale=1.0)
    d["target"][z] = probe[-1]                                     # d L / d (output bias) = V - 0
    for bad_pair in ((-1, src), (src, -1), (-2 ** 31, 2 ** 31 - 1)):
        bad, ok = base.clone(), base.clone()
        for pos, val in zip((0, 63, 64), (bad_pair[0], bad_pair[1], bad_pair[0])):
            bad[pos] = val
            ok[pos] = z
        for form in ROW_FORMS:
            what = (net, form, bad_pair)
            alone = _row_call(form, pol, cri, d, idx=one, n=src)
            got = _clones(_row_call(form, pol, cri, d, idx=bad, n=src))
            want = _row_call(form, pol, cri, d, idx=ok, n=src)
            torch.cuda.synchronize()
            for x in _split(alone)[0][:2 if form != "ppo" else 1]:  # (grad, grad_value: not grad_log_std, which has the entropy term)
                assert float(x.abs().max()) == 0.0, (what, "the zero row is not one")
            (g, st), (wg, wst) = _split(got), _split(want)
            _same(g, wg, what)
            print("%s: skipped %g, rows %g" % (what, float(st[-1]), float(st[-2])))
            assert float(st[-1]) == 3.0 and float(wst[-1]) == 0.0 and float(st[-2]) == rows and bool(torch.isfinite(st).all()), (what, st)
    for x in (pol, cri):
        x.close()
    if norm is not None:
        norm.close()


def _seq_policy(env, case, inp):
    from gym_art_amd.policy import GRUPolicy
    return GRUPolicy(env, inp["gru"], inp["head"], case.act, case.out_tanh, log_std=LOG_STD, value=(inp["wv"], inp["bv"]))


SEQ_KEYS = ("obs", "actions", "done", "logp_old", "adv", "ret", "v_old")


def _seq_data(case, inp, T, S_src):
    """the case's first T steps of S_src columns (its 130, repeated) as contiguous tensors, each a view between one slack column"""
    import torch
    cols = np.arange(S_src) % R.SMAX
    d, keep = {}, []
    for k in SEQ_KEYS:
        a = np.ascontiguousarray(inp[k][:T, cols])
        per = int(np.prod(a.shape[2:]))
        big, d[k] = _slack(a.shape, per, dtype=torch.uint8 if k == "done" else None, fill=1 if k == "done" else float("nan"))
        d[k].copy_(_t(a))
        keep.append(big)
    big, d["h0"] = _slack((S_src, case.H), case.H)
    d["h0"].copy_(_t(inp["h0"][cols]))
    keep.append(big)
    d["_keep"] = keep
    return d


def _seq_call(pol, d, idx=None, **kw):
    a = (d["obs"], d["actions"], d["done"], d["h0"], d["logp_old"], d["adv"], d["ret"], d["v_old"])
    if idx is None:
        return pol.ppo_seq_grad_dev(*a, vclip=R.VCLIP, **COEF, **kw)
    return pol.ppo_seq_grad_idx_dev(idx, *a, vclip=R.VCLIP, **COEF, **kw)


def _seq_gathered(d, idx):
    j = idx.long()
    g = {k: d[k][:, j].contiguous() for k in SEQ_KEYS}
    g["h0"] = d["h0"][j].contiguous()
    return g


@pytest.mark.parametrize("name", ["gru16-tanh-vclip", "gru64x64x64-tanh-vclip"])
def test_sequence_form_is_the_contiguous_call_on_gathered_columns(name, envs):
    """every (T, S, S_src): a perm_dev prefix with a duplicate column and, next to each other, the columns 0 (no done), 2 (resets at
    t = 3 and 4) and 1 (a reset after t = 0) gives the parent call's bits on x[:, idx], h0[idx]; the trailing statistic is 0"""
    import torch
    from gym_art_amd.policy import perm_dev
    case, inp = R.case_inputs(name)
    pol = _seq_policy(envs(case.D), case, inp)
    for T, S, S_src, groups in SEQ_CONFIGS:
        d = _seq_data(case, inp, T, S_src)
        idx = perm_dev(S_src, 99, epoch=T, device=_dev())[:S].clone()
        if S == 1:
            idx[0] = 2
        else:
            idx[1:5] = torch.tensor([int(idx[0]), 0, 2, 1], dtype=torch.int32, device=_dev())[:min(4, S - 1)]
        what = (name, T, S, S_src, groups)
        with _groups(groups):
            want = _clones(_seq_call(pol, _seq_gathered(d, idx)))
            got = _seq_call(pol, d, idx=idx)
            again = _seq_call(pol, _seq_gathered(d, idx))
            torch.cuda.synchronize()
        _same(got[:3], want[:3], what)
        assert S < 63 or (float(want[0].abs().max()) > 0.0 and float(want[1].abs().max()) > 0.0), what     # (as for the row forms)
        assert got[3].shape == (7,) and torch.equal(got[3][:6], want[3]) and float(got[3][6]) == 0.0 and float(got[3][5]) == T * S, (what, got[3])
        _same(again, want, what)
    pol.close()


@pytest.mark.parametrize("name", ["gru16-tanh-vclip", "gru64x64x64-tanh-vclip"])
def test_sequence_form_skips_and_counts_indices_out_of_range(name, envs):
    """(T, S, S_src) = (5, 130, 140) with -1 and S_src at the tile positions 0, 63 and 64, the sources between slack columns of NaN:
    the trailing statistic is exactly 3 (once per sequence, not per step), every output is finite, and every gradient equals the idx
    call with those entries replaced by a ZERO COLUMN -- adv = 0 and ret = v_old = V (evaluate_seq_dev's bits) at every step -- which
    is checked to be one: alone, it gives all-zero weight and value-head gradients."""
    import torch
    case, inp = R.case_inputs(name)
    pol = _seq_policy(envs(case.D), case, inp)
    T, S, S_src, z = 5, 130, 140, 135
    d = _seq_data(case, inp, T, S_src)
    _, v = pol.evaluate_seq_dev(d["obs"], d["actions"], d["done"], d["h0"])
    d["adv"][:, z] = 0.0
    d["ret"][:, z] = v[:, z]
    d["v_old"][:, z] = v[:, z]
    base = torch.arange(S, dtype=torch.int32, device=_dev())
    one = torch.tensor([z], dtype=torch.int32, device=_dev())
    alone = _seq_call(pol, d, idx=one)
    torch.cuda.synchronize()
    assert float(alone[0].abs().max()) == 0.0 and float(alone[1].abs().max()) == 0.0, "the zero column is not one"
    for lo, hi in ((-1, S_src), (S_src, -1)):
        bad, ok = base.clone(), base.clone()
        for pos, val in zip((0, 63, 64), (lo, hi, lo)):
            bad[pos] = val
            ok[pos] = z
        got = _clones(_seq_call(pol, d, idx=bad))
        want = _seq_call(pol, d, idx=ok)
        torch.cuda.synchronize()
        _same(got[:3], want[:3], (name, lo, hi))
        st = got[3]
        print("%s (%d, %d): skipped %g, T S %g" % (name, lo, hi, float(st[6]), float(st[5])))
        assert float(st[6]) == 3.0 and float(want[3][6]) == 0.0 and float(st[5]) == T * S and bool(torch.isfinite(st).all()), st
    pol.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 65537])
def test_perm_dev_is_the_reference_bit_for_bit(n):
    """perm_dev == tests/perm_ref.py at two epochs, by value and through epoch_dev; the word after idx_out[n - 1] is untouched"""
    import torch
    from gym_art_amd.policy import perm_dev
    seed = 0x1234567890ABCDEF
    buf = torch.full((n + 1,), -7, dtype=torch.int32, device=_dev())
    word = torch.zeros((1,), dtype=torch.int64, device=_dev())
    for epoch in (0, 5, (1 << 40) + 3):
        want = torch.from_numpy(perm_ref(n, seed, epoch))
        got = perm_dev(n, seed, epoch=epoch, device=_dev())
        assert got.dtype == torch.int32 and got.shape == (n,) and torch.equal(got.cpu(), want), (n, epoch)
        word.fill_(epoch)
        out = perm_dev(n, seed, epoch=12345, epoch_dev=word, out=buf[:n])      # (the by-value epoch is ignored)
        assert out.data_ptr() == buf.data_ptr() and torch.equal(buf[:n].cpu(), want) and int(buf[n]) == -7, (n, epoch)
        assert int(word) == epoch                                  # the kernel writes idx_out only


def test_a_captured_epoch_of_shuffled_minibatches_replays_with_the_eager_bits(envs):
    """perm_dev(epoch_dev=), two minibatches of ppo_ac_grad_idx_dev + AdamDev.step(sync_log_std=False) with learn_log_std=False, then
    epoch_dev.add_(1) -- one linear chain, captured on a side stream after a warm-up call: three replays leave the weights, the value
    head, m, v and the step count bit-equal to the same sequence run eagerly three times from the same start, and the three epochs
    drew three different permutations"""
    import torch
    from gym_art_amd.policy import AdamDev, perm_dev
    net = "18-16-tanh"
    env = envs(18)
    src, mb, seed = 300, 130, 4242
    hp = dict(lr=1e-3, max_grad_norm=0.5, learn_log_std=False)

    def read(pol, opt):
        sd = opt.state_dict()
        w, b = pol.get_value_head()
        return [pol.get_packed(), w, np.float32(b), sd["m"], sd["v"]], (sd["step"], sd["skipped"])

    def epoch(pol, opt, d, perm, word, outs):
        perm_dev(src, seed, epoch_dev=word, out=perm)
        for k in range(2):
            pol.ppo_ac_grad_idx_dev(perm[k * mb:(k + 1) * mb], d["obs"], d["actions"], d["logp_old"], d["adv"], d["ret"], d["v_old"], vclip=0.2,
                                    grad=outs[0], grad_value=outs[1], grad_log_std=outs[2], stats=outs[3], **COEF)
            opt.step(outs[0], outs[1], outs[2], sync_log_std=False)
        word.add_(1)

    def make():
        pol, cri, _ = _nets(env, net)
        cri.close()
        d = _row_data(pol, 18, src)
        perm = torch.empty((src,), dtype=torch.int32, device=_dev())
        word = torch.full((1,), 10, dtype=torch.int64, device=_dev())
        outs = [torch.empty_like(x) for x in pol.ppo_ac_grad_idx_dev(perm_dev(src, 1, device=_dev())[:mb], d["obs"], d["actions"], d["logp_old"],
                                                                     d["adv"], d["ret"], d["v_old"], vclip=0.2, **COEF)]     # the warm-up
        return pol, AdamDev(pol, **hp), d, perm, word, outs

    eager = make()
    perms = []
    for _ in range(3):
        epoch(*eager)
        perms.append(eager[3].clone())
    torch.cuda.synchronize()
    want = read(eager[0], eager[1])
    assert want[1] == (6, 0) and int(eager[4]) == 13
    assert not torch.equal(perms[0], perms[1]) and not torch.equal(perms[1], perms[2])

    cap = make()
    start = read(cap[0], cap[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        epoch(*cap)
    assert cap[1].step_count == 0 and int(cap[4]) == 10            # capturing ran nothing
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap[3], perms[k]), k                    # every replay drew the eager epoch's permutation
    got = read(cap[0], cap[1])
    assert got[1] == (6, 0) and int(cap[4]) == 13
    for x, y in zip(got[0], want[0]):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert not np.array_equal(got[0][0], start[0][0])
    for x in (cap[1], cap[0], eager[1], eager[0]):
        x.close()


def test_refusals(envs):
    """each returns its code and its text under the new function's name, launches nothing, and the first call repeated afterwards
    gives its bits"""
    import torch
    from gym_art_amd import _lib
    lib = _lib.load()
    env = envs(18)
    pol, cri, _ = _nets(env, "18-16-tanh")
    d = _row_data(pol, 18)
    rows, src = 65, SRC
    idx = _idx_kinds(rows, src, 3)["perm"].contiguous()
    cs = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    first = _clones(_row_call("ac-vclip", pol, cri, d, idx=idx, n=src))
    g, gv, gls, st = _clones(first)
    o, a, lo, adv, ret, vo = (d[k] for k in ("obs", "actions", "logp_old", "adv", "ret", "v_old"))

    def ac(rows=rows, idx=idx, src=src, obs=o, v_old=vo, clip=0.2, vclip=0.2, scale=1.0, grad=g, stats=st):
        return lib.gaq_policy_grad_ppo_ac_idx_dev(pol.handle, rows, _lib.ptr(idx), src, _lib.ptr(obs), _lib.ptr(a), _lib.ptr(lo), _lib.ptr(adv),
                                                  _lib.ptr(ret), _lib.ptr(v_old), clip, vclip, 0.5, 0.01, scale, _lib.ptr(grad), _lib.ptr(gv),
                                                  _lib.ptr(gls), _lib.ptr(stats), cs)

    def err():
        return lib.gaq_last_error()
    name = b"gaq_policy_grad_ppo_ac_idx_dev: "
    assert ac(idx=None) == -1 and b"null" in err()
    assert ac(idx=idx.data_ptr() + 2) == -1 and name + b"pointers must be 4-byte aligned" in err()
    assert ac(src=0) == -1 and name + b"src_rows must be at least 1" in err()
    assert ac(src=-5) == -1 and name + b"src_rows must be at least 1" in err()
    assert ac(src=2 ** 31) == -1 and name + b"src_rows must not exceed" in err()
    assert ac(idx=g.data_ptr()) == -1 and name + b"an output overlaps an input" in err()      # idx over an output
    assert ac(rows=-1) == -1 and name + b"rows must not be negative" in err()                 # the parent's refusals, the new name
    assert ac(clip=1.0) == -1 and name + b"clip_eps" in err()
    assert ac(vclip=-0.1) == -1 and name + b"vclip" in err()
    assert ac(scale=float("nan")) == -1 and name + b"scale is NaN" in err()
    assert ac(v_old=None) == -1 and name + b"vclip > 0 needs v_old" in err()
    assert ac(obs=None) == -1 and b"null" in err()
    assert ac(stats=st.data_ptr() + 4) == -1 and b"stats_out: 8" in err()
    assert ac(grad=o.view(-1)[:g.numel()]) == -1 and b"overlap" in err()
    assert ac(rows=0, idx=None, src=0) == 0                          # nothing to do: no idx, no source needed; zeros
    torch.cuda.synchronize()
    assert float(g.abs().sum()) == 0.0 and float(st.abs().sum()) == 0.0
    pol.set_value_head(None)
    assert ac() == -4 and b"value head" in err()
    pol.set_value_head(*_value_head())
    pol.set_log_std(None)
    assert ac() == -4 and b"no log_std set" in err()
    pol.set_log_std(LOG_STD)
    # the other three: null and misaligned idx, src_rows, the name in the text
    g2, gls2, st2 = (x.clone() for x in pol.ppo_grad_idx_dev(idx, o, a, lo, adv, clip=0.2))

    def ppo(idx=idx, src=src, rows=rows):
        return lib.gaq_policy_grad_ppo_idx_dev(pol.handle, rows, _lib.ptr(idx), src, _lib.ptr(o), _lib.ptr(a), _lib.ptr(lo), _lib.ptr(adv), 0.2,
                                               1.0, _lib.ptr(g2), _lib.ptr(gls2), _lib.ptr(st2), cs)
    gc, stc = (x.clone() for x in cri.mse_grad_idx_dev(idx, o, d["target"]))

    def mse(idx=idx, src=src, rows=rows):
        return lib.gaq_critic_grad_mse_idx_dev(cri.handle, rows, _lib.ptr(idx), src, _lib.ptr(o), _lib.ptr(d["target"]), 1.0, _lib.ptr(gc),
                                               _lib.ptr(stc), cs)
    for fn, nm in ((ppo, b"gaq_policy_grad_ppo_idx_dev: "), (mse, b"gaq_critic_grad_mse_idx_dev: ")):
        assert fn(idx=None) == -1 and b"null" in err()
        assert fn(idx=idx.data_ptr() + 1) == -1 and nm + b"pointers must be 4-byte aligned" in err()
        assert fn(src=0) == -1 and nm + b"src_rows must be at least 1" in err()
        assert fn(src=2 ** 31) == -1 and nm + b"src_rows must not exceed" in err()
        assert fn(rows=-1) == -1 and nm + b"rows must not be negative" in err()
    assert ppo(idx=g2.data_ptr()) == -1 and b"overlap" in err()
    # the Python checks come before the library
    for bad, text in ((idx.long(), "torch.int32"), (idx.cpu(), "device"), (idx.view(1, -1), "shape \\[rows\\]"),
                      (torch.stack([idx, idx], 1)[:, 0], "contiguous"), (list(range(4)), "shape \\[rows\\]")):
        with pytest.raises(ValueError, match=text):
            pol.ppo_ac_grad_idx_dev(bad, o, a, lo, adv, ret, vo, vclip=0.2)
        with pytest.raises(ValueError, match=text):
            cri.mse_grad_idx_dev(bad, o, d["target"])
    with pytest.raises(ValueError, match="v_old"):
        pol.ppo_ac_grad_idx_dev(idx, o, a, lo, adv, ret, None, vclip=0.2)
    # the sequence form
    case, inp = R.case_inputs("gru16-tanh-vclip")
    gp = _seq_policy(env, case, inp)
    sd = _seq_data(case, inp, 2, 65)
    sidx = torch.arange(63, dtype=torch.int32, device=_dev())
    sfirst = _clones(_seq_call(gp, sd, idx=sidx))
    sg, sgv, sgls, sst = _clones(sfirst)

    def seq(idx=sidx, S=63, S_src=65, T=2):
        return lib.gaq_policy_grad_ppo_seq_idx_dev(gp.handle, T, S, _lib.ptr(idx), S_src, *[_lib.ptr(sd[k]) for k in
                                                   ("obs", "actions", "done", "h0", "logp_old", "adv", "ret", "v_old")], 0.2, 0.2, 0.5, 0.01,
                                                   1.0, _lib.ptr(sg), _lib.ptr(sgv), _lib.ptr(sgls), _lib.ptr(sst), cs)
    nm = b"gaq_policy_grad_ppo_seq_idx_dev: "
    assert seq(idx=None) == -1 and b"null" in err()
    assert seq(idx=sidx.data_ptr() + 2) == -1 and nm + b"pointers must be 4-byte aligned" in err()
    assert seq(S_src=0) == -1 and nm + b"S_src must be at least 1" in err()
    assert seq(S_src=2 ** 31) == -1 and nm + b"S_src must not exceed" in err()
    assert seq(idx=sg.data_ptr()) == -1 and nm + b"an output overlaps an input" in err()
    assert seq(T=0) == -1 and nm + b"T must be at least 1" in err()
    assert seq(S=-1) == -1 and nm + b"S must not be negative" in err()
    assert lib.gaq_policy_grad_ppo_seq_idx_dev(pol.handle, 2, 63, _lib.ptr(sidx), 65, *[None] * 8, 0.2, 0.2, 0.5, 0.01, 1.0, *[None] * 5) == -1
    assert b"recurrent" in err()                                   # a feed-forward policy: policy_grad_seq_view's text
    with pytest.raises(ValueError, match="torch.int32"):
        gp.ppo_seq_grad_idx_dev(sidx.long(), *[sd[k] for k in ("obs", "actions", "done", "h0", "logp_old", "adv", "ret", "v_old")], vclip=0.2)
    # nothing was launched, nothing is broken: the first calls repeated give their bits
    torch.cuda.synchronize()
    _same(_row_call("ac-vclip", pol, cri, d, idx=idx, n=src), first, "row form after the refusals")
    _same(_seq_call(gp, sd, idx=sidx), sfirst, "sequence form after the refusals")
    for x in (gp, pol, cri):
        x.close()


def _value_head():
    """_nets' value head again"""
    rng = np.random.RandomState(5)
    return (rng.randn(16) / np.sqrt(16)).astype(np.float32), np.float32(0.1)
