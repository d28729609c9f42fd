"""The optimiser's reference (tests/optim_ref.py) against torch.optim.Adam / AdamW with clip_grad_norm_ in fp64, the conditions its
cases meet, the committed torch fp32 table, the state-layout helpers and the refusals that need no device -- no GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P
from tests import optim_ref as R

IDS = [c.name for c in R.CASES]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_reference_agrees_with_torch_fp64(case):
    """theta, m and v of every group after each of the ten steps, and every step's norm and coef: <= 1e-12 relative"""
    import torch
    errs, scal = R.torch_errors(case, torch.float64, at=tuple(range(1, R.STEPS + 1)))
    worst = max(max(e) for k in errs for e in errs[k].values())
    print("%s: torch fp64 differs by %.3g (theta, m, v), %.3g (norm, coef)" % (case.name, worst, scal))
    assert worst <= 1e-12 and scal <= 1e-12


def test_the_case_list_is_the_stated_one():
    sizes = {c.name: c.sizes for c in R.CASES}
    assert sizes["mlp16-head-logstd"] == (372, 17, 4) and sizes["mlp128x128x128"][0] == 35972 and sizes["critic16"] == (321, 0, 0)
    assert [c.kind for c in R.CASES] == ["mlp", "mlp", "mlp", "mlp", "critic", "gru", "gru", "lstm"] and R.CASES[3].engine == "valu"
    assert R.CASES[3].D == 19 and R.CASES[5].sizes[1] == 0 and R.CASES[6].sizes[1] == 65 and R.CASES[7].widths == [16]
    assert (372 + 17 + 4) % 64 != 0 and 372 % 64 != 0 and (372 + 17) % 64 != 0        # three groups that end inside a wave
    assert any(sum(c.sizes) > 2048 and sum(c.sizes) % 2048 for c in R.CASES)          # more than one chunk, the last one partial
    assert set(R.BASELINE) == set(sizes) and all(set(R.BASELINE[n]) == set(R.AT) == {1, 2, R.STEPS} for n in sizes)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_inputs_meet_the_conditions(case):
    """conditions on the inputs, not measurements: magnitudes over [1e-6, 10], about 5 % exact zeros, gradients that change from step
    to step, and both branches of the clip reached -- one case far above max_grad_norm at every step, one far below"""
    g = [np.concatenate(R.gradients(case, k)) for k in range(R.STEPS)]
    for x in g:
        nz = np.abs(x[x != 0])
        assert 1e-6 * 0.999 <= nz.min() and nz.max() <= 10.0 and nz.min() < 1e-4 and nz.max() > 1.0
        assert 0.01 <= float((x == 0).mean()) <= 0.1
    assert not np.array_equal(g[0], g[1])
    stats = [r[3] for r in R.reference(case.name)]
    if case.clip == "above":
        assert all(s[0] > 20.0 * case.hp["max_grad_norm"] and s[1] < 0.05 for s in stats)
    if case.clip == "below":
        assert all(s[0] < 0.05 * case.hp["max_grad_norm"] and s[1] == 1.0 for s in stats)
    assert [s[2] for s in stats] == list(range(1, R.STEPS + 1)) and not any(s[3] for s in stats)


def test_both_branches_of_the_clip_are_among_the_cases():
    assert sorted(c.clip for c in R.CASES if c.clip) == ["above", "below"]
    assert any(c.hp["weight_decay"] > 0 and c.log_std for c in R.CASES) and any(c.hp["max_grad_norm"] is None for c in R.CASES)


def test_the_skip_rule_of_the_reference():
    case = R.BY_NAME["mlp16-head-logstd"]
    for bad in (np.nan, np.inf, -np.inf):
        st = R.State(R.theta0(case))
        R.step(st, R.gradients(case, 0), **case.hp)
        before = [x.copy() for x in st.theta + st.m + st.v]
        g = [x.copy() for x in R.gradients(case, 1)]
        g[1][3] = bad
        stats = R.step(st, g, **case.hp)
        assert stats[1:] == (0.0, 1.0, 1.0) and not np.isfinite(stats[0]) and (st.t, st.skipped) == (1, 1)
        assert all(np.array_equal(a, b) for a, b in zip(before, st.theta + st.m + st.v))


def test_weight_decay_never_touches_log_std():
    case = R.BY_NAME["valu64x64-d19"]
    a, b = R.State(R.theta0(case)), R.State(R.theta0(case))
    g = R.gradients(case, 0)
    R.step(a, g, **case.hp)
    R.step(b, g, **dict(case.hp, weight_decay=0.0))
    assert np.array_equal(a.theta[2], b.theta[2]) and not np.array_equal(a.theta[0], b.theta[0])


def test_one_committed_baseline_is_what_torch_fp32_gives_here():
    """as tests/test_policy_grad_ac_cpu.py holds its table: maxima over many elements within a factor of 8 of the committed numbers"""
    import torch
    case = R.BY_NAME["mlp128x128x128"]
    got, _ = R.torch_errors(case, torch.float32)
    want = R.BASELINE[case.name]
    print("torch fp32: %s, committed %s" % (got, want))
    for k in R.AT:
        for what in ("theta", "m", "v"):
            for g, w in zip(got[k][what][:2], want[k][what][:2]):
                assert w / 8.0 <= g <= w * 8.0, (k, what, got, want)
    assert R.bound(case.name, 1, "theta", 0) == max(8.0 * want[1]["theta"][0], 2.0 ** -24)
    assert R.bound("lstm16", 1, "m", 0) == 8.0 * R.BASELINE["lstm16"][1]["m"][0] > 2.0 ** -24
    assert R.bound("mlp48x80x32", R.STEPS, "theta", 2) == R.STEPS * 2.0 ** -24     # the floor: one rounding per step


def test_state_count_and_layout_helpers():
    for case in R.CASES:
        nw, nh, nl = case.sizes
        groups, total = P.optim_groups(nw, case.widths[-1] if case.head else None, case.log_std)
        assert total == nw + nh + nl
        assert groups[0] == ("weights", 0, nw) and [g[0] for g in groups] == [n for n, s in zip(R.GROUPS, case.sizes) if s]
        for (_, off, n), (_, off2, _) in zip(groups, groups[1:]):
            assert off + n == off2                                               # concatenated, no gaps
        assert groups[-1][1] + groups[-1][2] == total
    assert P.optim_groups(372, 16, True) == ([("weights", 0, 372), ("value_head", 372, 17), ("log_std", 389, 4)], 393)
    # the cases' weight counts are the library's
    lib = _lib.load()
    d = P._fill_desc(P._DescEx(), 18, [128, 128, 128], "tanh", out_tanh=0, engine=P.ENGINES["mfma"])
    assert lib.gaq_policy_weight_count_ex(C.byref(d)) == R.BY_NAME["mlp128x128x128"].weight_count
    d = P._fill_desc(P._DescRnn(), 18, [64, 64, 64], "tanh", out_tanh=0, engine=P.ENGINES["mfma"], cell=P.CELL_GRU)
    assert lib.gaq_policy_weight_count_rnn(C.byref(d)) == R.BY_NAME["gru64x64x64-head"].weight_count
    d = P._fill_desc(P._DescRnn(), 18, [16], "tanh", out_tanh=0, engine=P.ENGINES["mfma"], cell=P.CELL_LSTM)
    assert lib.gaq_policy_weight_count_rnn(C.byref(d)) == R.BY_NAME["lstm16"].weight_count
    d = P._fill_desc(P._CriticDesc(), 18, [16], "tanh")
    assert lib.gaq_critic_weight_count(C.byref(d)) == 321
    d = P.optim_desc(1e-3, (0.8, 0.99), 1e-6, 0.01, None, False)
    assert (d.struct_size, d.flags, d.lr, d.beta1, d.beta2, d.eps, d.weight_decay, d.max_grad_norm) == (56, 0, 1e-3, 0.8, 0.99, 1e-6, 0.01, 0.0)
    assert P.optim_desc().flags == P.OPTIM_STEP_LOG_STD == 1


def test_the_header_and_the_binding_agree_on_the_description():
    import subprocess
    import tempfile
    root = os.path.dirname(_lib._HERE)
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "gaq.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(gaq_optim_desc),'
            ' offsetof(gaq_optim_desc, lr), offsetof(gaq_optim_desc, max_grad_norm), (size_t)GAQ_OPTIM_STEP_LOG_STD);return 0;}')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", exe, src])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out == [C.sizeof(P._OptimDesc), P._OptimDesc.lr.offset, P._OptimDesc.max_grad_norm.offset, P.OPTIM_STEP_LOG_STD]


def test_unpack_lstm_weights_inverts_pack_lstm_weights():
    rng = np.random.RandomState(3)
    H, I = 16, 18
    lstm = (rng.randn(4 * H, I), rng.randn(4 * H, H), rng.randn(4 * H), rng.randn(4 * H))
    head = [(rng.randn(32, H), rng.randn(32)), (rng.randn(4, 32), rng.randn(4))]
    packed = P.pack_lstm_weights(lstm, head)
    cell, layers = P.unpack_lstm_weights(packed, I, H, [32])
    for a, b in zip(cell, lstm):
        assert np.array_equal(a, b.astype(np.float32))
    for (W, b), (W2, b2) in zip(layers, head):
        assert np.array_equal(W, W2.astype(np.float32)) and np.array_equal(b, b2.astype(np.float32))
    with pytest.raises(ValueError, match="LSTM"):
        P.unpack_lstm_weights(packed[:-1], I, H, [32])
    gru = tuple(x[:3 * H] for x in lstm)
    cell, _ = P.unpack_gru_weights(P.pack_gru_weights(gru, head), I, H, [32])            # the GRU form is what it was
    assert np.array_equal(cell[1], gru[1].astype(np.float32))
    with pytest.raises(ValueError, match=r"a GRU\(18, 16\) with head \[32, 4\] packs into"):
        P.unpack_gru_weights(packed, I, H, [32])


def test_refusals_that_need_no_device():
    """null pointers, a wrong struct_size and every hyper-parameter out of range are refused before a handle is looked at"""
    lib = _lib.load()
    out = C.c_void_p()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))       # never dereferenced: the description is checked first
    good = P.optim_desc()
    for create in (lib.gaq_optim_create_policy, lib.gaq_optim_create_critic):
        assert create(None, C.byref(good), C.byref(out)) == -1 and b"null" in lib.gaq_last_error()
        assert create(fake, None, C.byref(out)) == -1 and b"null" in lib.gaq_last_error()
        assert create(fake, C.byref(good), None) == -1 and b"null" in lib.gaq_last_error()
        bad = P.optim_desc()
        bad.struct_size -= 8
        assert create(fake, C.byref(bad), C.byref(out)) == -1 and b"struct_size" in lib.gaq_last_error()
        nan = float("nan")
        for kw, word in ((dict(betas=(1.0, 0.999)), b"beta1"), (dict(betas=(-0.1, 0.999)), b"beta1"), (dict(betas=(0.9, 1.0)), b"beta2"),
                         (dict(betas=(0.9, nan)), b"beta2"), (dict(eps=0.0), b"eps"), (dict(eps=-1e-8), b"eps"), (dict(eps=nan), b"eps"),
                         (dict(lr=-1e-3), b"lr"), (dict(lr=nan), b"lr"), (dict(weight_decay=-0.1), b"weight_decay"),
                         (dict(weight_decay=nan), b"weight_decay"), (dict(max_grad_norm=-1.0), b"max_grad_norm"),
                         (dict(max_grad_norm=nan), b"max_grad_norm")):
            bad = P.optim_desc(**kw)
            assert create(fake, C.byref(bad), C.byref(out)) == -1 and word in lib.gaq_last_error(), kw
        bad = P.optim_desc()
        bad.flags = 2
        assert create(fake, C.byref(bad), C.byref(out)) == -1 and b"flags" in lib.gaq_last_error()
        assert out.value is None
    assert lib.gaq_optim_step_dev(None, None, None, None, None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_optim_set_lr_dev(None, 1e-3, None) == -1 and lib.gaq_optim_sync_log_std(None, None) == -1
    assert lib.gaq_optim_state_count(None) == -1 and lib.gaq_optim_get_log_std(None, None) == -1
    assert lib.gaq_optim_get_state(None, None, None, None, None) == -1 and lib.gaq_optim_set_state(None, None, None, None, None) == -1
    assert lib.gaq_policy_get_weights(None, None) == -1 and lib.gaq_policy_get_value_head(None, None) == -1
    assert lib.gaq_critic_get_weights(None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_optim_destroy(None) == 0 and lib.gaq_abi_version() == 5


def test_python_surface():
    def sig(f):
        return str(inspect.signature(f))
    assert sig(P.AdamDev.__init__) == ("(self, handle, lr=0.0003, betas=(0.9, 0.999), eps=1e-08, weight_decay=0.0, max_grad_norm=None, "
                                       "learn_log_std=True)")
    assert sig(P.AdamDev.step) == "(self, grad, grad_value=None, grad_log_std=None, stats=None, stream=None, sync_log_std=True)"
    assert sig(P.AdamDev.set_lr) == "(self, lr, stream=None)" and sig(P.AdamDev.sync_log_std) == "(self, stream=None)"
    for name in ("state_dict", "load_state_dict", "close"):
        assert getattr(P.AdamDev, name).__doc__ or name == "close"
    for cls in (P.MLPPolicy, P.GRUPolicy, P.LSTMPolicy, P.MLPCritic):
        assert cls.get_weights.__doc__ and callable(cls.unpack)
    for cls in (P.MLPPolicy, P.GRUPolicy, P.LSTMPolicy):
        assert cls.get_value_head.__doc__
    with pytest.raises(ValueError, match="AdamDev steps"):
        P.AdamDev(object())
