"""Host side of the LSTM policy engine (gaq_policy_desc_rnn with GAQ_POLICY_CELL_LSTM, gym_art_amd.policy.LSTMPolicy): the weight count
against pack_lstm_weights, the packed layout element by element, the refusals of the _rnn entry points, the layer checks of the Python
side, the LDS formula at the largest accepted shape, and the fp64 reference the GPU tests use against torch.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd.policy import (CELL_LSTM, LSTMPolicy, _DescEx, _DescRnn, check_lstm_layers, pack_lstm_weights, pack_weights, torch_gru,
                                torch_lstm)
from tests.gru_util import _desc_rnn, _gru, _head
from tests.lstm_util import _desc_lstm, _lstm, lstm_step64, reference_rollout, torch_head32, torch_step32

LDS_MAX = 160 * 1024             # gaq_policy.hip kLdsMax: the CU's LDS


def lstm_lds(D, H, head=(), value_parts=True):
    """the LSTM launch's LDS as gaq.h / DESIGN.md state it: the GRU engine's, c takes no region"""
    return 1024 + (1024 if value_parts else 0) + 256 * (((D + 3) & ~3) + H + max((H,) + tuple(head)))


def test_cell_constant_and_import():
    assert CELL_LSTM == 3 and LSTMPolicy.engine == "mfma"
    assert hasattr(_lib.load(), "gaq_policy_set_cell_dev")


@pytest.mark.parametrize("D,H,head", [(18, 16, ()), (18, 64, ()), (18, 128, (64,)), (18, 256, (256, 128)), (36, 128, ()),
                                      (108, 256, (16,)), (17, 48, (32,)), (19, 240, (64,))])
def test_weight_count_lstm_matches_the_packing(D, H, head):
    lib = _lib.load()
    n = lib.gaq_policy_weight_count_rnn(C.byref(_desc_lstm([H] + list(head), in_dim=D)))
    packed = pack_lstm_weights(_lstm(H, D), _head(H, head))
    assert n == packed.size
    assert n == 4 * H * (D + H) + 8 * H + pack_weights(_head(H, head)).size
    # the GRU's count is what it was
    assert lib.gaq_policy_weight_count_rnn(C.byref(_desc_rnn([H] + list(head), in_dim=D))) \
        == 3 * H * (D + H) + 6 * H + pack_weights(_head(H, head)).size


def test_packed_lstm_layout():
    """W_ih' [4H/16][I][16] with W_ih'[c][k][j] = W_ih[16c + j][k], then b_ih, then W_hh' likewise, then b_hh, then the head: every
    element"""
    H, D = 32, 19
    lstm, head = _lstm(H, D), _head(H, (16,))
    p = pack_lstm_weights(lstm, head)
    W_ih, W_hh, b_ih, b_hh = lstm
    wi = p[:4 * H * D].reshape(4 * H // 16, D, 16)
    for c in range(4 * H // 16):
        assert np.array_equal(wi[c], W_ih[16 * c:16 * c + 16].T)
    assert np.array_equal(p[4 * H * D:4 * H * D + 4 * H], b_ih)
    o = 4 * H * D + 4 * H
    wh = p[o:o + 4 * H * H].reshape(4 * H // 16, H, 16)
    for c in range(4 * H // 16):
        assert np.array_equal(wh[c], W_hh[16 * c:16 * c + 16].T)
    assert np.array_equal(wh[7, 31, 15], W_hh[16 * 7 + 15, 31])       # gate o, unit 15 of chunk 7 - 3 * 2 = 1
    assert np.array_equal(p[o + 4 * H * H:o + 4 * H * H + 4 * H], b_hh)
    assert np.array_equal(p[o + 4 * H * H + 4 * H:], pack_weights(head))


def test_weight_count_lstm_refusals():
    lib = _lib.load()

    def count(d):
        return lib.gaq_policy_weight_count_rnn(C.byref(d))
    assert count(_desc_lstm([64])) == 4 * 64 * (18 + 64) + 8 * 64 + 4 * 64 + 4
    assert count(_desc_lstm([64], cell=2)) == -1         # unassigned, as the GRU engine's release left it
    assert count(_desc_lstm([64], cell=-1)) == -1
    assert count(_desc_lstm([64], cell=0)) == -1
    assert count(_desc_lstm([64], cell=4)) == -1
    for engine in (0, 2, 3):                             # VALU, unassigned, bf16
        assert count(_desc_lstm([64], engine=engine)) == -1
    for widths in ([24], [272], [0], [64, 24], [64, 272]):
        assert count(_desc_lstm(widths)) == -1
    d = _desc_lstm([64])
    d.struct_size = C.sizeof(_DescEx)
    assert count(d) == -1
    d = _desc_lstm([64])
    d.n_hidden = 0
    assert count(d) == -1
    d = _desc_lstm([64, 64, 64])
    d.n_hidden = 4
    assert count(d) == -1
    d = _desc_lstm([64])
    d.in_dim = 0
    assert count(d) == -1


def test_null_arguments():
    lib = _lib.load()
    assert lib.gaq_policy_set_cell_dev(None, None) == -1
    assert lib.gaq_policy_set_cell_dev(None, C.c_void_p(64)) == -1
    h = C.c_void_p()
    assert lib.gaq_policy_create_rnn(None, C.byref(_desc_lstm([64])), C.byref(h)) == -1
    assert lib.gaq_policy_create_rnn(None, C.byref(_desc_lstm([64])), None) == -1
    assert C.sizeof(_DescRnn) == C.sizeof(_DescEx) + 4   # gaq_policy_desc_rnn is unchanged


def test_lds_formula_at_the_largest_shape():
    """H = 256 on 108 inputs with the value parts: 2 KiB + 256 B x (108 + 256 + 256) = 157 KiB of the 160 KiB; a third block of H rows
    for c would not fit"""
    assert lstm_lds(108, 256) == 157 * 1024 <= LDS_MAX
    assert lstm_lds(108, 256, (64,)) == 157 * 1024
    assert lstm_lds(108, 256, value_parts=False) == 156 * 1024
    assert lstm_lds(108, 256) + 256 * 256 > LDS_MAX
    assert lstm_lds(18, 128, value_parts=False) == 1024 + 256 * (20 + 128 + 128)


def test_check_lstm_layers():
    H = 64
    check_lstm_layers(_lstm(H), _head(H), 18, "tanh")
    check_lstm_layers(_lstm(H), _head(H, (256, 16)), 18, "relu")
    with pytest.raises(ValueError, match="multiple of 16"):
        check_lstm_layers(_lstm(24), _head(24), 18, "tanh")
    with pytest.raises(ValueError, match="multiple of 16"):
        check_lstm_layers(_lstm(272), _head(272), 18, "tanh")
    with pytest.raises(ValueError, match="4H"):
        check_lstm_layers(_gru(H), _head(H), 18, "tanh")              # 3H rows: a GRU's weights
    with pytest.raises(ValueError, match="obs_dim"):
        check_lstm_layers(_lstm(H, D=17), _head(H), 18, "tanh")
    with pytest.raises(ValueError, match="W_hh"):
        g = _lstm(H)
        check_lstm_layers((g[0], g[1][:, :32], g[2], g[3]), _head(H), 18, "tanh")
    with pytest.raises(ValueError, match="b_ih and b_hh"):
        g = _lstm(H)
        check_lstm_layers((g[0], g[1], g[2][:-1], g[3]), _head(H), 18, "tanh")
    with pytest.raises(ValueError, match="0 to 2 hidden layers"):
        check_lstm_layers(_lstm(H), _head(H, (16, 16, 16)), 18, "tanh")
    with pytest.raises(ValueError, match="takes"):
        check_lstm_layers(_lstm(H), _head(32), 18, "tanh")
    with pytest.raises(ValueError, match="4 outputs"):
        check_lstm_layers(_lstm(H), [(np.zeros((3, H), np.float32), np.zeros(3, np.float32))], 18, "tanh")
    with pytest.raises(ValueError, match="activation"):
        check_lstm_layers(_lstm(H), _head(H), 18, "elu")
    with pytest.raises(ValueError, match="W_ih, W_hh, b_ih, b_hh"):
        check_lstm_layers(_lstm(H)[:3], _head(H), 18, "tanh")


def test_torch_lstm():
    import torch
    nn = torch.nn
    torch.manual_seed(0)
    cell = nn.LSTMCell(18, 32)
    W_ih, W_hh, b_ih, b_hh = torch_lstm(cell)
    assert W_ih.shape == (128, 18) and W_hh.shape == (128, 32)
    assert np.array_equal(W_ih, cell.weight_ih.detach().numpy()) and np.array_equal(b_hh, cell.bias_hh.detach().numpy())
    m = nn.LSTM(18, 32, num_layers=1)
    assert np.array_equal(torch_lstm(m)[1], m.weight_hh_l0.detach().numpy())
    nb = torch_lstm(nn.LSTMCell(18, 32, bias=False))
    assert nb[2].shape == (128,) and not nb[2].any() and not nb[3].any()
    nb = torch_lstm(nn.LSTM(18, 32, bias=False))
    assert nb[2].shape == (128,) and not nb[2].any() and not nb[3].any()
    with pytest.raises(ValueError, match="num_layers"):
        torch_lstm(nn.LSTM(18, 32, num_layers=2))
    with pytest.raises(ValueError, match="bidirectional"):
        torch_lstm(nn.LSTM(18, 32, bidirectional=True))
    with pytest.raises(ValueError, match="proj_size"):
        torch_lstm(nn.LSTM(18, 32, proj_size=8))
    with pytest.raises(ValueError, match="LSTMCell or nn.LSTM, got GRUCell"):
        torch_lstm(nn.GRUCell(18, 32))
    with pytest.raises(ValueError, match="got GRU"):
        torch_lstm(nn.GRU(18, 32))
    with pytest.raises(ValueError, match="GRUCell or nn.GRU, got LSTMCell"):   # and torch_gru keeps refusing an LSTM
        torch_gru(cell)


def test_reference_step_matches_torch_lstmcell():
    """in double to 1e-12: a wrong gate order does not pass"""
    import torch
    torch.manual_seed(1)
    cell = torch.nn.LSTMCell(18, 48).double()
    x, h, c = (torch.randn(5, k, dtype=torch.float64) for k in (18, 48, 48))
    lstm = tuple(t.detach().numpy() for t in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh))
    hn, cn = cell(x, (h, c))
    rh, rc = lstm_step64(lstm, x.numpy(), h.numpy(), c.numpy())
    assert np.allclose(rh, hn.detach().numpy(), rtol=0, atol=1e-12) and np.allclose(rc, cn.detach().numpy(), rtol=0, atol=1e-12)
    # teeth: the GRU-style order (or any swap of two gates) is off by far more
    W_ih, W_hh, b_ih, b_hh = lstm
    perm = np.concatenate([np.arange(48, 96), np.arange(0, 48), np.arange(96, 192)])
    sh, _ = lstm_step64((W_ih[perm], W_hh[perm], b_ih[perm], b_hh[perm]), x.numpy(), h.numpy(), c.numpy())
    assert np.max(np.abs(sh - rh)) > 1e-3


def test_reference_rollout_resets_both_states_and_the_yardstick_follows_it():
    """h and c are zeroed where done is set; values have T + 1 rows; the fp32 torch cell (the GPU tests' yardstick) stays within
    fp32 rounding of the fp64 rollout"""
    rng = np.random.RandomState(0)
    N, H, D, T = 9, 32, 18, 6
    lstm, layers = _lstm(H, D, scale=0.15), _head(H, (16,))
    value = ((rng.randn(16) / 4).astype(np.float32), np.float32(0.1))
    obs0, obs = rng.randn(N, D).astype(np.float32), rng.randn(T, N, D).astype(np.float32)
    done = np.zeros((T, N), np.uint8)
    done[2, :4] = 1
    done[T - 1, 5:] = 1
    tt = rng.randn(T, N, D).astype(np.float32)
    h0, c0 = rng.randn(N, H).astype(np.float32), rng.randn(N, H).astype(np.float32)
    ref = reference_rollout(lstm, layers, "tanh", True, obs0, obs, done, h0, c0, value, tt)
    assert ref["a"].shape == (T, N, 4) and ref["v"].shape == (T + 1, N) and ref["tv"].shape == (T, N)
    assert not ref["h"][5:].any() and not ref["c"][5:].any() and ref["h"][:5].all() and ref["c"][:5].all()
    assert np.array_equal(ref["tv"] != 0, done != 0)
    y = reference_rollout(lstm, layers, "tanh", True, obs0, obs, done, h0, c0, value, tt, step=torch_step32(lstm),
                          head=torch_head32(layers, "tanh", True, value))
    for key in ("a", "h", "c", "v", "tv"):
        err = np.max(np.abs(y[key] - ref[key]))
        assert 0 < err < 1e-5, (key, err)


def test_recurrent_policies_keep_their_public_signatures_and_names():
    """GRUPolicy and LSTMPolicy share one base: what a caller sees of either -- the parameters of its public members and the helper
    names importable from gym_art_amd.policy -- is what it was while each class was written out"""
    import inspect

    import gym_art_amd.policy as pol
    shared = {"from_torch": "(cell, head, env, log_std=None, value=None)", "reset_hidden": "(self, mask=None)",
              "set_log_std": "(self, log_std=None)", "set_value_head": "(self, w=None, b=None)"}
    want = {"GRUPolicy": dict(shared, __init__="(self, env, gru, head_layers, hidden_act='tanh', out_tanh=False, log_std=None, value=None)",
                              set_hidden="(self, h)"),
            "LSTMPolicy": dict(shared, __init__="(self, env, lstm, head_layers, hidden_act='tanh', out_tanh=False, log_std=None, value=None)",
                               set_hidden="(self, h, c)")}
    for cls, members in want.items():
        assert len(members) == 6
        for name, sig in members.items():
            assert str(inspect.signature(getattr(getattr(pol, cls), name))) == sig, (cls, name)
    for name in ("check_lstm_layers", "check_gru_layers", "torch_lstm", "torch_gru", "pack_lstm_weights", "pack_gru_weights"):
        assert callable(getattr(pol, name)), name
