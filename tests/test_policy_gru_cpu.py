"""Host side of the GRU policy engine (gaq_policy_desc_rnn, gym_art_amd.policy.GRUPolicy): the weight count against pack_gru_weights,
the refusals of the _rnn entry points, the layer checks of the Python side, and the fp64 reference the GPU tests use.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd.policy import _DescEx, _DescRnn, check_gru_layers, pack_gru_weights, pack_weights, torch_gru, torch_head
from tests.gru_util import _desc_rnn, _gru, _head, gru_step64
from tests.policy_util import _desc_ex


def test_desc_rnn_is_desc_ex_plus_cell():
    assert C.sizeof(_DescRnn) == C.sizeof(_DescEx) + 4
    assert _DescRnn.cell.offset == C.sizeof(_DescEx)


@pytest.mark.parametrize("D,H,head", [(18, 16, ()), (18, 64, ()), (18, 128, (64,)), (18, 256, (256, 128)), (36, 128, ()),
                                      (36, 256, (16,)), (17, 48, (32,))])
def test_weight_count_rnn_matches_the_packing(D, H, head):
    lib = _lib.load()
    n = lib.gaq_policy_weight_count_rnn(C.byref(_desc_rnn([H] + list(head), in_dim=D)))
    packed = pack_gru_weights(_gru(H, D), _head(H, head))
    assert n == packed.size
    assert n == 3 * H * (D + H) + 6 * H + pack_weights(_head(H, head)).size


def test_packed_gru_layout():
    """W_ih' [3H/16][I][16] with W_ih'[c][k][j] = W_ih[16c + j][k], then b_ih, then W_hh' likewise, then b_hh, then the head"""
    H, D = 32, 18
    gru, head = _gru(H, D), _head(H, (16,))
    p = pack_gru_weights(gru, head)
    W_ih, W_hh, b_ih, b_hh = gru
    wi = p[:3 * H * D].reshape(3 * H // 16, D, 16)
    assert np.array_equal(wi[5, 7, 3], W_ih[16 * 5 + 3, 7])
    assert np.array_equal(p[3 * H * D:3 * H * D + 3 * H], b_ih)
    o = 3 * H * D + 3 * H
    wh = p[o:o + 3 * H * H].reshape(3 * H // 16, H, 16)
    assert np.array_equal(wh[4, 31, 15], W_hh[16 * 4 + 15, 31])
    assert np.array_equal(p[o + 3 * H * H:o + 3 * H * H + 3 * H], b_hh)
    assert np.array_equal(p[o + 3 * H * H + 3 * H:], pack_weights(head))


def test_weight_count_rnn_refusals():
    lib = _lib.load()

    def count(d):
        return lib.gaq_policy_weight_count_rnn(C.byref(d))
    assert count(_desc_rnn([64])) > 0
    d = _desc_rnn([64])
    d.struct_size = C.sizeof(_DescEx)
    assert count(d) == -1
    d.struct_size = C.sizeof(_DescRnn) + 4
    assert count(d) == -1
    assert count(_desc_rnn([64], engine=0)) == -1        # VALU
    assert count(_desc_rnn([64], engine=3)) == -1        # bf16
    assert count(_desc_rnn([64], engine=2)) == -1
    assert count(_desc_rnn([64], cell=0)) == -1          # feed-forward: the _ex entry points build those
    assert count(_desc_rnn([64], cell=2)) == -1
    assert count(_desc_rnn([64], cell=-1)) == -1
    assert count(_desc_rnn([24])) == -1
    assert count(_desc_rnn([272])) == -1
    assert count(_desc_rnn([64, 24])) == -1
    d = _desc_rnn([64])
    d.n_hidden = 0
    assert count(d) == -1
    d = _desc_rnn([64, 64, 64])
    d.n_hidden = 4
    assert count(d) == -1
    d = _desc_rnn([64])
    d.in_dim = 0
    assert count(d) == -1


def test_create_rnn_refuses_null_arguments():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gaq_policy_create_rnn(None, C.byref(_desc_rnn([64])), C.byref(h)) == -1
    assert lib.gaq_policy_cell(None) == -1
    assert lib.gaq_policy_set_hidden_dev(None, None) == -1
    assert lib.gaq_policy_reset_hidden_dev(None, None, None) == -1


def test_unassigned_engine_values_stay_refused_by_desc_ex():
    lib = _lib.load()
    assert lib.gaq_policy_weight_count_ex(C.byref(_desc_ex([64], 2))) == -1
    assert lib.gaq_policy_weight_count_ex(C.byref(_desc_ex([64], 4))) == -1


def test_check_gru_layers():
    H = 64
    check_gru_layers(_gru(H), _head(H), 18, "tanh")
    check_gru_layers(_gru(H), _head(H, (256, 16)), 18, "relu")
    with pytest.raises(ValueError, match="multiple of 16"):
        check_gru_layers(_gru(24), _head(24), 18, "tanh")
    with pytest.raises(ValueError, match="multiple of 16"):
        check_gru_layers(_gru(272), _head(272), 18, "tanh")
    with pytest.raises(ValueError, match="obs_dim"):
        check_gru_layers(_gru(H, D=17), _head(H), 18, "tanh")
    with pytest.raises(ValueError, match="W_hh"):
        g = _gru(H)
        check_gru_layers((g[0], g[1][:, :32], g[2], g[3]), _head(H), 18, "tanh")
    with pytest.raises(ValueError, match="0 to 2 hidden layers"):
        check_gru_layers(_gru(H), _head(H, (16, 16, 16)), 18, "tanh")
    with pytest.raises(ValueError, match="takes"):
        check_gru_layers(_gru(H), _head(32), 18, "tanh")
    with pytest.raises(ValueError, match="4 outputs"):
        check_gru_layers(_gru(H), [(np.zeros((3, H), np.float32), np.zeros(3, np.float32))], 18, "tanh")
    with pytest.raises(ValueError, match="activation"):
        check_gru_layers(_gru(H), _head(H), 18, "elu")


def test_torch_gru_and_head():
    import torch
    nn = torch.nn
    torch.manual_seed(0)
    cell = nn.GRUCell(18, 32)
    W_ih, W_hh, b_ih, b_hh = torch_gru(cell)
    assert np.array_equal(W_ih, cell.weight_ih.detach().numpy()) and np.array_equal(b_hh, cell.bias_hh.detach().numpy())
    g = nn.GRU(18, 32, num_layers=1)
    assert np.array_equal(torch_gru(g)[1], g.weight_hh_l0.detach().numpy())
    nb = torch_gru(nn.GRUCell(18, 32, bias=False))
    assert not nb[2].any() and not nb[3].any()
    with pytest.raises(ValueError, match="num_layers"):
        torch_gru(nn.GRU(18, 32, num_layers=2))
    with pytest.raises(ValueError, match="bidirectional"):
        torch_gru(nn.GRU(18, 32, bidirectional=True))
    with pytest.raises(ValueError, match="GRUCell"):
        torch_gru(nn.LSTMCell(18, 32))
    layers, act, out_tanh = torch_head(nn.Linear(32, 4))
    assert len(layers) == 1 and not out_tanh
    layers, act, out_tanh = torch_head(nn.Sequential(nn.Linear(32, 4), nn.Tanh()))
    assert len(layers) == 1 and out_tanh
    layers, act, out_tanh = torch_head(nn.Sequential(nn.Linear(32, 64), nn.ReLU(), nn.Linear(64, 4)))
    assert len(layers) == 2 and act == "relu" and not out_tanh


def test_reference_step_matches_torch_grucell():
    import torch
    torch.manual_seed(1)
    cell = torch.nn.GRUCell(18, 48).double()
    x, h = torch.randn(5, 18, dtype=torch.float64), torch.randn(5, 48, dtype=torch.float64)
    gru = tuple(t.detach().numpy() for t in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh))
    assert np.allclose(gru_step64(gru, x.numpy(), h.numpy()), cell(x, h).detach().numpy(), rtol=0, atol=1e-12)
