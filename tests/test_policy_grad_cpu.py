"""Gradients on the device, without a GPU: the fp64 reference (tests/policy_grad_ref.py) against torch fp64 autograd on every case of the
matrix, the conditions on each case's inputs, unpack_weights as the inverse of pack_weights, the committed torch fp32 baselines, and the
refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P
from tests import policy_grad_ref as G

ALL = G.POLICY_CASES + G.CRITIC_CASES


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_reference_agrees_with_torch_fp64_autograd(case):
    """<= 1e-12 relative, per parameter tensor and for log_std, logp / V and the sums, at every row count of the matrix"""
    import torch
    _, inp = G.case_inputs(case.name)
    for rows in G.ROWS:
        assert max(G.torch_errors(case, inp, rows, torch.float64)) <= 1e-12, rows


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_inputs_meet_the_conditions(case):
    """conditions on the inputs, not measurements: margins of every fp32 / fp64 branch, 10 % to 70 % of the ratios outside the clip range,
    both signs of advantage, units off their flat tails"""
    _, inp = G.case_inputs(case.name)
    assert G.conditions(case, inp) is None
    assert G.R == 64 * 7 + 5 and set(G.BASELINE[case.name]) == set(G.ROWS)


def test_one_committed_baseline_is_what_torch_fp32_gives_here():
    """The table is a measurement of torch on the CPU.  torch's fp32 sums depend on its build and its thread count, so another host gives
    other numbers of the same size: the gradient's and logp's errors are maxima over thousands of elements and come out within a factor
    of 8 of the committed ones; the loss and kl sums are single scalars, whose error is one draw (anywhere below the committed size, 0
    included), so they are only held below the bound bounds() derives from the family's cases."""
    import torch
    case, inp = G.case_inputs("policy-64x64-tanh")
    got = G.torch_errors(case, inp, G.R, torch.float32)
    want = G.BASELINE[case.name][G.R]
    for g, w in zip(got[:2], want[:2]):
        assert w / 8.0 <= g <= w * 8.0, (got, want)
    for g, b in zip(got[2:], G.bounds(case.name, G.R)[2:]):
        assert g <= b, (got, G.bounds(case.name, G.R))


@pytest.mark.parametrize("n_out", [4, 1])
def test_unpack_weights_round_trips(n_out):
    import torch
    for widths, D in (([16], 18), ([48, 80, 32], 19), ([128, 128, 128], 18), ([256], 13)):
        rng = np.random.RandomState(len(widths) + D)
        dims = [D] + widths + [n_out]
        layers = [(rng.randn(dims[k + 1], dims[k]).astype(np.float32), rng.randn(dims[k + 1]).astype(np.float32)) for k in range(len(dims) - 1)]
        packed = P.pack_weights(layers) if n_out == 4 else P.pack_critic_weights(layers)
        for src in (packed, torch.from_numpy(packed)):
            back = P.unpack_weights(src, D, widths, n_out)
            assert len(back) == len(layers)
            for (W, b), (W0, b0) in zip(back, layers):
                assert type(W) is type(src) and tuple(W.shape) == W0.shape and tuple(b.shape) == b0.shape
                assert np.array_equal(np.asarray(W), W0) and np.array_equal(np.asarray(b), b0)
        assert np.array_equal(P.pack_weights([(np.asarray(W), np.asarray(b)) for W, b in P.unpack_weights(packed, D, widths, n_out)]), packed)
    with pytest.raises(ValueError, match="packs into"):
        P.unpack_weights(np.zeros(10, np.float32), 18, [16], 4)
    with pytest.raises(ValueError, match="multiples of 16"):
        P.unpack_weights(np.zeros(10, np.float32), 18, [10], 4)


def test_entry_points_are_declared_bound_and_refuse_null_handles():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    want = {"gaq_policy_logp_dev": 7, "gaq_policy_backward_dev": 7, "gaq_policy_grad_ppo_dev": 12, "gaq_critic_backward_dev": 7,
            "gaq_critic_grad_mse_dev": 8}
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib._HERE), "include", "gaq.h")).read()
    for name, nargs in want.items():
        assert len(sig[name]) == nargs and sig[name][1] is C.c_int64 and name + "(" in header, name
    assert lib.gaq_abi_version() == 5                              # additive entry points: the ABI version stays
    assert lib.gaq_policy_logp_dev(None, 4, None, None, None, None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_backward_dev(None, 4, None, None, 1.0, None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_grad_ppo_dev(None, 4, None, None, None, None, 0.2, 1.0, None, None, None, None) == -1
    assert lib.gaq_critic_backward_dev(None, 4, None, None, 1.0, None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_critic_grad_mse_dev(None, 4, None, None, 1.0, None, None, None) == -1 and b"null" in lib.gaq_last_error()


def test_python_surface():
    import inspect

    def sig(f):
        return str(inspect.signature(f))
    assert sig(P.MLPPolicy.logp_dev) == "(self, obs, actions, out=None, mean=None, stream=None)"
    assert sig(P.MLPPolicy.backward_dev) == "(self, obs, dout, scale=1.0, grad=None, stream=None)"
    assert sig(P.MLPPolicy.ppo_grad_dev) == ("(self, obs, actions, logp_old, adv, clip=0.2, scale=None, grad=None, grad_log_std=None, "
                                             "stats=None, stream=None)")
    assert sig(P.MLPCritic.backward_dev) == "(self, obs, dout, scale=1.0, grad=None, stream=None)"
    assert sig(P.MLPCritic.mse_grad_dev) == "(self, obs, target, scale=None, grad=None, stats=None, stream=None)"
    assert sig(P.unpack_weights) == "(packed, in_dim, widths, n_out)"
    for cls in (P.MLPPolicy, P.MLPCritic):
        assert sig(cls.set_weights) == "(self, layers)" and sig(cls.set_weights_dev) == "(self, packed)"
