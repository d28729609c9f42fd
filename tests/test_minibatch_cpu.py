"""Shuffled minibatches without a GPU (gaq.h "shuffled minibatches"): the five entry points are declared, bound and refuse null
handles; the Python surface; and tests/perm_ref.py, the NumPy restatement of gaq_perm_dev's formula that the device test compares
with bit for bit -- it is a permutation at every size class, depends on the epoch and the seed, and shuffles well enough that an
epoch's minibatches are unbiased samples.  Every figure a test bounds is printed before it is asserted."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P
from tests.perm_ref import half_bits, perm_ref

ENTRY_POINTS = {"gaq_policy_grad_ppo_idx_dev": 14, "gaq_policy_grad_ppo_ac_idx_dev": 20, "gaq_critic_grad_mse_idx_dev": 10,
                "gaq_policy_grad_ppo_seq_idx_dev": 23, "gaq_perm_dev": 6}
PARENTS = {"gaq_policy_grad_ppo_idx_dev": "gaq_policy_grad_ppo_dev", "gaq_policy_grad_ppo_ac_idx_dev": "gaq_policy_grad_ppo_ac_dev",
           "gaq_critic_grad_mse_idx_dev": "gaq_critic_grad_mse_dev"}


def test_entry_points_are_declared_bound_and_refuse_null_handles():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert len(sig[name]) == nargs and name + "(" in header and hasattr(lib, name), name
    for name, parent in PARENTS.items():                           # (handle, rows, idx, src_rows), then the parent's from obs on
        assert sig[name][:4] == [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] and sig[name][4:] == sig[parent][2:], name
    seq, par = sig["gaq_policy_grad_ppo_seq_idx_dev"], sig["gaq_policy_grad_ppo_seq_dev"]
    assert seq[:5] == [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64] and seq[5:] == par[3:]
    assert sig["gaq_perm_dev"] == [C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.gaq_abi_version() == 5                              # additive entry points: the ABI version stays
    assert lib.gaq_policy_grad_ppo_idx_dev(None, 4, None, 8, *[None] * 4, 0.2, 1.0, *[None] * 4) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_grad_ppo_ac_idx_dev(None, 4, None, 8, *[None] * 6, 0.2, 0.2, 0.5, 0.01, 1.0, *[None] * 5) == -1
    assert b"null" in lib.gaq_last_error()
    assert lib.gaq_critic_grad_mse_idx_dev(None, 4, None, 8, None, None, 1.0, *[None] * 3) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_grad_ppo_seq_idx_dev(None, 2, 4, None, 8, *[None] * 8, 0.2, 0.2, 0.5, 0.01, 1.0, *[None] * 5) == -1
    assert b"null" in lib.gaq_last_error()
    # gaq_perm_dev has no handle: its host-side refusals need no device
    assert lib.gaq_perm_dev(8, 1, 0, None, None, None) == -1 and b"null" in lib.gaq_last_error()
    for n in (0, -1, 2 ** 31):
        assert lib.gaq_perm_dev(n, 1, 0, None, 4096, None) == -1 and b"n must be in [1, 2^31 - 1]" in lib.gaq_last_error(), n
    assert lib.gaq_perm_dev(8, 1, 0, None, 4098, None) == -1 and b"4-byte aligned" in lib.gaq_last_error()
    assert lib.gaq_perm_dev(8, 1, 0, 4100, 4096, None) == -1 and b"epoch_dev: 8" in lib.gaq_last_error()


def test_python_surface():
    def sig(f):
        return str(inspect.signature(f))
    tail = "clip=0.2, scale=None, grad=None, grad_log_std=None, stats=None, stream=None)"
    assert sig(P.MLPPolicy.ppo_grad_idx_dev) == "(self, idx, obs, actions, logp_old, adv, " + tail
    assert sig(P.MLPPolicy.ppo_grad_idx_dev) == sig(P.MLPPolicy.ppo_grad_dev).replace("(self, ", "(self, idx, ")
    for new, old in ((P.MLPPolicy.ppo_ac_grad_idx_dev, P.MLPPolicy.ppo_ac_grad_dev), (P.MLPCritic.mse_grad_idx_dev, P.MLPCritic.mse_grad_dev),
                     (P.GRUPolicy.ppo_seq_grad_idx_dev, P.GRUPolicy.ppo_seq_grad_dev)):
        assert sig(new) == sig(old).replace("(self, ", "(self, idx, "), new
    assert sig(P.MLPCritic.mse_grad_idx_dev) == "(self, idx, obs, target, scale=None, grad=None, stats=None, stream=None)"
    assert sig(P.perm_dev) == "(n, seed, epoch=0, epoch_dev=None, out=None, device=None, stream=None)"
    for f in (P.MLPPolicy.ppo_grad_idx_dev, P.MLPPolicy.ppo_ac_grad_idx_dev, P.MLPCritic.mse_grad_idx_dev, P.GRUPolicy.ppo_seq_grad_idx_dev,
              P.perm_dev):
        assert f.__doc__ and ("idx" in f.__doc__ or f is P.perm_dev), f
    assert not hasattr(P.LSTMPolicy, "ppo_seq_grad_idx_dev")
    with pytest.raises(ValueError, match="n must be in"):
        P.perm_dev(0, 1)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 1000, 65537, 2 ** 20])
def test_perm_ref_is_a_permutation(n):
    p = perm_ref(n, seed=12345, epoch=3)
    assert p.dtype == np.int32 and p.shape == (n,)
    assert np.array_equal(np.sort(p), np.arange(n, dtype=np.int32))
    b = 2 * half_bits(n)
    assert b % 2 == 0 and b >= 2 and (1 << b) >= n and (b == 2 or (1 << (b - 2)) < n)      # the smallest even b, so 2^b <= 4 n


def test_perm_ref_depends_on_epoch_and_seed():
    n = 1000
    base = perm_ref(n, 7, 0)
    assert np.array_equal(base, perm_ref(n, 7, 0))
    for other in (perm_ref(n, 7, 1), perm_ref(n, 8, 0), perm_ref(n, 7, 1 << 32), perm_ref(n, 7 + (1 << 32), 0)):
        same = int((other == base).sum())
        print("positions equal to (seed 7, epoch 0): %d of %d" % (same, n))
        assert same < 20                                           # two independent permutations agree in 1 place on average
    assert not np.array_equal(perm_ref(64, 7, 0), perm_ref(64, 7, 1))


def test_perm_ref_shuffles_minibatches_evenly():
    """Over 256 epochs at n = 4096, against a uniformly random permutation.  Fixed points per epoch: mean 1, variance 1, so their mean
    over 256 epochs has sigma 1 / 16: the band is 1 +- 5 sigma = [0.6875, 1.3125].  The mean index of a minibatch of 512 drawn without
    replacement: mean 2047.5, variance (n^2 - 1) / 12 / 512 x (n - 512) / (n - 1) = 48.9^2; over 256 epochs sigma 3.06: the band is
    2047.5 +- 5 sigma = +- 15.3.  (The bands come from these distributions, not from the values observed.)"""
    n, epochs, k = 4096, 256, 8
    mb = n // k
    fixed, means = 0, np.zeros(k)
    ident = np.arange(n)
    for e in range(epochs):
        p = perm_ref(n, 2024, e)
        fixed += int((p == ident).sum())
        means += p.reshape(k, mb).mean(axis=1)
    fixed_mean, means = fixed / epochs, means / epochs
    sigma_mb = np.sqrt((n * n - 1) / 12.0 / mb * (n - mb) / (n - 1)) / np.sqrt(epochs)
    print("fixed points per epoch: %.4f (band 0.6875 .. 1.3125)" % fixed_mean)
    print("minibatch mean index - 2047.5: %s (band +- %.2f)" % (" ".join("%+.2f" % (m - 2047.5) for m in means), 5 * sigma_mb))
    assert 1.0 - 5.0 / 16.0 <= fixed_mean <= 1.0 + 5.0 / 16.0
    assert np.all(np.abs(means - (n - 1) / 2.0) <= 5 * sigma_mb)
