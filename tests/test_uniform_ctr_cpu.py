"""The host's advance of a synchronised batch's tick / SVD counter word (quad_core.hpp: uniform_ctr_advance -- what gaq.hip passes to a
step launch instead of the counter plane) against the evolution of `tick` and `since_last_svd` in oracle/quad_oracle.py.  No GPU.

The oracle flies one Hummingbird with random actions for 1200 env steps at sim_freq 200; after every step its tick and the number of
sub-steps since its last re-orthonormalisation (since_last_svd / dt: the oracle accumulates dt and fires at > 0.5 s) must be the two
halves of the word.  Like the reference the oracle leaves the reset to its caller: with auto_reset the test resets it when it reports
done, which is what the step kernel does in the launch.  ep_len 3 (an episode every four steps) and 500 (two episode ends in the run),
sim_steps 1 and 2 (the SVD period of 100 sub-steps is crossed 12 and 24 times), auto_reset on and off."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import quad_oracle as qo
from tests import golden_util as gu

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "uniform_ctr.cpp")
STEPS = 1200


@pytest.fixture(scope="module")
def uc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("uniform_ctr") / "libuc.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", out, SRC])
    lib = C.CDLL(out)
    for name, n in (("uc_advance", 5), ("uc_pack", 1), ("uc_unpack", 1), ("uc_valid_bit", 0), ("uc_svd_max", 0)):
        f = getattr(lib, name)
        f.restype = C.c_uint32
        f.argtypes = [C.c_uint32] + [C.c_int32] * (n - 1) if n else []
    return lib


@pytest.mark.parametrize("auto_reset", [1, 0])
@pytest.mark.parametrize("sim_steps", [1, 2])
@pytest.mark.parametrize("ep_len", [3, 500])
def test_advance_follows_the_oracle(uc, ep_len, sim_steps, auto_reset):
    d = gu.load("g2_hummingbird_raw")
    p = qo.Params.from_golden_const(1, gu.sub(d, "const_"))
    cfg = qo.Config(sim_freq=200., sim_steps=sim_steps)
    cfg.ep_len = ep_len
    period = qo.svd_period(cfg.dt)
    assert period == 100
    s = qo.State(1)
    rng = np.random.RandomState(5)
    qo.reset(s, p, cfg, rng)
    word, resets, fires = 0, 0, 0
    for t in range(STEPS):
        before = float(s.since_last_svd[0])
        _, _, done = qo.env_step(s, p, cfg, rng.uniform(-1, 1, size=(1, 4)))
        fires += float(s.since_last_svd[0]) < before
        if auto_reset and done[0]:
            qo.reset(s, p, cfg, rng)                     # (tick <- 0; since_last_svd survives, like the dynamics object it lives in)
            resets += 1
        word = uc.uc_advance(word, sim_steps, period, ep_len, auto_reset)
        assert (word & 0xFFFF) == int(s.tick[0]), t
        assert (word >> 16) == int(round(float(s.since_last_svd[0]) / cfg.dt)), t
    assert fires == STEPS * sim_steps // period
    assert resets == (STEPS // (ep_len + 1) if auto_reset else 0)
    if not auto_reset:
        assert (word & 0xFFFF) == STEPS                  # past ep_len: `done` every step, the clock runs on


def test_tick_saturates_where_the_kernel_does(uc):
    w = uc.uc_advance(0xFFFE, 2, 100, 70000, 0)
    assert w == (0xFFFF | (2 << 16))
    assert uc.uc_advance(w, 2, 100, 70000, 0) == (0xFFFF | (4 << 16))
    assert uc.uc_advance(0xFFFF | (99 << 16), 2, 100, 0xFFFF, 1) == (0xFFFF | (1 << 16))      # tick > ep_len is never true there
    assert uc.uc_advance(5 | (98 << 16), 3, 100, 5, 1) == (0 | (1 << 16))


def test_the_word_survives_the_argument(uc):
    """[valid | svd_ctr : 14 | tick : 16] above the sweep bit of StepCfg::sweep"""
    valid, svd_max = uc.uc_valid_bit(), uc.uc_svd_max()
    assert valid == 2 and svd_max == 0x3FFF
    rng = np.random.RandomState(3)
    words = [0, 0xFFFF, svd_max << 16, 0xFFFF | (svd_max << 16)] + [int(rng.randint(0, 1 << 16)) | (int(rng.randint(0, svd_max + 1)) << 16) for _ in range(2000)]
    for w in words:
        a = uc.uc_pack(w)
        assert a & valid and not a & 1                   # (bit 0 is the sweep order's)
        assert uc.uc_unpack(a) == w and uc.uc_unpack(a | 1) == w
