"""-m gpu: gaq_step's three transports (csrc/gaq.hip: mapped host memory, a pinned mirror with copies, pageable copies) and its info
mirror, pinned bit for bit to the device-pointer step of a twin handle at the sizes where each can go wrong: one lane, a ragged second
tile (65), the last staged size (11274) and the first pageable one (11275).  The scenario is tests/host_transports.py."""
import contextlib

import numpy as np
import pytest

from tests import host_transports as ht

pytestmark = pytest.mark.gpu
STAGED = [(n, c, t) for n, c in ht.STAGED_CASES for t in ("mapped", "pinned")]
PAGEABLE = [(n, c, "pageable") for n, c in ht.PAGEABLE_CASES]
MIRRORED = [(n, c, t) for n, c, t in STAGED if c.endswith("_info")]
ids = lambda cases: ["%d-%s-%s" % c for c in cases]


def same(a, b, names):
    bad = [k for k in names if not np.array_equal(a[k], b[k])]
    assert not bad, bad


@pytest.mark.parametrize("n,config,transport", STAGED + PAGEABLE, ids=ids(STAGED + PAGEABLE))
def test_every_transport_returns_the_device_pointer_steps_bits(n, config, transport):
    """reset, 25 steps through four auto-resets, then the state (and aux rows), observe(), and both again: what the host-pointer calls
    hand back is what a twin stepped with step_dev on device tensors holds"""
    sc, twin = ht.scenario(n, config, transport), ht.scenario(n, config, "dev")
    assert sc["done"].any() and not sc["done"].all() and np.isfinite(sc["reward"]).all()      # episodes ended inside the window
    names = [k for k in sc if not k.startswith("info/")]
    assert sorted(names) == sorted(k for k in twin if not k.startswith("info/"))
    same(sc, twin, names)


@pytest.mark.parametrize("n,config,transport", MIRRORED, ids=ids(MIRRORED))
def test_the_info_mirror_equals_the_device_export_of_the_same_handle(n, config, transport):
    """an info handle without sensor noise on a staged transport: get_state / gaq_get_aux right after a step read the mirror the step
    brought home.  observe() changes no state.  On the planes layout it is a launch, which drops the mirror: the second reading is
    export_kernel's from the device, the path every handle takes when there is no mirror.  (On the split layouts observe() reads the
    heads without a launch and the mirror stands; the twin of the test above, which never has one, is the device reading there.)"""
    sc = ht.scenario(n, config, transport)
    assert np.array_equal(sc["state"], sc["state_after_observe"]) and np.array_equal(sc["aux"], sc["aux_after_observe"])
    assert np.array_equal(sc["observed"], sc["obs"][-1])


def test_a_pageable_handle_builds_its_info_dict_from_the_device():
    """above the 1 MiB stage no mirror comes home: the info dict of step() is built from gaq_get_state + gaq_get_aux on the device, and
    equals the one built from the step_dev twin's state and aux rows, entry by entry"""
    sc, twin = ht.scenario(ht.PAGEABLE_SIZE, "info", "pageable"), ht.scenario(ht.PAGEABLE_SIZE, "info", "dev")
    names = [k for k in sc if k.startswith("info/")]
    assert len(names) > 40 and sorted(names) == sorted(k for k in twin if k.startswith("info/"))
    same(sc, twin, names)


@pytest.mark.parametrize("transport", ["mapped", "pinned"])
def test_set_state_drops_the_info_mirror(transport):
    """step (the mirror comes home), set_state with other planes, get_state: the planes just set, not the mirror's.  The other planes
    are the handle's own, one env further along: every value is one the state encoding holds exactly."""
    n = 65
    with ht.zero_copy_off() if transport == "pinned" else contextlib.nullcontext():
        env = ht.make(n, "info")
        env.reset()
        env.step(ht.actions(n)[0])
    mirror = env.get_state()
    moved = np.roll(mirror, 1, axis=1)
    assert not np.array_equal(moved[0:3], mirror[0:3])
    env.set_state(moved)
    got = env.get_state()
    assert np.array_equal(got, moved)
    env.close()


@pytest.mark.parametrize("n,transport", [(8, "mapped"), (8, "pinned"), (ht.PAGEABLE_SIZE, "pageable")])
def test_nan_reward_raises_on_every_transport_and_leaves_the_handle_usable(n, transport):
    """tests/test_gpu_env_api.py::test_nan_reward_raises_value_error on the other two transports as well (quadrotor.py:633-636), and
    afterwards: the step that raised has cleared the device's count, so a handle put back to a finite state has nothing to report"""
    from gym_art_amd import QuadrotorEnv
    with ht.zero_copy_off() if transport == "pinned" else contextlib.nullcontext():
        env = QuadrotorEnv(num_envs=n, seed=0, auto_reset=False)
        finite = env.get_state()
        st = finite.copy()
        st[0, 3] = np.nan
        env.set_state(st)
        with pytest.raises(ValueError, match="reward is Nan"):
            env.step(np.zeros((n, 4), np.float32))
    env.set_state(finite)
    env.check_finite()
    _, rew, _, _ = env.step(np.zeros((n, 4), np.float32))
    assert np.isfinite(rew).all()
    env.check_finite()
    env.close()
