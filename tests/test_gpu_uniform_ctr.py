"""-m gpu: keeping the tick / SVD counters of a synchronised batch on the host (quad_core.hpp: uniform counters) changes no bit.

While every env of a handle carries the same `tick | svd_ctr << 16` word, gaq_step_dev passes that word to its launch and the launch
neither reads nor writes the counter plane; every other path that looks at the counters first writes the word into the plane
(gaq.hip: counters_to_plane).  So a handle with the default setting and a twin created under GAQ_UNIFORM_CTR=0 -- which keeps its
counters in the plane for life, as every earlier release did -- given the same seed and actions, agree to the bit in everything
the caller can see: observations, rewards, dones after every step and the full exported state at the end of every script.  (The
state is NOT exported after every step: that would put the default handle on the plane path after its first step.)

Shapes: N = 200 (three full tiles and a partial one, one workgroup) and N = 64 (one full tile), Hummingbird, thrust noise on.
ep_len = 3, so every env auto-resets every fourth step, several times in each script; one run of 60 steps at sim_steps = 2 crosses
the SVD period of 100 sub-steps.  gaq_uniform_counters tells which path the next launch takes, so every script also checks that it
ran the path it is about, and its guard words show that the fill wrote ntiles * 64 words and none behind them."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from gym_art_amd import _lib

pytestmark = pytest.mark.gpu
SIZES = [200, 64]
F_CTR, F_GENERIC = 8192, 8


@contextlib.contextmanager
def environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dev():
    import torch
    return torch.device("cuda", 0)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Handle(object):
    def __init__(self, n, uniform, kw, env):
        import torch
        from gym_art_amd import QuadrotorEnv
        common = dict(num_envs=n, ep_time=0.035, seed=43, init_random_state=True, auto_reset=True, info=False, alias_obs=True)
        common.update(kw)
        with environ(**dict(env, **({} if uniform else {"GAQ_UNIFORM_CTR": "0"}))):
            self.e = QuadrotorEnv(**common)
        assert self.e.ep_len == 3
        self.n = n
        self.obs = torch.zeros((n, self.e.obs_dim), device=dev())
        self.rew = torch.zeros(n, device=dev())
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev())
        self.e.reset_dev(self.obs)

    def uniform(self):
        """(the next step takes its counters as an argument, the word the host keeps)"""
        v, w = C.c_int32(-1), C.c_uint32(0)
        _lib.check(self.e._lib.gaq_uniform_counters(self.e._handle, C.byref(v), C.byref(w), None))
        return bool(v.value), int(w.value)

    def guard_intact(self):
        g = C.c_int32(-1)
        _lib.check(self.e._lib.gaq_uniform_counters(self.e._handle, None, None, C.byref(g)))
        return g.value == 1

    def out(self):
        return self.obs.cpu().numpy(), self.rew.cpu().numpy(), self.done.cpu().numpy()


class Pair(object):
    """u: the default setting; p: its twin under GAQ_UNIFORM_CTR=0.  Every call goes to both."""

    def __init__(self, n, kw=None, env=None):
        import torch
        self.n = n
        self.u, self.p = Handle(n, True, kw or {}, env or {}), Handle(n, False, kw or {}, env or {})
        self.gen = torch.Generator(device=dev()); self.gen.manual_seed(11)
        self.t = 0
        self.finished = 0
        assert self.u.e.launch_variant == self.p.e.launch_variant          # the setting takes no part in the kernel selection
        assert not self.p.uniform()[0]
        self.compare("reset")

    def both(self):
        return (self.u, self.p)

    def actions(self, *shape):
        import torch
        return torch.rand(shape + (self.n, 4), device=dev(), generator=self.gen) * 2 - 1

    def compare(self, what):
        for k, a, b in zip(("obs", "reward", "done"), self.u.out(), self.p.out()):
            assert same(a, b), "%s, step %d: %s differs from the GAQ_UNIFORM_CTR=0 twin's" % (what, self.t, k)

    def step(self, k=1, what="step", uniform=None):
        for _ in range(k):
            a = self.actions()
            if uniform is not None:
                assert self.u.uniform()[0] == uniform, (what, self.t)
            for h in self.both():
                h.e.step_dev(a, h.obs, h.rew, h.done)
            self.t += 1
            self.compare(what)
            self.finished += int(self.u.done.sum())
        assert not self.p.uniform()[0]

    def states(self, what):
        a, b = self.u.e.get_state(), self.p.e.get_state()
        assert same(a, b), "%s, step %d: the exported state differs; planes %s" % (what, self.t, sorted(set(np.nonzero(a != b)[0])))
        return a

    def finish(self, what):
        self.states(what)
        assert self.u.guard_intact() and self.p.guard_intact(), what
        for h in self.both():
            h.e.close()


def svd_period(dt=1.0 / 200.0):
    """sub-steps between two re-orthonormalisations: `since_last_svd += dt; if since_last_svd > 0.5` (oracle/quad_oracle.py)"""
    t, k = 0.0, 0
    while not t > 0.5:
        t += dt
        k += 1
    return k


PERIOD = svd_period()
assert PERIOD == 100


def expected_word(steps_since_reset, substeps, ep_len=3):
    return (steps_since_reset % (ep_len + 1)) | ((substeps % PERIOD) << 16)


@pytest.mark.parametrize("n", SIZES)
def test_plain_stepping(n):
    q = Pair(n)
    assert q.u.e.launch_variant & (F_CTR | F_GENERIC) == 0
    assert q.u.uniform() == (True, 0)
    q.step(13, "plain stepping", uniform=True)
    assert q.finished == 3 * n                                              # every env ended three episodes on the way
    assert q.u.uniform() == (True, expected_word(13, 26))
    st = q.states("plain stepping")
    assert np.all(st[37] == 13 % 4) and np.all(st[38] == 26)
    q.finish("plain stepping")


@pytest.mark.parametrize("n", SIZES)
def test_sixty_steps_cross_the_svd_period(n):
    q = Pair(n)
    assert q.u.e.sim_steps == 2
    q.step(60, "60 steps", uniform=True)
    assert q.u.uniform() == (True, expected_word(60, 120))
    st = q.states("60 steps")
    assert np.all(st[38] == 20) and np.all(st[37] == 0)
    q.finish("60 steps")


@pytest.mark.parametrize("n", SIZES)
def test_get_state_in_the_middle(n):
    q = Pair(n)
    q.step(6, "before get_state", uniform=True)
    st = q.states("get_state in the middle")
    assert np.all(st[37] == 6 % 4) and np.all(st[38] == 12)                 # the plane was filled with the host's word first
    assert not q.u.uniform()[0]
    q.step(7, "after get_state", uniform=False)
    q.finish("after get_state")


@pytest.mark.parametrize("n", SIZES)
def test_set_state_with_staggered_ticks(n):
    q = Pair(n)
    q.step(5, "before set_state", uniform=True)
    st = q.states("before set_state")
    st[37] = np.arange(n) % 4
    st[38] = (np.arange(n) * 7) % 100
    for h in q.both():
        h.e.set_state(st)
    assert not q.u.uniform()[0]
    q.step(9, "after set_state", uniform=False)
    # ... and a full reset does NOT return this handle to the argument path: the envs' svd_ctr differ now
    for h in q.both():
        h.e.reset_dev(h.obs)
    q.compare("full reset after set_state")
    assert not q.u.uniform()[0]
    q.step(5, "after set_state and a full reset", uniform=False)
    q.finish("after set_state")


@pytest.mark.parametrize("n", SIZES)
def test_masked_reset_then_full_reset(n):
    import torch
    q = Pair(n)
    q.step(5, "before the masked reset", uniform=True)
    mask = (torch.arange(n, device=dev()) % 3 == 0).to(torch.uint8)
    for h in q.both():
        h.e.reset_dev(h.obs, mask)
    q.compare("masked reset")
    assert not q.u.uniform()[0]
    q.step(6, "after the masked reset", uniform=False)
    st = q.states("after the masked reset")
    assert len(set(st[37])) == 2 and np.all(st[38] == 22)                   # two episode phases, one svd_ctr
    # a full reset synchronises the episode clocks again, and the host still knows svd_ctr: back to the argument path
    for h in q.both():
        h.e.reset_dev(h.obs)
    q.compare("full reset")
    assert q.u.uniform() == (True, 22 << 16)
    q.step(9, "after the full reset", uniform=True)
    assert q.u.uniform() == (True, expected_word(9, 22 + 18))
    q.finish("after the full reset")


@pytest.mark.parametrize("n", SIZES)
def test_step_many_between_single_steps(n):
    import torch
    q = Pair(n)
    q.step(3, "before step_many", uniform=True)
    T = 6
    a = q.actions(T)
    outs = []
    for h in q.both():
        o, r, d = torch.zeros((T, n, 18), device=dev()), torch.zeros((T, n), device=dev()), torch.zeros((T, n), dtype=torch.uint8, device=dev())
        h.e.step_many_dev(a, o, r, d)
        h.obs = o[T - 1]                                                    # (alias layout: the last rows are the state's heads now)
        outs.append((o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()))
    q.t += T
    assert all(same(x, y) for x, y in zip(*outs)), "step_many_dev"
    assert not q.u.uniform()[0]
    q.step(5, "after step_many", uniform=False)
    st = q.states("after step_many")
    assert np.all(st[37] == 14 % 4) and np.all(st[38] == 28)
    for h in q.both():
        h.e.reset_dev(h.obs)
    assert q.u.uniform() == (True, 28 << 16)                                # (the host counted the rollout's sub-steps)
    q.step(5, "after step_many and a full reset", uniform=True)
    q.finish("after step_many")


@pytest.mark.parametrize("n", SIZES)
def test_graph_safe_on_and_off(n):
    q = Pair(n)
    q.step(5, "before graph-safe mode", uniform=True)
    for h in q.both():
        h.e.set_graph_safe(True)
    assert not q.u.uniform()[0]
    assert q.u.e.launch_variant == q.p.e.launch_variant
    q.step(6, "graph-safe mode", uniform=False)
    for h in q.both():
        h.e.reset_dev(h.obs)
    q.compare("full reset in graph-safe mode")
    assert not q.u.uniform()[0]                                             # never in graph-safe mode
    q.step(3, "graph-safe mode after a full reset", uniform=False)
    for h in q.both():
        h.e.set_graph_safe(False)
    q.step(6, "graph-safe mode off again", uniform=False)
    q.finish("graph-safe mode")


@pytest.mark.parametrize("case", ["crazyflie", "shadow", "plain", "generic"])
def test_other_kernels(case):
    kw, env = {"crazyflie": (dict(dynamics_params="Crazyflie"), {}), "shadow": (dict(alias_obs=None), {}),
               "plain": (dict(alias_obs=False), {}), "generic": (dict(alias_obs=False), dict(GAQ_FORCE_GENERIC="1"))}[case]
    q = Pair(200, kw, env)
    assert bool(q.u.e.launch_variant & F_GENERIC) == (case == "generic")
    q.step(9, case, uniform=True)
    st = q.states(case)
    assert np.all(st[37] == 1) and np.all(st[38] == 18)
    q.step(5, case + " after get_state", uniform=False)
    for h in q.both():
        h.e.reset_dev(h.obs)
    q.compare(case + " full reset")
    assert q.u.uniform()[0]
    q.step(5, case + " after a full reset", uniform=True)
    q.finish(case)


def test_the_fill_ends_at_the_plane():
    """N = 129: three tiles, the last one with one env.  The plane's 192 words are filled (the padding lanes' too), the guard words
    behind it keep their pattern; N = 1 and a plane of exactly one block of the fill (N = 256) likewise."""
    for n in (129, 1, 256):
        q = Pair(n)
        q.step(2, "fill, N = %d" % n, uniform=True)
        st = q.states("fill, N = %d" % n)                                   # (fills the plane)
        assert np.all(st[37] == 2) and np.all(st[38] == 4) and st.shape[1] == n
        q.step(1, "fill, N = %d" % n, uniform=False)
        q.finish("fill, N = %d" % n)
