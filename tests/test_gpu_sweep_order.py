"""-m gpu: the order in which step_kernel walks the batch (GAQ_SWEEP, StepCfg::sweep) changes no bit of any result.

With the alternating sweep on, the workgroups of an odd step take the blocks of four tiles in descending order within each class
b mod 8 (workgroups b and b + 8 share an XCD and its L2, so a tile stays on its XCD).  Every tile is still stepped by exactly one wave
and every random stream is keyed by the global env index and the step index, so two handles created under GAQ_SWEEP=0 (always
ascending: the order of every earlier release) and GAQ_SWEEP=1, given the same seed, start state and actions, have to agree to the bit
after every step: observations, rewards, dones, the exported state planes, the counters, and whatever else the step launch writes
(packed rows, terminal observations, the done-index list -- compared as a set, its order was never defined).  Six consecutive steps
from step index 0 are compared, so both the window that starts on an even step and the one that starts on an odd step are in them.

Shapes: one partial tile (1, 63), one full tile (64), a tile and one env (65), two blocks with a partial last one (257: 5 tiles), four
blocks whose last one holds one tile of one env (833: 14 tiles) -- up to eight blocks every class has one member and the order stays as
it is -- and 4609: 73 tiles in 19 blocks, so three classes have three members, five have two, and the last block, one tile of one env,
is taken by workgroup 2 on odd steps.  The swarm cases need whole worlds of 8 agents: the nearest multiples of 8.  Episodes last five
steps and start at staggered phases (tick = i mod 6), so every step resets -- and, with per-env parameters, promotes -- envs in every
block, mirrored ones included."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from gym_art_amd import _lib

pytestmark = pytest.mark.gpu
SAMPLER = {"class": "RelativeSampler", "noise_ratio": 0.2, "sampler": "normal"}
SIZES = [1, 63, 64, 65, 257, 833, 4609]
STEPS = 6
F_ROWS, F_CTR, F_GENERIC, F_PACK, F_PREDRAW, F_NT = 4096, 8192, 8, 1024, 128, 256

# name -> (constructor kwargs, creation environment, extras)
CASES = {
    "alias_20": (dict(alias_obs=True), dict(GAQ_PREDRAW="0", GAQ_NT="0"), ()),
    "alias_148": (dict(alias_obs=True), dict(GAQ_PREDRAW="1", GAQ_NT="0"), ()),
    "shadow": (dict(alias_obs=None), {}, ()),
    "plain_4": (dict(alias_obs=False), {}, ()),
    "crazyflie_lag": (dict(alias_obs=True, dynamics_params="Crazyflie"), {}, ()),
    "per_env_randomize_every_1": (dict(dyn_sampler_1=dict(SAMPLER), dynamics_randomize_every=1), {}, ()),
    "packed_rows": (dict(alias_obs=True), dict(GAQ_PREDRAW="0", GAQ_NT="0"), ("rows",)),
    "sense_noise_pack": (dict(alias_obs=None, sense_noise="default"), {}, ()),
    "swarm_8": (dict(), {}, ("swarm",)),
    "generic": (dict(alias_obs=False), dict(GAQ_FORCE_GENERIC="1"), ()),
    "terminal_observation": (dict(alias_obs=True, terminal_observation=True), {}, ("term",)),
    "done_list": (dict(alias_obs=True, compact_done=True), {}, ("done_list",)),
}


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


def make(n, kw, env, swarm, sweep):
    """One env created under GAQ_SWEEP=<sweep> (the handle keeps it), episodes of five steps at staggered phases."""
    from gym_art_amd import QuadrotorEnv, QuadrotorEnvMulti
    common = dict(ep_time=0.05, seed=41, init_random_state=True, auto_reset=True, info=False)
    with environ(GAQ_SWEEP=str(sweep), **env):
        if swarm:
            e = QuadrotorEnvMulti(num_agents=8, num_worlds=n // 8, goal_radius=0.5, **common, **kw)
        else:
            e = QuadrotorEnv(num_envs=n, **common, **kw)
    return e


def stagger(e, n):
    st = e.get_state()
    st[37] = np.arange(n) % (e.ep_len + 1)
    e.set_state(st)


def counters(e):
    d = e.state_dict()
    return d["step_index"], d["reset_calls"], d["episodes"], d["resamples"]


def same(a, b):
    """bit for bit (NaN-safe: the bytes are compared)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Flight(object):
    """An env with its device buffers; step() returns everything the launch wrote, as host arrays."""

    def __init__(self, n, kw, env, extras, sweep):
        import torch
        self.e = make(n, kw, env, "swarm" in extras, sweep)
        self.n, self.extras = n, extras
        dev = torch.device("cuda", 0)
        D = self.e.obs_dim
        self.obs = torch.zeros((n, D), device=dev)
        self.rew = torch.zeros(n, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.rows = None
        if "rows" in extras:
            self.rows = torch.zeros((n, D + 2), device=dev)
            self.e.set_packed_rows(self.rows)
        self.e.reset_dev(self.obs)
        stagger(self.e, n)

    def step(self, a):
        self.e.step_dev(a, self.obs, self.rew, self.done)
        out = {"obs": self.obs.cpu().numpy(), "reward": self.rew.cpu().numpy(), "done": self.done.cpu().numpy()}
        out["state"] = self.e.get_state()
        si, rc, ep, rs = counters(self.e)
        out["counters"] = np.array([si, rc], dtype=np.uint64)
        if ep is not None:
            out["episodes"], out["resamples"] = ep, rs
        if self.rows is not None:
            out["rows"] = self.rows.cpu().numpy()
        if "term" in self.extras:
            d = out["done"].astype(bool)
            out["terminal_obs"] = self.e._term_buf.cpu().numpy()[d]
        if "done_list" in self.extras:
            out["done_list"] = self.e.done_indices()          # (sorted: a set)
        return out

    def close(self):
        self.e.close()


def swarm_size(n):
    return max(8, (n + 7) // 8 * 8)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_alternating_sweep_changes_no_bit(case, n):
    import torch
    kw, env, extras = CASES[case]
    if "swarm" in extras:
        n = swarm_size(n)
    asc, alt = Flight(n, kw, env, extras, 0), Flight(n, kw, env, extras, 1)
    try:
        v = alt.e.launch_variant
        assert v == asc.e.launch_variant                      # GAQ_SWEEP takes no part in the kernel selection
        if case in ("alias_20", "alias_148"):
            assert (v & ~F_PREDRAW) == 20 and bool(v & F_PREDRAW) == (case == "alias_148"), v
        if case == "packed_rows":
            assert v & F_ROWS, v
        if case == "sense_noise_pack":
            assert v & F_PACK, v
        if case == "generic":
            assert v & F_GENERIC, v
        gen = torch.Generator(device=self_device()); gen.manual_seed(7)
        actions = torch.rand((STEPS, n, 4), device=self_device(), generator=gen) * 2 - 1
        assert same(asc.obs.cpu().numpy(), alt.obs.cpu().numpy()) and same(asc.e.get_state(), alt.e.get_state())
        finished = 0
        for t in range(STEPS):
            a, b = asc.step(actions[t]), alt.step(actions[t])
            assert a.keys() == b.keys()
            for k in a:
                assert same(a[k], b[k]), "%s, N = %d, step %d: %s differs between the ascending and the alternating sweep" % (case, n, t, k)
            assert int(a["counters"][0]) == t + 1
            finished += int(a["done"].sum())
            if "done_list" in extras:
                assert same(a["done_list"], np.flatnonzero(a["done"]).astype(np.uint32)), t
        assert finished >= n, "every env ends an episode within the six steps: resets in every block"
    finally:
        asc.close(); alt.close()


def self_device():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.parametrize("case,n", [("shadow", 4609), ("plain_4", 4609), ("alias_20", 4609), ("alias_by_size", 833)])
def test_a_captured_step_alternates_with_the_device_counter(case, n):
    """Graph-safe mode: ONE captured step launch, replayed 6 times (step indices 1 .. 6), equals 6 eager steps of an ascending handle.  The
    kernels without an F_CTR twin (plain, the alias kernel <20> forced with GAQ_NT=0) take the step index -- and with it the sweep's
    direction -- from the device counter with a scalar load: nothing in the graph's arguments changes from replay to replay.  The F_CTR
    twins (of the non-temporal small-batch forms the size rule picks for shadow and alias handles) keep the ascending order."""
    import torch
    kw, env, _ = CASES["alias_20"] if case == "alias_by_size" else CASES[case]
    if case == "alias_by_size":
        env = {}
    dev = self_device()
    asc, alt = Flight(n, kw, env, (), 0), Flight(n, kw, env, (), 1)
    try:
        alt.e.set_graph_safe(True)
        twin = bool(alt.e.launch_variant & F_CTR)
        assert twin == bool(alt.e.kernel_variant & F_NT), alt.e.launch_variant      # (the twins are those of the non-temporal small-batch forms)
        assert not (twin and case in ("plain_4", "alias_20")), (case, alt.e.launch_variant)
        gen = torch.Generator(device=dev); gen.manual_seed(9)
        actions = torch.rand((n, 4), device=dev, generator=gen) * 2 - 1
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):          # one step outside the capture: from here on the state heads are read where this step wrote them
            alt.e.step_dev(actions, alt.obs, alt.rew, alt.done)
        torch.cuda.current_stream().wait_stream(s)
        asc.e.step_dev(actions, asc.obs, asc.rew, asc.done)
        torch.cuda.synchronize()
        assert same(asc.obs.cpu().numpy(), alt.obs.cpu().numpy())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            alt.e.step_dev(actions, alt.obs, alt.rew, alt.done)
        for t in range(STEPS):
            graph.replay()
            torch.cuda.synchronize()
            asc.e.step_dev(actions, asc.obs, asc.rew, asc.done)
            torch.cuda.synchronize()
            for k, x, y in (("obs", asc.obs, alt.obs), ("reward", asc.rew, alt.rew), ("done", asc.done, alt.done)):
                assert same(x.cpu().numpy(), y.cpu().numpy()), "%s, N = %d, replay %d: %s" % (case, n, t, k)
        assert same(asc.e.get_state(), alt.e.get_state())
        assert counters(alt.e)[0] == STEPS + 1 == counters(asc.e)[0]
    finally:
        asc.close(); alt.close()


@pytest.mark.parametrize("n", [65, 833, 4609])
def test_a_reversed_partial_block_writes_nothing_behind_its_arrays(n):
    """N = 65: two tiles in one block whose waves 2 and 3 have no tile, and the second tile holds one env.  N = 833, 4609: the same partial block
    behind 3 and 18 full ones; of the 19, workgroup 2 takes it on odd steps.  The observation (= state heads), reward and done arrays each end
    in a guard band; after odd (descending) and even steps the bands are what they were."""
    import torch
    from tests.test_plan_cpu import base_cfg
    guard = 4096
    lib = _lib.load()
    dev = self_device()
    cfg = base_cfg(n, obs_state_alias=1, auto_reset=1, noise=1)
    h = C.c_void_p()
    with environ(GAQ_SWEEP="1"):
        _lib.check(lib.gaq_create(C.byref(cfg), C.byref(h)))
    try:
        assert lib.gaq_obs_dim(h) == 18
        obs_all = torch.full((n * 18 + guard,), -7.25, device=dev)
        rew_all = torch.full((n + guard,), -7.25, device=dev)
        done_all = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev)
        obs, rew, done = obs_all[:n * 18], rew_all[:n], done_all[:n]
        act = torch.zeros((n, 4), device=dev)
        _lib.check(lib.gaq_reset_dev(h, None, _lib.ptr(obs), None))
        for t in range(4):
            _lib.check(lib.gaq_step_dev(h, _lib.ptr(act), _lib.ptr(obs), _lib.ptr(rew), _lib.ptr(done), None))
            torch.cuda.synchronize()
            assert bool((obs_all[n * 18:] == -7.25).all()) and bool((rew_all[n:] == -7.25).all()) and bool((done_all[n:] == 0xA5).all()), t
            assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all()) and bool((done <= 1).all()), t
    finally:
        lib.gaq_destroy(h)
