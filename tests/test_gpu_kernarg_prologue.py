"""-m gpu: the step kernels' opening (gaq_kernels.hpp kernarg_warm / kernarg_batch: every argument line requested at entry, one wait
before the first state load) at the tile and block edges and in the three counter modes -- sizes the workload never runs at.

  N = 1, 64, 65, 257   a partial tile; waves of the last (only) block that find no tile and leave through the early exit
  N = 4097             65 tiles: a second..17th block, the last with one tile and three waves without
  layouts              alias (heads in the caller's tensor), shadow (library-owned heads), plain (fp64 planes)
  modes                eager (host step index); graph-safe: one eager step, THREE steps captured in one HIP graph and replayed twice,
                       then three eager steps in graph-safe mode -- at these sizes the alias / shadow handles launch the self-counting
                       twin (F_CTR: the exit path checks in too), the plain handle the bump launch behind the step

Check 1: all ten steps are bit-equal (obs, reward, done) to envs [0, N) of an 8192-env handle with the same seed (RNG keyed by the global
env index: test_gpu_properties.py's shard invariance), thrust noise on, episodes of five steps so that in-kernel resets fall inside.
Check 2: a canary region behind obs, reward and done is untouched.
The reference runs once per layout and is shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_REF, STEPS, F_CTR = 8192, 10, 8192
# ep_len 5: every env is reset in the kernel twice inside the ten steps.  info=False: the class turns the info dict on for a single env,
# which selects the packed-observation kernels (observation rounded to nearest instead of the truncated heads): another output; and it
# leaves a single env's reset to the caller, so auto_reset is asked for
KW = dict(ep_time=0.05, seed=11, info=False, auto_reset=True)
LAYOUTS = {"alias": True, "shadow": None, "plain": False}
CANARY = 4096                                             # elements behind each output
SENTINEL_F, SENTINEL_B = 12345.678, 0xA5


@functools.lru_cache(maxsize=None)
def _actions():
    import torch
    gen = torch.Generator(device="cuda"); gen.manual_seed(77)
    return torch.rand((STEPS, N_REF, 4), device="cuda", generator=gen) * 2 - 1


@functools.lru_cache(maxsize=None)
def _reference(layout):
    """(reset obs, [STEPS] obs, reward, done) of the 8192-env handle, on the device; never modified afterwards."""
    import torch
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(num_envs=N_REF, alias_obs=LAYOUTS[layout], **KW)
    assert env.ep_len == 5
    o = torch.empty((N_REF, 18), device="cuda"); r = torch.empty(N_REF, device="cuda"); d = torch.empty(N_REF, dtype=torch.uint8, device="cuda")
    env.reset_dev(o)
    o0 = o.clone()
    obs, rew, done = [], [], []
    for t in range(STEPS):
        env.step_dev(_actions()[t], o, r, d)
        obs.append(o.clone()); rew.append(r.clone()); done.append(d.clone())
    torch.cuda.synchronize()
    env.close()
    assert int(torch.stack(done).sum().item()) >= N_REF       # resets happened
    return o0, torch.stack(obs), torch.stack(rew), torch.stack(done)


class _Outputs(object):
    """obs / reward / done of an n-env handle, each the front of a larger allocation whose tail is the canary."""

    def __init__(self, n):
        import torch
        self.n = n
        self.ob = torch.full((n * 18 + CANARY,), SENTINEL_F, device="cuda")
        self.rb = torch.full((n + CANARY,), SENTINEL_F, device="cuda")
        self.db = torch.full((n + CANARY,), SENTINEL_B, dtype=torch.uint8, device="cuda")
        self.o, self.r, self.d = self.ob[:n * 18].view(n, 18), self.rb[:n], self.db[:n]

    def canary_intact(self):
        n = self.n
        return (bool((self.ob[n * 18:] == SENTINEL_F).all()) and bool((self.rb[n:] == SENTINEL_F).all())
                and bool((self.db[n:] == SENTINEL_B).all()))


def _same(out, ref, t, n):
    import torch
    _, obs, rew, done = ref
    return torch.equal(out.o, obs[t, :n]) and torch.equal(out.r, rew[t, :n]) and torch.equal(out.d, done[t, :n])


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("n", [1, 64, 65, 257, 4097])
def test_prologue_at_tile_and_block_edges(n, layout):
    import torch
    from gym_art_amd import QuadrotorEnv
    ref = _reference(layout)
    acts = _actions()[:, :n].contiguous()

    # eager
    env, out = QuadrotorEnv(num_envs=n, alias_obs=LAYOUTS[layout], **KW), _Outputs(n)
    env.reset_dev(out.o)
    torch.cuda.synchronize()
    assert torch.equal(out.o, ref[0][:n])
    for t in range(STEPS):
        env.step_dev(acts[t], out.o, out.r, out.d)
        torch.cuda.synchronize()
        assert _same(out, ref, t, n), ("eager", t)
    assert out.canary_intact(), "eager"
    env.close()

    # graph-safe: 1 eager step, 3 captured steps replayed twice, 3 eager steps
    env, out = QuadrotorEnv(num_envs=n, alias_obs=LAYOUTS[layout], **KW), _Outputs(n)
    env.reset_dev(out.o)
    env.set_graph_safe(True)
    if layout != "plain":
        assert env.launch_variant & F_CTR, "the size rule picks the self-counting twin at this size"
    a_g = torch.empty((3, n, 4), device="cuda")
    keep = [_Outputs(n) for _ in range(3)]                   # what each captured step handed out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step_dev(acts[0], out.o, out.r, out.d)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same(out, ref, 0, n), ("graph-safe, eager", 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(3):
            env.step_dev(a_g[k], out.o, out.r, out.d)
            keep[k].o.copy_(out.o); keep[k].r.copy_(out.r); keep[k].d.copy_(out.d)
    for rep in range(2):
        t0 = 1 + 3 * rep
        a_g.copy_(acts[t0:t0 + 3])
        g.replay()
        torch.cuda.synchronize()
        for k in range(3):
            assert _same(keep[k], ref, t0 + k, n), ("replay", rep, k)
    for t in range(7, STEPS):
        env.step_dev(acts[t], out.o, out.r, out.d)
        torch.cuda.synchronize()
        assert _same(out, ref, t, n), ("graph-safe, eager", t)
    assert out.canary_intact() and all(k.canary_intact() for k in keep), "graph-safe"
    del g
    env.close()
