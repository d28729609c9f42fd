"""The passes of the per-env parameter pipeline (csrc/gaq_params.hip) side by side: one scenario per (batch size, sampler) that brings
several handles to the SAME draw of every env by different passes -- redrawn now (gaq_randomize_dev), rebuilt from the counts
(gaq_set_counters), promoted by the step launches and refilled (dynamics_randomize_every = 1), read through the rows pass
(gaq_get_params after hot-planes-only promotions), caught up (the parameter flags change under the live randomizer), derived from the
trees read back (gaq_get_param_trees -> gaq_set_param_trees) -- and returns what each of them holds.  tests/test_gpu_param_passes.py
asserts that they are the same bits; `python -m tests.param_passes` prints a hash per array, for comparing two builds of the library
(GAQ_LIB)."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np

from gym_art_amd import _lib

SIZES = (1, 65, 257)            # a single lane; a ragged second tile; a second workgroup that holds one env
KINDS = ("relative", "randomquad")
DRAWS = 3                       # k: redraws of handle A = finished episodes of the stepping handle
SAMPLER = {"class": "RelativeSampler", "noise_ratio": 0.2, "sampler": "normal"}


def make(n, kind):
    from gym_art_amd import QuadrotorEnv
    kw = dict(num_envs=n, ep_time=0.05, seed=13, dynamics_randomize_every=1, randomize_on_device=True, auto_reset=True)   # six steps an episode
    if kind == "randomquad":
        return QuadrotorEnv(dynamics_params="RandomQuad", **kw)
    return QuadrotorEnv(dynamics_params="Crazyflie", dyn_sampler_1=dict(SAMPLER), **kw)


def rows(env):
    out = np.empty((env.num_envs, _lib.MODEL_DOUBLES), dtype=np.float64)
    _lib.check(env._lib.gaq_get_params(env._handle, _lib.ptr(out), 0, env.num_envs))
    return out


def counters(env):
    cnt = _lib.GaqCounters()
    ep, rc = np.empty(env.num_envs, np.uint32), np.empty(env.num_envs, np.uint32)
    _lib.check(env._lib.gaq_get_counters(env._handle, C.byref(cnt), _lib.ptr(ep), _lib.ptr(rc)))
    return cnt, ep, rc


def randomizer_of(env, kind):
    """the gaq_randomizer the class installed at construction"""
    from gym_art_amd import quad_params as qp
    base = env.dynamics_params_batched
    rz = _lib.GaqRandomizer()
    rz.every = 1
    if kind == "randomquad":
        rz.sampler = 2
    else:
        rz.sampler = 0
        rz.ratio[:] = list(qp.ratio_rows(base, SAMPLER["noise_ratio"], None)[0])
    C.memmove(C.byref(rz.base), qp.flatten_tree(base)[0].ctypes.data, C.sizeof(rz.base))
    return rz


@functools.lru_cache(maxsize=None)
def scenario(n, kind):
    """{name: array} of everything the passes left behind; read-only for the callers"""
    import torch
    from gym_art_amd import quad_params as qp
    dev = torch.device("cuda", 0)
    out = {}
    lib = _lib.load()
    # A: redrawn DRAWS times, now
    a = make(n, kind)
    _, _, rc0 = counters(a)
    for _ in range(DRAWS):
        _lib.check(lib.gaq_randomize_dev(a._handle, None, None))
    _lib.check(lib.gaq_synchronize(a._handle))
    out["redrawn"] = rows(a)
    cnt_a, ep_a, rc_a = counters(a)
    out["fresh_resamples"], out["redrawn_resamples"] = rc0, rc_a
    # B: a fresh handle given A's counters: rebuilt from the counts
    b = make(n, kind)
    _lib.check(lib.gaq_set_counters(b._handle, C.byref(cnt_a), _lib.ptr(ep_a), _lib.ptr(rc_a)))
    out["rebuilt"] = rows(b)
    # ... then one env of it redrawn: the last one (env 64 of 65: the only lane of the second tile)
    mask = np.zeros(n, np.uint8); mask[n - 1] = 1
    mask_dev = torch.as_tensor(mask, device=dev)
    _lib.check(lib.gaq_randomize_dev(b._handle, _lib.ptr(mask_dev), None))
    torch.cuda.synchronize()
    _lib.check(lib.gaq_synchronize(b._handle))
    out["rebuilt_masked_redraw"] = rows(b)
    # S: stepped until every env has finished DRAWS episodes; promoted in the step launches, staged planes from the refill pass
    s = make(n, kind)
    obs, rew, done = torch.empty((n, 18), device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    s.reset_dev(obs)
    gen = torch.Generator(device=dev); gen.manual_seed(3)
    for _ in range(DRAWS * (s.ep_len + 1)):
        s.step_dev(torch.rand((n, 4), device=dev, generator=gen) * 2 - 1, obs, rew, done)
    torch.cuda.synchronize()
    cnt_s, ep_s, rc_s = counters(s)
    out["stepped_resamples"] = rc_s
    out["stepped_models"] = _lib.models_to_rows(s.models)                    # (the class's read: gaq_get_params into its cache)
    state = s.get_state()
    out["stepped"] = rows(s)                                                 # the rows pass
    out["stepped_again"] = rows(s)
    cnt_2, ep_2, rc_2 = counters(s)
    out["stepped_state"], out["stepped_state_after_reads"] = state, s.get_state()
    out["stepped_counters"] = np.array([cnt_s.step_index, cnt_s.reset_calls], np.uint64)
    out["stepped_counters_after_reads"] = np.array([cnt_2.step_index, cnt_2.reset_calls], np.uint64)
    out["stepped_episodes"], out["stepped_episodes_after_reads"] = ep_s, ep_2
    out["stepped_resamples_after_reads"] = rc_2
    # ... the parameter flags change under the live randomizer (every plane is loaded now: a promotion moves all 45), and one step (of a
    # fresh episode: nobody finishes) brings the planes left behind by the hot-planes-only promotions up to date first
    rz = randomizer_of(s, kind)
    os.environ["GAQ_NO_COMPACT"] = "1"
    try:
        _lib.check(lib.gaq_set_randomizer(s._handle, C.byref(rz)))
    finally:
        os.environ.pop("GAQ_NO_COMPACT", None)
    s.step_dev(torch.rand((n, 4), device=dev, generator=gen) * 2 - 1, obs, rew, done)
    torch.cuda.synchronize()
    out["caught_up_done"] = done.cpu().numpy()
    out["caught_up"] = rows(s)
    out["caught_up_resamples"] = counters(s)[2]
    # F: a fresh handle given the trees of A's draws
    trees = np.empty((n, qp.TREE_DOUBLES), dtype=np.float64)
    _lib.check(lib.gaq_get_param_trees(a._handle, _lib.ptr(trees), 0, n))
    out["trees"] = trees
    f = make(n, kind)
    _lib.check(lib.gaq_set_param_trees(f._handle, _lib.ptr(trees), 1 if kind == "randomquad" else 0, 0, n))
    out["from_trees"] = rows(f)
    for env in (a, b, s, f):
        env.check_finite()
        env.close()
    for v in out.values():
        v.setflags(write=False)
    return out


def fields(rows_):
    """[N, MODEL_DOUBLES] -> {field of gaq_model: array}"""
    return _lib.rows_to_models(rows_)


if __name__ == "__main__":
    for n_ in SIZES:
        for kind_ in KINDS:
            for name_, arr_ in sorted(scenario(n_, kind_).items()):
                print("%4d %-10s %-30s %s" % (n_, kind_, name_, hashlib.sha256(np.ascontiguousarray(arr_).tobytes()).hexdigest()[:32]))
