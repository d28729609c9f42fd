"""The host-pointer step (csrc/gaq.hip gaq_step) on each of its three transports -- mapped host memory, a pinned mirror with copies
(GAQ_ZERO_COPY=0), pageable copies above the 1 MiB stage -- beside the device-pointer step: one scenario per (batch size, configuration,
transport) that resets a handle, gives it the same 25 actions (ep_time = 0.05: every env is auto-reset four times inside the window) and
returns what came back, the state planes and aux rows read afterwards (on the staged transports of an info handle: from the info
mirror), and the same two read again after observe().  gaq_step is the launch of gaq_step_dev plus a transport, so every transport has
to return the bits of the "dev" twin.  tests/test_gpu_host_transports.py asserts that; `python -m tests.host_transports` prints a hash
per array, for comparing two builds of the library (GAQ_LIB)."""
import functools
import hashlib
import os

import numpy as np

from gym_art_amd import _lib

STEPS = 25
# the stage is round16(21 N) + 4 D N bytes: with an 18-word observation 11274 envs are the last that fit 1 MiB, 11275 the first that do not
STAGED_SIZES = (1, 65, 11274)   # a single lane; a ragged second tile; the last staged size
PAGEABLE_SIZE = 11275
LAYOUTS = {"default": {}, "alias": dict(alias_obs=True), "planes": dict(alias_obs=False)}   # shadow (the class default), alias proper, fp64 planes
CONFIGS = dict(LAYOUTS, mellinger_info=dict(raw_control=False, info=True), info=dict(info=True), planes_info=dict(alias_obs=False, info=True))
STAGED_CASES = [(n, c) for n in STAGED_SIZES for c in LAYOUTS] + [(n, c) for n in (1, 65) for c in ("mellinger_info", "planes_info")]
PAGEABLE_CASES = [(PAGEABLE_SIZE, c) for c in (*LAYOUTS, "info")]
SEED = 23


def make(n, config):
    from gym_art_amd import QuadrotorEnv
    return QuadrotorEnv(num_envs=n, ep_time=0.05, seed=SEED, **CONFIGS[config])


def actions(n):
    rng = np.random.RandomState(4)
    return [rng.uniform(-1, 1, (n, 4)).astype(np.float32) for _ in range(STEPS)]


def aux_rows(env):
    aux = np.empty((env.num_envs, _lib.AUX_WORDS), dtype=np.float32)
    _lib.check(env._lib.gaq_get_aux(env._handle, _lib.ptr(aux)))
    return aux


def flatten_info(info):
    """{"info/<key>/<entry>": array} of an info dict"""
    return {"info/%s/%s" % (k, q): np.asarray(x) for k, v in info.items() for q, x in v.items()}


class zero_copy_off:
    """GAQ_ZERO_COPY=0 while a handle is made and steps (the library reads it in the handle's first gaq_step)"""
    def __enter__(self):
        os.environ["GAQ_ZERO_COPY"] = "0"

    def __exit__(self, *exc):
        os.environ.pop("GAQ_ZERO_COPY", None)


def _readings(env, info, out):
    """state and aux rows now; then observe() -- a launch on the planes layout, which drops the info mirror; a read of the heads on the
    split layouts -- and both again"""
    out["state"] = env.get_state()
    if info:
        out["aux"] = aux_rows(env)
    out["observed"] = np.asarray(env.observe(), np.float32).reshape(env.num_envs, -1)
    out["state_after_observe"] = env.get_state()
    if info:
        out["aux_after_observe"] = aux_rows(env)


def _host(n, config):
    """step() on NumPy arrays; obs as float32 [n, D], reward float32 [n], done bool [n] whatever the single-env call shapes are"""
    acts = actions(n)
    out = {}
    env = make(n, config)
    info = env._info                     # (a single env builds its info dict by default)
    out["reset_obs"] = np.asarray(env.reset(), np.float32).reshape(n, -1)
    obs, rew, done = [], [], []
    for a in acts:
        o, r, d, last = env.step(a[0] if n == 1 else a)
        obs.append(np.asarray(o, np.float32).reshape(n, -1)); rew.append(np.asarray(r, np.float32).reshape(n)); done.append(np.asarray(d, bool).reshape(n))
    out["obs"], out["reward"], out["done"] = np.stack(obs), np.stack(rew), np.stack(done)
    if info:
        out.update(flatten_info(last))
    _readings(env, info, out)
    env.check_finite()
    env.close()
    return out


def _dev(n, config):
    """the twin: the same handle stepped through gaq_step_dev on device tensors (the class's torch path with out=)"""
    import torch
    dev = torch.device("cuda", 0)
    acts = actions(n)
    out = {}
    env = make(n, config)
    info = env._info                     # (a single env builds its info dict by default)
    obs = torch.empty((n, env.obs_dim), device=dev); rew = torch.empty(n, device=dev); done = torch.empty(n, dtype=torch.uint8, device=dev)
    env.reset_dev(obs)
    out["reset_obs"] = obs.cpu().numpy()
    o_, r_, d_ = [], [], []
    for a in acts:
        env.step(torch.from_numpy(a).to(dev), out=(obs, rew, done))       # (alias layouts: `obs` is the state's heads, the same tensor every step)
        o_.append(obs.cpu().numpy()); r_.append(rew.cpu().numpy()); d_.append(done.cpu().numpy().astype(bool))
    out["obs"], out["reward"], out["done"] = np.stack(o_), np.stack(r_), np.stack(d_)
    if info and n > 1:
        # the info dict of the last step as the NumPy path builds it, from THIS handle's device state and aux rows (the torch path keeps
        # no action history: hand it the two actions the dict reads)
        env.actions = [acts[-1].astype(np.float64), acts[-2].astype(np.float64)]
        out.update(flatten_info(env._make_info(acts[-1], r_[-1])))
    _readings(env, info, out)
    env.check_finite()
    env.close()
    return out


@functools.lru_cache(maxsize=8)      # (a case's transports and its twin are asked for together; the big cases hold 20 MB each)
def scenario(n, config, transport):
    """{name: array}; transport: "mapped" / "pinned" (staged sizes), "pageable" (larger ones), "dev" (the twin).  Read-only for the callers."""
    assert (transport == "pageable") == (n >= PAGEABLE_SIZE) or transport == "dev"
    if transport == "pinned":
        with zero_copy_off():
            out = _host(n, config)
    else:
        out = _dev(n, config) if transport == "dev" else _host(n, config)
    for v in out.values():
        v.setflags(write=False)
    return out


if __name__ == "__main__":
    def digest(arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()[:32]
    for n_, config_ in STAGED_CASES + PAGEABLE_CASES:
        for transport_ in (("pageable",) if n_ >= PAGEABLE_SIZE else ("mapped", "pinned")) + ("dev",):
            sc_ = scenario(n_, config_, transport_)
            lines = {k: digest([v]) for k, v in sc_.items() if not k.startswith("info/")}
            if any(k.startswith("info/") for k in sc_):
                lines["info/*"] = digest(sc_[k] for k in sorted(sc_) if k.startswith("info/"))     # the dict's entries, in the order of their names
            for name_, hash_ in sorted(lines.items()):
                print("%5d %-14s %-8s %-20s %s" % (n_, config_, transport_, name_, hash_))
