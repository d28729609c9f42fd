"""Helpers shared by the device-policy tests: random layers and _ex descriptions for the host-side files, and for the GPU files a torch
net, the rollout buffers, one closed-loop rollout and the open-loop replay of its actions."""
import contextlib
import ctypes as C
import os

import numpy as np


def _layers(widths, D=18, seed=0):
    rng = np.random.RandomState(seed)
    dims = [D] + list(widths) + [4]
    return [(rng.randn(dims[k + 1], dims[k]).astype(np.float32), rng.randn(dims[k + 1]).astype(np.float32)) for k in range(len(dims) - 1)]


def _desc_ex(widths, engine, in_dim=18):
    from gym_art_amd.policy import ENGINES, _DescEx
    d = _DescEx()
    d.struct_size = C.sizeof(_DescEx)
    d.in_dim, d.n_hidden = in_dim, len(widths)
    for k, w in enumerate(widths[:3]):
        d.width[k] = w
    d.engine = ENGINES[engine] if isinstance(engine, str) else engine
    return d


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _dev():
    import torch
    return torch.device("cuda", 0)


def _net(widths, act="tanh", out_tanh=True, D=18, seed=0):
    import torch
    nn = torch.nn
    torch.manual_seed(seed)
    mods, prev = [], D
    for w in widths:
        mods += [nn.Linear(prev, w), nn.Tanh() if act == "tanh" else nn.ReLU()]
        prev = w
    mods.append(nn.Linear(prev, 4))
    if out_tanh:
        mods.append(nn.Tanh())
    return nn.Sequential(*mods)


def _bufs(env, T_):
    import torch
    n, dev = env.num_envs, _dev()
    return (torch.empty((T_, n, env.obs_dim), device=dev), torch.empty((T_, n), device=dev),
            torch.empty((T_, n), dtype=torch.uint8, device=dev), torch.empty((T_, n, 4), device=dev))


def _closed_loop(env, policy, T_):
    """reset_dev, then one closed-loop rollout: (obs0, obs, rew, done, actions)"""
    import torch
    o0 = torch.empty((env.num_envs, env.obs_dim), device=_dev())
    env.reset_dev(o0)
    o0c = o0.clone()
    o, r, d, a = _bufs(env, T_)
    env.rollout_policy_dev(policy, o, r, d, a)
    torch.cuda.synchronize()
    return o0c, o, r, d, a


def _replay(env, actions):
    import torch
    o0 = torch.empty((env.num_envs, env.obs_dim), device=_dev())
    env.reset_dev(o0)
    o, r, d, _ = _bufs(env, actions.shape[0])
    env.step_many_dev(actions, o, r, d)
    torch.cuda.synchronize()
    return o, r, d
