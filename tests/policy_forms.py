"""Closed-loop rollouts (csrc/gaq_policy.hip rollout_plan / rollout_run) in every form the four entry points can take: one scenario per
(batch size, actor, where V comes from, normaliser, outputs asked for, window split, entry point, fused or two-launch critic) that resets
a fresh handle, runs 8 steps at ep_time = 0.05 (episodes end every few steps) and returns every array the calls wrote, the recurrent
states afterwards, and -- where there is a critic -- values_dev of the recorded rows.  (logp_dev of the recorded rows is not here: it
recomputes z from the rounded action, so it equals the rollout's logp to a tolerance, which tests/test_gpu_policy_grad.py holds it to.)  Which launches a call makes, with which LDS size and which weights offset, is chosen per call from the handles and the outputs
asked for; whatever is chosen, the arrays a narrower call also writes have to be that call's bits.  tests/test_gpu_policy_forms.py
asserts those identities; `python -m tests.policy_forms` prints a hash per (case, array), for comparing two builds of the library (GAQ_LIB).

The shapes are the smallest at which a wrong choice still shows: N = 1 (a single lane) and 65 (a ragged second tile); one hidden layer
of 16, except where the LDS of the fused actor + critic launch is sized by the wider of the two ([48, 256] beside [16], [16] beside
[256, 48]).  The observation has 20 floats (the 18 of the default plus thrust-to-weight and thrust-to-torque): a call of more than one
step needs N * obs_dim * 4 to be a multiple of 16, which 18 floats do not give at N = 1 or 65."""
import collections
import contextlib
import functools
import hashlib

import numpy as np

from gym_art_amd import _lib
from tests.policy_util import environ

T = 8
SPLIT = (3, 5)
SIZES = (1, 65)
SEED = 23
OBS_REPR = "xyz_vxyz_R_omega_t2w_t2t"
LOG_STD = np.asarray([-0.7, -0.9, -1.1, -0.5], np.float32)

# name: (kind, engine or cell units, hidden widths of the MLP / of the head behind the cell)
ACTORS = {"valu16": ("mlp", "valu", [16]), "bf16_32": ("mlp", "bf16", [32]), "mfma16": ("mlp", "mfma", [16]),
          "mfma48x256": ("mlp", "mfma", [48, 256]), "gru16": ("gru", 16, []), "lstm16_32": ("lstm", 16, [32])}
AC_ACTORS = ("mfma16", "mfma48x256", "gru16", "lstm16_32")          # the ones with values and log-probabilities
CRITICS = {"c16": [16], "c256x48": [256, 48]}
# the fused launch's LDS: the critic wider than the actor, the actor wider than the critic; then the recurrent actors (two launches)
PAIRS = (("mfma16", "c256x48"), ("mfma48x256", "c16"), ("gru16", "c16"), ("lstm16_32", "c256x48"))

# source: "none" (no V), "head" (the policy's value head) or a critic's name; norm: "none", "actor" (an ObsNorm on the actor only) or
# "both" (one on actor and critic); ask: the outputs besides obs / rew / done / actions, of "v" (values), "l" (logp), "t" (term_values);
# calls: the window as consecutive calls; entry: "py" (rollout_policy_dev's choice), "ac_term" / "critic" (that entry point through
# ctypes, its further arguments null); fused: the critic created without GAQ_NO_FUSED_CRITIC=1
Case = collections.namedtuple("Case", "n actor source norm ask calls entry fused", defaults=("none", "none", "", (T,), "py", True))


def plain(case):
    """the plain entry point's call of a case: same batch, actor, actor normaliser and split, nothing else asked for"""
    return Case(case.n, case.actor, norm="none" if case.norm == "none" else "actor", calls=case.calls)


def _cases():
    asked = [Case(n, a, "head", ask="vlt") for n in SIZES for a in AC_ACTORS]
    asked += [Case(65, "mfma16", "head", ask="v"), Case(65, "mfma16", ask="l"), Case(65, "gru16", "head", ask="vl")]
    paired = [Case(n, a, c, ask="vlt") for n in SIZES for a, c in PAIRS]
    normed = [Case(n, "mfma16", "c256x48", norm, "vlt") for n in SIZES for norm in ("both", "actor")]
    normed += [Case(65, "mfma48x256", "c16", "both", "vlt"), Case(65, "gru16", "c16", "both", "vlt"), Case(65, "lstm16_32", "head", "actor", "vlt")]
    wide = [Case(65, a, entry=e) for a in ACTORS for e in ("ac_term", "critic")] + [Case(1, "mfma16", entry=e) for e in ("ac_term", "critic")]
    wide += [Case(n, a, "head", ask="vl", entry="ac_term") for n in SIZES for a in AC_ACTORS]
    wide += [Case(n, a, "head", ask="vlt", entry="critic") for n in SIZES for a in AC_ACTORS]
    split = [Case(65, a, calls=SPLIT) for a in ACTORS] + [Case(65, a, "head", ask="vlt", calls=SPLIT) for a in AC_ACTORS]
    split += [Case(65, a, c, ask="vlt", calls=SPLIT) for a, c in PAIRS] + [Case(65, "mfma16", "c256x48", "both", "vlt", SPLIT)]
    split += [Case(1, "gru16", "head", ask="vlt", calls=SPLIT), Case(1, "mfma16", "c256x48", ask="vlt", calls=SPLIT)]
    return dict(asked=asked, paired=paired, normed=normed, wide=wide, split=split)


CASES = _cases()
UNFUSED = [c._replace(fused=False) for c in CASES["paired"] + CASES["normed"] if c.source in CRITICS]


def _layers(dims, seed):
    rng = np.random.RandomState(seed)
    return [((rng.randn(o, i) / np.sqrt(i)).astype(np.float32), (0.1 * rng.randn(o)).astype(np.float32)) for i, o in zip(dims[:-1], dims[1:])]


def _actor(env, name, source, norm):
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPPolicy
    kind, arg, widths = ACTORS[name]
    seed = 100 + sorted(ACTORS).index(name)
    rng = np.random.RandomState(seed + 50)
    last = (widths or [arg])[-1]
    value = ((np.random.RandomState(seed + 90).randn(last) / np.sqrt(last)).astype(np.float32), np.float32(0.05)) if source == "head" else None
    if kind == "mlp":
        pol = MLPPolicy.from_arrays(env, _layers([env.obs_dim] + widths + [4], seed), "tanh", True, log_std=LOG_STD, engine=arg, value=value)
    else:
        G, H = (3, arg) if kind == "gru" else (4, arg)
        cell = ((rng.randn(G * H, env.obs_dim) / 4).astype(np.float32), (rng.randn(G * H, H) / 4).astype(np.float32),
                (0.1 * rng.randn(G * H)).astype(np.float32), (0.1 * rng.randn(G * H)).astype(np.float32))
        pol = (GRUPolicy if kind == "gru" else LSTMPolicy)(env, cell, _layers([H] + widths + [4], seed), "relu", True, log_std=LOG_STD, value=value)
    if norm is not None:
        pol.set_obs_norm(norm)
    return pol


def _critic(env, name, norm, fused):
    from gym_art_amd.policy import MLPCritic
    with contextlib.nullcontext() if fused else environ(GAQ_NO_FUSED_CRITIC="1"):      # (read at create)
        crit =MLPCritic.from_arrays(env, _layers([env.obs_dim] + CRITICS[name] + [1], 300 + len(name)), "tanh")
    if norm is not None:
        crit.set_obs_norm(norm)
    return crit


def _call(env, pol, crit, entry, steps, ask):
    """one call of `steps` steps -> {name: tensor}"""
    import torch
    n, dev = env.num_envs, torch.device("cuda", env.device)
    out = dict(obs=torch.empty((steps, n, env.obs_dim), device=dev), rew=torch.empty((steps, n), device=dev),
               done=torch.empty((steps, n), dtype=torch.uint8, device=dev), actions=torch.empty((steps, n, 4), device=dev))
    # (filled with NaN: a row the call should have written and did not cannot pass for one it did)
    if "v" in ask:
        out["values"] = torch.full((steps + 1, n), float("nan"), device=dev)
    if "l" in ask:
        out["logp"] = torch.full((steps, n), float("nan"), device=dev)
    if "t" in ask:
        out["term_values"] = torch.full((steps, n), float("nan"), device=dev)
    v, lp, tv = out.get("values"), out.get("logp"), out.get("term_values")
    if entry == "py":
        env.rollout_policy_dev(pol, out["obs"], out["rew"], out["done"], out["actions"], values=v, logp=lp, term_values=tv, critic=crit)
        return out
    common = (steps, _lib.ptr(out["obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["done"]), _lib.ptr(out["actions"]), _lib.ptr(v), _lib.ptr(lp))
    if entry == "ac_term":
        assert crit is None
        _lib.check(env._lib.gaq_step_policy_ac_term_many_dev(env._handle, pol.handle, *common, _lib.ptr(tv), env._stream(out["obs"])))
    else:
        _lib.check(env._lib.gaq_step_policy_critic_many_dev(env._handle, pol.handle, None if crit is None else crit.handle, *common,
                                                            _lib.ptr(tv), env._stream(out["obs"])))
    env._obs_ref = out["obs"]                                         # (what rollout_policy_dev does: the next call reads its last row)
    return out


@functools.lru_cache(maxsize=None)   # (a case is a few KB)
def scenario(case):
    """{name: array} of one Case.  Read-only for the callers."""
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import ObsNorm
    env = QuadrotorEnv(num_envs=case.n, ep_time=0.05, seed=SEED, obs_repr=OBS_REPR, auto_reset=True)    # (a single env does not reset itself by default)
    assert env.obs_dim == 20
    rng = np.random.RandomState(7)
    norm = None if case.norm == "none" else ObsNorm.from_stats(env, 0.2 * rng.randn(env.obs_dim), rng.uniform(0.5, 2.0, env.obs_dim), count=100.0)
    pol = _actor(env, case.actor, case.source, norm)
    crit = _critic(env, case.source, norm if case.norm == "both" else None, case.fused) if case.source in CRITICS else None
    o0 = torch.empty((case.n, env.obs_dim), device=torch.device("cuda", env.device))
    env.reset_dev(o0)
    o0 = o0.clone()
    calls = [_call(env, pol, crit, case.entry, steps, case.ask) for steps in case.calls]
    torch.cuda.synchronize()
    t = {k: torch.cat([c[k] for c in calls]) for k in calls[0] if k != "values"}
    if "v" in case.ask:
        # every call's rows but its bootstrap row, then the last call's; the seams: a call's bootstrap row beside the next call's row 0
        t["values"] = torch.cat([c["values"][:-1] for c in calls] + [calls[-1]["values"][-1:]])
        if len(calls) > 1:
            t["seam_boot"] = torch.stack([c["values"][-1] for c in calls[:-1]])
            t["seam_next"] = torch.stack([c["values"][0] for c in calls[1:]])
    if crit is not None and "v" in case.ask:
        t["values_dev"] = crit.values_dev(torch.cat([o0[None], t["obs"]]))     # the observation row t of values was computed from
    for name in (pol.CELL.states if hasattr(pol, "CELL") else ()):      # a recurrent policy's states after the window
        t[name] = getattr(pol, name)
    torch.cuda.synchronize()
    out = {"obs0": o0.cpu().numpy(), **{k: v.cpu().numpy() for k, v in t.items()}}
    for x in (crit, pol, norm, env):
        if x is not None:
            x.close()
    for v in out.values():
        v.setflags(write=False)
    return out


if __name__ == "__main__":
    every = [plain(c) for cs in CASES.values() for c in cs] + [c for cs in CASES.values() for c in cs] + UNFUSED
    for case_ in sorted(set(every)):
        for name_, a_ in sorted(scenario(case_).items()):
            print("%-90s %-12s %s" % (" ".join(str(f) for f in case_), name_, hashlib.sha256(np.ascontiguousarray(a_).tobytes()).hexdigest()[:32]))
