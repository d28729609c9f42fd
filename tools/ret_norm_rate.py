#!/usr/bin/env python3
"""Return normalisation on one device: what RetNorm costs on a rollout's own rew / done tensors (alias layout, T = 64), against what a user
writes today and against the rollout it follows.
  update_dev        RetNorm.update_dev(rew, done): the streaming pass (5 B per env-step) + the merge launch
  update_normalize  update_dev, then normalize_dev(rew, out=rew) in place
  torch_loop        the yardstick: a torch loop over T on the same tensors -- ret = ret * gamma + rew[t], torch.var_mean of ret and Chan's
                    merge into fp64 running statistics (a torch RunningMeanStd), ret[done[t]] = 0 -- then rew * inv_std clamped in place
  rollout           one rollout_policy_dev of T steps with an 18-128-128-4 policy, for scale
Every batch size is a child process under a time limit of its own; the first one that fails or runs out of time ends the run (nothing
more is started on the device).  Warm-up, then ROUNDS rounds with the paths interleaved; each sample is a host clock around CALLS[path]
back-to-back calls ending in a device synchronise, in microseconds per call; median with min..max.  update_dev is also given as TB/s of
the bytes it has to move and as a fraction of the device's recorded copy rate (COPY_TBS, profiles/).
python3 tools/ret_norm_rate.py [OUT.json] [--sizes 1048576,65536]      (OUT defaults to profiles/rNN_ret_norm_rate.json, NN the next
free round prefix)"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, ROUNDS, D = 64, 7, 18
CALLS = {"update_dev": 10, "update_normalize": 10, "torch_loop": 1, "rollout": 1}
COPY_TBS = 6.3                                   # the device-to-device copy rate recorded in profiles/ (TB/s of bytes read)
STEP_LIMIT = 600                                 # seconds per child process


def stats(v):
    v = sorted(v)
    return {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2)}


def child(n):
    """--child N: one line of JSON with the samples of every path at batch size N"""
    sys.path.insert(0, ROOT)
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy, RetNorm
    dev, nn = torch.device("cuda", 0), torch.nn
    torch.manual_seed(0)
    env = QuadrotorEnv(num_envs=n, ep_time=5, seed=0, alias_obs=True)
    net = nn.Sequential(nn.Linear(D, 128), nn.Tanh(), nn.Linear(128, 128), nn.Tanh(), nn.Linear(128, 4), nn.Tanh())
    pol = MLPPolicy.from_torch(net, env, log_std=[-1.0] * 4)
    obs, rew = torch.empty((T, n, D), device=dev), torch.empty((T, n), device=dev)
    done = torch.empty((T, n), dtype=torch.uint8, device=dev)
    env.reset_dev(obs[T - 1])
    norm = RetNorm(env)
    gamma, eps, clip = norm.gamma, norm.eps, norm.clip
    run = {"count": torch.zeros((), dtype=torch.float64, device=dev), "mean": torch.zeros((), dtype=torch.float64, device=dev),
           "m2": torch.zeros((), dtype=torch.float64, device=dev), "ret": torch.zeros(n, dtype=torch.float64, device=dev)}

    def torch_loop():
        ret = run["ret"]
        for t in range(T):
            ret = ret * gamma + rew[t]
            var, mean = torch.var_mean(ret, unbiased=False)
            tot = run["count"] + float(n)
            delta = mean - run["mean"]
            run["m2"] = run["m2"] + var * float(n) + delta * delta * run["count"] * float(n) / tot
            run["mean"] = run["mean"] + delta * float(n) / tot
            run["count"] = tot
            ret = ret.masked_fill(done[t] != 0, 0.0)
        run["ret"] = ret
        inv = torch.rsqrt(run["m2"] / run["count"] + eps).float()
        torch.clamp(rew * inv, -clip, clip, out=rew)

    def update_normalize():
        norm.update_dev(rew, done)
        norm.normalize_dev(rew, out=rew)

    paths = {"update_dev": lambda: norm.update_dev(rew, done), "update_normalize": update_normalize, "torch_loop": torch_loop,
             "rollout": lambda: env.rollout_policy_dev(pol, obs, rew, done)}
    for _ in range(2):                                              # (the rollout last: every round starts from fresh rewards)
        for key in ("update_dev", "update_normalize", "torch_loop", "rollout"):
            paths[key]()
    times = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for key in ("update_dev", "update_normalize", "torch_loop", "rollout"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS[key]):
                paths[key]()
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e6 / CALLS[key])
    print(json.dumps({"N": n, "times": times}), flush=True)
    norm.close(); pol.close(); env.close()


def step(n):
    """one batch size: a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n)]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("ret_norm_rate: N = %d ran past %d s; nothing more is started on the device" % (n, STEP_LIMIT))
    if out.returncode:
        sys.exit("ret_norm_rate: N = %d ended with status %d; nothing more is started on the device" % (n, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def next_round_file():
    """profiles/rNN_ret_norm_rate.json, NN one past every round that has a file in profiles/ or an entry in profiles/HISTORY.md"""
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    rounds += [int(x) for x in re.findall(r"^r(\d+) — ", open(os.path.join(ROOT, "profiles", "HISTORY.md")).read(), re.M)]
    return os.path.join(ROOT, "profiles", "r%02d_ret_norm_rate.json" % (max(rounds, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--sizes", default="%d,%d" % (1 << 20, 65536))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    out = args.out or next_round_file()
    res = {"T": T, "rounds": ROUNDS, "calls_per_sample": CALLS, "copy_TBps": COPY_TBS, "unit": "us per call",
           "config": "DefaultQuad, alias layout, auto-reset (ep_time 5 s), policy 18-128-128-4", "cases": []}
    for n in (int(x) for x in args.sizes.split(",")):
        row = step(n)
        case = {"N": n, "bytes_update": T * n * 5 + n * 16}
        case.update({k: stats(v) for k, v in row["times"].items()})
        med = {k: case[k]["us_median"] for k in row["times"]}
        tbs = case["bytes_update"] / (med["update_dev"] * 1e-6) / 1e12
        case["update_dev_TBps"], case["update_dev_fraction_of_copy"] = round(tbs, 3), round(tbs / COPY_TBS, 3)
        case["torch_loop_over_update_normalize"] = round(med["torch_loop"] / med["update_normalize"], 2)
        case["rollout_over_update_normalize"] = round(med["rollout"] / med["update_normalize"], 2)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
