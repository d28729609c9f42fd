#!/usr/bin/env python3
"""Observation normalisation on one device: what it costs, and that rollouts without it did not slow down.
  rollouts   rollout_policy_dev in the alias layout, T = 64, per net (MFMA 18-64-64-4, bf16 18-256-256-4, GRU 128) and batch size:
             `plain` without a normaliser and, in this tree, `norm` with an ObsNorm attached (the *_norm_kernel twins: the
             <PolObsNorm> instantiations of the kernel templates).  With --parent-tree (a checkout of the parent commit with its library built) `plain` is timed in child processes that import that
             tree (`plain_parent`) and this one (`plain_child`) in turn, ROUNDS rounds each: "existing rollouts did not slow down" holds
             if the child's median lies inside the min..max of the parent's own rounds
  update     ObsNorm.update_dev on a [64, N, 18] rollout against the torch passes a user writes today (torch.var_mean over the first two
             dims + Chan's merge into running statistics), as GB/s of the one read of the data and as a fraction of the device's
             recorded copy rate (COPY_TBS, profiles/): the floor of a pass that reads every byte once
  apply      ObsNorm.normalize_dev against the torch expression clamp((x - mean) * inv_std, -clip, clip)
Every GPU step is a child process under a time limit of its own; the first one that fails or runs out of time ends the run (nothing more
is started on the device).  Warm-up, then the paths interleaved, REPS timed repetitions per round; median with min..max, microseconds per
step (rollouts) or per call (update, apply).
python3 tools/obs_norm_rate.py [profiles/r16_obs_norm.json] [--sizes 1048576,65536] [--parent-tree DIR] [--rounds 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, REPS, D = 64, 5, 18
NETS = ["mfma:64-64", "bf16:256-256", "gru:128"]
COPY_TBS = 6.3                                   # the device-to-device copy rate recorded in profiles/ (TB/s of bytes read)
STEP_LIMIT = 600                                 # seconds per child process


def stats(v):
    v = sorted(v)
    return {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2)}


def timed(fn, torch, per):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / per


def child_rollouts(args):
    """--child rollouts: the rollouts of the tree this process imported (GAQ_OBS_NORM_RATE_TREE), one line of JSON per case"""
    sys.path.insert(0, os.environ.get("GAQ_OBS_NORM_RATE_TREE") or ROOT)
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd import policy as P
    dev, nn = torch.device("cuda", 0), torch.nn
    with_norm = args.norm and hasattr(P, "ObsNorm")
    for n in (int(x) for x in args.sizes.split(",")):
        for net in NETS:
            kind, widths = net.split(":")
            torch.manual_seed(0)
            envs = {"plain": QuadrotorEnv(num_envs=n, ep_time=5, seed=0, alias_obs=True)}
            if with_norm:
                envs["norm"] = QuadrotorEnv(num_envs=n, ep_time=5, seed=0, alias_obs=True)
            pols, keep = {}, []
            for key, env in envs.items():
                if kind == "gru":
                    H = int(widths)
                    pol = P.GRUPolicy.from_torch(nn.GRUCell(D, H), nn.Sequential(nn.Linear(H, 4), nn.Tanh()), env)
                else:
                    mods, prev = [], D
                    for w in (int(x) for x in widths.split("-")):
                        mods += [nn.Linear(prev, w), nn.Tanh()]
                        prev = w
                    pol = P.MLPPolicy.from_torch(nn.Sequential(*mods, nn.Linear(prev, 4), nn.Tanh()), env, engine=kind)
                if key == "norm":
                    norm = P.ObsNorm(env)
                    pol.set_obs_norm(norm)
                    keep.append(norm)
                pols[key] = pol
            bufs = {k: (torch.empty((T, n, D), device=dev), torch.empty((T, n), device=dev),
                        torch.empty((T, n), dtype=torch.uint8, device=dev)) for k in envs}
            for k, e in envs.items():
                e.reset_dev(bufs[k][0][T - 1])
            if with_norm:                                           # real statistics: the clamp and both table rows at work
                envs["norm"].rollout_policy_dev(pols["norm"], *bufs["norm"])
                keep[0].update_dev(bufs["norm"][0])
            paths = {k: (lambda k=k: envs[k].rollout_policy_dev(pols[k], *bufs[k])) for k in envs}
            for fn in paths.values():
                for _ in range(3):
                    fn()
            times = {k: [] for k in paths}
            for _ in range(REPS):
                for k, fn in paths.items():
                    times[k].append(timed(fn, torch, T))
            print(json.dumps({"N": n, "net": net, "times": times}), flush=True)
            for x in list(pols.values()) + keep + list(envs.values()):
                x.close()
            del bufs
            torch.cuda.empty_cache()


def child_stats(args):
    """--child stats: update_dev and normalize_dev against torch on a [64, N, 18] rollout, one line of JSON per batch size"""
    sys.path.insert(0, ROOT)
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import ObsNorm
    dev = torch.device("cuda", 0)
    for n in (int(x) for x in args.sizes.split(",")):
        env = QuadrotorEnv(num_envs=n, ep_time=5, seed=0, alias_obs=True)
        norm = ObsNorm(env)
        obs = torch.randn((T, n, D), device=dev) * 3.0 + 1.0
        out = torch.empty_like(obs)
        run = {"count": torch.zeros((), dtype=torch.float64, device=dev), "mean": torch.zeros(D, dtype=torch.float64, device=dev),
               "m2": torch.zeros(D, dtype=torch.float64, device=dev)}

        def torch_update():
            var, mean = torch.var_mean(obs, dim=(0, 1), unbiased=False)
            nb = float(T * n)
            tot = run["count"] + nb
            delta = mean.double() - run["mean"]
            run["m2"] = run["m2"] + var.double() * nb + delta * delta * run["count"] * nb / tot
            run["mean"] = run["mean"] + delta * nb / tot
            run["count"] = tot

        norm.update_dev(obs)
        mean32 = torch.from_numpy(norm.mean).to(dev, torch.float32)
        inv32 = torch.from_numpy(1.0 / (norm.var + norm.eps) ** 0.5).to(dev, torch.float32)
        paths = {"update_dev": lambda: norm.update_dev(obs), "update_torch": torch_update,
                 "apply_dev": lambda: norm.normalize_dev(obs, out=out),
                 "apply_torch": lambda: torch.clamp((obs - mean32) * inv32, -norm.clip, norm.clip, out=out)}
        for fn in paths.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in paths}
        for _ in range(REPS):
            for k, fn in paths.items():
                times[k].append(timed(fn, torch, 1))
        print(json.dumps({"N": n, "bytes": obs.numel() * 4, "times": times}), flush=True)
        norm.close(); env.close()
        del obs, out
        torch.cuda.empty_cache()


def step(mode, sizes, tree=None, norm=False):
    """one GPU step: a fresh child process under its own time limit; its JSON lines.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--sizes", sizes] + (["--norm"] if norm else [])
    env = dict(os.environ, **({"GAQ_OBS_NORM_RATE_TREE": tree} if tree else {}))
    try:
        out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("obs_norm_rate: the %s step ran past %d s; nothing more is started on the device" % (mode, STEP_LIMIT))
    if out.returncode:
        sys.exit("obs_norm_rate: the %s step ended with status %d; nothing more is started on the device" % (mode, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--sizes", default="%d,%d" % (1 << 20, 65536))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with libgaq.so built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--norm", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return {"rollouts": child_rollouts, "stats": child_stats}[args.child](args)
    res = {"T": T, "reps_per_round": REPS, "rounds": args.rounds, "copy_TBps": COPY_TBS,
           "unit": "us per step (rollouts), us per call (update, apply)", "config": "DefaultQuad, alias layout, auto-reset (ep_time 5 s)",
           "rollouts": [], "stats": []}
    pooled = {}
    for size in args.sizes.split(","):                              # the trees in turn, round by round, per batch size
        for _ in range(args.rounds):
            trees = ([("plain_parent", os.path.abspath(args.parent_tree), False)] if args.parent_tree else []) + [("plain_child", ROOT, True)]
            for key, tree, norm in trees:
                for row in step("rollouts", size, tree, norm):
                    slot = pooled.setdefault((row["N"], row["net"]), {})
                    slot.setdefault(key, []).extend(row["times"]["plain"])
                    if "norm" in row["times"]:
                        slot.setdefault("norm", []).extend(row["times"]["norm"])
    for (n, net), slot in pooled.items():
        case = {"N": n, "net": net}
        case.update({k: stats(v) for k, v in slot.items()})
        if "norm" in slot:
            case["norm_over_plain"] = round(case["norm"]["us_median"] / case["plain_child"]["us_median"], 4)
        if "plain_parent" in slot:
            p, c = case["plain_parent"], case["plain_child"]["us_median"]
            case["child_inside_parent_spread"] = p["us_min"] <= c <= p["us_max"]
        res["rollouts"].append(case)
        print(json.dumps(case), flush=True)
    for row in step("stats", args.sizes):
        case = {"N": row["N"], "bytes": row["bytes"]}
        case.update({k: stats(v) for k, v in row["times"].items()})
        tbs = row["bytes"] / (case["update_dev"]["us_median"] * 1e-6) / 1e12
        case["update_dev_TBps"], case["update_dev_fraction_of_copy"] = round(tbs, 3), round(tbs / COPY_TBS, 3)
        case["update_torch_over_dev"] = round(case["update_torch"]["us_median"] / case["update_dev"]["us_median"], 3)
        case["apply_torch_over_dev"] = round(case["apply_torch"]["us_median"] / case["apply_dev"]["us_median"], 3)
        res["stats"].append(case)
        print(json.dumps(case), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
