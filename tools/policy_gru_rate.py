#!/usr/bin/env python3
"""Closed-loop rollouts with a recurrent actor on one device: the GRU engine (policy_gru_kernel + step launch per step, GRUPolicy), the host
loop it replaces (step_dev + a torch fp32 nn.GRUCell and head per step, h zeroed by torch.where on done) and, for scale, the MFMA engine
on a feed-forward MLP of the same widths (18-H-4 for GRU H -> 4).  T = 64 steps, default configuration (alias layout).  Warm-up, then the
paths interleaved, REPS timed rounds each; median and spread (min..max) reported.  FLOP per env-step of a GRU net = 2 x 3H (18 + H) +
the head's, against the fp32 peak.
python3 tools/policy_gru_rate.py [out.json] [--paths gru,host_loop,mlp] [--nets 64,128,256,128-64] [--sizes 1048576,65536]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gym_art_amd import QuadrotorEnv  # noqa: E402
from gym_art_amd.policy import GRUPolicy, MLPPolicy  # noqa: E402

dev = torch.device("cuda", 0)
T, REPS, D = 64, 7, 18
PEAK_FLOPS = 155e12          # fp32 (vector = MFMA) peak measured on this part


def head(widths):
    mods, prev = [], widths[0]
    for w in widths[1:]:
        mods += [torch.nn.Linear(prev, w), torch.nn.Tanh()]
        prev = w
    return torch.nn.Sequential(*(mods + [torch.nn.Linear(prev, 4), torch.nn.Tanh()]))


def mlp_flops(widths, first=D):
    dims = [first] + widths + [4]
    return sum(2 * dims[k] * dims[k + 1] for k in range(len(dims) - 1))


def gru_flops(widths):
    H = widths[0]
    return 2 * 3 * H * (D + H) + mlp_flops(widths[1:], H)


ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--paths", default="gru,host_loop,mlp")
ap.add_argument("--nets", default="64,128,256,128-64")
ap.add_argument("--sizes", default="%d,%d" % (1 << 20, 65536))
args = ap.parse_args()
want = args.paths.split(",")
res = {"T": T, "reps": REPS, "config": "DefaultQuad, alias layout (fp64 split state), thrust noise on, auto-reset (ep_time 5 s)",
       "cases": []}
for n in (int(x) for x in args.sizes.split(",")):
    for widths in ([int(w) for w in net_.split("-")] for net_ in args.nets.split(",")):
        torch.manual_seed(0)
        H = widths[0]
        cell, hd = torch.nn.GRUCell(D, H), head(widths)
        mlp = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.Tanh(), *list(hd.children()))
        kw = dict(num_envs=n, ep_time=5, seed=0, alias_obs=True)
        envs = {k: QuadrotorEnv(**kw) for k in want}
        pol = {}
        if "gru" in envs:
            pol["gru"] = GRUPolicy.from_torch(cell, hd, envs["gru"])
        if "mlp" in envs:
            pol["mlp"] = MLPPolicy.from_torch(mlp, envs["mlp"], engine="mfma")
        celld, hdd = cell.to(dev), hd.to(dev)
        o = torch.empty((T, n, D), device=dev); r = torch.empty((T, n), device=dev); d = torch.empty((T, n), dtype=torch.uint8, device=dev)
        o1 = torch.empty((n, D), device=dev); r1 = torch.empty(n, device=dev); d1 = torch.empty(n, dtype=torch.uint8, device=dev)
        h1 = torch.zeros((n, H), device=dev)
        for k in pol:
            envs[k].reset_dev(o[T - 1])
        if "host_loop" in envs:
            envs["host_loop"].reset_dev(o1)

        def run_pol(k):
            envs[k].rollout_policy_dev(pol[k], o, r, d)

        def run_host():
            global h1
            with torch.no_grad():
                for _ in range(T):
                    h1 = celld(o1, h1)
                    envs["host_loop"].step_dev(hdd(h1), o1, r1, d1)
                    h1 = torch.where(d1.bool()[:, None], torch.zeros((), device=dev), h1)

        paths = {k: (lambda k=k: run_pol(k)) for k in pol}
        if "host_loop" in envs:
            paths["host_loop"] = run_host
        for fn in paths.values():       # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(REPS):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e6 / T)
        name = "18-GRU%d-%s4" % (H, "".join("%d-" % w for w in widths[1:]))
        case = {"N": n, "net": name, "mlp_net": "-".join(str(x) for x in [D] + widths + [4]), "flop_per_env_step": gru_flops(widths),
                "mlp_flop_per_env_step": mlp_flops(widths), "flop_floor_us": round(n * gru_flops(widths) / PEAK_FLOPS * 1e6, 1)}
        for k, v in times.items():
            v = sorted(v)
            med = v[len(v) // 2]
            fl = mlp_flops(widths) if k == "mlp" else gru_flops(widths)
            case[k] = {"us_per_step_median": round(med, 2), "us_per_step_min": round(v[0], 2), "us_per_step_max": round(v[-1], 2),
                       "env_steps_per_s": float("%.3g" % (n / (med * 1e-6))),
                       "frac_flop_floor": round(n * fl / PEAK_FLOPS / (med * 1e-6), 3)}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        for p in pol.values():
            p.close()
        for e in envs.values():
            e.close()
        del o, r, d
        torch.cuda.empty_cache()
out = args.out
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res))
