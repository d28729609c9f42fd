#!/usr/bin/env python3
"""Closed-loop rollouts on one device: the fused policy rollout (policy_rollout_kernel), its fallback (policy launch + step launch per
step, GAQ_NO_FUSED=1), the MFMA engine (policy_mfma_kernel + step launch per step), the bf16 engine (policy_mfma_bf16_kernel + step launch
per step) and the host loops they replace (step_dev + a torch fp32 forward pass per step; host_loop_bf16: the same with the module in
bf16), same policy, T = 64 steps, default configuration (alias layout).  Warm-up, then the paths interleaved, REPS timed
rounds each; median and spread (min..max) reported.  The VALU paths (fused, fallback) take widths up to 128: for wider nets they are
recorded as absent.
python3 tools/policy_rollout_rate.py [out.json] [--paths fused,fallback,mfma,bf16,host_loop,host_loop_bf16] [--nets 64-64,256-256] [--sizes 1048576,65536]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gym_art_amd import QuadrotorEnv  # noqa: E402
from gym_art_amd.policy import MLPPolicy  # noqa: E402

dev = torch.device("cuda", 0)
T, REPS = 64, 7
PEAK_FLOPS, HBM_BPS = 155e12, 8e12          # fp32 (vector = MFMA) peak measured on this part; HBM nominal
PEAK_BF16 = 2.5e15                          # bf16 MFMA dense peak (spec, ~2.5 PF)


def net(widths):
    torch.manual_seed(0)
    mods, prev = [], 18
    for w in widths:
        mods += [torch.nn.Linear(prev, w), torch.nn.Tanh()]
        prev = w
    mods += [torch.nn.Linear(prev, 4), torch.nn.Tanh()]
    return torch.nn.Sequential(*mods)


def flops(widths):
    dims = [18] + widths + [4]
    return sum(2 * dims[k] * dims[k + 1] for k in range(len(dims) - 1))


ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--paths", default="fused,fallback,mfma,host_loop")
ap.add_argument("--nets", default="64-64,128-128,256-256,256-256-256")
ap.add_argument("--sizes", default="%d,%d" % (1 << 20, 65536))
args = ap.parse_args()
want = args.paths.split(",")
res = {"T": T, "reps": REPS, "config": "DefaultQuad, alias layout (fp64 split state), thrust noise on", "cases": []}
for n in (int(x) for x in args.sizes.split(",")):
    for widths in ([int(w) for w in net_.split("-")] for net_ in args.nets.split(",")):
        m = net(widths)
        kw = dict(num_envs=n, ep_time=5, seed=0, alias_obs=True)
        valu = max(widths) <= 128
        envs, pol = {}, {}
        if valu and "fused" in want:
            envs["fused"] = QuadrotorEnv(**kw)
        if valu and "fallback" in want:
            os.environ["GAQ_NO_FUSED"] = "1"
            envs["fallback"] = QuadrotorEnv(**kw)
            del os.environ["GAQ_NO_FUSED"]
        for k in ("mfma", "bf16"):
            if k in want:
                envs[k] = QuadrotorEnv(**kw)
        for k, e in envs.items():
            pol[k] = MLPPolicy.from_torch(m, e, engine=k if k in ("mfma", "bf16") else "valu")
        for k in ("host_loop", "host_loop_bf16"):
            if k in want:
                envs[k] = QuadrotorEnv(**kw)
        hosts = {k: envs[k] for k in ("host_loop", "host_loop_bf16") if k in envs}
        mdev = m.to(dev)
        mbf = net(widths).to(dev).to(torch.bfloat16)
        o = torch.empty((T, n, 18), device=dev); r = torch.empty((T, n), device=dev); d = torch.empty((T, n), dtype=torch.uint8, device=dev)
        o1 = torch.empty((n, 18), device=dev); r1 = torch.empty(n, device=dev); d1 = torch.empty(n, dtype=torch.uint8, device=dev)
        for k in pol:
            envs[k].reset_dev(o[T - 1])
        for host in hosts.values():
            host.reset_dev(o1)

        def run_pol(k):
            envs[k].rollout_policy_dev(pol[k], o, r, d)

        def run_host():
            with torch.no_grad():
                for _ in range(T):
                    hosts["host_loop"].step_dev(mdev(o1), o1, r1, d1)

        def run_host_bf16():
            with torch.no_grad():
                for _ in range(T):
                    hosts["host_loop_bf16"].step_dev(mbf(o1.to(torch.bfloat16)).float(), o1, r1, d1)

        paths = {k: (lambda k=k: run_pol(k)) for k in pol}
        if "host_loop" in hosts:
            paths["host_loop"] = run_host
        if "host_loop_bf16" in hosts:
            paths["host_loop_bf16"] = run_host_bf16
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
        case = {"N": n, "mlp": "-".join(str(x) for x in [18] + widths + [4]), "flop_per_env_step": flops(widths),
                "flop_floor_us": round(n * flops(widths) / PEAK_FLOPS * 1e6, 1),
                "bf16_flop_floor_us": round(n * flops(widths) / PEAK_BF16 * 1e6, 1)}
        if "fused" in envs:
            case["fused_variant"] = envs["fused"].kernel_variant
        for k in ("fused", "fallback"):
            if k in want and not valu:
                case[k] = None           # absent: the VALU engine takes widths up to 128
        for k, v in times.items():
            v = sorted(v)
            med = v[len(v) // 2]
            case[k] = {"us_per_step_median": round(med, 2), "us_per_step_min": round(v[0], 2), "us_per_step_max": round(v[-1], 2),
                       "env_steps_per_s": float("%.3g" % (n / (med * 1e-6))),
                       "frac_flop_floor": round(n * flops(widths) / PEAK_FLOPS / (med * 1e-6), 3),
                       "frac_bf16_flop_floor": round(n * flops(widths) / PEAK_BF16 / (med * 1e-6), 3),
                       # ~93 B per env-step of the fused loop (obs rows, reward, done) -- the same floor the open-loop rollout has
                       "frac_hbm_floor_93B": round(n * 93 / HBM_BPS / (med * 1e-6), 3)}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        for p in pol.values():
            p.close()
        for e in envs.values():
            e.close()
out = args.out
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res))
