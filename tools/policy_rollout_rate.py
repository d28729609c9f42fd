#!/usr/bin/env python3
"""Closed-loop rollouts on one device: the fused policy rollout (policy_rollout_kernel), its fallback (policy launch + step launch per
step, GAQ_NO_FUSED=1) and the host loop they replace (step_dev + a torch fp32 forward pass per step), same policy, T = 64 steps, default
configuration (alias layout).  Warm-up, then the three paths interleaved, REPS timed rounds each; median and spread (min..max) reported.
python3 tools/policy_rollout_rate.py [out.json]"""
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


res = {"T": T, "reps": REPS, "config": "DefaultQuad, alias layout (fp64 split state), thrust noise on", "cases": []}
for n in (1 << 20, 65536):
    for widths in ([64, 64], [128, 128]):
        m = net(widths)
        kw = dict(num_envs=n, ep_time=5, seed=0, alias_obs=True)
        fused = QuadrotorEnv(**kw)
        os.environ["GAQ_NO_FUSED"] = "1"
        fb = QuadrotorEnv(**kw)
        del os.environ["GAQ_NO_FUSED"]
        host = QuadrotorEnv(**kw)
        mdev = m.to(dev)
        pol = {id(fused): MLPPolicy.from_torch(m, fused), id(fb): MLPPolicy.from_torch(m, fb)}
        o = torch.empty((T, n, 18), device=dev); r = torch.empty((T, n), device=dev); d = torch.empty((T, n), dtype=torch.uint8, device=dev)
        o1 = torch.empty((n, 18), device=dev); r1 = torch.empty(n, device=dev); d1 = torch.empty(n, dtype=torch.uint8, device=dev)
        for e in (fused, fb):
            e.reset_dev(o[T - 1])
        host.reset_dev(o1)

        def run_pol(e):
            e.rollout_policy_dev(pol[id(e)], o, r, d)

        def run_host():
            with torch.no_grad():
                for _ in range(T):
                    host.step_dev(mdev(o1), o1, r1, d1)

        paths = {"fused": lambda: run_pol(fused), "fallback": lambda: run_pol(fb), "host_loop": run_host}
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
                "fused_variant": fused.kernel_variant}
        for k, v in times.items():
            v = sorted(v)
            med = v[len(v) // 2]
            case[k] = {"us_per_step_median": round(med, 2), "us_per_step_min": round(v[0], 2), "us_per_step_max": round(v[-1], 2),
                       "env_steps_per_s": float("%.3g" % (n / (med * 1e-6))),
                       "frac_flop_floor": round(n * flops(widths) / PEAK_FLOPS / (med * 1e-6), 3),
                       # ~93 B per env-step of the fused loop (obs rows, reward, done) -- the same floor the open-loop rollout has
                       "frac_hbm_floor_93B": round(n * 93 / HBM_BPS / (med * 1e-6), 3)}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        for p in pol.values():
            p.close()
        for e in (fused, fb, host):
            e.close()
out = sys.argv[1] if len(sys.argv) > 1 else None
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res))
