#!/usr/bin/env python3
"""Closed-loop rollouts with an LSTM actor on one device: the LSTM engine (policy_lstm_kernel + step launch per step, LSTMPolicy), its
actor-critic form (values, log-probabilities and terminal values asked for: policy_lstm_ac_kernel, the gather and policy_lstm_term_kernel),
the GRU engine on a GRU of the same H (tools/policy_gru_rate.py's path), and the host loop the engine replaces (step_dev + a torch fp32
nn.LSTMCell and head per step, h and c zeroed by torch.where on done).  T = 64 steps, default configuration (alias layout), N = 65 536
and 2^20, H = 64, 128, 256.  Warm-up, then the paths interleaved, REPS = 7 timed rounds each; median and spread (min..max) reported.
FLOP per env-step of an LSTM net = 2 x 4H (18 + H) + the head's: 4/3 of the GRU's cell.
python3 tools/policy_lstm_rate.py [out.json] [--paths lstm,lstm_ac,gru,host_loop] [--nets 64,128,256] [--sizes 65536,1048576]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gym_art_amd import QuadrotorEnv  # noqa: E402
from gym_art_amd.policy import GRUPolicy, LSTMPolicy  # noqa: E402

dev = torch.device("cuda", 0)
T, REPS, D = 64, 7, 18
LOG_STD = (-1.0, -1.0, -1.0, -1.0)


def cell_flops(gates, H):
    return 2 * gates * H * (D + H) + 2 * H * 4


ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--paths", default="lstm,lstm_ac,gru,host_loop")
ap.add_argument("--nets", default="64,128,256")
ap.add_argument("--sizes", default="%d,%d" % (65536, 1 << 20))
args = ap.parse_args()
want = args.paths.split(",")
res = {"T": T, "reps": REPS, "config": "DefaultQuad, alias layout (fp64 split state), thrust noise on, auto-reset (ep_time 5 s)",
       "cases": []}
for n in (int(x) for x in args.sizes.split(",")):
    for H in (int(w) for w in args.nets.split(",")):
        torch.manual_seed(0)
        lstm, gru = torch.nn.LSTMCell(D, H), torch.nn.GRUCell(D, H)
        hd = torch.nn.Sequential(torch.nn.Linear(H, 4), torch.nn.Tanh())
        val = torch.nn.Linear(H, 1)
        kw = dict(num_envs=n, ep_time=5, seed=0, alias_obs=True)
        envs = {k: QuadrotorEnv(**kw) for k in want}
        pol = {}
        if "lstm" in envs:
            pol["lstm"] = LSTMPolicy.from_torch(lstm, hd, envs["lstm"])
        if "lstm_ac" in envs:
            pol["lstm_ac"] = LSTMPolicy.from_torch(lstm, hd, envs["lstm_ac"], log_std=LOG_STD, value=val)
        if "gru" in envs:
            pol["gru"] = GRUPolicy.from_torch(gru, hd, envs["gru"])
        celld, hdd = lstm.to(dev), hd.to(dev)
        o = torch.empty((T, n, D), device=dev); r = torch.empty((T, n), device=dev); d = torch.empty((T, n), dtype=torch.uint8, device=dev)
        v = torch.empty((T + 1, n), device=dev); lp = torch.empty((T, n), device=dev); tv = torch.empty((T, n), device=dev)
        o1 = torch.empty((n, D), device=dev); r1 = torch.empty(n, device=dev); d1 = torch.empty(n, dtype=torch.uint8, device=dev)
        state = [torch.zeros((n, H), device=dev), torch.zeros((n, H), device=dev)]
        for k in pol:
            envs[k].reset_dev(o[T - 1])
        if "host_loop" in envs:
            envs["host_loop"].reset_dev(o1)

        def run_pol(k):
            if k == "lstm_ac":
                envs[k].rollout_policy_dev(pol[k], o, r, d, values=v, logp=lp, term_values=tv)
            else:
                envs[k].rollout_policy_dev(pol[k], o, r, d)

        def run_host():
            zero = torch.zeros((), device=dev)
            with torch.no_grad():
                for _ in range(T):
                    h1, c1 = celld(o1, (state[0], state[1]))
                    envs["host_loop"].step_dev(hdd(h1), o1, r1, d1)
                    m = d1.bool()[:, None]
                    state[0], state[1] = torch.where(m, zero, h1), torch.where(m, zero, c1)

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
        case = {"N": n, "net": "18-LSTM%d-4" % H, "gru_net": "18-GRU%d-4" % H, "flop_per_env_step": cell_flops(4, H),
                "gru_flop_per_env_step": cell_flops(3, H)}
        for k, x in times.items():
            x = sorted(x)
            med = x[len(x) // 2]
            case[k] = {"us_per_step_median": round(med, 2), "us_per_step_min": round(x[0], 2), "us_per_step_max": round(x[-1], 2),
                       "env_steps_per_s": float("%.3g" % (n / (med * 1e-6)))}
        if "lstm" in case and "gru" in case:
            case["lstm_over_gru"] = round(case["lstm"]["us_per_step_median"] / case["gru"]["us_per_step_median"], 3)
        if "lstm" in case and "host_loop" in case:
            case["host_loop_over_lstm"] = round(case["host_loop"]["us_per_step_median"] / case["lstm"]["us_per_step_median"], 3)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        for p in pol.values():
            p.close()
        for e in envs.values():
            e.close()
        del o, r, d, v, lp, tv, state
        torch.cuda.empty_cache()
out = args.out
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res))
