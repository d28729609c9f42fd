#!/usr/bin/env python3
"""Closed-loop rollouts with an encoder in front of a GRU on one device: the device path (policy_encode_kernel + policy_gru_kernel + step
launch per step, GRUPolicy.from_torch_encoder), the host loop it replaces (step_dev + a torch fp32 nn.Sequential encoder, nn.GRUCell and head per
step, h zeroed by torch.where on done) and, for scale, the encoder-less GRU engine of the same H (tools/policy_gru_rate.py's path).
T = 64 steps, default configuration (alias layout).  3 warm-up rounds, then the paths interleaved, REPS = 7 timed rounds each; median and
spread (min..max) reported.  Per env-step the device path writes and reads again 8 E bytes of features (E = the encoder's last width).
python3 tools/policy_enc_rate.py [out.json] [--paths enc,host_loop,gru] [--nets 64-64:64,256:128] [--sizes 1048576,65536]
A net is <encoder widths joined by '-'>:<H>."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gym_art_amd import QuadrotorEnv  # noqa: E402
from gym_art_amd.policy import GRUPolicy  # noqa: E402

dev = torch.device("cuda", 0)
T, REPS, D = 64, 7, 18
PEAK_FLOPS = 155e12          # fp32 (vector = MFMA) peak measured on this part


def encoder(widths):
    mods, prev = [], D
    for w in widths:
        mods += [torch.nn.Linear(prev, w), torch.nn.Tanh()]
        prev = w
    return torch.nn.Sequential(*mods)


def flops(enc, H):
    dims = [D] + enc
    return sum(2 * dims[k] * dims[k + 1] for k in range(len(enc))) + 2 * 3 * H * (enc[-1] + H) + 2 * H * 4


ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--paths", default="enc,host_loop,gru")
ap.add_argument("--nets", default="64-64:64,256:128")
ap.add_argument("--sizes", default="%d,%d" % (1 << 20, 65536))
args = ap.parse_args()
want = args.paths.split(",")
res = {"T": T, "reps": REPS, "config": "DefaultQuad, alias layout (fp64 split state), thrust noise on, auto-reset (ep_time 5 s)",
       "cases": []}
for n in (int(x) for x in args.sizes.split(",")):
    for net_ in args.nets.split(","):
        enc_w, H = [int(w) for w in net_.split(":")[0].split("-")], int(net_.split(":")[1])
        E = enc_w[-1]
        torch.manual_seed(0)
        enc, cell, hd = encoder(enc_w), torch.nn.GRUCell(E, H), torch.nn.Sequential(torch.nn.Linear(H, 4), torch.nn.Tanh())
        bare = torch.nn.GRUCell(D, H)                                 # the encoder-less GRU of the same H
        kw = dict(num_envs=n, ep_time=5, seed=0, alias_obs=True)
        envs = {k: QuadrotorEnv(**kw) for k in want}
        pol = {}
        if "enc" in envs:
            pol["enc"] = GRUPolicy.from_torch_encoder(enc, cell, hd, envs["enc"])
        if "gru" in envs:
            pol["gru"] = GRUPolicy.from_torch(bare, hd, envs["gru"])
        encd, celld, hdd = enc.to(dev), cell.to(dev), hd.to(dev)
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
                    h1 = celld(encd(o1), h1)
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
        name = "18-enc%s-GRU%d-4" % ("-".join(str(w) for w in enc_w), H)
        case = {"N": n, "net": name, "gru_net": "18-GRU%d-4" % H, "flop_per_env_step": flops(enc_w, H),
                "feature_bytes_per_env_step": 8 * E, "feature_buffer_bytes": 4 * n * E}
        for k, v in times.items():
            v = sorted(v)
            med = v[len(v) // 2]
            case[k] = {"us_per_step_median": round(med, 2), "us_per_step_min": round(v[0], 2), "us_per_step_max": round(v[-1], 2),
                       "env_steps_per_s": float("%.3g" % (n / (med * 1e-6)))}
        if "enc" in case and "host_loop" in case:
            case["host_loop_over_enc"] = round(case["host_loop"]["us_per_step_median"] / case["enc"]["us_per_step_median"], 2)
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
