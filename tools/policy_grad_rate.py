#!/usr/bin/env python3
"""The whole-batch PPO gradient of an MLP actor on one device: MLPPolicy.ppo_grad_dev (one tile kernel + one reduction) against what a
user writes today, torch fp32 forward + backward of the same clipped surrogate on the same rows with the same packed parameters.
  dev           ppo_grad_dev(obs, actions, logp_old, adv) with the default number of workgroups
  dev_g<G>      the same under GAQ_GRAD_GROUPS=<G> (the sweep behind the default: --groups)
  torch         torch.nn.functional.linear layers on views of ONE packed parameter tensor, loss.backward(); chunked over the rows only as
                far as memory requires (the chunk is recorded: rows = not chunked)
Nets 18-64-64-4 and 18-128-128-4 (tanh, output tanh), rows 2^20 and 2^22.  Every (net, rows) is a child process under a time limit of its
own; the first one that fails or runs out of time ends the run (nothing more is started on the device).  3 warm-up rounds, then 7 rounds
with the paths interleaved; each sample is a host clock around CALLS back-to-back calls ending in a device synchronise, in milliseconds per
call; median with min..max.  No kernel-only trace is taken: the figures include the launches.  Beside each figure stand the floors: 6 x
parameters x rows / 155 TFLOPS (dense fp32 matrix peak) and 96 B/row / the device's recorded copy rate.
python3 tools/policy_grad_rate.py [OUT.json] [--rows 1048576,4194304] [--groups 128,256,512,1024]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"18-64-64-4": [64, 64], "18-128-128-4": [128, 128]}
WARMUP, ROUNDS, CALLS = 3, 7, 3
PEAK_TFLOPS, COPY_TBS, ROW_BYTES = 155.0, 6.3, 96
STEP_LIMIT = 400                                 # seconds per child process
CLIP = 0.2


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}


def child(net, rows, groups):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy, pack_weights, unpack_weights
    dev = torch.device("cuda", 0)
    widths = NETS[net]
    rng = np.random.RandomState(0)
    dims = [18] + widths + [4]
    layers = [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
              for k in range(len(dims) - 1)]
    log_std = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
    env = QuadrotorEnv(num_envs=64, seed=0)
    pol = MLPPolicy.from_arrays(env, layers, "tanh", True, log_std=log_std, engine="mfma")
    torch.manual_seed(0)
    obs = torch.randn((rows, 18), device=dev)
    mean_t = torch.empty((rows, 4), device=dev)
    pol.logp_dev(obs, torch.zeros((rows, 4), device=dev), mean=mean_t)
    std = torch.as_tensor(np.exp(log_std), device=dev)
    z = torch.randn((rows, 4), device=dev)
    actions = (mean_t + 0.15 * std * torch.randn((rows, 4), device=dev) + std * z).contiguous()
    logp_old = ((-0.5 * z * z).sum(dim=1) - float(log_std.sum()) - 2.0 * float(np.log(2.0 * np.pi))).contiguous()
    adv = torch.randn(rows, device=dev)
    del mean_t, z
    grad, gls, st = pol.ppo_grad_dev(obs, actions, logp_old, adv, clip=CLIP)

    theta = torch.as_tensor(pack_weights(layers), device=dev).requires_grad_(True)
    ls = torch.as_tensor(log_std, device=dev).requires_grad_(True)
    chunk = rows                                                    # halved below until a forward + backward fits

    def torch_once():
        theta.grad, ls.grad = None, None
        for r0 in range(0, rows, chunk):
            views = unpack_weights(theta, 18, widths, 4)
            y = obs[r0:r0 + chunk]
            for W, b in views[:-1]:
                y = torch.tanh(F.linear(y, W, b))
            m = torch.tanh(F.linear(y, views[-1][0], views[-1][1]))
            zz = (actions[r0:r0 + chunk] - m) * torch.exp(-ls)
            lp = (-0.5 * zz * zz - ls).sum(dim=1) - 2.0 * float(np.log(2.0 * np.pi))
            r = torch.exp(lp - logp_old[r0:r0 + chunk])
            a = adv[r0:r0 + chunk]
            loss = -torch.minimum(r * a, torch.clamp(r, 1.0 - CLIP, 1.0 + CLIP) * a).sum() / rows
            loss.backward()

    while True:
        try:
            torch_once()
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            chunk //= 2
            torch.cuda.empty_cache()
    agree = float((theta.grad - grad).abs().max() / grad.abs().max())

    def dev_path(g=None):
        def run():
            if g is None:
                os.environ.pop("GAQ_GRAD_GROUPS", None)
            else:
                os.environ["GAQ_GRAD_GROUPS"] = str(g)
            pol.ppo_grad_dev(obs, actions, logp_old, adv, clip=CLIP, grad=grad, grad_log_std=gls, stats=st)
        return run
    paths = {"dev": dev_path(), "torch": torch_once}
    paths.update({"dev_g%d" % g: dev_path(g) for g in groups})
    times = {k: [] for k in paths}
    for rnd in range(WARMUP + ROUNDS):
        for key, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            if rnd >= WARMUP:
                times[key].append((time.perf_counter() - t0) * 1e3 / CALLS)
    os.environ.pop("GAQ_GRAD_GROUPS", None)
    print(json.dumps({"net": net, "rows": rows, "parameters": int(theta.numel()), "torch_chunk_rows": chunk,
                      "torch_vs_dev_max_rel_diff": agree, "times": times}), flush=True)
    pol.close(); env.close()


def step(net, rows, groups):
    """one (net, rows): a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", net, "--rows", str(rows), "--groups", ",".join(map(str, groups))]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("policy_grad_rate: %s at %d rows ran past %d s; nothing more is started on the device" % (net, rows, STEP_LIMIT))
    if out.returncode:
        sys.exit("policy_grad_rate: %s at %d rows ended with status %d; nothing more is started on the device" % (net, rows, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r29_policy_grad.json"))
    ap.add_argument("--rows", default="%d,%d" % (1 << 20, 1 << 22))
    ap.add_argument("--groups", default="128,256,512,1024")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    groups = [int(x) for x in args.groups.split(",") if x]
    if args.child:
        return child(args.child, int(args.rows), groups)
    res = {"warmup_rounds": WARMUP, "rounds": ROUNDS, "calls_per_sample": CALLS, "unit": "ms per call", "peak_TFLOPS": PEAK_TFLOPS,
           "copy_TBps": COPY_TBS, "row_bytes": ROW_BYTES, "kernel_only_trace": "none taken: host clocks around whole calls",
           "config": "tanh nets with output tanh, Gaussian rows, behaviour means 0.15 sigma off, clip %g, scale 1 / rows" % CLIP, "cases": []}
    for net in NETS:
        for rows in (int(x) for x in args.rows.split(",")):
            row = step(net, rows, groups)
            case = {k: row[k] for k in ("net", "rows", "parameters", "torch_chunk_rows", "torch_vs_dev_max_rel_diff")}
            case.update({k: stats(v) for k, v in row["times"].items()})
            case["flop_floor_ms"] = round(6.0 * row["parameters"] * rows / (PEAK_TFLOPS * 1e12) * 1e3, 3)
            case["hbm_floor_ms"] = round(ROW_BYTES * rows / (COPY_TBS * 1e12) * 1e3, 3)
            case["torch_over_dev"] = round(case["torch"]["ms_median"] / case["dev"]["ms_median"], 2)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
