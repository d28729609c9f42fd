#!/usr/bin/env python3
"""The two learner-side passes between a rollout's buffers and the loss, on one device: what vtrace_dev and AdvNorm.normalize_dev cost on
[T, N] tensors (T = 64), against what a user writes today.
  vtrace            env.vtrace_dev(..., vs) without pg_adv: 21 B per env-step
  vtrace_pg         with pg_adv: 25 B per env-step
  vtrace_term       with term_values, without pg_adv: 25 B per env-step
  vtrace_term_pg    with both: 29 B per env-step
  torch_vtrace      the yardstick: a torch loop over T on the same tensors (the ratios clipped in three whole-tensor passes, then per row
                    the two selects, td, acc, vs and pg_adv), with term_values and pg_adv
  adv_norm          AdvNorm.normalize_dev(adv, out=adv) in place: two passes, 12 B per element
  torch_adv_norm    the yardstick: a = (a - a.mean()) / (a.std() + 1e-8)
Every batch size is a child process under a time limit of its own; the first one that fails or runs out of time ends the run (nothing
more is started on the device).  Warm-up, then ROUNDS rounds with the paths interleaved; each sample is a host clock around CALLS[path]
back-to-back calls ending in a device synchronise, in microseconds per call; median with min..max.  The device passes are also given as
TB/s of the bytes they have to move and as a fraction of the device's recorded copy rate (COPY_TBS, profiles/).
python3 tools/learn_passes_rate.py [OUT.json] [--sizes 1048576,65536]      (OUT defaults to profiles/rNN_learn_passes.json, NN the next
free round prefix)"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, ROUNDS = 64, 7
CALLS = {"vtrace": 10, "vtrace_pg": 10, "vtrace_term": 10, "vtrace_term_pg": 10, "torch_vtrace": 1, "adv_norm": 10, "torch_adv_norm": 3}
BYTES = {"vtrace": 21, "vtrace_pg": 25, "vtrace_term": 25, "vtrace_term_pg": 29, "adv_norm": 12}        # per env-step
COPY_TBS = 6.3                                   # the device-to-device copy rate recorded in profiles/ (TB/s of bytes read)
STEP_LIMIT = 600                                 # seconds per child process
GAMMA, LAM, RHO_BAR, C_BAR, PG_RHO_BAR = 0.99, 0.95, 1.0, 1.0, 1.0


def stats(v):
    v = sorted(v)
    return {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2)}


def child(n):
    """--child N: one line of JSON with the samples of every path at batch size N"""
    sys.path.insert(0, ROOT)
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.norm import AdvNorm
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    env = QuadrotorEnv(num_envs=n, seed=0)
    rew, lb = torch.randn((T, n), device=dev), -4.0 + 2.0 * torch.randn((T, n), device=dev)
    lt = lb + 0.3 * torch.randn((T, n), device=dev)
    values, term = 3.0 * torch.randn((T + 1, n), device=dev), 3.0 * torch.randn((T, n), device=dev)
    done = (torch.rand((T, n), device=dev) < 0.02).to(torch.uint8)
    vs, pg, adv = torch.empty_like(rew), torch.empty_like(rew), torch.empty_like(rew)
    norm = AdvNorm(env)
    kw = dict(lam=LAM, rho_bar=RHO_BAR, c_bar=C_BAR, pg_rho_bar=PG_RHO_BAR)

    def torch_vtrace():
        w = torch.exp(lt - lb)
        rho, c, rho_pg = w.clamp(max=RHO_BAR), LAM * w.clamp(max=C_BAR), w.clamp(max=PG_RHO_BAR)
        d = done != 0
        acc, vn, vsn = torch.zeros(n, device=dev), values[T], values[T]
        for t in range(T - 1, -1, -1):
            nv, nvs = torch.where(d[t], term[t], vn), torch.where(d[t], term[t], vsn)
            td = rew[t] + GAMMA * nv - values[t]
            acc = rho[t] * td + torch.where(d[t], 0.0, GAMMA * c[t]) * acc
            vs[t] = values[t] + acc
            pg[t] = rho_pg[t] * (rew[t] + GAMMA * nvs - values[t])
            vn, vsn = values[t], vs[t]

    def torch_adv_norm():
        adv.copy_((adv - adv.mean()) / (adv.std() + 1e-8))

    paths = {"vtrace": lambda: env.vtrace_dev(rew, done, values, lb, lt, GAMMA, vs, **kw),
             "vtrace_pg": lambda: env.vtrace_dev(rew, done, values, lb, lt, GAMMA, vs, pg, **kw),
             "vtrace_term": lambda: env.vtrace_dev(rew, done, values, lb, lt, GAMMA, vs, term_values=term, **kw),
             "vtrace_term_pg": lambda: env.vtrace_dev(rew, done, values, lb, lt, GAMMA, vs, pg, term_values=term, **kw),
             "torch_vtrace": torch_vtrace,
             "adv_norm": lambda: norm.normalize_dev(adv, out=adv),
             "torch_adv_norm": torch_adv_norm}
    adv.copy_(rew)
    for _ in range(2):
        for key in paths:
            paths[key]()
    times = {k: [] for k in paths}
    for _ in range(ROUNDS):
        adv.copy_(rew)                                              # (standardising a standardised batch again changes no cost)
        for key in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS[key]):
                paths[key]()
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e6 / CALLS[key])
    print(json.dumps({"N": n, "times": times}), flush=True)
    norm.close(); env.close()


def step(n):
    """one batch size: a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n)]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("learn_passes_rate: N = %d ran past %d s; nothing more is started on the device" % (n, STEP_LIMIT))
    if out.returncode:
        sys.exit("learn_passes_rate: N = %d ended with status %d; nothing more is started on the device" % (n, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def next_round_file():
    """profiles/rNN_learn_passes.json, NN one past every round that has a file in profiles/ or an entry in profiles/HISTORY.md"""
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    rounds += [int(x) for x in re.findall(r"^r(\d+) — ", open(os.path.join(ROOT, "profiles", "HISTORY.md")).read(), re.M)]
    return os.path.join(ROOT, "profiles", "r%02d_learn_passes.json" % (max(rounds, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--sizes", default="%d,%d" % (1 << 20, 65536))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    args.out = args.out or next_round_file()
    res = {"T": T, "rounds": ROUNDS, "calls_per_sample": CALLS, "bytes_per_env_step": BYTES, "copy_TBps": COPY_TBS, "unit": "us per call",
           "config": "synthetic [T, N] tensors, done density 0.02, gamma %g lambda %g, clips %g %g %g" % (GAMMA, LAM, RHO_BAR, C_BAR, PG_RHO_BAR),
           "cases": []}
    for n in (int(x) for x in args.sizes.split(",")):
        row = step(n)
        case = {"N": n}
        case.update({k: stats(v) for k, v in row["times"].items()})
        med = {k: case[k]["us_median"] for k in row["times"]}
        for key, per in BYTES.items():
            tbs = per * T * n / (med[key] * 1e-6) / 1e12
            case[key + "_TBps"], case[key + "_fraction_of_copy"] = round(tbs, 3), round(tbs / COPY_TBS, 3)
        case["torch_vtrace_over_vtrace_term_pg"] = round(med["torch_vtrace"] / med["vtrace_term_pg"], 2)
        case["torch_adv_norm_over_adv_norm"] = round(med["torch_adv_norm"] / med["adv_norm"], 2)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
