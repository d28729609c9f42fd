#!/usr/bin/env python3
"""The whole-batch gradient of the combined PPO loss of a shared-trunk actor-critic on one device: MLPPolicy.ppo_ac_grad_dev (one tile
kernel + one reduction) against, interleaved in the same run,
  torch         torch fp32 forward + backward of the same combined loss on a shared-trunk module (F.linear layers on views of one packed
                parameter tensor plus the head's tensor, loss.backward(); chunked over the rows only as far as memory requires)
  ppo           ppo_grad_dev alone on the same net (the policy loss only: what the value head adds to the pass)
  ppo + mse     ppo_grad_dev on the net and mse_grad_dev on an MLPCritic of the same hidden shape, back to back (the two-network
                learner: two trunk forwards and two trunk backwards); their own medians are recorded too
Nets 18-64-64-4 and 18-128-128-4 (tanh, output tanh), rows 2^20 and 2^22, vclip 0.2, vf_coef 0.5, ent_coef 0.01.  The method is
tools/policy_grad_rate.py's: every (net, rows) is a child process under a time limit of its own, and the first that fails or runs out of
time ends the run; 3 warm-up rounds, then 7 rounds with the paths interleaved; each sample is a host clock around CALLS back-to-back
calls ending in a device synchronise, in milliseconds per call; median with min..max.  No kernel-only trace is taken.
python3 tools/policy_grad_ac_rate.py [OUT.json] [--rows 1048576,4194304]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"18-64-64-4": [64, 64], "18-128-128-4": [128, 128]}
WARMUP, ROUNDS, CALLS = 3, 7, 3
STEP_LIMIT = 400                                 # seconds per child process
CLIP, VCLIP, VF_COEF, ENT_COEF = 0.2, 0.2, 0.5, 0.01


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}


def child(net, rows):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPCritic, MLPPolicy, pack_weights, unpack_weights
    dev = torch.device("cuda", 0)
    widths = NETS[net]
    rng = np.random.RandomState(0)

    def make(n_out):
        dims = [18] + widths + [n_out]
        return [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
                for k in range(len(dims) - 1)]
    layers, clayers = make(4), make(1)
    W = widths[-1]
    head = np.concatenate([rng.randn(W) / np.sqrt(W), [0.1]]).astype(np.float32)
    log_std = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
    env = QuadrotorEnv(num_envs=64, seed=0)
    pol = MLPPolicy.from_arrays(env, layers, "tanh", True, log_std=log_std, engine="mfma", value=(head[:W], head[W]))
    crit = MLPCritic.from_arrays(env, clayers, "tanh")
    torch.manual_seed(0)
    obs = torch.randn((rows, 18), device=dev)
    mean_t = torch.empty((rows, 4), device=dev)
    _, v0 = pol.evaluate_dev(obs, torch.zeros((rows, 4), device=dev), mean=mean_t)
    std = torch.as_tensor(np.exp(log_std), device=dev)
    z = torch.randn((rows, 4), device=dev)
    actions = (mean_t + 0.15 * std * torch.randn((rows, 4), device=dev) + std * z).contiguous()
    logp_old = ((-0.5 * z * z).sum(dim=1) - float(log_std.sum()) - 2.0 * float(np.log(2.0 * np.pi))).contiguous()
    adv = torch.randn(rows, device=dev)
    ret = (v0 + 0.5 * torch.randn(rows, device=dev)).contiguous()
    v_old = (v0 + 0.25 * torch.randn(rows, device=dev)).contiguous()
    del mean_t, z, v0
    grad, gv, gls, st = pol.ppo_ac_grad_dev(obs, actions, logp_old, adv, ret, v_old, clip=CLIP, vclip=VCLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF)
    pgrad, pgls, pst = pol.ppo_grad_dev(obs, actions, logp_old, adv, clip=CLIP)
    cgrad, cst = crit.mse_grad_dev(obs, ret)

    theta = torch.as_tensor(pack_weights(layers), device=dev).requires_grad_(True)
    hd = torch.as_tensor(head, device=dev).requires_grad_(True)
    ls = torch.as_tensor(log_std, device=dev).requires_grad_(True)
    chunk = rows                                                    # halved below until a forward + backward fits

    def torch_once():
        theta.grad, hd.grad, ls.grad = None, None, None
        for r0 in range(0, rows, chunk):
            views = unpack_weights(theta, 18, widths, 4)
            y = obs[r0:r0 + chunk]
            for Wl, b in views[:-1]:
                y = torch.tanh(F.linear(y, Wl, b))
            m = torch.tanh(F.linear(y, views[-1][0], views[-1][1]))
            v = y @ hd[:W] + hd[W]
            zz = (actions[r0:r0 + chunk] - m) * torch.exp(-ls)
            lp = (-0.5 * zz * zz - ls).sum(dim=1) - 2.0 * float(np.log(2.0 * np.pi))
            r = torch.exp(lp - logp_old[r0:r0 + chunk])
            a, rt, vo = adv[r0:r0 + chunk], ret[r0:r0 + chunk], v_old[r0:r0 + chunk]
            e1, e2 = v - rt, vo + torch.clamp(v - vo, -VCLIP, VCLIP) - rt
            n = y.shape[0]
            loss = (-torch.minimum(r * a, torch.clamp(r, 1.0 - CLIP, 1.0 + CLIP) * a).sum()
                    + VF_COEF * 0.5 * torch.maximum(e1 * e1, e2 * e2).sum() - ENT_COEF * n * ls.sum()) / rows
            loss.backward()

    while True:
        try:
            torch_once()
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            chunk //= 2
            torch.cuda.empty_cache()
    agree = {"grad": float((theta.grad - grad).abs().max() / grad.abs().max()), "grad_value": float((hd.grad - gv).abs().max() / gv.abs().max()),
             "grad_log_std": float((ls.grad - gls).abs().max() / gls.abs().max())}

    def ac():
        pol.ppo_ac_grad_dev(obs, actions, logp_old, adv, ret, v_old, clip=CLIP, vclip=VCLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF, grad=grad,
                            grad_value=gv, grad_log_std=gls, stats=st)

    def ppo():
        pol.ppo_grad_dev(obs, actions, logp_old, adv, clip=CLIP, grad=pgrad, grad_log_std=pgls, stats=pst)

    def mse():
        crit.mse_grad_dev(obs, ret, grad=cgrad, stats=cst)

    def both():
        ppo()
        mse()
    paths = {"ac": ac, "torch": torch_once, "ppo": ppo, "mse": mse, "ppo_then_mse": both}
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
    print(json.dumps({"net": net, "rows": rows, "parameters": int(theta.numel() + hd.numel()), "torch_chunk_rows": chunk,
                      "torch_vs_dev_max_rel_diff": agree, "times": times}), flush=True)
    pol.close(); crit.close(); env.close()


def step(net, rows):
    """one (net, rows): a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", net, "--rows", str(rows)]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("policy_grad_ac_rate: %s at %d rows ran past %d s; nothing more is started on the device" % (net, rows, STEP_LIMIT))
    if out.returncode:
        sys.exit("policy_grad_ac_rate: %s at %d rows ended with status %d; nothing more is started on the device" % (net, rows, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r31_policy_grad_ac.json"))
    ap.add_argument("--rows", default="%d,%d" % (1 << 20, 1 << 22))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, int(args.rows))
    res = {"warmup_rounds": WARMUP, "rounds": ROUNDS, "calls_per_sample": CALLS, "unit": "ms per call",
           "kernel_only_trace": "none taken: host clocks around whole calls",
           "config": "tanh nets with output tanh and a value head, Gaussian rows, behaviour means 0.15 sigma off, clip %g, vclip %g, vf_coef %g, "
                     "ent_coef %g, scale 1 / rows" % (CLIP, VCLIP, VF_COEF, ENT_COEF), "cases": []}
    for net in NETS:
        for rows in (int(x) for x in args.rows.split(",")):
            row = step(net, rows)
            case = {k: row[k] for k in ("net", "rows", "parameters", "torch_chunk_rows", "torch_vs_dev_max_rel_diff")}
            case.update({k: stats(v) for k, v in row["times"].items()})
            case["torch_over_ac"] = round(case["torch"]["ms_median"] / case["ac"]["ms_median"], 2)
            case["ac_over_ppo"] = round(case["ac"]["ms_median"] / case["ppo"]["ms_median"], 3)
            case["ac_over_ppo_plus_mse"] = round(case["ac"]["ms_median"] / (case["ppo"]["ms_median"] + case["mse"]["ms_median"]), 3)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
