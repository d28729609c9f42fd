#!/usr/bin/env python3
"""The wide learner's gradient calls on one device (gaq.h "the wide learner"): MLPPolicy.ppo_wide_grad_dev on a policy with a value
head and MLPCritic.mse_wide_grad_dev, contiguous and index-gathered (a perm_dev permutation of the rows), against, interleaved in the
same run,
  torch         torch fp32 forward + backward of the same loss on the same packed parameters (F.linear layers on views of one packed
                tensor, loss.backward(); chunked over the rows only as far as memory requires; the idx form gathers with obs[idx])
  narrow        on a net the narrow calls take (18-128-128), ppo_ac_grad_dev / mse_grad_dev and their idx forms on the same handle:
                the cost of the new form (the bits are equal)
Nets 18-256-256-4 (the flagship width) and 18-128-128-4, tanh with output tanh, rows 2^14 and 2^20, vclip 0.2, vf_coef 0.5, ent_coef
0.01.  The method is tools/policy_grad_rate.py's: every (net, rows) is a child process under a time limit of its own, and the first that
fails or runs out of time ends the run; 3 warm-up rounds, then 7 rounds with the paths interleaved; each sample is a host clock around
CALLS back-to-back calls ending in a device synchronise, in milliseconds per call; median with min..max.  No kernel-only trace is taken.
Recorded beside the times: the FLOP floor 6 P rows, and the bytes a tile reads and writes of its workgroup's partial (2 x 4 P').
python3 tools/policy_grad_wide_rate.py OUT.json [--rows 16384,1048576]    (OUT.json is required: a run never overwrites a committed record by default)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"18-256-256-4": [256, 256], "18-128-128-4": [128, 128]}
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
    from gym_art_amd.policy import MLPCritic, MLPPolicy, pack_critic_weights, pack_weights, perm_dev, unpack_weights
    dev = torch.device("cuda", 0)
    widths = NETS[net]
    narrow = max(widths) <= 128
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
    _, v0 = pol.evaluate_wide_dev(obs, torch.zeros((rows, 4), device=dev), mean=mean_t)
    std = torch.as_tensor(np.exp(log_std), device=dev)
    z = torch.randn((rows, 4), device=dev)
    actions = (mean_t + 0.15 * std * torch.randn((rows, 4), device=dev) + std * z).contiguous()
    logp_old = ((-0.5 * z * z).sum(dim=1) - float(log_std.sum()) - 2.0 * float(np.log(2.0 * np.pi))).contiguous()
    adv = torch.randn(rows, device=dev)
    ret = (v0 + 0.5 * torch.randn(rows, device=dev)).contiguous()
    v_old = (v0 + 0.25 * torch.randn(rows, device=dev)).contiguous()
    del mean_t, z, v0
    idx = perm_dev(rows, 7, device=dev)
    lidx = idx.long()
    coef = dict(clip=CLIP, vclip=VCLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF)
    rowsets = (obs, actions, logp_old, adv, ret, v_old)
    grad, gv, gls, st = pol.ppo_wide_grad_dev(*rowsets, **coef)
    st7 = pol.ppo_wide_grad_dev(*rowsets, idx=idx, **coef)[3]
    cgrad, cst = crit.mse_wide_grad_dev(obs, ret)
    cst3 = crit.mse_wide_grad_dev(obs, ret, idx=idx)[1]

    theta = torch.as_tensor(pack_weights(layers), device=dev).requires_grad_(True)
    hd = torch.as_tensor(head, device=dev).requires_grad_(True)
    ls = torch.as_tensor(log_std, device=dev).requires_grad_(True)
    ctheta = torch.as_tensor(pack_critic_weights(clayers), device=dev).requires_grad_(True)
    chunk = [rows]                                                  # halved below until a forward + backward fits

    def torch_ac(gather=False):
        theta.grad, hd.grad, ls.grad = None, None, None
        for r0 in range(0, rows, chunk[0]):
            sl = lidx[r0:r0 + chunk[0]] if gather else slice(r0, r0 + chunk[0])
            views = unpack_weights(theta, 18, widths, 4)
            y = obs[sl]
            for Wl, b in views[:-1]:
                y = torch.tanh(F.linear(y, Wl, b))
            m = torch.tanh(F.linear(y, views[-1][0], views[-1][1]))
            v = y @ hd[:W] + hd[W]
            zz = (actions[sl] - m) * torch.exp(-ls)
            lp = (-0.5 * zz * zz - ls).sum(dim=1) - 2.0 * float(np.log(2.0 * np.pi))
            r = torch.exp(lp - logp_old[sl])
            a, rt, vo = adv[sl], ret[sl], v_old[sl]
            e1, e2 = v - rt, vo + torch.clamp(v - vo, -VCLIP, VCLIP) - rt
            loss = (-torch.minimum(r * a, torch.clamp(r, 1.0 - CLIP, 1.0 + CLIP) * a).sum()
                    + VF_COEF * 0.5 * torch.maximum(e1 * e1, e2 * e2).sum() - ENT_COEF * y.shape[0] * ls.sum()) / rows
            loss.backward()

    def torch_mse(gather=False):
        ctheta.grad = None
        for r0 in range(0, rows, chunk[0]):
            sl = lidx[r0:r0 + chunk[0]] if gather else slice(r0, r0 + chunk[0])
            views = unpack_weights(ctheta, 18, widths, 1)
            y = obs[sl]
            for Wl, b in views[:-1]:
                y = torch.tanh(F.linear(y, Wl, b))
            e = F.linear(y, views[-1][0], views[-1][1])[:, 0] - ret[sl]
            (0.5 * (e * e).sum() / rows).backward()

    while True:
        try:
            torch_ac(True)
            torch_mse(True)
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            chunk[0] //= 2
            torch.cuda.empty_cache()
    torch_ac()
    torch_mse()
    agree = {"grad": float((theta.grad - grad).abs().max() / grad.abs().max()), "grad_value": float((hd.grad - gv).abs().max() / gv.abs().max()),
             "grad_log_std": float((ls.grad - gls).abs().max() / gls.abs().max()),
             "critic_grad": float((ctheta.grad - cgrad).abs().max() / cgrad.abs().max())}

    out = dict(grad=grad, grad_value=gv, grad_log_std=gls)
    paths = {
        "wide": lambda: pol.ppo_wide_grad_dev(*rowsets, stats=st, **out, **coef),
        "wide_idx": lambda: pol.ppo_wide_grad_dev(*rowsets, idx=idx, stats=st7, **out, **coef),
        "torch": torch_ac,
        "torch_idx": lambda: torch_ac(True),
        "critic_wide": lambda: crit.mse_wide_grad_dev(obs, ret, grad=cgrad, stats=cst),
        "critic_wide_idx": lambda: crit.mse_wide_grad_dev(obs, ret, idx=idx, grad=cgrad, stats=cst3),
        "critic_torch": torch_mse,
        "critic_torch_idx": lambda: torch_mse(True),
    }
    if narrow:
        paths.update({
            "narrow": lambda: pol.ppo_ac_grad_dev(*rowsets, stats=st, **out, **coef),
            "narrow_idx": lambda: pol.ppo_ac_grad_idx_dev(idx, *rowsets, stats=st7, **out, **coef),
            "critic_narrow": lambda: crit.mse_grad_dev(obs, ret, grad=cgrad, stats=cst),
            "critic_narrow_idx": lambda: crit.mse_grad_idx_dev(idx, obs, ret, grad=cgrad, stats=cst3),
        })
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
    P, Pc = int(theta.numel() + hd.numel()), int(ctheta.numel())
    print(json.dumps({"net": net, "rows": rows, "parameters": P, "critic_parameters": Pc, "torch_chunk_rows": chunk[0],
                      "flop_floor": 6 * P * rows, "critic_flop_floor": 6 * Pc * rows,
                      "partial_rmw_bytes_per_tile": 8 * ((P + 15) & ~15), "critic_partial_rmw_bytes_per_tile": 8 * ((Pc + 15) & ~15),
                      "torch_vs_dev_max_rel_diff": agree, "times": times}), flush=True)
    pol.close(); crit.close(); env.close()


def step(net, rows):
    """one (net, rows): a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", net, "--rows", str(rows)]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("policy_grad_wide_rate: %s at %d rows ran past %d s; nothing more is started on the device" % (net, rows, STEP_LIMIT))
    if out.returncode:
        sys.exit("policy_grad_wide_rate: %s at %d rows ended with status %d; nothing more is started on the device" % (net, rows, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None, help="the JSON file to write (required unless --child)")
    ap.add_argument("--rows", default="%d,%d" % (1 << 14, 1 << 20))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, int(args.rows))
    if not args.out:
        ap.error("OUT.json is required")
    res = {"warmup_rounds": WARMUP, "rounds": ROUNDS, "calls_per_sample": CALLS, "unit": "ms per call",
           "kernel_only_trace": "none taken: host clocks around whole calls",
           "config": "tanh nets with output tanh and a value head, and a critic of the same hidden shape; Gaussian rows, behaviour means 0.15 "
                     "sigma off, clip %g, vclip %g, vf_coef %g, ent_coef %g, scale 1 / rows; idx = perm_dev(rows)" % (CLIP, VCLIP, VF_COEF, ENT_COEF),
           "cases": []}
    for net in NETS:
        for rows in (int(x) for x in args.rows.split(",")):
            row = step(net, rows)
            case = {k: v for k, v in row.items() if k != "times"}
            case.update({k: stats(v) for k, v in row["times"].items()})
            med = lambda k: case[k]["ms_median"]
            case["torch_over_wide"] = round(med("torch") / med("wide"), 2)
            case["torch_idx_over_wide_idx"] = round(med("torch_idx") / med("wide_idx"), 2)
            case["critic_torch_over_wide"] = round(med("critic_torch") / med("critic_wide"), 2)
            case["critic_torch_idx_over_wide_idx"] = round(med("critic_torch_idx") / med("critic_wide_idx"), 2)
            case["wide_tflops_of_floor"] = round(case["flop_floor"] / (med("wide") * 1e-3) / 1e12, 2)
            if "narrow" in case:
                case["wide_over_narrow"] = round(med("wide") / med("narrow"), 3)
                case["wide_idx_over_narrow_idx"] = round(med("wide_idx") / med("narrow_idx"), 3)
                case["critic_wide_over_narrow"] = round(med("critic_wide") / med("critic_narrow"), 3)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
