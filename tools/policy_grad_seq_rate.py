#!/usr/bin/env python3
"""The truncated-BPTT gradient of the combined PPO loss of a GRU actor-critic over stored sequences on one device:
GRUPolicy.ppo_seq_grad_dev (one tile kernel + one reduction) and evaluate_seq_dev (the forward pass alone) against, interleaved in the
same run,
  torch         torch fp32 forward + backward of the same loss: a torch.gru_cell loop of T steps with torch.where resets on views of one
                packed parameter tensor (unpack_gru_weights), F.linear head layers, a value head, loss.backward(); chunked over the
                sequences (never over time) as far as memory requires, the chunk recorded
Nets 18-GRU64-4 and 18-GRU64-64-4 (tanh, output tanh) with a value head; T = 16 and 64; S = 65536 and 2^20; 5 % dones; vclip 0.2,
vf_coef 0.5, ent_coef 0.01.  The method is tools/policy_grad_rate.py's: every (net, T, S) is a child process under a time limit of its
own, and the first that fails or runs out of time ends the run; 3 warm-up rounds, then 7 rounds with the paths interleaved; each sample
is a host clock around CALLS back-to-back calls ending in a device synchronise, in milliseconds per call; median with min..max.  No
kernel-only trace is taken.  Beside each time stand the FLOP floor -- forward + recompute + dW + dh = 4 x the cell's forward
2 x 3H (D + H) FLOPs per row-step -- and the read-modify-write traffic of the workgroups' partials, 8 bytes x the partial's words per
(tile, t).
python3 tools/policy_grad_seq_rate.py [OUT.json] [--sizes 16x65536,64x65536,16x1048576,64x1048576]
--wide: the wide recurrent learner (gaq.h "the wide recurrent learner") instead -- the nets 18-GRU128-4 and 18-GRU128-64-4 through
ppo_seq_wide_grad_dev and evaluate_seq_wide_dev against the same torch loop, then the two H = 64 nets through the wide calls beside the
narrow ones (seq_wide, eval_wide beside seq, eval; no torch path: the default run has it), which shows what the group loop costs at one
group.  OUT.json is then required."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"18-GRU64-4": (64, []), "18-GRU64-64-4": (64, [64])}
WIDE_NETS = {"18-GRU128-4": (128, []), "18-GRU128-64-4": (128, [64])}
WARMUP, ROUNDS, CALLS = 3, 7, 2
STEP_LIMIT = 400                                 # seconds per child process
CLIP, VCLIP, VF_COEF, ENT_COEF = 0.2, 0.2, 0.5, 0.01
D = 18


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}


def child(net, T, S, wide=False):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import GRUPolicy, pack_gru_weights, unpack_gru_weights
    dev = torch.device("cuda", 0)
    H, hw = WIDE_NETS[net] if net in WIDE_NETS else NETS[net]
    beside = wide and H <= 64                                       # --wide at one group: the wide calls beside the narrow ones
    rng = np.random.RandomState(0)
    gru = tuple((0.3 * rng.randn(*s)).astype(np.float32) for s in ((3 * H, D), (3 * H, H), (3 * H,), (3 * H,)))
    dims = [H] + hw + [4]
    head = [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
            for k in range(len(dims) - 1)]
    W = dims[-2]
    vh = np.concatenate([rng.randn(W) / np.sqrt(W), [0.1]]).astype(np.float32)
    log_std = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
    env = QuadrotorEnv(num_envs=64, seed=0)
    pol = GRUPolicy(env, gru, head, "tanh", True, log_std=log_std, value=(vh[:W], vh[W]))
    grad_call, eval_call = (pol.ppo_seq_wide_grad_dev, pol.evaluate_seq_wide_dev) if H > 64 else (pol.ppo_seq_grad_dev, pol.evaluate_seq_dev)
    torch.manual_seed(0)
    obs = torch.randn((T, S, D), device=dev)
    done = (torch.rand((T, S), device=dev) < 0.05).to(torch.uint8)
    h0 = 0.5 * torch.randn((S, H), device=dev)
    mean_t = torch.empty((T, S, 4), device=dev)
    pol.set_log_std(None)
    _, v0 = eval_call(obs, None, done, h0, mean=mean_t)
    pol.set_log_std(log_std)
    std = torch.as_tensor(np.exp(log_std), device=dev)
    z = torch.randn((T, S, 4), device=dev)
    actions = (mean_t + 0.15 * std * torch.randn((T, S, 4), device=dev) + std * z).contiguous()
    logp_old = ((-0.5 * z * z).sum(dim=2) - float(log_std.sum()) - 2.0 * float(np.log(2.0 * np.pi))).contiguous()
    adv = torch.randn((T, S), device=dev)
    ret = (v0 + 0.5 * torch.randn((T, S), device=dev)).contiguous()
    v_old = (v0 + 0.25 * torch.randn((T, S), device=dev)).contiguous()
    del mean_t, z, v0
    kw = dict(clip=CLIP, vclip=VCLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF)
    grad, gv, gls, st = grad_call(obs, actions, done, h0, logp_old, adv, ret, v_old, **kw)
    lp, val = eval_call(obs, actions, done, h0)

    theta = torch.as_tensor(pack_gru_weights(gru, head), device=dev).requires_grad_(True)
    hd = torch.as_tensor(vh, device=dev).requires_grad_(True)
    ls = torch.as_tensor(log_std, device=dev).requires_grad_(True)
    chunk = S                                                       # halved below until a forward + backward fits

    def torch_once():
        theta.grad, hd.grad, ls.grad = None, None, None
        for s0 in range(0, S, chunk):
            sl = slice(s0, s0 + chunk)
            (W_ih, W_hh, b_ih, b_hh), layers = unpack_gru_weights(theta, D, H, hw)
            h = h0[sl]
            loss = 0.0
            for t in range(T):
                if t > 0:
                    h = torch.where(done[t - 1, sl, None] != 0, torch.zeros_like(h), h)
                h = torch.gru_cell(obs[t, sl], h, W_ih, W_hh, b_ih, b_hh)
                y = h
                for Wl, b in layers[:-1]:
                    y = torch.tanh(F.linear(y, Wl, b))
                m = torch.tanh(F.linear(y, layers[-1][0], layers[-1][1]))
                v = y @ hd[:W] + hd[W]
                zz = (actions[t, sl] - m) * torch.exp(-ls)
                lpt = (-0.5 * zz * zz - ls).sum(dim=1) - 2.0 * float(np.log(2.0 * np.pi))
                r = torch.exp(lpt - logp_old[t, sl])
                a, rt, vo = adv[t, sl], ret[t, sl], v_old[t, sl]
                e1, e2 = v - rt, vo + torch.clamp(v - vo, -VCLIP, VCLIP) - rt
                loss = loss + (-torch.minimum(r * a, torch.clamp(r, 1.0 - CLIP, 1.0 + CLIP) * a).sum()
                               + VF_COEF * 0.5 * torch.maximum(e1 * e1, e2 * e2).sum() - ENT_COEF * y.shape[0] * ls.sum())
            (loss / (T * S)).backward()

    if not beside:
        while True:
            try:
                torch_once()
                torch.cuda.synchronize()
                break
            except torch.cuda.OutOfMemoryError:
                chunk //= 2
                torch.cuda.empty_cache()
    agree = None if beside else {"grad": float((theta.grad - grad).abs().max() / grad.abs().max()), "grad_value": float((hd.grad - gv).abs().max() / gv.abs().max()),
             "grad_log_std": float((ls.grad - gls).abs().max() / gls.abs().max())}

    def seq():
        grad_call(obs, actions, done, h0, logp_old, adv, ret, v_old, grad=grad, grad_value=gv, grad_log_std=gls, stats=st, **kw)

    def fwd():
        eval_call(obs, actions, done, h0, logp=lp, value=val)

    def seq_wide():
        pol.ppo_seq_wide_grad_dev(obs, actions, done, h0, logp_old, adv, ret, v_old, grad=grad, grad_value=gv, grad_log_std=gls, stats=st, **kw)

    def fwd_wide():
        pol.evaluate_seq_wide_dev(obs, actions, done, h0, logp=lp, value=val)
    paths = {"seq": seq, "seq_wide": seq_wide, "eval": fwd, "eval_wide": fwd_wide} if beside else {"seq": seq, "eval": fwd, "torch": torch_once}
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
    words = int(theta.numel() + hd.numel())
    tiles = (S + 63) // 64
    print(json.dumps({"net": net, "T": T, "S": S, "parameters": words, "torch_chunk_sequences": chunk, "torch_vs_dev_max_rel_diff": agree,
                      "flop_floor": 4 * 2 * 3 * H * (D + H) * T * S, "partial_rmw_bytes": 8 * words * tiles * T,
                      "tape_bytes": min(tiles, 512) * T * 64 * H * 4, "times": times}), flush=True)
    pol.close(); env.close()


def step(net, T, S, wide=False):
    """one (net, T, S): a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", net, "--sizes", "%dx%d" % (T, S)] + (["--wide"] if wide else [])
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("policy_grad_seq_rate: %s at (%d, %d) ran past %d s; nothing more is started on the device" % (net, T, S, STEP_LIMIT))
    if out.returncode:
        sys.exit("policy_grad_seq_rate: %s at (%d, %d) ended with status %d; nothing more is started on the device" % (net, T, S, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--wide", action="store_true", help="the wide recurrent learner's nets, and H = 64 through the wide calls beside the narrow")
    ap.add_argument("--sizes", default="16x65536,64x65536,16x1048576,64x1048576", help="T x S, comma-separated")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in x.split("x")) for x in args.sizes.split(",")]
    if args.child:
        return child(args.child, *sizes[0], wide=args.wide)
    if args.out is None:
        if args.wide:
            ap.error("--wide needs OUT.json")
        args.out = os.path.join(ROOT, "profiles", "r32_policy_grad_seq.json")
    res = {"warmup_rounds": WARMUP, "rounds": ROUNDS, "calls_per_sample": CALLS, "unit": "ms per call",
           "kernel_only_trace": "none taken: host clocks around whole calls",
           "config": "tanh GRU nets with output tanh and a value head, Gaussian observations and h0, 5 %% dones, behaviour means 0.15 sigma "
                     "off, clip %g, vclip %g, vf_coef %g, ent_coef %g, scale 1 / (T S)" % (CLIP, VCLIP, VF_COEF, ENT_COEF), "cases": []}
    for net in (list(WIDE_NETS) + list(NETS) if args.wide else NETS):
        for T, S in sizes:
            row = step(net, T, S, args.wide)
            case = {k: v for k, v in row.items() if k != "times"}
            case.update({k: stats(v) for k, v in row["times"].items()})
            if "torch" in case:
                case["torch_over_seq"] = round(case["torch"]["ms_median"] / case["seq"]["ms_median"], 2)
            else:
                case["seq_wide_over_seq"] = round(case["seq_wide"]["ms_median"] / case["seq"]["ms_median"], 3)
                case["eval_wide_over_eval"] = round(case["eval_wide"]["ms_median"] / case["eval"]["ms_median"], 3)
            case["seq_tflops_at_floor"] = round(row["flop_floor"] / (case["seq"]["ms_median"] * 1e-3) / 1e12, 2)
            case["partial_rmw_gb_per_s"] = round(row["partial_rmw_bytes"] / (case["seq"]["ms_median"] * 1e-3) / 1e9, 1)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
