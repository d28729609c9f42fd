#!/usr/bin/env python3
"""The truncated-BPTT gradient of the combined PPO loss of an LSTM actor-critic over stored sequences on one device:
LSTMPolicy.ppo_bptt_grad_dev (one tile kernel + one reduction) and evaluate_seq_dev (the forward pass alone) against, interleaved in
the same run,
  gru           GRUPolicy.ppo_seq_grad_dev of a GRU of the same H and head on the same data (the expectation to confirm or correct: the
                LSTM call costs about 4/3 of it per row-step, as the cell's FLOPs and the partial's words both do)
  torch         torch fp32 forward + backward of the same loss: a torch.lstm_cell loop of T steps with torch.where resets of h and c on
                views of one packed parameter tensor (unpack_lstm_weights), F.linear head layers, a value head, loss.backward(); chunked
                over the sequences (never over time) as far as memory requires, the chunk recorded
and, with --idx, ppo_bptt_grad_idx_dev on 2^14 of 2^16 sequences against gather + the contiguous call.
Nets 18-LSTM64-4 and 18-LSTM64-64-4 (tanh, output tanh) with a value head; T = 16 and 64; S = 65536 and 2^20; 5 % dones; vclip 0.2,
vf_coef 0.5, ent_coef 0.01.  The method is tools/policy_grad_seq_rate.py's: every (net, T, S) is a child process under a time limit of
its own, and the first that fails or runs out of time ends the run; 3 warm-up rounds, then 7 rounds with the paths interleaved; each
sample is a host clock around CALLS back-to-back calls ending in a device synchronise, in milliseconds per call; median with min..max.
No kernel-only trace is taken.
python3 tools/policy_grad_lstm_rate.py [OUT.json] [--sizes 16x65536,64x65536,16x1048576,64x1048576] [--no-idx]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"18-LSTM64-4": (64, []), "18-LSTM64-64-4": (64, [64])}
WARMUP, ROUNDS, CALLS = 3, 7, 2
STEP_LIMIT = 400                                 # seconds per child process
CLIP, VCLIP, VF_COEF, ENT_COEF = 0.2, 0.2, 0.5, 0.01
D = 18
IDX_SRC, IDX_MB = 1 << 16, 1 << 14


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}


def measure(paths):
    """3 warm-up rounds, then 7 with the paths interleaved: ms per call of each"""
    import torch
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
    return times


def child(net, T, S, idx_mode):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, pack_lstm_weights, unpack_lstm_weights
    dev = torch.device("cuda", 0)
    H, hw = NETS[net]
    rng = np.random.RandomState(0)
    lstm = tuple((0.3 * rng.randn(*s)).astype(np.float32) for s in ((4 * H, D), (4 * H, H), (4 * H,), (4 * H,)))
    gru = tuple(a[:3 * H].copy() for a in lstm)
    dims = [H] + hw + [4]
    head = [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
            for k in range(len(dims) - 1)]
    W = dims[-2]
    vh = np.concatenate([rng.randn(W) / np.sqrt(W), [0.1]]).astype(np.float32)
    log_std = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
    env = QuadrotorEnv(num_envs=64, seed=0)
    pol = LSTMPolicy(env, lstm, head, "tanh", True, log_std=log_std, value=(vh[:W], vh[W]))
    torch.manual_seed(0)
    obs = torch.randn((T, S, D), device=dev)
    done = (torch.rand((T, S), device=dev) < 0.05).to(torch.uint8)
    h0, c0 = 0.5 * torch.randn((S, H), device=dev), 0.5 * torch.randn((S, H), device=dev)
    mean_t = torch.empty((T, S, 4), device=dev)
    pol.set_log_std(None)
    _, v0 = pol.evaluate_seq_dev(obs, None, done, h0, c0, mean=mean_t)
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
    grad, gv, gls, st = pol.ppo_bptt_grad_dev(obs, actions, done, h0, c0, logp_old, adv, ret, v_old, **kw)

    if idx_mode:                                                    # the minibatch call against gather + the contiguous call
        idx = torch.randperm(S, device=dev)[:IDX_MB].to(torch.int32).contiguous()
        st7 = torch.empty(7, dtype=torch.float64, device=dev)

        def by_idx():
            pol.ppo_bptt_grad_idx_dev(idx, obs, actions, done, h0, c0, logp_old, adv, ret, v_old, grad=grad, grad_value=gv, grad_log_std=gls,
                                      stats=st7, **kw)

        def gathered():
            i = idx.long()
            pol.ppo_bptt_grad_dev(obs[:, i].contiguous(), actions[:, i].contiguous(), done[:, i].contiguous(), h0[i].contiguous(),
                                  c0[i].contiguous(), logp_old[:, i].contiguous(), adv[:, i].contiguous(), ret[:, i].contiguous(),
                                  v_old[:, i].contiguous(), grad=grad, grad_value=gv, grad_log_std=gls, stats=st, **kw)
        times = measure({"idx": by_idx, "gather_then_contiguous": gathered})
        print(json.dumps({"net": net, "T": T, "S_src": S, "S": IDX_MB, "times": times}), flush=True)
        pol.close(); env.close()
        return

    lp, val = pol.evaluate_seq_dev(obs, actions, done, h0, c0)
    gpol = GRUPolicy(env, gru, head, "tanh", True, log_std=log_std, value=(vh[:W], vh[W]))
    ggrad, ggv, ggls, gst = gpol.ppo_seq_grad_dev(obs, actions, done, h0, logp_old, adv, ret, v_old, **kw)

    theta = torch.as_tensor(pack_lstm_weights(lstm, head), device=dev).requires_grad_(True)
    hd = torch.as_tensor(vh, device=dev).requires_grad_(True)
    ls = torch.as_tensor(log_std, device=dev).requires_grad_(True)
    chunk = S                                                       # halved below until a forward + backward fits

    def torch_once():
        theta.grad, hd.grad, ls.grad = None, None, None
        for s0 in range(0, S, chunk):
            sl = slice(s0, s0 + chunk)
            (W_ih, W_hh, b_ih, b_hh), layers = unpack_lstm_weights(theta, D, H, hw)
            h, c = h0[sl], c0[sl]
            loss = 0.0
            for t in range(T):
                if t > 0:
                    cut = done[t - 1, sl, None] != 0
                    h, c = torch.where(cut, torch.zeros_like(h), h), torch.where(cut, torch.zeros_like(c), c)
                h, c = torch.lstm_cell(obs[t, sl], (h, c), W_ih, W_hh, b_ih, b_hh)
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

    def bptt():
        pol.ppo_bptt_grad_dev(obs, actions, done, h0, c0, logp_old, adv, ret, v_old, grad=grad, grad_value=gv, grad_log_std=gls, stats=st, **kw)

    def fwd():
        pol.evaluate_seq_dev(obs, actions, done, h0, c0, logp=lp, value=val)

    def gru_call():
        gpol.ppo_seq_grad_dev(obs, actions, done, h0, logp_old, adv, ret, v_old, grad=ggrad, grad_value=ggv, grad_log_std=ggls, stats=gst, **kw)
    times = measure({"lstm": bptt, "eval": fwd, "gru": gru_call, "torch": torch_once})
    words = int(theta.numel() + hd.numel())
    tiles = (S + 63) // 64
    print(json.dumps({"net": net, "T": T, "S": S, "parameters": words, "gru_parameters": int(ggrad.numel() + ggv.numel()),
                      "torch_chunk_sequences": chunk, "torch_vs_dev_max_rel_diff": agree,
                      "flop_floor": 4 * 2 * 4 * H * (D + H) * T * S, "partial_rmw_bytes": 8 * words * tiles * T,
                      "tape_bytes": min(tiles, 512) * T * 64 * 2 * H * 4, "times": times}), flush=True)
    gpol.close(); pol.close(); env.close()


def step(net, T, S, idx_mode=False):
    """one (net, T, S): a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", net, "--sizes", "%dx%d" % (T, S)] + (["--idx-child"] if idx_mode else [])
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("policy_grad_lstm_rate: %s at (%d, %d) ran past %d s; nothing more is started on the device" % (net, T, S, STEP_LIMIT))
    if out.returncode:
        sys.exit("policy_grad_lstm_rate: %s at (%d, %d) ended with status %d; nothing more is started on the device" % (net, T, S, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r36_policy_grad_lstm.json"))
    ap.add_argument("--sizes", default="16x65536,64x65536,16x1048576,64x1048576", help="T x S, comma-separated")
    ap.add_argument("--no-idx", action="store_true", help="leave out the idx call against gather + contiguous")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--idx-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in x.split("x")) for x in args.sizes.split(",")]
    if args.child:
        return child(args.child, *sizes[0], args.idx_child)
    res = {"warmup_rounds": WARMUP, "rounds": ROUNDS, "calls_per_sample": CALLS, "unit": "ms per call",
           "kernel_only_trace": "none taken: host clocks around whole calls", "sizes": ["%dx%d" % s for s in sizes],
           "config": "tanh LSTM nets with output tanh and a value head (the GRU beside them: the same H, head and data), Gaussian "
                     "observations, h0 and c0, 5 %% dones, behaviour means 0.15 sigma off, clip %g, vclip %g, vf_coef %g, ent_coef %g, "
                     "scale 1 / (T S)" % (CLIP, VCLIP, VF_COEF, ENT_COEF), "cases": [], "idx": []}
    for net in NETS:
        for T, S in sizes:
            row = step(net, T, S)
            case = {k: v for k, v in row.items() if k != "times"}
            case.update({k: stats(v) for k, v in row["times"].items()})
            case["torch_over_lstm"] = round(case["torch"]["ms_median"] / case["lstm"]["ms_median"], 2)
            case["lstm_over_gru"] = round(case["lstm"]["ms_median"] / case["gru"]["ms_median"], 3)
            case["lstm_tflops_at_floor"] = round(row["flop_floor"] / (case["lstm"]["ms_median"] * 1e-3) / 1e12, 2)
            case["partial_rmw_gb_per_s"] = round(row["partial_rmw_bytes"] / (case["lstm"]["ms_median"] * 1e-3) / 1e9, 1)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    if not args.no_idx:
        for net in NETS:
            row = step(net, 16, IDX_SRC, idx_mode=True)
            case = {k: v for k, v in row.items() if k != "times"}
            case.update({k: stats(v) for k, v in row["times"].items()})
            case["gather_over_idx"] = round(case["gather_then_contiguous"]["ms_median"] / case["idx"]["ms_median"], 2)
            res["idx"].append(case)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
