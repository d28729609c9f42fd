#!/usr/bin/env python3
"""One minibatch iteration of a recurrent actor-critic with an encoder over stored sequences on one device: ppo_enc_seq_grad_dev (the
split passes: encoder forward over the T S rows, the cell's sequence kernel with dfeat, its reduce, the encoder's backward over the
rows, its reduce) + AdamEncDev.step (two launches, four groups, joint clip) against, interleaved in the same run,
  plain         the encoder-less sequence gradient of the same cell, H and head on the 18-wide observation + AdamDev.step, for scale:
                what the serial sequence kernel costs alone
  torch         torch fp32 forward + backward of the same loss on the device: F.linear encoder layers over all T S rows at once, a
                torch.gru_cell / torch.lstm_cell loop of T steps with torch.where resets on views of the two packed parameter tensors,
                F.linear head layers, a value head, loss.backward(), clip_grad_norm_ + torch.optim.Adam.step() on the three tensors,
                then set_weights_dev + set_encoder_weights_dev (the two uploads a torch learner pays per minibatch); chunked over
                the sequences as far as memory requires, the chunk recorded
  enc_grad      the gradient call alone, without the optimiser's step
Nets 18-enc64-GRU64-64-4 and 18-enc64-64-LSTM64-4 (tanh, output tanh) with a value head; 5 % dones; vclip 0.2, vf_coef 0.5, ent_coef
0.01; lr 1e-5 (the weights move, the timing does not depend on it), max_grad_norm 0.5, log_std not stepped.  The method is
tools/policy_grad_lstm_rate.py's: every (net, T, S) is a child process under a time limit of its own, and the first that fails or runs
out of time ends the run; 3 warm-up rounds, then 7 rounds with the paths interleaved; each sample is a host clock around CALLS
back-to-back calls ending in a device synchronise, in milliseconds per call; median with min..max.  For the split into passes run one
child under `rocprofv3 --kernel-trace --stats -- python3 tools/policy_grad_enc_rate.py --child NET --sizes TxS`.
python3 tools/policy_grad_enc_rate.py [OUT.json] [--sizes 16x65536,64x65536]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"18-enc64-GRU64-64-4": ("gru", [64], 64, [64]), "18-enc64-64-LSTM64-4": ("lstm", [64, 64], 64, [])}
WARMUP, ROUNDS, CALLS = 3, 7, 2
STEP_LIMIT = 400                                 # seconds per child process
CLIP, VCLIP, VF_COEF, ENT_COEF = 0.2, 0.2, 0.5, 0.01
D = 18


def stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}


def measure(paths):
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


def child(net, T, S):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd import policy as P
    dev = torch.device("cuda", 0)
    cell, ew, H, hw = NETS[net]
    G = 3 if cell == "gru" else 4
    E = ew[-1]
    rng = np.random.RandomState(0)
    edims = [D] + ew
    enc = [((rng.randn(edims[k + 1], edims[k]) / np.sqrt(edims[k])).astype(np.float32), (0.1 * rng.randn(edims[k + 1])).astype(np.float32))
           for k in range(len(ew))]
    mk = lambda I: tuple((0.3 * rng.randn(*s)).astype(np.float32) for s in ((G * H, I), (G * H, H), (G * H,), (G * H,)))
    cw, cw_plain = mk(E), mk(D)
    dims = [H] + hw + [4]
    head = [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
            for k in range(len(dims) - 1)]
    W = dims[-2]
    vh = np.concatenate([rng.randn(W) / np.sqrt(W), [0.1]]).astype(np.float32)
    log_std = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
    env = QuadrotorEnv(num_envs=64, seed=0)
    cls = P.GRUPolicy if cell == "gru" else P.LSTMPolicy
    pol = cls.with_encoder(env, enc, cw, head, "tanh", True, log_std=log_std, value=(vh[:W], vh[W]))
    plain = cls(env, cw_plain, head, "tanh", True, log_std=log_std, value=(vh[:W], vh[W]))
    torch.manual_seed(0)
    obs = torch.randn((T, S, D), device=dev)
    done = (torch.rand((T, S), device=dev) < 0.05).to(torch.uint8)
    s0 = [0.5 * torch.randn((S, H), device=dev) for _ in pol.CELL.states]
    mean_t = torch.empty((T, S, 4), device=dev)
    pol.set_log_std(None)
    _, v0 = pol.evaluate_enc_seq_dev(obs, None, done, *s0, mean=mean_t)
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
    grad, genc, gv, gls, st = pol.ppo_enc_seq_grad_dev(obs, actions, done, *s0, logp_old, adv, ret, v_old, **kw)
    plain_call = plain.ppo_seq_grad_dev if cell == "gru" else plain.ppo_bptt_grad_dev
    pgrad, pgv, pgls, pst = plain_call(obs, actions, done, *s0, logp_old, adv, ret, v_old, **kw)

    theta = torch.as_tensor(P.pack_gru_weights(cw, head), device=dev).requires_grad_(True)
    theta_e = torch.as_tensor(P.pack_encoder_weights(enc), device=dev).requires_grad_(True)
    hd = torch.as_tensor(vh, device=dev).requires_grad_(True)
    ls = torch.as_tensor(log_std, device=dev).requires_grad_(True)
    unpack = P.unpack_gru_weights if cell == "gru" else P.unpack_lstm_weights
    step_fn = torch.gru_cell if cell == "gru" else torch.lstm_cell
    chunk = S
    topt = torch.optim.Adam([theta, theta_e, hd], lr=1e-5)
    opt = P.AdamEncDev(pol, lr=1e-5, max_grad_norm=0.5, learn_log_std=False)
    popt = P.AdamDev(plain, lr=1e-5, max_grad_norm=0.5, learn_log_std=False)

    def torch_once(step=True):
        theta.grad, theta_e.grad, hd.grad, ls.grad = None, None, None, None
        for a0 in range(0, S, chunk):
            sl = slice(a0, a0 + chunk)
            (W_ih, W_hh, b_ih, b_hh), layers = unpack(theta, E, H, hw)
            y = obs[:, sl]
            for We, be in P.unpack_encoder_weights(theta_e, D, ew):
                y = torch.tanh(F.linear(y, We, be))
            feat = y
            state = [s[sl] for s in s0]
            loss = 0.0
            for t in range(T):
                if t > 0:
                    cut = done[t - 1, sl, None] != 0
                    state = [torch.where(cut, torch.zeros_like(s), s) for s in state]
                out = step_fn(feat[t], state[0] if cell == "gru" else tuple(state), W_ih, W_hh, b_ih, b_hh)
                state = [out] if cell == "gru" else list(out)
                y = state[0]
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
        if not step:
            return
        torch.nn.utils.clip_grad_norm_([theta, theta_e, hd], 0.5)
        topt.step()
        pol.set_weights_dev(theta.detach())
        pol.set_encoder_weights_dev(theta_e.detach())

    while True:
        try:
            torch_once(step=False)
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            chunk //= 2
            torch.cuda.empty_cache()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    agree = {"grad": rel(theta.grad, grad), "grad_encoder": rel(theta_e.grad, genc), "grad_value": rel(hd.grad, gv),
             "grad_log_std": rel(ls.grad, gls)}

    def enc_grad():
        pol.ppo_enc_seq_grad_dev(obs, actions, done, *s0, logp_old, adv, ret, v_old, grad=grad, grad_encoder=genc, grad_value=gv,
                                 grad_log_std=gls, stats=st, **kw)

    def enc_call():
        enc_grad()
        opt.step(grad, genc, gv)

    def plain_once():
        plain_call(obs, actions, done, *s0, logp_old, adv, ret, v_old, grad=pgrad, grad_value=pgv, grad_log_std=pgls, stats=pst, **kw)
        popt.step(pgrad, pgv)
    times = measure({"enc": enc_call, "plain": plain_once, "torch": torch_once, "enc_grad": enc_grad})
    print(json.dumps({"net": net, "T": T, "S": S, "parameters": int(theta.numel() + hd.numel()), "encoder_parameters": int(theta_e.numel()),
                      "torch_chunk_sequences": chunk, "torch_vs_dev_max_rel_diff": agree, "feat_and_dfeat_traffic_bytes": 4 * T * S * E * 4,
                      "times": times}), flush=True)
    opt.close(); popt.close(); plain.close(); pol.close(); env.close()


def step(net, T, S):
    """one (net, T, S): a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", net, "--sizes", "%dx%d" % (T, S)]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("policy_grad_enc_rate: %s at (%d, %d) ran past %d s; nothing more is started on the device" % (net, T, S, STEP_LIMIT))
    if out.returncode:
        sys.exit("policy_grad_enc_rate: %s at (%d, %d) ended with status %d; nothing more is started on the device" % (net, T, S, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r40_policy_grad_enc.json"))
    ap.add_argument("--sizes", default="16x65536,64x65536", help="T x S, comma-separated")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in x.split("x")) for x in args.sizes.split(",")]
    if args.child:
        return child(args.child, *sizes[0])
    res = {"warmup_rounds": WARMUP, "rounds": ROUNDS, "calls_per_sample": CALLS, "unit": "ms per call", "sizes": ["%dx%d" % s for s in sizes],
           "config": "tanh nets with output tanh and a value head, Gaussian observations and states, 5 %% dones, behaviour means 0.15 sigma "
                     "off, clip %g, vclip %g, vf_coef %g, ent_coef %g, scale 1 / (T S); every path but enc_grad ends in its optimiser's step (lr 1e-5, "
                     "max_grad_norm 0.5)"
                     % (CLIP, VCLIP, VF_COEF, ENT_COEF), "cases": []}
    for net in NETS:
        for T, S in sizes:
            row = step(net, T, S)
            case = {k: v for k, v in row.items() if k != "times"}
            case.update({k: stats(v) for k, v in row["times"].items()})
            case["torch_over_enc"] = round(case["torch"]["ms_median"] / case["enc"]["ms_median"], 2)
            case["enc_over_plain"] = round(case["enc"]["ms_median"] / case["plain"]["ms_median"], 3)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
