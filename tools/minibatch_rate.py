#!/usr/bin/env python3
"""One shuffled-minibatch iteration of the learner on one device -- the minibatch's rows, the gradient call, AdamDev.step -- three ways,
interleaved in the same run:
  gather        the loop as it had to be written before the index-gathered calls: torch.index_select of every input (6 tensors; the
                GRU's 8, its observations a strided [T, S, D] block), the contiguous gradient call on the copies, AdamDev.step
  idx           the *_idx_dev gradient call on the rollout's own buffers, AdamDev.step
  graph         an epoch captured once and replayed: perm_dev(epoch_dev=), EPOCH_MB minibatches of (idx call, AdamDev.step),
                epoch_dev.add_(1); its time is divided by EPOCH_MB, so it carries 1 / EPOCH_MB of the permutation launch
and the gradient calls alone: the idx call on the source buffers against the contiguous call on rows gathered beforehand, whose
difference is the price of reading 72-byte rows at random.  gather and idx walk through the same EPOCH_MB minibatches of one permutation.
Every path has a policy handle and an optimiser of its own (learn_log_std=False, sync_log_std=False on all of them, as a captured loop
needs), so none reads weights another has stepped.
Points: 18-64-64-4 and 18-128-128-128-4 (tanh, output tanh, value head), minibatches of 2^14 and 2^17 rows out of 2^20 and 2^22; the GRU
18-GRU64-64-4 at T = 16 with 2^12 and 2^14 of 2^16 sequences.  The method is tools/optim_rate.py's: every point is a child process
under a time limit of its own, and the first that fails or runs out of time ends the run; 3 warm-up rounds, then 7 rounds with the
paths interleaved; each sample is a host clock around CALLS back-to-back iterations ending in a device synchronise, in microseconds per
minibatch; median with min..max.  No kernel-only trace is taken.
python3 tools/minibatch_rate.py [OUT.json] [--quick]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"18-64-64-4": [64, 64], "18-128-128-128-4": [128, 128, 128]}
GRU = "18-GRU64-64-4"
WARMUP, ROUNDS, CALLS, EPOCH_MB = 3, 7, 8, 4
STEP_LIMIT = 300                                 # seconds per child process
CLIP, VCLIP, VF_COEF, ENT_COEF = 0.2, 0.2, 0.5, 0.01
LR, MAX_NORM = 3e-4, 0.5
KW = dict(clip=CLIP, vclip=VCLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF)


def stats(v):
    v = sorted(v)
    return {"us_median": round(v[len(v) // 2], 1), "us_min": round(v[0], 1), "us_max": round(v[-1], 1)}


def measure(paths):
    """paths: name -> (callable, minibatches per call) -> name -> samples in microseconds per minibatch"""
    import torch
    times = {k: [] for k in paths}
    for rnd in range(WARMUP + ROUNDS):
        for key, (fn, per) in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            if rnd >= WARMUP:
                times[key].append((time.perf_counter() - t0) * 1e6 / (CALLS * per))
    return times


def captured(fn, dev):
    import torch
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    return graph


class Walk:
    """the minibatches of one permutation, one after the other"""

    def __init__(self, perm, mb):
        self.perm, self.mb, self.k = perm, mb, 0

    def next(self):
        k = self.k
        self.k = (k + 1) % EPOCH_MB
        return self.perm[k * self.mb:(k + 1) * self.mb]


def run_paths(dev, src, mb, make, srcs, select, call, call_idx):
    """the five paths of one point.  make(): a new policy; srcs: the source tensors; select(srcs, idx): their gathered copies;
    call(pol, tensors, out) / call_idx(pol, idx, srcs, out): the gradient calls into `out` (None: allocate)"""
    import torch
    from gym_art_amd.policy import AdamDev, perm_dev
    perm = perm_dev(src, 7, device=dev)
    loops = {}
    for name in ("gather", "idx", "graph", "alone_idx", "alone_contiguous"):
        pol = make()
        out = call_idx(pol, perm[:mb], srcs, None)                 # the warm-up: it sizes the handle's scratch
        opt = AdamDev(pol, lr=LR, max_grad_norm=MAX_NORM, learn_log_std=False)
        opt.step(*out[:2], sync_log_std=False)
        loops[name] = (pol, opt, out, Walk(perm, mb))

    def gather_loop():
        pol, opt, out, walk = loops["gather"]
        call(pol, select(srcs, walk.next()), out)
        opt.step(*out[:2], sync_log_std=False)

    def idx_loop():
        pol, opt, out, walk = loops["idx"]
        call_idx(pol, walk.next(), srcs, out)
        opt.step(*out[:2], sync_log_std=False)

    word = torch.zeros((1,), dtype=torch.int64, device=dev)
    gperm = torch.empty((src,), dtype=torch.int32, device=dev)

    def epoch():
        pol, opt, out, _ = loops["graph"]
        perm_dev(src, 7, epoch_dev=word, out=gperm)
        for k in range(EPOCH_MB):
            call_idx(pol, gperm[k * mb:(k + 1) * mb], srcs, out)
            opt.step(*out[:2], sync_log_std=False)
        word.add_(1)
    epoch()                                                        # (every kernel has run once before the capture)
    graph = captured(epoch, dev)
    fixed = select(srcs, perm[:mb])

    paths = {"gather": (gather_loop, 1), "idx": (idx_loop, 1), "graph": (graph.replay, EPOCH_MB),
             "alone_idx": (lambda: call_idx(loops["alone_idx"][0], perm[:mb], srcs, loops["alone_idx"][2]), 1),
             "alone_contiguous": (lambda: call(loops["alone_contiguous"][0], fixed, loops["alone_contiguous"][2]), 1)}
    times = measure(paths)
    for pol, opt, _, _ in loops.values():
        opt.close()
        pol.close()
    return times


def child_mlp(net, mb, src):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPPolicy
    dev = torch.device("cuda", 0)
    widths = NETS[net]
    rng = np.random.RandomState(0)
    dims = [18] + widths + [4]
    layers = [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
              for k in range(len(dims) - 1)]
    W = widths[-1]
    head = np.concatenate([rng.randn(W) / np.sqrt(W), [0.1]]).astype(np.float32)
    log_std = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
    env = QuadrotorEnv(num_envs=64, seed=0)

    def make():
        return MLPPolicy.from_arrays(env, layers, "tanh", True, log_std=log_std, engine="mfma", value=(head[:W], head[W]))
    torch.manual_seed(0)
    obs = torch.randn((src, 18), device=dev)
    mean_t = torch.empty((src, 4), device=dev)
    probe = make()
    _, v0 = probe.evaluate_dev(obs, torch.zeros((src, 4), device=dev), mean=mean_t)
    probe.close()
    std = torch.as_tensor(np.exp(log_std), device=dev)
    z = torch.randn((src, 4), device=dev)
    actions = (mean_t + 0.15 * std * torch.randn((src, 4), device=dev) + std * z).contiguous()
    logp_old = ((-0.5 * z * z).sum(dim=1) - float(log_std.sum()) - 2.0 * float(np.log(2.0 * np.pi))).contiguous()
    adv = torch.randn(src, device=dev)
    ret = (v0 + 0.5 * torch.randn(src, device=dev)).contiguous()
    v_old = (v0 + 0.25 * torch.randn(src, device=dev)).contiguous()
    del mean_t, z, v0
    srcs = (obs, actions, logp_old, adv, ret, v_old)

    def outs(out):
        return {} if out is None else dict(grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])

    def select(s, idx):
        return tuple(torch.index_select(x, 0, idx) for x in s)

    def call(pol, t, out):                                         # (the contiguous call's statistics are 6 doubles of out's 7)
        return pol.ppo_ac_grad_dev(*t, **KW, **outs(None if out is None else (out[0], out[1], out[2], out[3][:6])))

    def call_idx(pol, idx, s, out):
        return pol.ppo_ac_grad_idx_dev(idx, *s, **KW, **outs(out))
    times = run_paths(dev, src, mb, make, srcs, select, call, call_idx)
    print(json.dumps({"net": net, "minibatch": mb, "source": src, "times": times}), flush=True)
    env.close()


def child_gru(S, S_src, T=16):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import GRUPolicy
    dev = torch.device("cuda", 0)
    H, D = 64, 18
    rng = np.random.RandomState(0)
    gru = ((rng.randn(3 * H, D) / np.sqrt(D)).astype(np.float32), (rng.randn(3 * H, H) / np.sqrt(H)).astype(np.float32),
           (0.1 * rng.randn(3 * H)).astype(np.float32), (0.1 * rng.randn(3 * H)).astype(np.float32))
    head_layers = [((rng.randn(64, H) / np.sqrt(H)).astype(np.float32), (0.1 * rng.randn(64)).astype(np.float32)),
                   ((rng.randn(4, 64) / 8.0).astype(np.float32), (0.1 * rng.randn(4)).astype(np.float32))]
    wv = (rng.randn(64) / 8.0).astype(np.float32)
    log_std = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
    env = QuadrotorEnv(num_envs=64, seed=0)

    def make():
        return GRUPolicy(env, gru, head_layers, "tanh", True, log_std=log_std, value=(wv, np.float32(0.1)))
    torch.manual_seed(0)
    obs = torch.randn((T, S_src, D), device=dev)
    done = (torch.rand((T, S_src), device=dev) < 0.05).to(torch.uint8)
    h0 = 0.5 * torch.randn((S_src, H), device=dev)
    mean_t = torch.empty((T, S_src, 4), device=dev)
    probe = make()
    probe.set_log_std(None)
    _, v0 = probe.evaluate_seq_dev(obs, None, done, h0, mean=mean_t)
    probe.close()
    std = torch.as_tensor(np.exp(log_std), device=dev)
    z = torch.randn((T, S_src, 4), device=dev)
    actions = (mean_t + 0.15 * std * torch.randn((T, S_src, 4), device=dev) + std * z).contiguous()
    logp_old = ((-0.5 * z * z).sum(dim=2) - float(log_std.sum()) - 2.0 * float(np.log(2.0 * np.pi))).contiguous()
    adv = torch.randn((T, S_src), device=dev)
    ret = (v0 + 0.5 * torch.randn((T, S_src), device=dev)).contiguous()
    v_old = (v0 + 0.25 * torch.randn((T, S_src), device=dev)).contiguous()
    del mean_t, z, v0
    srcs = (obs, actions, done, h0, logp_old, adv, ret, v_old)

    def outs(out):
        return {} if out is None else dict(grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])

    def select(s, idx):
        return tuple(torch.index_select(x, 0 if k == 3 else 1, idx) for k, x in enumerate(s))

    def call(pol, t, out):
        return pol.ppo_seq_grad_dev(*t, **KW, **outs(None if out is None else (out[0], out[1], out[2], out[3][:6])))

    def call_idx(pol, idx, s, out):
        return pol.ppo_seq_grad_idx_dev(idx, *s, **KW, **outs(out))
    times = run_paths(dev, S_src, S, make, srcs, select, call, call_idx)
    print(json.dumps({"net": GRU, "T": T, "minibatch": S, "source": S_src, "times": times}), flush=True)
    env.close()


def step(args):
    """one point: a fresh child process under its own time limit.  A failure or a time-out ends the whole run."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit("minibatch_rate: %s ran past %d s; nothing more is started on the device" % (args, STEP_LIMIT))
    if out.returncode:
        sys.exit("minibatch_rate: %s ended with status %d; nothing more is started on the device" % (args, out.returncode))
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r34_minibatch.json"))
    ap.add_argument("--quick", action="store_true", help="one small point of each kind (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == GRU:
            return child_gru(int(args.child[1]), int(args.child[2]))
        return child_mlp(args.child[0], int(args.child[1]), int(args.child[2]))
    if args.quick:
        points = [("18-64-64-4", 1 << 10, 1 << 13), (GRU, 1 << 8, 1 << 10)]
    else:
        points = [(net, mb, src) for net in NETS for mb in (1 << 14, 1 << 17) for src in (1 << 20, 1 << 22)] + \
                 [(GRU, 1 << 12, 1 << 16), (GRU, 1 << 14, 1 << 16)]
    res = {"warmup_rounds": WARMUP, "rounds": ROUNDS, "iterations_per_sample": CALLS, "minibatches_per_captured_epoch": EPOCH_MB,
           "unit": "microseconds per minibatch", "kernel_only_trace": "none taken: host clocks around whole iterations",
           "config": "tanh nets with output tanh, a value head and log_std; AdamDev lr %g, max_grad_norm %g, learn_log_std=False, "
                     "sync_log_std=False; clip %g, vclip %g, vf_coef %g, ent_coef %g; the GRU at T = 16" % (LR, MAX_NORM, CLIP, VCLIP, VF_COEF,
                                                                                                          ENT_COEF), "cases": []}
    for point in points:
        row = step(point)
        case = {k: v for k, v in row.items() if k != "times"}
        case.update({k: stats(v) for k, v in row["times"].items()})
        med = lambda k: case[k]["us_median"]
        case["gather_over_idx"] = round(med("gather") / med("idx"), 2)
        case["gather_over_graph"] = round(med("gather") / med("graph"), 2)
        case["alone_idx_over_contiguous"] = round(med("alone_idx") / med("alone_contiguous"), 3)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
