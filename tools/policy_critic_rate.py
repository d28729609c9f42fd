#!/usr/bin/env python3
"""A separate critic on one device: what rollout_policy_dev(critic=) costs against the shared-trunk actor-critic rollout, fused against
two launches, and against what a user does without it.  Per actor / critic pair and batch, interleaved in one run (own env per path):
  ac               rollout_policy_dev(values=, logp=) with a value head on the actor's trunk (no critic): the existing path.  With
                   --parent-tree (a checkout of the parent commit with its library built) the same call is also timed in child processes
                   that import that tree (`ac_parent`, the yardstick; `ac_parent2`, the same again: the null run that gives the margin)
                   and this one (`ac_child`), in turn per batch size
  ac_term          the same + term_values=
  critic_fused     rollout_policy_dev(values=, logp=, critic=), an MLP actor's fused launch (policy_mfma_critic_kernel)
  critic_2launch   the same with the critic built under GAQ_NO_FUSED_CRITIC=1: the actor's launch, then critic_mfma_kernel (a GRU actor has
                   this form only: `critic`)
  *_term           each + term_values=
  torch_critic     what a user does today: the actor-only rollout (logp=), then a torch pass of the critic over the [T + 1, N, D]
                   observations, row by row
T = 64 steps, default configuration (alias layout, default episode length, so hardly any env finishes: the _term paths pay their two
small launches per step and gather next to nothing).  3 warm-ups, then the paths interleaved, REPS timed rounds each; median and spread
(min..max) in microseconds per step.
python3 tools/policy_critic_rate.py [out.json] [--pairs 128-128+128-128,256-256+256-256,gru128+128-128] [--sizes 65536,1048576]
                                    [--parent-tree DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("GAQ_CRITIC_RATE_TREE") or ROOT)     # (the --child processes: the tree whose package they time)
import torch  # noqa: E402
from gym_art_amd import QuadrotorEnv  # noqa: E402
from gym_art_amd.policy import GRUPolicy, MLPPolicy  # noqa: E402

dev = torch.device("cuda", 0)
T, REPS, D = 64, 7, 18
LOG_STD = [-1.0, -1.0, -1.0, -1.0]


def mlp(widths, out):
    nn = torch.nn
    mods, prev = [], D
    for w in widths:
        mods += [nn.Linear(prev, w), nn.Tanh()]
        prev = w
    return mods, nn.Linear(prev, out)


def build_actor(net, env, value):
    """the actor of `net` ("128-128" / "gru128"), with a value head on its trunk or without"""
    torch.manual_seed(0)
    nn = torch.nn
    if net.startswith("gru"):
        H = int(net[3:])
        cell, actor, head = nn.GRUCell(D, H), nn.Linear(H, 4), nn.Linear(H, 1)
        return GRUPolicy.from_torch(cell, nn.Sequential(actor, nn.Tanh()), env, log_std=LOG_STD, value=head if value else None)
    mods, actor = mlp([int(w) for w in net.split("-")], 4)
    head = nn.Linear(actor.in_features, 1)
    return MLPPolicy.from_torch(nn.Sequential(*mods, actor, nn.Tanh()), env, log_std=LOG_STD, engine="mfma", value=head if value else None)


def build_critic(net, env, fused=True):
    """(MLPCritic, the same net as a torch module on the device)"""
    from gym_art_amd.policy import MLPCritic
    torch.manual_seed(1)
    mods, out = mlp([int(w) for w in net.split("-")], 1)
    module = torch.nn.Sequential(*mods, out)
    old = os.environ.pop("GAQ_NO_FUSED_CRITIC", None)
    if not fused:
        os.environ["GAQ_NO_FUSED_CRITIC"] = "1"
    try:
        crit = MLPCritic.from_torch(module, env)
    finally:
        os.environ.pop("GAQ_NO_FUSED_CRITIC", None)
        if old is not None:
            os.environ["GAQ_NO_FUSED_CRITIC"] = old
    return crit, module.to(dev)


def name_of(pair):
    actor, critic = pair.split("+")
    return "%s with critic 18-%s-1" % ("18-GRU%s-4" % actor[3:] if actor.startswith("gru") else "18-%s-4" % actor, critic)


def stats(v):
    v = sorted(v)
    return {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2)}


class Bufs:
    def __init__(self, n):
        self.o = torch.empty((T, n, D), device=dev)
        self.r = torch.empty((T, n), device=dev)
        self.d = torch.empty((T, n), dtype=torch.uint8, device=dev)
        self.a = torch.empty((T, n, 4), device=dev)
        self.v = torch.empty((T + 1, n), device=dev)
        self.lp = torch.empty((T, n), device=dev)
        self.tv = torch.empty((T, n), device=dev)
        self.o0 = torch.empty((n, D), device=dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / T


def ac_only(args):
    """--child: the shared-trunk actor-critic rollout of the tree this process imported, one line of JSON per case"""
    for n in (int(x) for x in args.sizes.split(",")):
        for pair in args.pairs.split(","):
            env = QuadrotorEnv(num_envs=n, seed=0, alias_obs=True)
            pol = build_actor(pair.split("+")[0], env, True)
            b = Bufs(n)
            env.reset_dev(b.o[T - 1])

            def run():
                env.rollout_policy_dev(pol, b.o, b.r, b.d, b.a, values=b.v, logp=b.lp)
            for _ in range(3):
                run()
            print(json.dumps({"N": n, "pair": name_of(pair), "ac": stats([timed(run) for _ in range(REPS)])}), flush=True)
            pol.close(); env.close()
            del b
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--pairs", default="128-128+128-128,256-256+256-256,gru128+128-128")
    ap.add_argument("--sizes", default="65536,%d" % (1 << 20))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with libgaq.so built: its actor-critic rollout is timed too")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return ac_only(args)
    res = {"T": T, "reps": REPS, "unit": "us per step",
           "config": "DefaultQuad, alias layout (fp64 split state), thrust noise on, auto-reset, default episode length", "cases": []}
    for n in (int(x) for x in args.sizes.split(",")):
        for pair in args.pairs.split(","):
            actor, critic = pair.split("+")
            gru = actor.startswith("gru")
            forms = [("critic", False)] if gru else [("critic_fused", True), ("critic_2launch", False)]
            keys = ["ac", "ac_term"] + [k + s for k, _ in forms for s in ("", "_term")] + ["torch_critic"]
            envs = {k: QuadrotorEnv(num_envs=n, seed=0, alias_obs=True) for k in keys}
            bufs = {k: Bufs(n) for k in keys}
            pols = {k: build_actor(actor, envs[k], k.startswith("ac")) for k in keys}
            crits = {k + s: build_critic(critic, envs[k + s], fused) for k, fused in forms for s in ("", "_term")}
            crits["torch_critic"] = build_critic(critic, envs["torch_critic"])
            for k, e in envs.items():
                e.reset_dev(bufs[k].o[T - 1])

            def run(k):
                b = bufs[k]
                kw = {"term_values": b.tv} if k.endswith("_term") else {}
                if k in crits:
                    kw["critic"] = crits[k][0]
                envs[k].rollout_policy_dev(pols[k], b.o, b.r, b.d, b.a, values=b.v, logp=b.lp, **kw)

            def run_torch():
                b = bufs["torch_critic"]
                net = crits["torch_critic"][1]
                b.o0.copy_(b.o[T - 1])                              # the observation the call starts from
                envs["torch_critic"].rollout_policy_dev(pols["torch_critic"], b.o, b.r, b.d, b.a, logp=b.lp)
                with torch.no_grad():
                    b.v[0] = net(b.o0)[:, 0]
                    for t in range(T):
                        b.v[t + 1] = net(b.o[t])[:, 0]

            paths = {k: (lambda k=k: run(k)) for k in keys if k != "torch_critic"}
            paths["torch_critic"] = run_torch
            for fn in paths.values():       # warm-up
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in paths}
            for _ in range(REPS):
                for k, fn in paths.items():
                    times[k].append(timed(fn))
            case = {"N": n, "pair": name_of(pair)}
            case.update({k: stats(ts) for k, ts in times.items()})
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            for p in pols.values():
                p.close()
            for c in crits.values():
                c[0].close()
            for e in envs.values():
                e.close()
            del bufs
            torch.cuda.empty_cache()
    if args.parent_tree:
        # fresh child processes: the parent's tree, this one, and the parent's again (the null run), in turn per batch size
        parent = os.path.abspath(args.parent_tree)
        for size in args.sizes.split(","):
            for key, tree in (("ac_parent", parent), ("ac_child", ROOT), ("ac_parent2", parent)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--pairs", args.pairs, "--sizes", size],
                                     env=dict(os.environ, GAQ_CRITIC_RATE_TREE=tree), stdout=subprocess.PIPE, text=True, check=True,
                                     timeout=600).stdout
                for line in out.splitlines():
                    row = json.loads(line)
                    for case in res["cases"]:
                        if case["N"] == row["N"] and case["pair"] == row["pair"]:
                            case[key] = row["ac"]
                            print(json.dumps({"N": row["N"], "pair": row["pair"], key: row["ac"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
