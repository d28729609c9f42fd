#!/usr/bin/env python3
"""Time-limit bootstrapping on one device: what rollout_policy_dev(term_values=) costs on top of the actor-critic rollout, against what a
user does for it otherwise.  Per net and batch, interleaved in one run (own env per path):
  ac              rollout_policy_dev(values=, logp=) of this build.  With --parent-tree (a checkout of the parent commit with its library
                  built) the same call is also timed in child processes that import that tree (`ac_parent`, the yardstick) and this one
                  (`ac_child`), in turn per batch size: this build's must sit within the parent's min..max (the same instructions)
  term_aligned    the same + term_values=, every env on the same tick (episodes end together: most steps gather nothing)
  term_staggered  the same with the envs' ticks spread over the episode length L (about N / L envs finish in every step)
  host_loop       what a user does today (MLP): T single steps rollout_policy_dev(T = 1, values=, logp=), after each a torch pass of the
                  critic over the registered terminal tensor, selected by done.  (A GRU user cannot: the hidden rows the episodes ended
                  on are zeroed inside the call.)
T = 64 steps, default configuration (alias layout, default episode length).  3 warm-ups, then the paths interleaved, REPS timed rounds
each; median and spread (min..max) in microseconds per step; `finished_per_step` is the mean number of dones per step in the timed rounds.
python3 tools/policy_term_rate.py [out.json] [--nets 128-128,256-256,gru128] [--sizes 1048576,65536] [--parent-tree DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("GAQ_TERM_RATE_TREE") or ROOT)     # (the --child processes: the tree whose package they time)
import torch  # noqa: E402
from gym_art_amd import QuadrotorEnv  # noqa: E402
from gym_art_amd.policy import GRUPolicy, MLPPolicy  # noqa: E402

dev = torch.device("cuda", 0)
T, REPS, D = 64, 7, 18
STAGGER = 16                     # the staggered envs start in this many groups, L / STAGGER steps apart
LOG_STD = [-1.0, -1.0, -1.0, -1.0]


def build(net, env):
    """(policy with a value head, torch modules on the device: trunk (obs -> last hidden) or GRUCell, critic Linear)"""
    torch.manual_seed(0)
    nn = torch.nn
    if net.startswith("gru"):
        H = int(net[3:])
        cell, actor, critic = nn.GRUCell(D, H), nn.Linear(H, 4), nn.Linear(H, 1)
        pol = GRUPolicy.from_torch(cell, nn.Sequential(actor, nn.Tanh()), env, log_std=LOG_STD, value=critic)
        return pol, cell.to(dev), critic.to(dev)
    mods, prev = [], D
    for w in (int(w) for w in net.split("-")):
        mods += [nn.Linear(prev, w), nn.Tanh()]
        prev = w
    trunk, actor, critic = nn.Sequential(*mods), nn.Linear(prev, 4), nn.Linear(prev, 1)
    pol = MLPPolicy.from_torch(nn.Sequential(*mods, actor, nn.Tanh()), env, log_std=LOG_STD, engine="mfma", value=critic)
    return pol, trunk.to(dev), critic.to(dev)


def name_of(net):
    return "18-GRU%s-4" % net[3:] if net.startswith("gru") else "18-%s-4" % net


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


def ac_only(args):
    """--child: the actor-critic rollout of the tree this process imported, one line of JSON per case"""
    for n in (int(x) for x in args.sizes.split(",")):
        for net in args.nets.split(","):
            env = QuadrotorEnv(num_envs=n, seed=0, alias_obs=True)
            pol = build(net, env)[0]
            b = Bufs(n)
            env.reset_dev(b.o[T - 1])
            for _ in range(3):
                env.rollout_policy_dev(pol, b.o, b.r, b.d, b.a, values=b.v, logp=b.lp)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                env.rollout_policy_dev(pol, b.o, b.r, b.d, b.a, values=b.v, logp=b.lp)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6 / T)
            print(json.dumps({"N": n, "net": name_of(net), "ac": stats(ts)}), flush=True)
            pol.close(); env.close()
            del b
            torch.cuda.empty_cache()


def stagger(env, pol, b, ep_len):
    """spread the envs' ticks over the episode: STAGGER groups (env index mod STAGGER), started ep_len / STAGGER steps apart"""
    n = env.num_envs
    idx = torch.arange(n, device=dev)
    steps = max(1, ep_len // STAGGER)
    for g in range(STAGGER):
        left = steps
        while left > 0:
            k = min(left, T)
            env.rollout_policy_dev(pol, b.o[T - k:], b.r[:k], b.d[:k], b.a[:k])
            left -= k
        mask = (idx % STAGGER == g).to(torch.uint8)
        env.reset_dev(b.o[T - 1], mask)
        if hasattr(pol, "reset_hidden"):
            pol.reset_hidden(mask)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--nets", default="128-128,256-256,gru128")
    ap.add_argument("--sizes", default="%d,%d" % (1 << 20, 65536))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with libgaq.so built: its actor-critic rollout is timed too")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return ac_only(args)
    res = {"T": T, "reps": REPS, "stagger_groups": STAGGER, "unit": "us per step",
           "config": "DefaultQuad, alias layout (fp64 split state), thrust noise on, auto-reset, default episode length", "cases": []}
    for n in (int(x) for x in args.sizes.split(",")):
        for net in args.nets.split(","):
            gru = net.startswith("gru")
            keys = ["ac", "term_aligned", "term_staggered"] + ([] if gru else ["host_loop"])
            envs = {k: QuadrotorEnv(num_envs=n, seed=0, alias_obs=True) for k in keys}
            pols = {k: build(net, e) for k, e in envs.items()}
            bufs = {k: Bufs(n) for k in keys}
            ep_len = int(envs["ac"].ep_len)
            for k, e in envs.items():
                e.reset_dev(bufs[k].o[T - 1])
            stagger(envs["term_staggered"], pols["term_staggered"][0], bufs["term_staggered"], ep_len)
            dones = {k: 0 for k in keys}

            def run_ac(k="ac", term=False):
                b = bufs[k]
                envs[k].rollout_policy_dev(pols[k][0], b.o, b.r, b.d, b.a, values=b.v, logp=b.lp, **({"term_values": b.tv} if term else {}))

            def run_host_loop():
                b, e = bufs["host_loop"], envs["host_loop"]
                pol, trunk, critic = pols["host_loop"]
                v2 = torch.empty((2, n), device=dev)
                for t in range(T):
                    e.rollout_policy_dev(pol, b.o[t:t + 1], b.r[t:t + 1], b.d[t:t + 1], b.a[t:t + 1], values=v2, logp=b.lp[t:t + 1])
                    b.v[t] = v2[0]
                    with torch.no_grad():
                        b.tv[t] = torch.where(b.d[t].bool(), critic(trunk(term_rows))[:, 0], torch.zeros((), device=dev))
                b.v[T] = v2[1]

            paths = {"ac": run_ac, "term_aligned": lambda: run_ac("term_aligned", True), "term_staggered": lambda: run_ac("term_staggered", True)}
            if not gru:
                term_rows = torch.zeros((n, D), device=dev)
                envs["host_loop"].set_terminal_obs(term_rows)
                paths["host_loop"] = run_host_loop
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
                    dones[k] += int(bufs[k].d.sum())
            case = {"N": n, "net": name_of(net), "episode_steps": ep_len + 1}
            case.update({k: stats(ts) for k, ts in times.items()})
            case["finished_per_step"] = {k: round(dones[k] / (REPS * T), 1) for k in paths}
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            for p in pols.values():
                p[0].close()
            for e in envs.values():
                e.close()
            del bufs
            torch.cuda.empty_cache()
    if args.parent_tree:
        # fresh child processes, the parent's tree and this one in turn per batch size
        for size in args.sizes.split(","):
            for key, tree in (("ac_parent", os.path.abspath(args.parent_tree)), ("ac_child", ROOT)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--nets", args.nets, "--sizes", size],
                                     env=dict(os.environ, GAQ_TERM_RATE_TREE=tree), stdout=subprocess.PIPE, text=True, check=True,
                                     timeout=600).stdout
                for line in out.splitlines():
                    row = json.loads(line)
                    for case in res["cases"]:
                        if case["N"] == row["N"] and case["net"] == row["net"]:
                            case[key] = row["ac"]
                            print(json.dumps({"N": row["N"], "net": row["net"], key: row["ac"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
