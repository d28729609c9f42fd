#!/usr/bin/env python3
"""Actor-critic rollouts on one device: what values, log-probabilities and advantages cost on top of a closed-loop rollout, against what
a user computes them with otherwise.  Per net and batch, interleaved in one run:
  plain      rollout_policy_dev as it was.  With --parent-tree (a checkout of the parent commit with its library built) the same call is
             also timed in child processes that import that tree (`plain_parent`) and this one (`plain_child`), in turn per batch size:
             the yardstick for "existing rollouts did not slow down"
  ac         rollout_policy_dev(values=, logp=);  ac_gae  the same + gae_dev: everything `today` computes
  today      plain + a torch fp32 pass over the [T N, D] trajectory for means, log-probs and values (MLP), or the torch GRUCell host
             recurrence over the recorded observations and dones (GRU), + a torch GAE loop
  gae_dev    gae_dev alone;  gae_torch  the T-iteration torch loop alone
T = 64 steps, default configuration (alias layout).  Warm-up, then the paths interleaved, REPS timed rounds each; median and spread
(min..max) reported in microseconds per step (gae: per call).
python3 tools/policy_ac_rate.py [out.json] [--nets 128-128,256-256,gru128] [--sizes 1048576,65536] [--parent-tree DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("GAQ_AC_RATE_TREE") or ROOT)       # (the --child processes: the tree whose package they time)
import torch  # noqa: E402
from gym_art_amd import QuadrotorEnv  # noqa: E402
from gym_art_amd.policy import GRUPolicy, MLPPolicy  # noqa: E402

dev = torch.device("cuda", 0)
T, REPS, D = 64, 7, 18
GAMMA, LAM = 0.99, 0.95
LOG_STD = [-1.0, -1.0, -1.0, -1.0]


def build(net, env, value):
    """(policy, torch modules on the device: trunk (obs -> last hidden) or GRUCell, actor Linear, critic Linear)"""
    torch.manual_seed(0)
    nn = torch.nn
    if net.startswith("gru"):
        H = int(net[3:])
        cell, actor, critic = nn.GRUCell(D, H), nn.Linear(H, 4), nn.Linear(H, 1)
        kw = {"value": critic} if value else {}                  # (no keyword at all in --child: the parent's classes have none)
        pol = GRUPolicy.from_torch(cell, nn.Sequential(actor, nn.Tanh()), env, log_std=LOG_STD, **kw)
        return pol, cell.to(dev), actor.to(dev), critic.to(dev)
    widths = [int(w) for w in net.split("-")]
    mods, prev = [], D
    for w in widths:
        mods += [nn.Linear(prev, w), nn.Tanh()]
        prev = w
    trunk, actor, critic = nn.Sequential(*mods), nn.Linear(prev, 4), nn.Linear(prev, 1)
    kw = {"value": critic} if value else {}
    pol = MLPPolicy.from_torch(nn.Sequential(*mods, actor, nn.Tanh()), env, log_std=LOG_STD, engine="mfma", **kw)
    return pol, trunk.to(dev), actor.to(dev), critic.to(dev)


def name_of(net):
    return "18-GRU%s-4" % net[3:] if net.startswith("gru") else "18-%s-4" % net


def torch_gae(r, d, v, adv):
    nd = 1.0 - d.float()
    a = torch.zeros_like(r[0])
    for t in range(T - 1, -1, -1):
        delta = r[t] + GAMMA * nd[t] * v[t + 1] - v[t]
        a = delta + GAMMA * LAM * nd[t] * a
        adv[t] = a
    return adv


def stats(v):
    v = sorted(v)
    return {"us_median": round(v[len(v) // 2], 2), "us_min": round(v[0], 2), "us_max": round(v[-1], 2)}


def plain_only(args):
    """--child: the plain rollout of the tree this process imported, one line of JSON per case"""
    for n in (int(x) for x in args.sizes.split(",")):
        for net in args.nets.split(","):
            env = QuadrotorEnv(num_envs=n, ep_time=5, seed=0, alias_obs=True)
            pol = build(net, env, False)[0]
            o = torch.empty((T, n, D), device=dev); r = torch.empty((T, n), device=dev); d = torch.empty((T, n), dtype=torch.uint8, device=dev)
            env.reset_dev(o[T - 1])
            for _ in range(3):
                env.rollout_policy_dev(pol, o, r, d)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                env.rollout_policy_dev(pol, o, r, d)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6 / T)
            print(json.dumps({"N": n, "net": name_of(net), "plain": stats(ts)}), flush=True)
            pol.close(); env.close()
            del o, r, d
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--nets", default="128-128,256-256,gru128")
    ap.add_argument("--sizes", default="%d,%d" % (1 << 20, 65536))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with libgaq.so built: its plain rollout is timed too")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return plain_only(args)
    res = {"T": T, "reps": REPS, "gamma": GAMMA, "lambda": LAM, "unit": "us per step (gae_dev, gae_torch: us per call)",
           "config": "DefaultQuad, alias layout (fp64 split state), thrust noise on, auto-reset (ep_time 5 s)", "cases": []}
    for n in (int(x) for x in args.sizes.split(",")):
        for net in args.nets.split(","):
            gru = net.startswith("gru")
            envs = {k: QuadrotorEnv(num_envs=n, ep_time=5, seed=0, alias_obs=True) for k in ("plain", "ac", "today")}
            pols = {k: build(net, e, k == "ac") for k, e in envs.items()}
            _, body, actor, critic = pols["today"]
            # (an observation tensor per env: in the alias layout it is that env's state head)
            obs = {k: torch.empty((T, n, D), device=dev) for k in envs}
            r = torch.empty((T, n), device=dev); d = torch.empty((T, n), dtype=torch.uint8, device=dev)
            a = torch.empty((T, n, 4), device=dev)
            v = torch.empty((T + 1, n), device=dev); lp = torch.empty((T, n), device=dev)
            adv = torch.empty((T, n), device=dev); ret = torch.empty((T, n), device=dev)
            for k, e in envs.items():
                e.reset_dev(obs[k][T - 1])
            ls = torch.tensor(LOG_STD, device=dev)

            def logp_of(mean, act):
                z = (act - mean) * torch.exp(-ls)
                return (-0.5 * z * z - ls).sum(-1) - 3.6757541

            def run_plain():
                envs["plain"].rollout_policy_dev(pols["plain"][0], obs["plain"], r, d, a)

            def run_ac():
                envs["ac"].rollout_policy_dev(pols["ac"][0], obs["ac"], r, d, a, values=v, logp=lp)

            def run_ac_gae():
                run_ac()
                envs["ac"].gae_dev(r, d, v, GAMMA, LAM, adv, ret)

            def run_today():
                o = obs["today"]
                first = o[T - 1].clone()                        # what action 0 will see
                envs["today"].rollout_policy_dev(pols["today"][0], o, r, d, a)
                with torch.no_grad():
                    if gru:                                     # the recurrence again, step by step (h from 0 here: the cost is the same)
                        h = torch.zeros((n, body.hidden_size), device=dev)
                        for t in range(T + 1):
                            h = body(first if t == 0 else o[t - 1], h)
                            v[t] = critic(h)[:, 0]
                            if t < T:
                                lp[t] = logp_of(torch.tanh(actor(h)), a[t])
                                h = torch.where(d[t].bool()[:, None], torch.zeros((), device=dev), h)
                    else:                                       # one pass over the trajectory, a step's rows at a time to bound memory
                        for t in range(T + 1):
                            y = body(first if t == 0 else o[t - 1])
                            v[t] = critic(y)[:, 0]
                            if t < T:
                                lp[t] = logp_of(torch.tanh(actor(y)), a[t])
                    torch_gae(r, d, v, adv)

            paths = {"plain": run_plain, "ac": run_ac, "ac_gae": run_ac_gae, "today": run_today,
                     "gae_dev": lambda: envs["ac"].gae_dev(r, d, v, GAMMA, LAM, adv, ret),
                     "gae_torch": lambda: torch_gae(r, d, v, adv)}
            per_call = ("gae_dev", "gae_torch")
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
                    times[k].append((time.perf_counter() - t0) * 1e6 / (1 if k in per_call else T))
            case = {"N": n, "net": name_of(net)}
            case.update({k: stats(ts) for k, ts in times.items()})
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            for p in pols.values():
                p[0].close()
            for e in envs.values():
                e.close()
            del obs, r, d, a, v, lp, adv, ret
            torch.cuda.empty_cache()
    if args.parent_tree:
        # fresh child processes, the parent's tree and this one in turn per batch size
        for size in args.sizes.split(","):
            for key, tree in (("plain_parent", os.path.abspath(args.parent_tree)), ("plain_child", ROOT)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--nets", args.nets, "--sizes", size],
                                     env=dict(os.environ, GAQ_AC_RATE_TREE=tree), stdout=subprocess.PIPE, text=True, check=True,
                                     timeout=600).stdout
                for line in out.splitlines():
                    row = json.loads(line)
                    for case in res["cases"]:
                        if case["N"] == row["N"] and case["net"] == row["net"]:
                            case[key] = row["plain"]
                            print(json.dumps({"N": row["N"], "net": row["net"], key: row["plain"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
