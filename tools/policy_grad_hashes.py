#!/usr/bin/env python3
"""md5 of every output of a fixed set of calls of the five gradient entry points that predate the shared-trunk actor-critic form
(logp_dev, backward_dev and ppo_grad_dev of MLPPolicy, backward_dev and mse_grad_dev of MLPCritic): three nets x tanh / relu, with and
without a value head set on the policy (it takes no part), at 1, 65, 453 and 4096 rows and 453 rows under GAQ_GRAD_GROUPS=3.  One
line per output.  Run it under two builds of the library (GAQ_LIB selects the file) and compare the listings: equal listings mean
the kernels' bits did not move.  python3 tools/policy_grad_hashes.py > profiles/rNN_policy_grad_hashes_<build>.txt"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NETS = [[16], [64, 64], [128, 128, 128]]
STYLES = [("tanh", True), ("relu", False)]
ROWS = [1, 65, 453, 4096]
LOG_STD = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)


def layers(rng, D, widths, n_out):
    dims = [D] + widths + [n_out]
    return [((rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])).astype(np.float32), (0.1 * rng.randn(dims[k + 1])).astype(np.float32))
            for k in range(len(dims) - 1)]


def md5(t):
    return hashlib.md5(t.detach().cpu().numpy().tobytes()).hexdigest()


def main():
    import torch
    from gym_art_amd import QuadrotorEnv
    from gym_art_amd.policy import MLPCritic, MLPPolicy
    env = QuadrotorEnv(num_envs=64, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True)
    D, dev = env.obs_dim, torch.device("cuda", env.device)
    rng = np.random.RandomState(31)
    R = max(ROWS)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
    obs, act, lpo, adv, tgt = t(rng.randn(R, D)), t(rng.randn(R, 4)), t(-4.0 + rng.randn(R)), t(rng.randn(R)), t(rng.randn(R))
    lines = []
    for widths in NETS:
        for actn, out_tanh in STYLES:
            pl, cl = layers(rng, D, widths, 4), layers(rng, D, widths, 1)
            head = ((rng.randn(widths[-1]) / np.sqrt(widths[-1])).astype(np.float32), np.float32(0.1))
            for with_head in (False, True):
                pol = MLPPolicy.from_arrays(env, pl, actn, out_tanh, log_std=LOG_STD, engine="mfma", value=head if with_head else None)
                crit = MLPCritic.from_arrays(env, cl, actn)
                for rows, groups in [(r, None) for r in ROWS] + [(453, "3")]:
                    if groups:
                        os.environ["GAQ_GRAD_GROUPS"] = groups
                    o, a = obs[:rows], act[:rows]
                    mean = torch.zeros((rows, 4), device=dev)
                    outs = [("logp", pol.logp_dev(o, a, mean=mean)), ("mean", mean), ("backward", pol.backward_dev(o, a, scale=0.5))]
                    outs += list(zip(("ppo.grad", "ppo.grad_log_std", "ppo.stats"), pol.ppo_grad_dev(o, a, lpo[:rows], adv[:rows])))
                    if not with_head:
                        outs += [("critic.backward", crit.backward_dev(o, adv[:rows], scale=0.5))]
                        outs += list(zip(("mse.grad", "mse.stats"), crit.mse_grad_dev(o, tgt[:rows])))
                    torch.cuda.synchronize()
                    os.environ.pop("GAQ_GRAD_GROUPS", None)
                    tag = "%s %s head=%d rows=%d groups=%s" % ("x".join(map(str, widths)), actn, with_head, rows, groups or "default")
                    lines += ["%-48s %-18s %s" % (tag, name, md5(x)) for name, x in outs]
                pol.close()
                crit.close()
    env.close()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
