#!/usr/bin/env python3
"""md5 of every output of a fixed set of calls of the gradient entry points.  The five that predate the shared-trunk actor-critic form
(logp_dev, backward_dev and ppo_grad_dev of MLPPolicy, backward_dev and mse_grad_dev of MLPCritic): three nets x tanh / relu, with and
without a value head set on the policy (it takes no part), at 1, 65, 453 and 4096 rows and 453 rows under GAQ_GRAD_GROUPS=3; with the
head, evaluate_dev and ppo_ac_grad_dev on the same rows.  The three index-gathered forms (tanh nets) at 65 and 453 rows drawn from the
4096 (one index of the 453 out of range).  GRUPolicy's evaluate_seq_dev, ppo_seq_grad_dev and ppo_seq_grad_idx_dev for two nets, T in {1, 3},
S in {1, 65, 130} (of 130 source columns), with and without a value head, `done` set in the middle step, once under
GAQ_GRAD_GROUPS=2 (the larger net with its head, T = 3, S = 130); then LSTMPolicy's evaluate_seq_dev (with c_out), ppo_bptt_grad_dev and
ppo_bptt_grad_idx_dev over the same cases (after the GRU's, which keep their draws); last, one policy with an encoder per cell and size
(32-GRU16 without a value head, 64x64-GRU64-64 with one; the LSTM's the same): evaluate_enc_seq_dev, ppo_enc_seq_grad_dev and
ppo_enc_seq_grad_idx_dev at the same T and S.  One line per output.  Run it under two builds of the library (GAQ_LIB
selects the file) and compare the listings: equal listings mean the kernels' bits did not move.  python3 tools/policy_grad_hashes.py > profiles/rNN_policy_grad_hashes_<build>.txt"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NETS = [[16], [64, 64], [128, 128, 128]]
STYLES = [("tanh", True), ("relu", False)]
ROWS = [1, 65, 453, 4096]
LOG_STD = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)
IDX_ROWS = [65, 453]                                              # drawn from max(ROWS) source rows
AC = dict(clip=0.2, vclip=0.2, vf_coef=0.5, ent_coef=0.01)
SEQ_NETS = [(16, []), (64, [64])]                                 # the cell's H, the head's widths
SEQ_T, SEQ_S, SEQ_SRC = [1, 3], [1, 65, 130], 130
ENC_SEQ_NETS = [((32,), 16, []), ((64, 64), 64, [64])]           # the encoder's widths, the cell's H, the head's widths


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
    rng2 = np.random.RandomState(35)                             # (a stream of its own: the older cases keep their draws)
    vold = t(rng2.randn(R))
    ti = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)
    idxs = {n: rng2.permutation(R)[:n] for n in IDX_ROWS}
    idxs[IDX_ROWS[-1]][7] = R                                     # one index out of range
    idxs = {n: ti(v) for n, v in idxs.items()}
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
                    else:
                        outs += list(zip(("eval.logp", "eval.value"), pol.evaluate_dev(o, a)))
                        outs += list(zip(("ppo_ac.grad", "ppo_ac.grad_value", "ppo_ac.grad_log_std", "ppo_ac.stats"),
                                         pol.ppo_ac_grad_dev(o, a, lpo[:rows], adv[:rows], tgt[:rows], vold[:rows], **AC)))
                    torch.cuda.synchronize()
                    os.environ.pop("GAQ_GRAD_GROUPS", None)
                    tag = "%s %s head=%d rows=%d groups=%s" % ("x".join(map(str, widths)), actn, with_head, rows, groups or "default")
                    lines += ["%-48s %-18s %s" % (tag, name, md5(x)) for name, x in outs]
                for rows, idx in idxs.items() if actn == "tanh" else ():   # (an idx form differs from its parent in load addresses only)
                    if not with_head:
                        outs = list(zip(("ppo_idx.grad", "ppo_idx.grad_log_std", "ppo_idx.stats"), pol.ppo_grad_idx_dev(idx, obs, act, lpo, adv)))
                        outs += list(zip(("mse_idx.grad", "mse_idx.stats"), crit.mse_grad_idx_dev(idx, obs, tgt)))
                    else:
                        outs = list(zip(("ppo_ac_idx.grad", "ppo_ac_idx.grad_value", "ppo_ac_idx.grad_log_std", "ppo_ac_idx.stats"),
                                        pol.ppo_ac_grad_idx_dev(idx, obs, act, lpo, adv, tgt, vold, **AC)))
                    torch.cuda.synchronize()
                    tag = "%s %s head=%d rows=%d of %d" % ("x".join(map(str, widths)), actn, with_head, rows, R)
                    lines += ["%-48s %-22s %s" % (tag, name, md5(x)) for name, x in outs]
                pol.close()
                crit.close()
    lines += seq_lines(env, dev, rng2, t, ti, "gru") + seq_lines(env, dev, rng2, t, ti, "lstm")
    rng3 = np.random.RandomState(42)                             # (again a stream of its own)
    lines += enc_seq_lines(env, dev, rng3, t, ti, "gru") + enc_seq_lines(env, dev, rng3, t, ti, "lstm")
    env.close()
    print("\n".join(lines))


def seq_lines(env, dev, rng, t, ti, cell):
    """the sequence forms of one cell ("gru" / "lstm"): every source tensor has SEQ_SRC columns; the contiguous calls take the first S,
    the idx calls S drawn ones.  An LSTM has a second state: c0 beside h0, c_out beside h_out."""
    import torch
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy
    lstm = cell == "lstm"
    Policy, G, pre = (LSTMPolicy, 4, "ppo_bptt") if lstm else (GRUPolicy, 3, "ppo_seq")
    D, lines = env.obs_dim, []
    for H, hw in SEQ_NETS:
        gru = tuple((0.3 * rng.randn(*s)).astype(np.float32) for s in ((G * H, D), (G * H, H), (G * H,), (G * H,)))
        head = layers(rng, H, hw, 4)
        W = ([H] + hw)[-1]
        value = ((rng.randn(W) / np.sqrt(W)).astype(np.float32), np.float32(0.1))
        for with_head in (False, True):
            pol = Policy(env, gru, head, "tanh", True, log_std=LOG_STD, value=value if with_head else None)
            for T in SEQ_T:
                n = (T, SEQ_SRC)
                obs, act, h0 = t(rng.randn(*n, D)), t(rng.randn(*n, 4)), t(0.5 * rng.randn(SEQ_SRC, H))
                lpo, adv, ret, vold = t(-4.0 + rng.randn(*n)), t(rng.randn(*n)), t(rng.randn(*n)), t(rng.randn(*n))
                st0 = (h0, t(0.5 * rng.randn(SEQ_SRC, H))) if lstm else (h0,)   # the initial states
                done = np.zeros(n, np.uint8)
                done[T // 2, ::3] = 1                               # the middle step
                done = torch.as_tensor(done, device=dev)
                vargs = (ret, vold) if with_head else (None, None)
                for S, groups in [(S, None) for S in SEQ_S] + [(SEQ_SRC, "2")] * (with_head and T == SEQ_T[-1] and bool(hw)):
                    if groups:
                        os.environ["GAQ_GRAD_GROUPS"] = groups
                    cut = lambda x, dim=1: None if x is None else x.narrow(dim, 0, S).contiguous()
                    mean, h_out = torch.zeros((T, S, 4), device=dev), torch.zeros((S, H), device=dev)
                    fin = dict(h_out=h_out, c_out=torch.zeros((S, H), device=dev)) if lstm else dict(h_out=h_out)
                    cut0 = [cut(x, 0) for x in st0]
                    lp, val = pol.evaluate_seq_dev(cut(obs), cut(act), cut(done), *cut0, mean=mean, **fin)
                    outs = [("eval_seq.logp", lp), ("eval_seq.value", val), ("eval_seq.mean", mean)]
                    outs += [("eval_seq." + k, x) for k, x in fin.items()]
                    names = ("grad", "grad_value", "grad_log_std", "stats")
                    res = getattr(pol, pre + "_grad_dev")(cut(obs), cut(act), cut(done), *cut0, cut(lpo), cut(adv), *map(cut, vargs), **AC)
                    outs += [(pre + "." + k, x) for k, x in zip(names, res)]
                    idx = rng.permutation(SEQ_SRC)[:S]
                    if S == 65 and T == 3:
                        idx[5] = -1                                 # one index out of range
                    res = getattr(pol, pre + "_grad_idx_dev")(ti(idx), obs, act, done, *st0, lpo, adv, *vargs, **AC)
                    outs += [(pre + "_idx." + k, x) for k, x in zip(names, res)]
                    torch.cuda.synchronize()
                    os.environ.pop("GAQ_GRAD_GROUPS", None)
                    tag = cell + "%d-%s head=%d T=%d S=%d groups=%s" % (H, "x".join(map(str, hw)) or "none", with_head, T, S, groups or "default")
                    lines += ["%-48s %-26s %s" % (tag, k, md5(x)) for k, x in outs if x is not None]
            pol.close()
    return lines


def enc_seq_lines(env, dev, rng, t, ti, cell):
    """the encoder forms of one cell: seq_lines' sources and cuts for a policy with an encoder in front of the cell, the smaller one
    without a value head, the larger one with its own"""
    import torch
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy
    lstm = cell == "lstm"
    Policy, G = (LSTMPolicy, 4) if lstm else (GRUPolicy, 3)
    D, lines = env.obs_dim, []
    for (ew, H, hw), with_head in zip(ENC_SEQ_NETS, (False, True)):
        enc = layers(rng, D, list(ew), ew[-1])[:-1]                # (layers' last one is an output layer: not an encoder's)
        E = ew[-1]
        weights = tuple((0.3 * rng.randn(*s)).astype(np.float32) for s in ((G * H, E), (G * H, H), (G * H,), (G * H,)))
        head = layers(rng, H, hw, 4)
        W = ([H] + hw)[-1]
        value = ((rng.randn(W) / np.sqrt(W)).astype(np.float32), np.float32(0.1))
        pol = Policy.with_encoder(env, enc, weights, head, "tanh", True, log_std=LOG_STD, value=value if with_head else None)
        for T in SEQ_T:
            n = (T, SEQ_SRC)
            obs, act, h0 = t(rng.randn(*n, D)), t(rng.randn(*n, 4)), t(0.5 * rng.randn(SEQ_SRC, H))
            lpo, adv, ret, vold = t(-4.0 + rng.randn(*n)), t(rng.randn(*n)), t(rng.randn(*n)), t(rng.randn(*n))
            st0 = (h0, t(0.5 * rng.randn(SEQ_SRC, H))) if lstm else (h0,)
            done = np.zeros(n, np.uint8)
            done[T // 2, ::3] = 1
            done = torch.as_tensor(done, device=dev)
            vargs = (ret, vold) if with_head else (None, None)
            for S in SEQ_S:
                cut = lambda x, dim=1: None if x is None else x.narrow(dim, 0, S).contiguous()
                mean, h_out = torch.zeros((T, S, 4), device=dev), torch.zeros((S, H), device=dev)
                fin = dict(h_out=h_out, c_out=torch.zeros((S, H), device=dev)) if lstm else dict(h_out=h_out)
                cut0 = [cut(x, 0) for x in st0]
                lp, val = pol.evaluate_enc_seq_dev(cut(obs), cut(act), cut(done), *cut0, mean=mean, **fin)
                outs = [("eval_enc_seq.logp", lp), ("eval_enc_seq.value", val), ("eval_enc_seq.mean", mean)]
                outs += [("eval_enc_seq." + k, x) for k, x in fin.items()]
                names = ("grad", "grad_encoder", "grad_value", "grad_log_std", "stats")
                res = pol.ppo_enc_seq_grad_dev(cut(obs), cut(act), cut(done), *cut0, cut(lpo), cut(adv), *map(cut, vargs), **AC)
                outs += [("ppo_enc_seq." + k, x) for k, x in zip(names, res)]
                idx = rng.permutation(SEQ_SRC)[:S]
                if S == 65 and T == 3:
                    idx[5] = -1                                     # one index out of range
                res = pol.ppo_enc_seq_grad_idx_dev(ti(idx), obs, act, done, *st0, lpo, adv, *vargs, **AC)
                outs += [("ppo_enc_seq_idx." + k, x) for k, x in zip(names, res)]
                torch.cuda.synchronize()
                tag = "enc%s-%s%d-%s head=%d T=%d S=%d" % ("x".join(map(str, ew)), cell, H, "x".join(map(str, hw)) or "none", with_head, T, S)
                lines += ["%-48s %-30s %s" % (tag, k, md5(x)) for k, x in outs if x is not None]
        pol.close()
    return lines


if __name__ == "__main__":
    main()
