"""The edge shapes of the learner's passes for a recurrent policy with an encoder: a second case list over the reference of
tests/policy_grad_enc_ref.py (its EncCase, inputs, ppo_enc_seq, torch_errors and conditions, imported; its tables stay what they are).

Cases, each for a shape the parent list never reaches:
  enc112-lstm64x64x64-tanh-vclip    the largest LDS the backward sequence kernel is launched with (gaq.h's formula: 160 768 B, 161 024 B
                                    in the idx form, against 163 840 B; E = 128 in front of the same cell is refused)
  enc128x128-gru64x64-relu          both encoder layers at the width limit: grad_feat_kernel's LDS is 272 B x (32 + 256) = 78 336 B,
                                    above the 64 KiB a launch may use without hipFuncSetAttribute
  enc64x32-lstm48x32-tanh-vclip-d19 a first layer wider than the second (W_l^T delta: two input chunks and a single unit chunk per wave),
                                    H = 48 (hc = 3: wave 3 idle in the cell stages, 12 gate chunks in the dfeat product), D = 19
  enc128x16-gru48-relu-norm         the steepest narrowing pair, H = 48 on a GRU (9 gate chunks), behind the normaliser
  enc16x16-gru16-tanh-nohead        the smallest pair: three of the four waves idle in every stage; no value head
Every case has the parent's TMAX = 6 steps of SMAX = 130 sequences; CONFIGS is (1, 1), (5, 65), (6, 130).

SEEDS: the first seed of each case that meets the parent's conditions(); BASELINE: torch fp32 autograd's errors on the CPU against the
fp64 reference, per case and (T, S), as the parent's table holds them (python -m tests.policy_grad_enc_edges prints both).  bounds() is
the parent's rule unchanged -- FACTOR = 8 x torch's error: the two gradients' the case's own, logp's and V's the case's own at more than
one row, the true scalars (the three sums at every size, logp and V at (1, 1)) pooled over BOTH case lists at that size."""
import numpy as np

from tests import policy_grad_enc_ref as R

G = R.G
TMAX, SMAX, FACTOR = R.TMAX, R.SMAX, R.FACTOR
VCLIP = R.VCLIP
CONFIGS = [(1, 1), (5, 65), (6, 130)]
LDS_MAX = 160 * 1024

EDGE_CASES = [R.EncCase("lstm", (112,), 64, (64, 64), "tanh", True, vclip=VCLIP),
              R.EncCase("gru", (128, 128), 64, (64,), "relu", False),
              R.EncCase("lstm", (64, 32), 48, (32,), "tanh", True, D=19, vclip=VCLIP),
              R.EncCase("gru", (128, 16), 48, (), "relu", False, norm=True),
              R.EncCase("gru", (16, 16), 16, (), "tanh", True, value=False)]
CASES = {c.name: c for c in EDGE_CASES}


def seq_lds(E, lstm, H, head, idx=False, bwd=True):
    """gaq.h's formula for the sequence kernel's LDS in bytes: 8.25 KiB + 272 B x (in_dim rounded up to 16 + carried H + max(4 H, H +
    the head widths)), carried = 2 (hin, dh; the LSTM 3: dc), + 256 B for the idx form; the forward call: E + 2 H + the head widths"""
    kx = (E + 15) & ~15
    rows = kx + ((3 if lstm else 2) * H + max(4 * H, H + sum(head)) if bwd else 2 * H + sum(head))
    return 8448 + 272 * rows + (256 if idx else 0)


def grad_feat_lds(D, enc, idx=False):
    """gaq.h's formula for the encoder's backward: 272 B x (obs_dim rounded up to 16 + the encoder's widths) (+ 256 B for the idx form)"""
    return 272 * (((D + 15) & ~15) + sum(enc)) + (256 if idx else 0)


def case_lds(case, idx=False):
    """(the backward sequence kernel's, grad_feat_kernel's) LDS bytes of a gradient call of the case"""
    return seq_lds(case.enc[-1], case.cell == "lstm", case.H, case.head, idx), grad_feat_lds(case.D, case.enc, idx)


# the seed of each case: the first that meets policy_grad_enc_ref.conditions() (python -m tests.policy_grad_enc_edges)
SEEDS = {
    'enc112-lstm64x64x64-tanh-vclip': 3,
    'enc128x128-gru64x64-relu': 269,
    'enc64x32-lstm48x32-tanh-vclip-d19': 21,
    'enc128x16-gru48-relu-norm': 14,
    'enc16x16-gru16-tanh-nohead': 9,
}

# per case and (T, S): torch fp32 autograd's (gradient, encoder gradient, logp, V, sum L_clip, sum k3, sum L_V) errors against the
# reference (python -m tests.policy_grad_enc_edges; torch on the CPU)
BASELINE = {
    'enc112-lstm64x64x64-tanh-vclip': {(1, 1): (5.04e-07, 6.73e-07, 2.61e-08, 4.24e-07, 1.39e-07, 1.13e-05, 1.54e-07), (5, 65): (1.29e-06, 1.07e-06, 1.5e-07, 4.29e-07, 3.09e-07, 1.24e-07, 3.41e-08), (6, 130): (6.94e-07, 1.09e-06, 1.24e-07, 3.59e-07, 1.27e-07, 3.02e-08, 1.17e-08)},
    'enc128x128-gru64x64-relu': {(1, 1): (4e-07, 2.49e-07, 2.99e-08, 4.19e-08, 1.05e-08, 0.000342, 1.78e-07), (5, 65): (4.29e-06, 1.03e-06, 2.6e-07, 3.84e-07, 2.75e-06, 9.45e-08, 1.7e-08), (6, 130): (1.8e-06, 1.01e-06, 2.8e-07, 3.28e-07, 1.42e-06, 3.56e-07, 4.09e-08)},
    'enc64x32-lstm48x32-tanh-vclip-d19': {(1, 1): (1.76e-07, 5.48e-07, 4.42e-08, 5.73e-08, 1.9e-07, 5.31e-06, 1.32e-07), (5, 65): (9.92e-07, 7.85e-07, 1.02e-07, 1.86e-07, 4.6e-07, 2.18e-07, 5.25e-08), (6, 130): (5.04e-07, 5.93e-07, 7.13e-08, 1.9e-07, 2.31e-07, 1.57e-07, 7.65e-08)},
    'enc128x16-gru48-relu-norm': {(1, 1): (5.52e-07, 1.98e-07, 1.63e-07, 1.25e-07, 4.29e-07, 5.85e-05, 1.16e-07), (5, 65): (8.86e-07, 7.44e-07, 1.78e-07, 3e-07, 1.11e-06, 3.18e-07, 2.44e-08), (6, 130): (1.45e-06, 7.13e-07, 3.04e-07, 3.05e-07, 2.38e-07, 4.64e-08, 6.33e-08)},
    'enc16x16-gru16-tanh-nohead': {(1, 1): (2.69e-07, 5.33e-07, 6.8e-08, 1.02e-07, 2.55e-07, 5.27e-07, 0), (5, 65): (1.11e-06, 6.73e-07, 1.21e-07, 1.68e-07, 8.48e-07, 1.86e-07, 0), (6, 130): (7.03e-07, 5.34e-07, 1.26e-07, 1.5e-07, 8.89e-08, 1.28e-07, 0)},
}

_INPUTS, _REFS = {}, {}


def case_inputs(name):
    """the case and its inputs at its seed, computed once and shared: treat them as read-only"""
    if name not in _INPUTS:
        _INPUTS[name] = R.inputs(CASES[name], SEEDS[name])
    return CASES[name], _INPUTS[name]


def case_ref(name, T, S):
    """ppo_enc_seq of the case at its defaults on the prefix (T, S), computed once and shared: read-only"""
    if (name, T, S) not in _REFS:
        case, inp = case_inputs(name)
        _REFS[name, T, S] = R.ppo_enc_seq(case, inp, T, S)
    return _REFS[name, T, S]


def bounds(name, T, S):
    """policy_grad_enc_ref.bounds' rule for a case of this list: (gradient, encoder gradient, logp, V, sum L_clip, sum k3, sum L_V)"""
    rows = [BASELINE[c.name][T, S] for c in EDGE_CASES] + [R.BASELINE[c.name][T, S] for c in R.ENC_CASES]
    pooled = [max(r[k] for r in rows) for k in range(2, 7)]
    own = BASELINE[name][T, S]
    one = T * S == 1
    return (FACTOR * own[0], FACTOR * own[1], FACTOR * (pooled[0] if one else own[2]), FACTOR * (pooled[1] if one else own[3]),
            FACTOR * pooled[2], FACTOR * pooled[3], FACTOR * pooled[4])


if __name__ == "__main__":
    import sys
    import torch
    seeds = {c.name: R.find_seed(c) for c in EDGE_CASES}
    out = ["SEEDS = {"] + ["    %r: %d," % kv for kv in seeds.items()] + ["}", "", "BASELINE = {"]
    for c in EDGE_CASES:
        inp = R.inputs(c, seeds[c.name])
        out.append("    %r: {%s}," % (c.name, ", ".join("(%d, %d): (%s)" % (T, S, ", ".join("%.3g" % e for e in R.torch_errors(c, inp, T, S, torch.float32)))
                                                        for T, S in CONFIGS)))
    out.append("}")
    print("\n".join(out))
    sys.stdout.flush()
