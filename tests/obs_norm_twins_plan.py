"""The case lists of tests/test_gpu_obs_norm_twins.py and the arithmetic its bit-for-bit argument stands on, in plain Python and numpy, so
that tests/test_obs_norm_twins_cpu.py can check both without a GPU.

A name X_norm_kernel here is a label: the <PolObsNorm> instantiation of the kernel template X_kernel, whose plain original is X_kernel<>.

The argument.  The thirteen *_norm_kernel twins of gym_art_amd/csrc/gaq_policy.hip differ from their plain originals by one staging line:
input k of a live row goes through obs_norm_elem(x, mean[k], inv_std[k], clip) on its way into the LDS.  With mean 0, clip +inf and
inv_std[k] = s[k] a power of two, the staged value is x s[k] EXACTLY (fp32 and bf16 alike: a power-of-two scaling moves the exponent
only, as long as nothing leaves the normal range), and (x s) w and x (w s) are the same real number.  Every sum the first layer forms --
an fmaf chain, a matrix-core k-step, in whatever order -- is a function of those real products and of the roundings applied to their
sums, so the twin with the table and weights W computes, bit for bit, what the plain kernel computes with weights W s[None, :] and no
table.  Everything downstream (the other layers, the env's step, the value, the log-probability, the terminal pass) sees the same bits.
The scales differ from column to column, so a twin that reads another column's scale, drops the scale, or reads the table with another
`dim` breaks the equality: emulate_first_layer and its MUTANTS show by how much."""
import collections

import numpy as np

from tests.obs_norm_ref import WIDTHS

T = 20                                           # ep_time = 0.15: episodes of 16 steps, every env finishes inside the window
STAGGER_AFTER, STAGGER_MASKED = 5, 63            # the staggered regime: 5 steps, then envs 0 .. 62 start over
KERNELS = ["policy_mfma_norm_kernel", "policy_gru_norm_kernel", "policy_lstm_norm_kernel", "policy_mfma_bf16_norm_kernel",
           "policy_mfma_ac_norm_kernel", "policy_gru_ac_norm_kernel", "policy_lstm_ac_norm_kernel",
           "policy_mfma_term_norm_kernel", "policy_gru_term_norm_kernel", "policy_lstm_term_norm_kernel",
           "critic_mfma_norm_kernel", "critic_mfma_term_norm_kernel", "policy_mfma_critic_norm_kernel"]

Family = collections.namedtuple("Family", "kind ask critic kernels")
# kind: the actor ("mlp" and "bf16": an MLPPolicy on that engine); ask: what the rollout is asked for beside the actions ("v" values,
# "lp" log-probabilities, "tv" terminal values); critic: V comes from an MLPCritic with the same normaliser; kernels: the twins reached
FAMILIES = collections.OrderedDict([
    ("mlp", Family("mlp", (), False, ("policy_mfma_norm_kernel",))),
    ("mlp_ac", Family("mlp", ("v", "lp", "tv"), False, ("policy_mfma_ac_norm_kernel", "policy_mfma_term_norm_kernel"))),
    ("gru", Family("gru", (), False, ("policy_gru_norm_kernel",))),
    ("gru_ac", Family("gru", ("v", "lp", "tv"), False, ("policy_gru_ac_norm_kernel", "policy_gru_term_norm_kernel"))),
    ("lstm", Family("lstm", (), False, ("policy_lstm_norm_kernel",))),
    ("lstm_ac", Family("lstm", ("v", "lp", "tv"), False, ("policy_lstm_ac_norm_kernel", "policy_lstm_term_norm_kernel"))),
    ("bf16", Family("bf16", (), False, ("policy_mfma_bf16_norm_kernel",))),
    # the fused launch per step, critic_mfma_norm_kernel for the bootstrap row
    ("mlp_critic", Family("mlp", ("v", "tv"), True, ("policy_mfma_critic_norm_kernel", "critic_mfma_norm_kernel", "critic_mfma_term_norm_kernel"))),
    # two launches per step
    ("gru_critic", Family("gru", ("v", "tv"), True, ("policy_gru_norm_kernel", "critic_mfma_norm_kernel", "critic_mfma_term_norm_kernel"))),
])
BIG_BATCH_FAMILIES = ("mlp_ac", "lstm_ac")       # the only ones that run N = 2096 in the sweep

# the smallest nets that reach each code path: 3 chunks of 16 units (wave 3 idle) and 5 chunks; bf16 first layers of 3 and 9 chunks
MLP_NETS = [[48], [80, 48]]
REC_H, REC_HEADS = [48, 80], [(), (16, 80)]
BF16_NETS = [[48, 48], [144, 48]]
CRITIC_NETS = [[80, 48], [48]]

# widths: an MLP's or a bf16 net's hidden widths; H, head: a recurrent cell and its head's hidden widths; critic: the critic's hidden
# widths (families with a critic); k: tests/test_gpu_policy_shapes.py _style(k) gives the hidden activation and the output tanh
Net = collections.namedtuple("Net", "widths H head critic k")
# single: the window runs as calls of ONE step each (bit-equal to one call: tests/test_gpu_policy_ac_shapes.py
# test_gather_at_done_counts_of_1_to_129), which is how a batch with N D % 4 != 0 runs at all -- a T > 1 call needs N D 4 bytes to be a
# multiple of 16
Case = collections.namedtuple("Case", "family D N layout net stagger single")


def scales(D):
    """s[k] = 2^((3 k mod 5) - 2): 1/4, 2, 1/2, 4, 1, ... as float32"""
    return (2.0 ** ((3 * np.arange(D)) % 5 - 2)).astype(np.float32)


def batches(agents):
    """tests/test_gpu_policy_shapes.py _batches: a single partial tile, one full tile, a tile plus a sliver, 32 tiles plus a tail"""
    q = max(4, agents)
    return [q, 64, 64 + q, 2096]


def net_of(family, i):
    """the net of `family` at the i-th observation width: the variants in turn by width, the style k = i + i // 2 so that every variant
    meets both activations (the CPU file checks this)"""
    kind = FAMILIES[family].kind
    k = i + i // 2
    widths = MLP_NETS[i % 2] if kind == "mlp" else BF16_NETS[i % 2] if kind == "bf16" else None
    H, head = (None, None) if widths else (REC_H[i % 2], REC_HEADS[(i // 2) % 2])
    return Net(widths, H, head, CRITIC_NETS[i % 2] if FAMILIES[family].critic else None, k)


def sweep(obs):
    """[(family, [Case, ...])] at one entry of OBS (obs_repr, agents, D): every family at q, 64 and 64 + q envs in the alias layout,
    BIG_BATCH_FAMILIES at 2096 too"""
    _, agents, D = obs
    i = WIDTHS.index(D)
    out = []
    for family in FAMILIES:
        ns = batches(agents)[:4 if family in BIG_BATCH_FAMILIES else 3]
        out.append((family, [Case(family, D, n, "alias", net_of(family, i), False, False) for n in ns]))
    return out


def extras():
    """the cases beside the sweep, [(id, Case)]"""
    out = []
    i20, i19 = WIDTHS.index(20), WIDTHS.index(19)
    for family in ("gru_ac", "lstm_ac"):                            # single rows and tile edges: D = 20 makes N D a multiple of 4
        out += [("d20-%s-n%d" % (family, n), Case(family, 20, n, "alias", net_of(family, i20), False, False)) for n in (1, 63, 65)]
    for family in ("gru_ac", "lstm_ac"):                            # the 157 KiB LDS case
        out += [("d108-%s-h256-n%d" % (family, n), Case(family, 108, n, "alias", Net(None, 256, (), None, 0), False, False)) for n in (16, 2096)]
    out.append(("d108-mlp256x3-critic256x2", Case("mlp_critic", 108, 80, "alias", Net([256, 256, 256], None, None, [256, 256], 0), False, False)))
    for family in FAMILIES:                                         # gathered passes of 67 and 63 rows, a partial k-step of 3
        out.append(("d19-%s-staggered" % family, Case(family, 19, 130, "alias", net_of(family, i19), True, True)))
    for D in (13, 108):                                             # both layouts (the sweep runs "alias")
        for family in BIG_BATCH_FAMILIES:
            n = batches(16 if D == 108 else 0)[2]
            out += [("d%d-%s-%s" % (D, family, layout), Case(family, D, n, layout, net_of(family, WIDTHS.index(D)), False, False))
                    for layout in ("alias", "plain")]
    return out


# ---- what a width reaches -------------------------------------------------------------------------------------------------------------
def partial_k_step(D):
    """the rows of the first layer's last fp32 k-step of 4 inputs that are real (0: the width is a multiple of 4, no padded input)"""
    return D % 4


def k_steps(D):
    """fp32 k-steps of 4 inputs, the partial one included"""
    return (D + 3) // 4


def bf16_k_steps(D):
    """bf16 k-steps of 32 inputs"""
    return (D + 31) // 32


def recurrent_ac_lds(D, H, head=()):
    """a recurrent actor-critic launch: 1 KiB of output sums + 1 KiB of value parts + 256 B x (kin + H + max(H, head widths))"""
    return 2048 + 256 * (((D + 3) & ~3) + H + max((H,) + tuple(head)))


# ---- the first layer in the device's number formats ---------------------------------------------------------------------------------
MUTANTS = ["next_column", "no_scale", "dim_minus_one"]


def staged(x, s, mutant=None):
    """what the twin stages from rows x [R, D] under the table (mean 0, inv_std s, clip inf): obs_norm_elem in float32.
    mutant "next_column": the scale of column k + 1 (the last column reads the clip, +inf, as tab[dim + k + 1] would); "no_scale": the
    table is not applied; "dim_minus_one": the table read with dim = D - 1 -- inv_std[k] = tab[D - 1 + k] is the last MEAN (0) for
    k = 0 and s[k - 1] after it, and the clip tab[2 D - 2] is s[D - 2]."""
    x, s = np.asarray(x, np.float32), np.asarray(s, np.float32)
    inv, clip = s, np.float32(np.inf)
    if mutant == "next_column":
        inv = np.concatenate([s[1:], [np.float32(np.inf)]]).astype(np.float32)
    elif mutant == "no_scale":
        return x.copy()
    elif mutant == "dim_minus_one":
        inv, clip = np.concatenate([[np.float32(0.0)], s[:-1]]).astype(np.float32), s[-2]
    else:
        assert mutant is None, mutant
    with np.errstate(invalid="ignore"):
        return np.minimum(np.maximum((x - np.float32(0.0)) * inv[None, :], -clip), clip).astype(np.float32)


def fmaf_chain(x, W, b):
    """one ascending fmaf chain per (row, unit) in float32: acc = b; acc = fma(x[k], W[u, k], acc) for k = 0 .. D - 1.  The fma is the
    float64 value of x w + acc rounded to float32: the product of two fp32 values is exact in float64, the sum is rounded there and
    again to float32 -- a double rounding that can differ from a true fma in rare ties, and differs the SAME way for every pair of
    inputs with the same real products, which is all the comparison needs.  x [R, D], W [U, D], b [U] -> [R, U] float32"""
    x, W = np.asarray(x, np.float32).astype(np.float64), np.asarray(W, np.float32).astype(np.float64)
    acc = np.broadcast_to(np.asarray(b, np.float32), (x.shape[0], W.shape[0])).astype(np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(x.shape[1]):
            acc = (x[:, k, None] * W[None, :, k] + acc.astype(np.float64)).astype(np.float32)
    return acc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
