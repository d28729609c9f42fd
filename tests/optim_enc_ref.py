"""The reference of the optimiser of a recurrent policy with an encoder (gaq.h gaq_optim_create_policy_enc, gaq_optim_step_enc_dev;
gym_art_amd.policy.AdamEncDev): the four groups -- weights, value head, log_std, encoder -- over tests/optim_ref.py's fp64 step.  That
module has three group slots and treats slots 0 and 1 alike, so the encoder's block rides behind the weights in slot 0 (the same
arithmetic per element, the same joint norm, weight decay as on the weights), as tests/test_gpu_optim_enc.py already does.

Cases: the layouts at which the four-group kernels can go wrong -- an index space [0, end[3]) cut into chunks of 2048 elements, group k
being [end[k-1], end[k]) -- chosen so that each property follows from the element counts (tests/test_optim_enc_cpu.py asserts them):
  enc16-gru16-head-logstd        all four groups inside one chunk: 1700 + 17 + 4 + 304 = 2025
  enc16-gru16-frozen-nohead      both middle groups empty (end[0] == end[1] == end[2]): no value head, log_std set but not learned
  enc16-lstm16-det-nohead        the same with no log_std at all; the chunk boundary at 2048 inside the weights (2244), the encoder's
                                 group wholly in the second chunk
  enc16x16-gru16-nohead          only the value head empty; the boundary inside the encoder's group (it starts at 1704)
  enc16x16-gru16-head-frozen     only log_std empty; the boundary inside the encoder's group (it starts at 1717)
  enc16x16-gru16-head-logstd     all four, the encoder's group from 1721 across the boundary
  enc128x128-gru16-head-logstd   thirteen chunks, the encoder at both width limits (19 072 of 26 169 elements), D = 19
The hyper-parameters vary as optim_ref.CASES' do: weight decay on and off, a clip far above and far below the norm, no clip,
non-default betas and eps.

Gradients: optim_ref.gradients' recipe (magnitudes log-uniform over [1e-6, 10], random signs, about 5 % exact zeros), a fresh draw per
step.  STEPS = 10, compared after 1, 2 and 10.  BASELINE: torch fp32's error (AdamW / Adam + clip_grad_norm_, foreach=False, CPU) against
the reference per case, step count, quantity and group; the device's bound is optim_ref.bound's rule, max(8 x that, k x 2^-24).

python -m tests.optim_enc_ref prints BASELINE."""
import numpy as np

from tests import optim_ref as O

FACTOR, STEPS, AT = O.FACTOR, O.STEPS, O.AT
GROUPS = ("weights", "value_head", "log_std", "encoder")
CHUNK = 2048                    # elements of one workgroup of the two-launch form (gaq_optim.hip kOptChunk)
FROZEN_LOG_STD = np.array([-0.5, -0.7, -0.4, -0.6], np.float32)     # what a policy explores with when the optimiser does not learn it


def encoder_count(D, enc):
    """floats of the encoder's block: W and b of each layer"""
    n, prev = 0, D
    for w in enc:
        n += w * prev + w
        prev = w
    return n


class Case:
    """cell: "gru" | "lstm"; enc: the encoder's widths; widths: the cell's H, then the head's widths; head: a value head; log_std:
    "learn" (group 2 holds it), "frozen" (the policy explores, the optimiser is made with learn_log_std=False) or None (deterministic);
    hp: lr, betas, eps, weight_decay, max_grad_norm; clip: "above" / "below" -- every step's norm far above / below max_grad_norm"""

    def __init__(self, name, cell, enc, widths, D=18, head=True, log_std="learn", lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=None, clip=None):
        self.name, self.cell, self.enc, self.widths, self.D = name, cell, tuple(enc), list(widths), D
        self.head, self.log_std, self.clip = head, log_std, clip
        self.hp = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)

    @property
    def sizes(self):
        """floats of each group: weights, value head, log_std, encoder (0: the group is empty)"""
        nw = O.Case(self.name, self.cell, self.widths, D=self.enc[-1]).weight_count          # the cell reads the features
        return (nw, self.widths[-1] + 1 if self.head else 0, 4 if self.log_std == "learn" else 0, encoder_count(self.D, self.enc))

    @property
    def ends(self):
        """the kernels' end[0 .. 3]"""
        return tuple(int(x) for x in np.cumsum(self.sizes))


CASES = [
    Case("enc16-gru16-head-logstd", "gru", (16,), [16], max_grad_norm=0.5, clip="above"),
    Case("enc16-gru16-frozen-nohead", "gru", (16,), [16], head=False, log_std="frozen"),
    Case("enc16-lstm16-det-nohead", "lstm", (16,), [16], head=False, log_std=None, lr=1e-3, betas=(0.8, 0.99), max_grad_norm=0.5),
    Case("enc16x16-gru16-nohead", "gru", (16, 16), [16], head=False, lr=1e-3, weight_decay=1e-2, max_grad_norm=1e4, clip="below"),
    Case("enc16x16-gru16-head-frozen", "gru", (16, 16), [16], log_std="frozen", eps=1e-5, weight_decay=0.1, max_grad_norm=0.5),
    Case("enc16x16-gru16-head-logstd", "gru", (16, 16), [16], weight_decay=1e-2),
    Case("enc128x128-gru16-head-logstd", "gru", (128, 128), [16], D=19, max_grad_norm=40.0),
]
BY_NAME = {c.name: c for c in CASES}
_SEED = {c.name: 3000 + 17 * k for k, c in enumerate(CASES)}


def theta0(case):
    """the initial parameters, one fp32 array per group (empty: absent): weights, head and encoder uniform in +-0.5, log_std around -0.5"""
    rng = np.random.RandomState(_SEED[case.name])
    nw, nh, nl, ne = case.sizes
    return [rng.uniform(-0.5, 0.5, nw).astype(np.float32), rng.uniform(-0.5, 0.5, nh).astype(np.float32),
            (-0.5 + rng.uniform(-0.2, 0.2, nl)).astype(np.float32), rng.uniform(-0.5, 0.5, ne).astype(np.float32)]


def gradients(case, step):
    """the synthetic gradients of step `step` (0-based), one fp32 array per group, by optim_ref.gradients' recipe"""
    rng = np.random.RandomState(_SEED[case.name] + 7919 * (step + 1))
    out = []
    for n in case.sizes:
        g = 10.0 ** rng.uniform(-6.0, 1.0, n) * rng.choice([-1.0, 1.0], n)
        g[rng.uniform(size=n) < 0.05] = 0.0
        out.append(g.astype(np.float32))
    return out


def _slots(x):
    """four groups -> optim_ref's three slots: the encoder's block behind the weights"""
    return [np.concatenate([x[0], x[3]]), x[1], x[2]]


def _groups(case, x):
    nw = case.sizes[0]
    return [x[0][:nw].copy(), x[1].copy(), x[2].copy(), x[0][nw:].copy()]


def trajectory(case, steps=STEPS):
    """the reference after each of `steps` steps: [(theta, m, v per group, stats), ...]"""
    st, out = O.State(_slots(theta0(case))), []
    for k in range(steps):
        stats = O.step(st, _slots(gradients(case, k)), **case.hp)
        out.append((_groups(case, st.theta), _groups(case, st.m), _groups(case, st.v), stats))
    return out


_TRAJ = {}


def reference(name):
    """trajectory(case), computed once and shared: treat it as read-only"""
    if name not in _TRAJ:
        _TRAJ[name] = trajectory(BY_NAME[name])
    return _TRAJ[name]


def torch_run(case, dtype, steps=STEPS):
    """torch.optim.Adam / AdamW (foreach=False) with clip_grad_norm_ on the CPU in `dtype`, on the same inputs -> after each step
    (theta, m, v) as lists of arrays per group, and (norm, coef)"""
    import torch
    params = [torch.tensor(t, dtype=dtype, requires_grad=True) for t in theta0(case)]
    live = [p for p in params if p.numel()]
    wd = case.hp["weight_decay"]
    kw = dict(lr=case.hp["lr"], betas=case.hp["betas"], eps=case.hp["eps"], foreach=False)
    if wd:
        groups = [{"params": [p for p in (params[0], params[1], params[3]) if p.numel()], "weight_decay": wd}]
        if params[2].numel():
            groups.append({"params": [params[2]], "weight_decay": 0.0})
        opt = torch.optim.AdamW(groups, **kw)
    else:
        opt = torch.optim.Adam(live, **kw)
    out = []
    for k in range(steps):
        for p, g in zip(params, gradients(case, k)):
            p.grad = torch.tensor(g, dtype=dtype)
        mgn = case.hp["max_grad_norm"]
        if mgn:
            norm = float(torch.nn.utils.clip_grad_norm_(live, mgn, foreach=False))
        else:
            norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in live])))
        coef = min(1.0, mgn / (norm + 1e-6)) if mgn else 1.0
        opt.step()
        zero = np.zeros(0)
        out.append(([p.detach().numpy().copy() for p in params],
                    [opt.state[p]["exp_avg"].numpy().copy() if p.numel() else zero for p in params],
                    [opt.state[p]["exp_avg_sq"].numpy().copy() if p.numel() else zero for p in params], (norm, coef)))
    return out


def torch_errors(case, dtype, at=AT):
    """torch in `dtype` against the reference: {steps: {"theta" | "m" | "v": (error per group)}} plus the worst error of norm and coef
    over the steps"""
    ref, got = reference(case.name), torch_run(case, dtype, max(at))
    errs = {}
    for k in at:
        errs[k] = {what: tuple(O.rel(a, b) for a, b in zip(got[k - 1][i], ref[k - 1][i])) for i, what in enumerate(("theta", "m", "v"))}
    scal = max(max(O.rel(g[3][0], r[3][0]), O.rel(g[3][1], r[3][1])) for g, r in zip(got, ref))
    return errs, scal


# per case: after 1, 2 and 10 steps, torch fp32's error (CPU, foreach=False) against the reference for theta, m and v of each
# group -- weights, value head, log_std, encoder; 0 for an empty group (python -m tests.optim_enc_ref)
BASELINE = {
    'enc16-gru16-head-logstd': {1: {'theta': (2.98e-08, 2.04e-08, 2.07e-08, 2.99e-08), 'm': (1.14e-07, 3.1e-08, 3.63e-08, 7.9e-08), 'v': (2.35e-07, 6.32e-08, 1.19e-07, 1.11e-07)}, 2: {'theta': (5.92e-08, 5.05e-08, 7.16e-08, 5.47e-08), 'm': (1.15e-07, 8.94e-08, 2.48e-07, 1.46e-07), 'v': (2.8e-07, 1.15e-07, 4.49e-07, 3.05e-07)}, 10: {'theta': (1.59e-07, 1.02e-07, 1.18e-07, 1.78e-07), 'm': (1.15e-07, 4.28e-08, 3.08e-08, 9.52e-08), 'v': (2.19e-07, 1.73e-07, 1.69e-07, 2.92e-07)}},
    'enc16-gru16-frozen-nohead': {1: {'theta': (2.97e-08, 0, 0, 4.11e-08), 'm': (3.61e-08, 0, 0, 3.58e-08), 'v': (1.12e-07, 0, 0, 8.67e-08)}, 2: {'theta': (6.84e-08, 0, 0, 5.41e-08), 'm': (7.02e-08, 0, 0, 4.86e-08), 'v': (1.02e-07, 0, 0, 9.82e-08)}, 10: {'theta': (1.72e-07, 0, 0, 1.27e-07), 'm': (1.1e-07, 0, 0, 7.75e-08), 'v': (1.95e-07, 0, 0, 2.35e-07)}},
    'enc16-lstm16-det-nohead': {1: {'theta': (4.5e-08, 0, 0, 2.98e-08), 'm': (1.75e-07, 0, 0, 1.76e-07), 'v': (2.76e-07, 0, 0, 2.38e-07)}, 2: {'theta': (8.93e-08, 0, 0, 5.46e-08), 'm': (1.46e-07, 0, 0, 1.57e-07), 'v': (2.4e-07, 0, 0, 2.39e-07)}, 10: {'theta': (1.92e-07, 0, 0, 1.31e-07), 'm': (1.35e-07, 0, 0, 1.92e-07), 'v': (2.14e-07, 0, 0, 2.49e-07)}},
    'enc16x16-gru16-nohead': {1: {'theta': (7.32e-08, 0, 2.44e-08, 6.65e-08), 'm': (3.59e-08, 0, 4.61e-08, 3.74e-08), 'v': (1.19e-07, 0, 5.15e-08, 1.04e-07)}, 2: {'theta': (1.07e-07, 0, 4.81e-08, 1.01e-07), 'm': (5.61e-08, 0, 7.23e-08, 3.19e-08), 'v': (1.33e-07, 0, 7.68e-08, 6.05e-08)}, 10: {'theta': (3.65e-07, 0, 1.59e-07, 3.11e-07), 'm': (7.44e-08, 0, 2.8e-08, 7.61e-08), 'v': (2.67e-07, 0, 1.56e-07, 1.61e-07)}},
    'enc16x16-gru16-head-frozen': {1: {'theta': (7.32e-08, 7.12e-08, 0, 6.88e-08), 'm': (1.7e-07, 1.22e-07, 0, 1.48e-07), 'v': (3.53e-07, 2.17e-07, 0, 2.49e-07)}, 2: {'theta': (1.35e-07, 1.26e-07, 0, 1.29e-07), 'm': (1.44e-07, 1.45e-07, 0, 1.03e-07), 'v': (2.96e-07, 1.96e-07, 0, 2.24e-07)}, 10: {'theta': (4.14e-07, 3.07e-07, 0, 3.97e-07), 'm': (1.36e-07, 1.09e-07, 0, 1.04e-07), 'v': (3.69e-07, 1.19e-07, 0, 3.74e-07)}},
    'enc16x16-gru16-head-logstd': {1: {'theta': (7.11e-08, 6.79e-08, 2.21e-08, 6.83e-08), 'm': (3.58e-08, 1.2e-08, 2.54e-08, 3.63e-08), 'v': (9.05e-08, 4.05e-08, 8.51e-08, 1.2e-07)}, 2: {'theta': (1.3e-07, 1.08e-07, 3.09e-08, 1.25e-07), 'm': (6.98e-08, 4.42e-08, 2.52e-08, 5.77e-08), 'v': (9.95e-08, 2.7e-08, 1.2e-07, 9.78e-08)}, 10: {'theta': (5.7e-07, 4.74e-07, 1.76e-07, 5.12e-07), 'm': (8.48e-08, 7.22e-08, 1.13e-07, 8.42e-08), 'v': (1.47e-07, 7.23e-08, 2.04e-07, 1.88e-07)}},
    'enc128x128-gru16-head-logstd': {1: {'theta': (2.99e-08, 2.39e-08, 2.93e-08, 5.72e-08), 'm': (4.7e-07, 3.72e-07, 4.49e-07, 4.62e-07), 'v': (8.94e-07, 8.37e-07, 8.78e-07, 9.36e-07)}, 2: {'theta': (5.85e-08, 4.05e-08, 5.72e-08, 9.51e-08), 'm': (3.93e-07, 3.32e-07, 5.42e-07, 4.69e-07), 'v': (8.29e-07, 8.43e-07, 9.36e-07, 9.15e-07)}, 10: {'theta': (2.26e-07, 1.62e-07, 2.47e-08, 2.19e-07), 'm': (5.07e-07, 5.52e-07, 5.52e-07, 5.26e-07), 'v': (1.02e-06, 1.05e-06, 9.96e-07, 9.97e-07)}},
}


def bound(name, steps, what, group):
    """optim_ref.bound's rule: FACTOR x torch fp32's committed error, and never below steps x 2^-24 -- one rounding of the value per step"""
    return max(FACTOR * BASELINE[name][steps][what][group], steps * 2.0 ** -24)


if __name__ == "__main__":
    import torch
    print("BASELINE = {")
    for c in CASES:
        errs, _ = torch_errors(c, torch.float32)
        print("    %r: {%s}," % (c.name, ", ".join("%d: {%s}" % (k, ", ".join("%r: (%s)" % (w, ", ".join("%.3g" % e for e in es))
                                                                            for w, es in errs[k].items())) for k in errs)))
    print("}")
