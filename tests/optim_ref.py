"""The reference of the optimiser on the device (gaq.h "the optimiser on the device"): an fp64 NumPy restatement of one Adam / AdamW
step on fp32 inputs with global-norm clipping, decoupled weight decay and the skip rule, the eight cases the CPU and GPU tests share
(the smallest shapes at which the chunking of the concatenated groups can go wrong), their seeded synthetic gradients, and the
committed table of torch fp32's error against the reference (CPU, foreach=False) from which the device's bounds are taken.

With t = steps taken + 1 and g' = coef g, coef = min(1, max_grad_norm / (norm + 1e-6)) (1 without clipping), norm the L2 norm over
all groups:  m = m + (1 - b1)(g' - m),  v = b2 v + (1 - b2) g'^2,
theta = theta (1 - lr wd) - [lr / (1 - b1^t)] m / (sqrt(v) / sqrt(1 - b2^t) + eps); wd never applies to log_std.  A squared norm that
is not finite skips the step: nothing changes but the skipped counter.

python -m tests.optim_ref prints BASELINE."""
import numpy as np

FACTOR = 8.0
STEPS = 10
AT = (1, 2, STEPS)          # the step counts at which theta, m and v are compared (2: what the skip test reaches)
GROUPS = ("weights", "value_head", "log_std")


class Case:
    """kind: "mlp" (engine mfma or valu), "critic", "gru", "lstm"; widths: the hidden widths (a cell's H first); D the observation
    width; head / log_std: whether the handle has a value head / explores; hp: lr, betas, eps, weight_decay, max_grad_norm"""

    def __init__(self, name, kind, widths, D=18, engine="mfma", head=False, log_std=True, lr=3e-4, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, max_grad_norm=None, clip=None):
        self.name, self.kind, self.widths, self.D, self.engine = name, kind, list(widths), D, engine
        self.head, self.log_std = head, log_std
        self.hp = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self.clip = clip                # "above": every step's norm is far above max_grad_norm; "below": far below; None: not stated

    @property
    def weight_count(self):
        w, D = self.widths, self.D
        if self.kind in ("gru", "lstm"):
            G, H = (3 if self.kind == "gru" else 4), w[0]
            n, prev, rest = G * H * (D + H) + 2 * G * H, H, w[1:]
        else:
            n, prev, rest = 0, D, w
        for x in rest:
            n += x * prev + x
            prev = x
        n_out = 1 if self.kind == "critic" else 4
        return n + n_out * prev + n_out

    @property
    def sizes(self):
        """floats of each group: weights, value head, log_std (0: the group is absent)"""
        return (self.weight_count, self.widths[-1] + 1 if self.head else 0, 4 if self.log_std else 0)


CASES = [
    Case("mlp16-head-logstd", "mlp", [16], head=True, max_grad_norm=0.5, clip="above"),          # 372 + 17 + 4
    Case("mlp48x80x32", "mlp", [48, 80, 32], lr=1e-3, weight_decay=1e-2, max_grad_norm=1e4, clip="below"),
    Case("mlp128x128x128", "mlp", [128, 128, 128], head=True, max_grad_norm=40.0),                # 35 972 + 129 + 4
    Case("valu64x64-d19", "mlp", [64, 64], D=19, engine="valu", weight_decay=1e-2),
    Case("critic16", "critic", [16], log_std=False, lr=1e-3, betas=(0.8, 0.99), max_grad_norm=0.5),   # 321
    Case("gru16", "gru", [16], max_grad_norm=10.0),
    Case("gru64x64x64-head", "gru", [64, 64, 64], head=True, eps=1e-5, weight_decay=0.1, max_grad_norm=0.5),
    Case("lstm16", "lstm", [16], log_std=False),
]
BY_NAME = {c.name: c for c in CASES}
_SEED = {c.name: 1000 + 17 * k for k, c in enumerate(CASES)}


def theta0(case):
    """the initial parameters, one fp32 array per group (empty: absent): weights and head uniform in +-0.5, log_std around -0.5"""
    rng = np.random.RandomState(_SEED[case.name])
    nw, nh, nl = case.sizes
    return [rng.uniform(-0.5, 0.5, nw).astype(np.float32), rng.uniform(-0.5, 0.5, nh).astype(np.float32),
            (-0.5 + rng.uniform(-0.2, 0.2, nl)).astype(np.float32)]


def gradients(case, step):
    """the synthetic gradients of step `step` (0-based), one fp32 array per group: magnitudes log-uniform over [1e-6, 10], random
    signs, about 5 % exact zeros"""
    rng = np.random.RandomState(_SEED[case.name] + 7919 * (step + 1))
    out = []
    for n in case.sizes:
        g = 10.0 ** rng.uniform(-6.0, 1.0, n) * rng.choice([-1.0, 1.0], n)
        g[rng.uniform(size=n) < 0.05] = 0.0
        out.append(g.astype(np.float32))
    return out


class State:
    """theta, m, v per group in fp64, the step count and the skipped count"""

    def __init__(self, theta):
        self.theta = [np.asarray(t, dtype=np.float64).copy() for t in theta]
        self.m = [np.zeros_like(t) for t in self.theta]
        self.v = [np.zeros_like(t) for t in self.theta]
        self.t, self.skipped = 0, 0


def step(state, grads, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
    """one step in place; returns the four statistics the device writes: (norm, coef, step count after the call, skipped)"""
    g = [np.asarray(x, dtype=np.float32).astype(np.float64) for x in grads]
    with np.errstate(over="ignore", invalid="ignore"):
        sumsq = float(sum(np.sum(x * x) for x in g))
        norm = float(np.sqrt(sumsq))
    if not np.isfinite(sumsq):
        state.skipped += 1
        return norm, 0.0, float(state.t), 1.0
    coef = 1.0 if not max_grad_norm else min(1.0, float(max_grad_norm) / (norm + 1e-6))
    b1, b2 = betas
    state.t += 1
    t = state.t
    step_size, bc2s = lr / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t)
    for k, x in enumerate(g):
        x = coef * x
        state.m[k] += (1.0 - b1) * (x - state.m[k])
        state.v[k] = b2 * state.v[k] + (1.0 - b2) * x * x
        decay = 1.0 if GROUPS[k] == "log_std" else 1.0 - lr * weight_decay
        state.theta[k] = state.theta[k] * decay - step_size * state.m[k] / (np.sqrt(state.v[k]) / bc2s + eps)
    return norm, coef, float(t), 0.0


def rel(got, want):
    """max|got - want| / max|want| (0 for empty arrays)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    scale = float(np.abs(want).max())
    return float(np.abs(got - want).max()) / (scale if scale > 0 else 1.0)


def trajectory(case, steps=STEPS):
    """the reference after each of `steps` steps: [(theta, m, v copies, stats), ...]"""
    st, out = State(theta0(case)), []
    for k in range(steps):
        stats = step(st, gradients(case, k), **case.hp)
        out.append(([x.copy() for x in st.theta], [x.copy() for x in st.m], [x.copy() for x in st.v], stats))
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
        groups = [{"params": [p for p in params[:2] if p.numel()], "weight_decay": wd}]
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
        errs[k] = {what: tuple(rel(a, b) for a, b in zip(got[k - 1][i], ref[k - 1][i])) for i, what in enumerate(("theta", "m", "v"))}
    scal = max(max(rel(g[3][0], r[3][0]), rel(g[3][1], r[3][1])) for g, r in zip(got, ref))
    return errs, scal


# per case: after 1, 2 and 10 steps, torch fp32's error (CPU, foreach=False) against the reference for theta, m and v of each
# group -- weights, value head, log_std; 0 for an absent group (python -m tests.optim_ref)
BASELINE = {
    'mlp16-head-logstd': {1: {'theta': (2.98e-08, 2.07e-08, 3.38e-08), 'm': (6.42e-08, 3.31e-08, 1.51e-08), 'v': (1.32e-07, 7.28e-08, 4.59e-08)}, 2: {'theta': (5.41e-08, 3.85e-08, 7.56e-08), 'm': (1.08e-07, 7.31e-08, 1.09e-07), 'v': (1.3e-07, 1.56e-07, 1.49e-07)}, 10: {'theta': (1.57e-07, 1e-07, 2.33e-07), 'm': (1.19e-07, 6.45e-08, 1.41e-07), 'v': (2.72e-07, 1.22e-07, 2.16e-07)}},
    'mlp48x80x32': {1: {'theta': (7.18e-08, 0, 2.03e-08), 'm': (3.59e-08, 0, 1.49e-08), 'v': (1.14e-07, 0, 5.1e-08)}, 2: {'theta': (1.31e-07, 0, 5.89e-08), 'm': (5.47e-08, 0, 3.07e-08), 'v': (1.13e-07, 0, 4.39e-08)}, 10: {'theta': (3.79e-07, 0, 3.94e-08), 'm': (9.46e-08, 0, 7.31e-08), 'v': (2e-07, 0, 1.76e-07)}},
    'mlp128x128x128': {1: {'theta': (4.01e-08, 2.96e-08, 2.36e-08), 'm': (1.13e-06, 1.13e-06, 1.16e-06), 'v': (2.27e-06, 2.23e-06, 2.26e-06)}, 2: {'theta': (9.49e-08, 5.57e-08, 3.41e-08), 'm': (9.85e-07, 9.12e-07, 8.32e-07), 'v': (1.94e-06, 1.85e-06, 1.74e-06)}, 10: {'theta': (2.37e-07, 1.55e-07, 1.74e-07), 'm': (9.6e-07, 9.56e-07, 9.23e-07), 'v': (2.15e-06, 2.13e-06, 1.88e-06)}},
    'valu64x64-d19': {1: {'theta': (7.52e-08, 0, 4.89e-08), 'm': (3.61e-08, 0, 6.01e-08), 'v': (1.26e-07, 0, 8.19e-08)}, 2: {'theta': (1.35e-07, 0, 8.94e-08), 'm': (5.24e-08, 0, 4.14e-08), 'v': (9.06e-08, 0, 3.87e-08)}, 10: {'theta': (6.36e-07, 0, 1.17e-07), 'm': (8.31e-08, 0, 5.65e-08), 'v': (2.03e-07, 0, 1.75e-07)}},
    'critic16': {1: {'theta': (2.99e-08, 0, 0), 'm': (9.6e-08, 0, 0), 'v': (2.5e-07, 0, 0)}, 2: {'theta': (5.42e-08, 0, 0), 'm': (1.77e-07, 0, 0), 'v': (2.32e-07, 0, 0)}, 10: {'theta': (1.31e-07, 0, 0), 'm': (8.26e-08, 0, 0), 'v': (1.04e-07, 0, 0)}},
    'gru16': {1: {'theta': (2.98e-08, 0, 4.17e-08), 'm': (2.81e-07, 0, 2.33e-07), 'v': (5.63e-07, 0, 4.58e-07)}, 2: {'theta': (5.71e-08, 0, 7.74e-08), 'm': (1.48e-07, 0, 2.57e-07), 'v': (3.23e-07, 0, 4.92e-07)}, 10: {'theta': (1.89e-07, 0, 1.71e-07), 'm': (1.66e-07, 0, 9.24e-08), 'v': (4.5e-07, 0, 3.04e-07)}},
    'gru64x64x64-head': {1: {'theta': (7.77e-08, 6.34e-08, 2.9e-08), 'm': (8.55e-07, 8.1e-07, 8.11e-07), 'v': (1.73e-06, 1.75e-06, 1.75e-06)}, 2: {'theta': (1.46e-07, 1.24e-07, 4.77e-08), 'm': (6.91e-07, 7.69e-07, 7.94e-07), 'v': (1.46e-06, 1.49e-06, 1.72e-06)}, 10: {'theta': (4.84e-07, 3.25e-07, 3.35e-08), 'm': (7.64e-07, 8.43e-07, 6.43e-07), 'v': (1.48e-06, 1.95e-06, 1.36e-06)}},
    'lstm16': {1: {'theta': (2.98e-08, 0, 0), 'm': (3.59e-08, 0, 0), 'v': (9.87e-08, 0, 0)}, 2: {'theta': (5.63e-08, 0, 0), 'm': (4.58e-08, 0, 0), 'v': (9.97e-08, 0, 0)}, 10: {'theta': (1.71e-07, 0, 0), 'm': (6.88e-08, 0, 0), 'v': (1.44e-07, 0, 0)}},
}


def bound(name, steps, what, group):
    """The device's bound for theta / m / v of one group after `steps` steps: FACTOR x torch fp32's committed error, and never below
    steps x 2^-24 -- one rounding of the value per step"""
    return max(FACTOR * BASELINE[name][steps][what][group], steps * 2.0 ** -24)


if __name__ == "__main__":
    import torch
    print("BASELINE = {")
    for c in CASES:
        errs, _ = torch_errors(c, torch.float32)
        print("    %r: {%s}," % (c.name, ", ".join("%d: {%s}" % (k, ", ".join("%r: (%s)" % (w, ", ".join("%.3g" % e for e in es))
                                                                            for w, es in errs[k].items())) for k in errs)))
    print("}")
