"""The edge-shape inputs of the two V-trace kernels (gaq.h gaq_vtrace_dev, gaq_vtrace_term_dev), an fp32 emulation of the kernels on the
CPU, and the checks both tests/test_vtrace_cpu.py (on the emulation) and tests/test_gpu_vtrace.py (on the device) run on a result.

The inputs are those of tests/gae_emul.py -- its BATCHES, STEPS, DENSITIES, SCALES and DONE_BYTES, its own draws of rew, done, values and
term (NaN where done is clear), so its SEEDS hold here as they stand: the p = 0.1, T >= 5 inputs of every N > 1 hold a done at t = 0, one
at t = T - 1 and two in a row -- with the two log-probabilities drawn from a second stream: logp_behaviour = -4 + 2 randn and
logp_target = logp_behaviour + x, x = 0.3 randn with 2 % of the entries +20, 2 % -20 and 1 % +100 (there expf overflows to inf, and the
clip must still give the bar).

The emulation evaluates the kernels' own expressions in their order, as gae_emul.emulate does: each fma is the fp32 rounding of the fp64
result, numpy's float32 exp stands in for expf, the scalars are rounded to fp32 as the C interface takes them.  It exists to show WITHOUT
a GPU that the inputs are fair to a correct fp32 kernel -- the error stays within the running bars of tests/vtrace_ref.py -- and that the
bars catch a wrong one (the VARIANTS)."""
import numpy as np

from tests import gae_emul as G
from tests import vtrace_ref as R

BATCHES, STEPS, DENSITIES, SCALES, DONE_BYTES, SEEDS = G.BATCHES, G.STEPS, G.DENSITIES, G.SCALES, G.DONE_BYTES, G.SEEDS
# (gamma, lambda, rho_bar, c_bar, pg_rho_bar)
PARAMS = [(0.99, 1.0, 1.0, 1.0, 1.0), (0.99, 0.95, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0, 1.0), (0.99, 1.0, 2.0, 1.5, 3.0),
          (0.5, 0.5, 1.0, 1.0, 1.0), (0.0, 1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1e9, 1.0, 1.0)]
VARIANTS = ["no_cut", "term_mul", "clip_after", "vs_in_td", "pg_rho", "drop_tail"]
rich_dones = G.rich_dones


def inputs(n):
    """gae_emul.inputs(n) with logp_b and logp_t [T, n] f32 added to every dict"""
    rng = np.random.RandomState(7919 + SEEDS[n])
    out = []
    for inp in G.inputs(n):
        shape = inp["rew"].shape
        lb = (-4.0 + 2.0 * rng.randn(*shape)).astype(np.float32)
        x, u = 0.3 * rng.randn(*shape), rng.rand(*shape)
        x = np.where(u < 0.02, 20.0, np.where(u < 0.04, -20.0, np.where(u < 0.05, 100.0, x)))
        out.append(dict(inp, logp_b=lb, logp_t=(lb + x.astype(np.float32)).astype(np.float32)))
    return out


def with_inf(inp):
    """the input with +inf instead of NaN where done is clear"""
    return dict(inp, term=np.where(inp["done"] != 0, inp["term"], np.inf).astype(np.float32))


def on_policy(inp):
    """the input with logp_target the bits of logp_behaviour"""
    return dict(inp, logp_t=inp["logp_b"].copy())


_fma = G._fma


def emulate(inp, params, term=False, variant=None):
    """(vs, pg) [T, n] f32 as vtrace_kernel (term=False) or vtrace_term_kernel (term=True) compute them.  variant: None, or one of
    VARIANTS -- "no_cut": the acc chain is not cut at a done; "term_mul": term is multiplied by the done mask instead of selected;
    "clip_after": the ratio is clipped after the product with td, fminf(rho_bar, w td); "vs_in_td": vs[t+1] stands where V[t+1] belongs in
    td; "pg_rho": rho_bar clips pg_adv's ratio where pg_rho_bar belongs; "drop_tail": the T % 4 rows that the unrolled loop leaves over (the
    first ones of the rollout) are not run, their outputs stay 0."""
    f = np.float32
    g, lam, rho_bar, c_bar, pg_bar = (f(v) for v in params)
    rew, values, lb, lt = inp["rew"], inp["values"], inp["logp_b"], inp["logp_t"]
    d = inp["done"] != 0
    T = rew.shape[0]
    zero = f(0.0)
    tv = inp["term"] if term else np.zeros_like(rew)
    vs_out, pg_out = np.zeros_like(rew), np.zeros_like(rew)
    acc, vn, vsn = np.zeros(rew.shape[1], f), values[T], values[T]
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, (T % 4 if variant == "drop_tail" else 0) - 1, -1):
            r, v = rew[t], values[t]
            x = (lt[t] - lb[t]).astype(f)
            w = np.exp(x).astype(f)
            rho = np.minimum(rho_bar, w)
            c = (lam * np.minimum(c_bar, w)).astype(f)
            if term and variant == "term_mul":
                m = d[t].astype(f)
                nv = (m * tv[t] + (f(1.0) - m) * vn).astype(f)
                nvs = (m * tv[t] + (f(1.0) - m) * vsn).astype(f)
            else:
                nv, nvs = np.where(d[t], tv[t], vn), np.where(d[t], tv[t], vsn)
            td = (_fma(g, nvs if variant == "vs_in_td" else nv, r) - v).astype(f)
            rtd = np.minimum(rho_bar, (w * td).astype(f)) if variant == "clip_after" else (rho * td).astype(f)
            k = (g * c).astype(f)
            acc = _fma(k if variant == "no_cut" else np.where(d[t], zero, k), acc, rtd)
            vs = (v + acc).astype(f)
            vs_out[t] = vs
            pg_out[t] = (np.minimum(rho_bar if variant == "pg_rho" else pg_bar, w) * (_fma(g, nvs, r) - v).astype(f)).astype(f)
            vn, vsn = v, vs
    return vs_out, pg_out


def reference(inp, params, term=False):
    """(ref, bar_vs, bar_pg): vtrace_ref.vtrace64's dict and vtrace_ref.vtrace_bars of it"""
    ref = R.vtrace64(inp["rew"], inp["done"], inp["values"], inp["logp_b"], inp["logp_t"], *params, term=inp["term"] if term else None)
    return (ref,) + R.vtrace_bars(ref)


def error_over_bar(got, want, bar):
    """the worst |got - want| / bar over every element; inf if any element is not finite or misses a finite comparison"""
    err = np.abs(np.asarray(got, np.float64) - want) / bar
    return float(err.max()) if np.isfinite(err).all() else float("inf")


def check(inp, params, term, vs, pg, ref, bar_vs, bar_pg):
    """everything a correct result holds; returns the worst error / bar of (vs, pg).  No element is excluded from any comparison."""
    what = "T=%d p=%g scale=%g params=%s term=%d" % (inp["T"], inp["p"], inp["scale"], params, term)
    cut = inp["done"] != 0
    for a in (ref["vs"], ref["pg"], bar_vs, bar_pg):
        assert np.isfinite(a).all(), what
    assert (bar_vs > 0).all() and (bar_pg >= 0).all(), what
    assert np.isfinite(vs).all() and np.isfinite(pg).all(), what
    fv, fp = error_over_bar(vs, ref["vs"], bar_vs), error_over_bar(pg, ref["pg"], np.maximum(bar_pg, np.finfo(np.float64).tiny))
    assert fv <= 1.0 and fp <= 1.0, (what, fv, fp)
    if inp["p"] == 0.0:
        assert not cut.any(), what
    if inp["p"] == 1.0:
        assert cut.all(), what
    return fv, fp


def teeth(ref, bar_vs):
    """the median over the elements of |acc_ref| / bar_vs: how far the quantity the scan carries stands above its bar"""
    return float(np.median(np.abs(ref["acc"]) / bar_vs))
