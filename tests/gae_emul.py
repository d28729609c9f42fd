"""The edge-shape inputs of the two GAE kernels (gaq.h gaq_gae_dev, gaq_gae_term_dev), an fp32 emulation of the kernels on the CPU, and
the checks both tests/test_gae_edges_cpu.py (on the emulation) and tests/test_gpu_gae_edges.py (on the device) run on a result.

The emulation evaluates the kernels' own expressions in their order: each fma is the fp32 rounding of the fp64 result (the product of two
fp32 numbers is exact in fp64), gamma and lambda are rounded to fp32 as the C interface takes them and gamma * lambda is the fp32 product
the host code hands to the kernel.  It exists to show WITHOUT a GPU that the inputs are fair to a correct fp32 kernel -- the error stays
within the derived bars of tests/ac_ref.py and tests/term_ref.py -- and that the bars catch a wrong one (the VARIANTS)."""
import numpy as np

from tests import ac_ref, term_ref

BATCHES = [1, 63, 255, 256, 257, 2096]           # the kernels' block is 256 threads
STEPS = [1, 2, 3, 4, 5, 7, 9, 65]                # the t loop is unrolled by 4
DENSITIES = [0.0, 0.1, 0.5, 1.0]
SCALES = [1.0, 100.0]
GAMMA_LAMBDA = [(0.99, 0.95), (0.99, 0.0), (0.99, 1.0), (1.0, 0.95), (1.0, 1.0), (0.0, 0.5), (0.5, 0.5)]
DONE_BYTES = np.array([1, 2, 255], np.uint8)
# per N, the seed of its draws: the smallest one with which every p = 0.1, T >= 5 input holds a done at t = 0, one at t = T - 1 and two
# in a row (rich_dones), and every case has teeth (check).  One env cannot hold all of that at p = 0.1, so N = 1 takes seed 0 as it is
# and is exempt from rich_dones
SEEDS = {1: 0, 63: 1,255: 0, 256: 0, 257: 0, 2096: 0}
VARIANTS = ["no_cut", "term_mul", "drop_tail"]


def inputs(n):
    """the inputs of batch size n, in a fixed order: dicts of T, p, scale, rew [T, n] f32, done [T, n] u8 (set bytes from DONE_BYTES),
    values [T + 1, n] f32 and term [T, n] f32 (a finite draw where done is set, NaN where it is clear)"""
    rng = np.random.RandomState(SEEDS[n])
    out = []
    for T in STEPS:
        for p in DENSITIES:
            for scale in SCALES:
                d = rng.rand(T, n) < p
                done = np.where(d, DONE_BYTES[rng.randint(0, 3, size=(T, n))], 0).astype(np.uint8)
                rew = (scale * rng.randn(T, n)).astype(np.float32)
                values = (3.0 * scale * rng.randn(T + 1, n)).astype(np.float32)
                term = np.where(d, 3.0 * scale * rng.randn(T, n), np.nan).astype(np.float32)
                out.append(dict(T=T, p=p, scale=scale, rew=rew, done=done, values=values, term=term))
    return out


def with_inf(inp):
    """the input with +inf instead of NaN where done is clear"""
    return dict(inp, term=np.where(inp["done"] != 0, inp["term"], np.inf).astype(np.float32))


def rich_dones(done):
    """some env has a done at t = 0, some has one at t = T - 1, some has two in a row"""
    d = done != 0
    return bool(d[0].any() and d[-1].any() and (d[1:] & d[:-1]).any())


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emulate(inp, gamma, lam, term=False, variant=None):
    """(adv, ret) [T, n] f32 as gae_kernel (term=False) or gae_term_kernel (term=True) compute them.  variant: None, or one of VARIANTS --
    "no_cut": the advantage chain is not cut at a done; "term_mul": term is multiplied by the done mask instead of selected;
    "drop_tail": the T % 4 steps that the unrolled loop leaves over (the first ones of the rollout) are not run, their outputs stay 0."""
    rew, values, tv = inp["rew"], inp["values"], inp["term"]
    d = inp["done"] != 0
    T = rew.shape[0]
    g = np.float32(gamma)
    gl = np.float32(g * np.float32(lam))
    zero = np.float32(0.0)
    adv, ret = np.zeros_like(rew), np.zeros_like(rew)
    a, vn = np.zeros(rew.shape[1], np.float32), values[T]
    with np.errstate(invalid="ignore"):
        for t in range(T - 1, (T % 4 if variant == "drop_tail" else 0) - 1, -1):
            r, v = rew[t], values[t]
            if not term:
                s = _fma(np.where(d[t], zero, g), vn, r)
            elif variant == "term_mul":
                m = d[t].astype(np.float32)
                s = _fma(g, (m * tv[t] + (np.float32(1.0) - m) * vn).astype(np.float32), r)
            else:
                s = _fma(g, np.where(d[t], tv[t], vn), r)
            delta = (s - v).astype(np.float32)
            a = _fma(gl if variant == "no_cut" else np.where(d[t], zero, gl), a, delta)
            adv[t], ret[t] = a, (a + v).astype(np.float32)
            vn = v
    return adv, ret


def reference(inp, gamma, lam, term=False):
    """(adv_ref [T, n] f64, bar [n]) from ac_ref.gae64 / gae_bar, or term_ref.gae_term64 / gae_term_bar"""
    if term:
        aref, _ = term_ref.gae_term64(inp["rew"], inp["done"], inp["values"], inp["term"], gamma, lam)
        return aref, term_ref.gae_term_bar(inp["rew"], inp["done"], inp["values"], inp["term"], aref, gamma, lam)
    aref, _ = ac_ref.gae64(inp["rew"], inp["done"], inp["values"], gamma, lam)
    return aref, ac_ref.gae_bar(inp["rew"], inp["values"], aref, gamma, lam)


def error_over_bar(adv, aref, bar):
    """the worst |adv - adv_ref| / bar over every element; inf if any element is not finite or misses a finite comparison"""
    err = np.abs(np.asarray(adv, np.float64) - aref) / bar[None]
    return float(err.max()) if np.isfinite(err).all() else float("inf")


def check(inp, gamma, lam, term, adv, ret, aref, bar):
    """everything a correct result holds; returns the worst error / bar.  No element is excluded from any comparison."""
    what = "T=%d p=%g scale=%g gamma=%g lam=%g term=%d" % (inp["T"], inp["p"], inp["scale"], gamma, lam, term)
    rew, values = inp["rew"], inp["values"]
    T = rew.shape[0]
    cut = inp["done"] != 0
    assert np.isfinite(aref).all() and np.isfinite(bar).all(), what
    assert np.isfinite(adv).all() and np.isfinite(ret).all(), what
    frac = error_over_bar(adv, aref, bar)
    assert frac <= 1.0, (what, frac)
    # teeth: the advantages are far above the bar
    assert float(np.abs(aref).max()) > 100.0 * float(bar.max()), (what, float(np.abs(aref).max()), float(bar.max()))
    # ret - adv == values[:T] within one ulp
    a64, v64 = np.asarray(adv, np.float64), values[:T].astype(np.float64)
    ulp_r = np.spacing(np.maximum(np.abs(ret), np.abs(values[:T])).astype(np.float32)).astype(np.float64)
    assert (np.abs(ret.astype(np.float64) - a64 - v64) <= ulp_r).all(), what
    if not term:
        # a done row cuts: adv = r - V within one fp32 ulp of it
        want = rew.astype(np.float64) - v64
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(a64 - want)[cut] <= ulp[cut]).all(), what
    if inp["p"] == 0.0:
        assert not cut.any(), what
    if inp["p"] == 1.0:
        assert cut.all(), what
    return frac
