"""fp64 reference of the V-trace targets (gaq.h gaq_vtrace_dev, gaq_vtrace_term_dev) on the fp32 inputs, and the error bars the tests hold
an fp32 evaluation to, derived from the number formats.

Semantics, one env, t descending, vs_T = V_T, acc_T = 0, d = done[t] != 0 (term form: 0 -> term[t] in V' and vs'):
    x = logp_target[t] - logp_behaviour[t];  w = exp(x);  rho = min(rho_bar, w);  c = lambda min(c_bar, w);  rho_pg = min(pg_rho_bar, w)
    V' = d ? 0 : V[t+1];  vs' = d ? 0 : vs[t+1];  td = r[t] + gamma V' - V[t];  k = d ? 0 : gamma c
    acc[t] = rho td + k acc[t+1];  vs[t] = V[t] + acc[t];  pg[t] = rho_pg (r[t] + gamma vs' - V[t])
gamma, lambda and the three clips are rounded to fp32 first, as the C interface takes them; everything else is exact in the inputs.

The bars (vtrace_bars).  u = 2^-24 is half an ulp of an fp32 value, relative; E = 2 is the error of expf in ulps (ROCm documents its
expf at 1 ulp; the margin is for that bound), i.e. 2 E u relative.  The device computes, in this order,
    x~ = fl(x): relative error u, which moves w by |x| u relative;  w~ = expf(x~): 2 E u more;  so rho~, min(c_bar, w~) and rho_pg~ are
         off by at most (|x| + 2 E) u relative (by nothing where the clip is active: the bound is kept);
    td~ = fl(fl(gamma V' + r) - V): two roundings of quantities no larger than m = |r| + gamma |V'| + |V|, so 2 u m;
    fl(rho~ td~): one more rounding, so rho td is off by at most rho (|x| + 2 E + 3) u m;
    k~ = fl(gamma fl(lambda min(c_bar, w~))): (|x| + 2 E + 2) u relative, which moves k acc[t+1] by k (|x| + 2 E + 2) u |acc[t+1]|;
    acc~[t] = fl(k~ acc~[t+1] + fl(rho~ td~)): one rounding, u |acc[t]|, and the error b[t+1] of acc~[t+1] arrives multiplied by k.
Hence the RUNNING bound, computed by the same backward scan as the reference (b[T] = 0):
    b[t] = k b[t+1] + u (rho (|x| + 2 E + 3) m + k (|x| + 2 E + 2) |acc[t+1]| + |acc[t]|)
    bar_vs[t] = b[t] + u |vs[t]|                                           (the rounding of V + acc)
    bar_pg[t] = rho_pg (gamma bar_vs'[t] + u (|x| + 2 E + 3) m'),  m' = |r| + gamma |vs'| + |V|,  bar_vs' = d ? 0 : bar_vs[t+1] (0 at t = T - 1:
                vs_T = V_T and a term entry are inputs) -- the same three roundings and the ratio's error on the pg expression.
These are first-order bounds; both are multiplied by 2 for the second-order terms.  A per-env max T / (1 - c) bound in the manner of
ac_ref.gae_bar loses its teeth as soon as c_bar > 1 or rho_bar is large, which is why the bound runs with the scan."""
import numpy as np

U24 = 2.0 ** -24
EXPF_ULPS = 2.0                  # E
SECOND_ORDER = 2.0


def _f32(v):
    return float(np.float32(v))


def vtrace64(rew, done, values, logp_b, logp_t, gamma, lam, rho_bar, c_bar, pg_rho_bar, term=None):
    """rew, done, logp_b, logp_t (and term) [T, N], values [T + 1, N] (the fp32 inputs) -> dict of float64 [T, N] arrays: vs, pg, acc and
    what the bars need (x, rho, rho_pg, k, m, m_pg, accn = acc[t+1], cut = d or t == T - 1)"""
    rew, values, lb, lt = (np.asarray(a, np.float64) for a in (rew, values, logp_b, logp_t))
    d = np.asarray(done) != 0
    g, lam, rho_bar, c_bar, pg_rho_bar = (_f32(v) for v in (gamma, lam, rho_bar, c_bar, pg_rho_bar))
    T = rew.shape[0]
    tv = np.zeros_like(rew) if term is None else np.where(d, np.asarray(term, np.float64), 0.0)
    x = lt - lb
    with np.errstate(over="ignore"):
        w = np.exp(x)
    rho, rho_pg = np.minimum(rho_bar, w), np.minimum(pg_rho_bar, w)
    k = np.where(d, 0.0, g * lam * np.minimum(c_bar, w))
    out = {key: np.zeros_like(rew) for key in ("vs", "pg", "acc", "accn", "m", "m_pg")}
    out.update(x=x, rho=rho, rho_pg=rho_pg, k=k, cut=d.copy())
    out["cut"][T - 1] = True
    acc, vsn = np.zeros(rew.shape[1:]), values[T]
    for t in range(T - 1, -1, -1):
        vn = np.where(d[t], tv[t], values[t + 1])
        vsn = np.where(d[t], tv[t], vsn)
        out["accn"][t] = acc
        acc = rho[t] * (rew[t] + g * vn - values[t]) + k[t] * acc
        out["acc"][t], out["vs"][t] = acc, values[t] + acc
        out["pg"][t] = rho_pg[t] * (rew[t] + g * vsn - values[t])
        out["m"][t] = np.abs(rew[t]) + g * np.abs(vn) + np.abs(values[t])
        out["m_pg"][t] = np.abs(rew[t]) + g * np.abs(vsn) + np.abs(values[t])
        vsn = out["vs"][t]
    out["gamma"] = g
    return out


def vtrace_bars(ref):
    """(bar_vs, bar_pg) [T, N] from vtrace64's dict: the running bound of the module docstring, times SECOND_ORDER"""
    T = ref["vs"].shape[0]
    ax = np.abs(ref["x"]) + 2.0 * EXPF_ULPS
    bar_vs, bar_pg = np.zeros_like(ref["vs"]), np.zeros_like(ref["vs"])
    b = np.zeros(ref["vs"].shape[1:])
    for t in range(T - 1, -1, -1):
        nxt = np.where(ref["cut"][t], 0.0, bar_vs[t + 1] if t + 1 < T else 0.0)
        bar_pg[t] = ref["rho_pg"][t] * (ref["gamma"] * nxt + U24 * (ax[t] + 3.0) * ref["m_pg"][t])
        b = ref["k"][t] * b + U24 * (ref["rho"][t] * (ax[t] + 3.0) * ref["m"][t] + ref["k"][t] * (ax[t] + 2.0) * np.abs(ref["accn"][t])
                                     + np.abs(ref["acc"][t]))
        bar_vs[t] = b + U24 * np.abs(ref["vs"][t])
    return SECOND_ORDER * bar_vs, SECOND_ORDER * bar_pg
