"""vtrace_kernel and vtrace_term_kernel (gaq.h gaq_vtrace_dev, gaq_vtrace_term_dev; QuadrotorEnv.vtrace_dev) on the device.

1. Edge shapes: the inputs of tests/vtrace_emul.py -- gae_emul's T of 1..65 (the t loop is unrolled by 4), N of 1..2096 (the block is 256
   threads), done densities, done bytes and scales, NaN in every unused term entry (+inf once), log-probability differences with +20,
   -20 and +100 (expf overflows) among them -- times the seven (gamma, lambda, rho_bar, c_bar, pg_rho_bar) tuples times both forms,
   against the fp64 reference at the running bars of tests/vtrace_ref.py, no element excluded; the call with pg_adv=None gives the same
   vs bits.  tests/test_vtrace_cpu.py shows without a GPU that these inputs are fair (the emulation's worst error / bar is 0.479 on vs,
   0.341 on pg_adv) and that the bars catch six wrong kernels.
2. The on-policy anchor: logp_target the bits of logp_behaviour and clips >= 1 -> vs is gae_dev's ret bit for bit, both forms, every
   (gamma, lambda) of gae_emul.GAMMA_LAMBDA.
3. The ratio itself: gamma = 0, V = 0, r = 1 make vs rho and pg_adv rho_pg.  Where exp(x) > the bar the result is the bar's bits (the
   overflow entries among them); elsewhere it is compared with fp64 exp in ulps of the result, bound E + |x| 2^-24 / ulp (E = 2,
   vtrace_ref.EXPF_ULPS; the second term is the one rounding of x).
4. +inf for NaN in the unused term entries: the same bits (part of 1).  5. The refusals.  6. One closed-loop rollout end to end.

Each case prints its figures.
FIGURES (MI355X): 20 cases, 7 s for the file, slowest case 1.0 s (edge shapes, N = 2096).  Worst error / bar over the 896 calls of each N,
vs and pg_adv (the two kernels differ in the third digit at most):
    N      1      63     255    256    257    2096
    vs     0.214  0.474  0.493  0.486  0.479  0.495
    pg     0.304  0.335  0.336  0.342  0.341  0.338
(the fp32 emulation with numpy's exp: 0.479 and 0.341 at N = 257).  On-policy: 2688 calls per N, every vs gae_dev's ret bit for bit.
The ratio: every clipped entry the bar's bits; the free ones at most 14.8 ulp from fp64 exp, at x = +20 where the one rounding of x
alone allows 20 ulp (0.74 of the bound); at most 9.2 ulp (0.70 of the bound) with the bars at 1 and 3.  End to end (N = 68, T = 20,
max |x| 1.62): 0.126 on vs, 0.146 on pg_adv."""
import numpy as np
import pytest

from tests import ac_ref
from tests import gae_emul as G
from tests import vtrace_emul as V
from tests import vtrace_ref as R
from tests.policy_util import _bufs, _dev

pytestmark = pytest.mark.gpu

KEYS = ("rew", "done", "values", "logp_b", "logp_t", "term")


def _to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _env(n):
    from gym_art_amd import QuadrotorEnv
    return QuadrotorEnv(num_envs=n)


def _run(env, dev, params, term):
    """the call with pg_adv and the vs-only call; (vs, pg) as numpy, after asserting that the two vs are the same bits"""
    import torch
    r, d, v, lb, lt, tv = dev
    vs, pg, vs_only = (torch.full_like(r, float("nan")) for _ in range(3))
    kw = dict(lam=params[1], rho_bar=params[2], c_bar=params[3], pg_rho_bar=params[4], term_values=tv if term else None)
    env.vtrace_dev(r, d, v, lb, lt, params[0], vs, pg, **kw)
    env.vtrace_dev(r, d, v, lb, lt, params[0], vs_only, **kw)
    torch.cuda.synchronize()
    assert torch.equal(vs.view(torch.int32), vs_only.view(torch.int32)), (params, term)
    return vs.cpu().numpy(), pg.cpu().numpy()


@pytest.mark.parametrize("n", V.BATCHES)
def test_vtrace_kernels_at_their_edge_shapes(n):
    env = _env(n)
    worst, cases = {False: np.zeros(2), True: np.zeros(2)}, 0
    for inp in V.inputs(n):
        if n > 1 and inp["p"] == 0.1 and inp["T"] >= 5:
            assert V.rich_dones(inp["done"]), (n, inp["T"], inp["scale"])
        dev = tuple(_to_dev(inp[key]) for key in KEYS)
        inf = inp["T"] == 9 and inp["p"] == 0.5                     # +inf instead of NaN where done is clear: the same bits
        dev_inf = dev[:5] + (_to_dev(V.with_inf(inp)["term"]),) if inf else None
        for params in V.PARAMS:
            for term in (False, True):
                vs, pg = _run(env, dev, params, term)
                ref, bar_vs, bar_pg = V.reference(inp, params, term)
                worst[term] = np.maximum(worst[term], V.check(inp, params, term, vs, pg, ref, bar_vs, bar_pg))
                cases += 1
            if inf:
                vs2, pg2 = _run(env, dev_inf, params, True)
                assert np.array_equal(vs2.view(np.uint32), vs.view(np.uint32)) and np.array_equal(pg2.view(np.uint32), pg.view(np.uint32))
    print("vtrace edges n=%d: %d cases, worst error / bar vs %.3g pg %.3g (vtrace_kernel), vs %.3g pg %.3g (vtrace_term_kernel)"
          % (n, cases, worst[False][0], worst[False][1], worst[True][0], worst[True][1]))
    env.close()


@pytest.mark.parametrize("n", V.BATCHES)
def test_on_policy_vs_is_gae_devs_return_bit_for_bit(n):
    import torch
    env = _env(n)
    cases = 0
    for inp in V.inputs(n):
        r, d, v, lb, _, tv = (_to_dev(inp[key]) for key in KEYS)
        lt = lb.clone()
        for gamma, lam in G.GAMMA_LAMBDA:
            for term in (False, True):
                adv, ret = torch.full_like(r, float("nan")), torch.full_like(r, float("nan"))
                env.gae_dev(r, d, v, gamma, lam, adv, ret, term_values=tv if term else None)
                for clips in ((1.0, 1.0, 1.0), (2.0, 1.5, 3.0), (float("inf"),) * 3):
                    vs = torch.full_like(r, float("nan"))
                    env.vtrace_dev(r, d, v, lb, lt, gamma, vs, lam=lam, rho_bar=clips[0], c_bar=clips[1], pg_rho_bar=clips[2],
                                   term_values=tv if term else None)
                    assert torch.equal(vs.view(torch.int32), ret.view(torch.int32)), (n, inp["T"], inp["p"], gamma, lam, term, clips)
                    cases += 1
    print("vtrace on-policy n=%d: %d calls, vs == gae_dev's ret bit for bit" % (n, cases))
    env.close()


@pytest.mark.parametrize("n", V.BATCHES)
def test_the_ratio_is_clipped_expf(n):
    """gamma = 0, V = 0, r = 1: vs IS rho and pg_adv IS rho_pg"""
    import torch
    env = _env(n)
    T = 9
    inp = [i for i in V.inputs(n) if i["T"] == T and i["p"] == 0.5][0]
    inp = dict(inp, logp_t=inp["logp_t"].copy())
    inp["logp_t"][0, 0] = inp["logp_b"][0, 0] + np.float32(100.0)  # every N holds an overflow entry, whatever it drew
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp((inp["logp_t"] - inp["logp_b"]).astype(np.float32))).any()
    lb, lt, d = (_to_dev(inp[key]) for key in ("logp_b", "logp_t", "done"))
    r, v = torch.ones((T, n), device=_dev()), torch.zeros((T + 1, n), device=_dev())
    x = inp["logp_t"].astype(np.float64) - inp["logp_b"].astype(np.float64)
    w = np.exp(x)
    worst = 0.0
    for rho_bar, pg_bar in ((1.0, 3.0), (1e30, 0.5)):
        vs, pg = torch.full_like(r, float("nan")), torch.full_like(r, float("nan"))
        env.vtrace_dev(r, d, v, lb, lt, 0.0, vs, pg, lam=1.0, rho_bar=rho_bar, c_bar=1.0, pg_rho_bar=pg_bar)
        for got, bar in ((vs.cpu().numpy(), np.float32(rho_bar)), (pg.cpu().numpy(), np.float32(pg_bar))):
            clipped = w > float(bar)
            assert (got[clipped].view(np.uint32) == bar.view(np.uint32)).all(), (n, float(bar))
            ref = w[~clipped]
            ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
            err = np.abs(got[~clipped].astype(np.float64) - ref) / ulp
            bound = R.EXPF_ULPS + np.abs(x[~clipped]) * R.U24 * ref / ulp
            if err.size:
                worst = max(worst, float(err.max()))
                print("ratio n=%d bar=%g: %d clipped, %d free, worst %.3f ulp (worst error / bound %.3f)"
                      % (n, float(bar), int(clipped.sum()), err.size, float(err.max()), float((err / bound).max())))
            assert (err <= bound).all(), (n, float(bar), float((err / bound).max()))
    print("ratio n=%d: worst %.3f ulp against fp64 exp" % (n, worst))
    env.close()


def test_refusals_leave_the_outputs_untouched():
    import torch
    n, T = 63, 5
    env = _env(n)
    inp = [i for i in V.inputs(n) if i["T"] == T and i["p"] == 0.5][0]
    r, d, v, lb, lt, tv = (_to_dev(inp[key]) for key in KEYS)
    vs, pg = torch.full_like(r, float("nan")), torch.full_like(r, float("nan"))
    ok = dict(lam=0.95, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0)
    nan, inf = float("nan"), float("inf")

    def refused(*args, **kw):
        with pytest.raises(ValueError):
            env.vtrace_dev(*args, **dict(ok, **kw))
        torch.cuda.synchronize()
        assert bool(torch.isnan(vs).all()) and bool(torch.isnan(pg).all())

    for gamma in (-0.1, 1.5, nan):
        refused(r, d, v, lb, lt, gamma, vs, pg)
    for lam in (-0.1, 1.5, nan):
        refused(r, d, v, lb, lt, 0.99, vs, pg, lam=lam)
    for key in ("rho_bar", "c_bar", "pg_rho_bar"):
        for bad in (0.0, -1.0, nan, -inf):
            refused(r, d, v, lb, lt, 0.99, vs, pg, **{key: bad})
    # a null required argument and T <= 0 (the C entry points; the method would stop at the shapes)
    import ctypes as C
    from gym_art_amd import _lib
    lib, st = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [_lib.ptr(t) for t in (r, d, v, lb, lt)]
    for k in range(5):
        a = list(args)
        a[k] = None
        assert lib.gaq_vtrace_dev(env._handle, T, *a, 0.99, 0.95, 1.0, 1.0, 1.0, _lib.ptr(vs), _lib.ptr(pg), st) == -1
        assert lib.gaq_vtrace_term_dev(env._handle, T, *a, _lib.ptr(tv), 0.99, 0.95, 1.0, 1.0, 1.0, _lib.ptr(vs), _lib.ptr(pg), st) == -1
    assert lib.gaq_vtrace_dev(env._handle, T, *args, 0.99, 0.95, 1.0, 1.0, 1.0, None, _lib.ptr(pg), st) == -1
    for bad_T in (0, -1):
        assert lib.gaq_vtrace_dev(env._handle, bad_T, *args, 0.99, 0.95, 1.0, 1.0, 1.0, _lib.ptr(vs), _lib.ptr(pg), st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(vs).all()) and bool(torch.isnan(pg).all())
    # an output that overlaps an input (each input in turn, as the output it can stand for), and the two outputs overlapping
    big = torch.full(((T + 1) * n,), float("nan"), device=_dev())
    for name in ("rew", "logp_b", "logp_t", "term"):
        src = {"rew": r, "logp_b": lb, "logp_t": lt, "term": tv}[name]
        keep = src.clone()
        with pytest.raises(ValueError):
            env.vtrace_dev(r, d, v, lb, lt, 0.99, src, pg, term_values=tv, **ok)
        with pytest.raises(ValueError):
            env.vtrace_dev(r, d, v, lb, lt, 0.99, vs, src, term_values=tv, **ok)
        torch.cuda.synchronize()
        assert torch.equal(src.view(torch.int32), keep.view(torch.int32)), name
    vkeep = v.clone()
    with pytest.raises(ValueError):
        env.vtrace_dev(r, d, v, lb, lt, 0.99, v[1:], pg, **ok)      # values' rows 1..T
    with pytest.raises(ValueError):
        env.vtrace_dev(r, d, v, lb, lt, 0.99, vs, v[:T], **ok)
    done_as_out = big[:T * n].view(T, n)
    d4 = big.view(torch.uint8)[:T * n].view(T, n)                   # a done that lives inside an output's bytes
    with pytest.raises(ValueError):
        env.vtrace_dev(r, d4, v, lb, lt, 0.99, done_as_out, pg, **ok)
    with pytest.raises(ValueError):
        env.vtrace_dev(r, d, v, lb, lt, 0.99, vs, vs, **ok)         # the two outputs
    half = big[:T * n + n]                                          # ... and overlapping by one row
    with pytest.raises(ValueError):
        env.vtrace_dev(r, d, v, lb, lt, 0.99, half[:T * n].view(T, n), half[n:].view(T, n), **ok)
    torch.cuda.synchronize()
    assert torch.equal(v, vkeep) and bool(torch.isnan(big).all())
    assert bool(torch.isnan(vs).all()) and bool(torch.isnan(pg).all())
    # shapes, dtypes and devices stop in the method
    for bad in (lb[:-1], lb.double(), lb.cpu(), lb.t()):
        with pytest.raises(ValueError):
            env.vtrace_dev(r, d, v, bad, lt, 0.99, vs, pg, **ok)
        with pytest.raises(ValueError):
            env.vtrace_dev(r, d, v, lb, bad, 0.99, vs, pg, **ok)
    with pytest.raises(ValueError):
        env.vtrace_dev(r, d, v, lb, lt, 0.99, vs, pg, term_values=tv[:-1], **ok)
    # ... and after all that the call works
    env.vtrace_dev(r, d, v, lb, lt, 0.99, vs, pg, term_values=tv, **ok)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(vs).all()) and bool(torch.isfinite(pg).all())
    env.close()


def test_a_closed_loop_rollout_end_to_end():
    """N = 68, T = 20, every env auto-resets inside the window; an 18-48-4 "mfma" policy with a value head writes values, logp and
    term_values; logp_target is a torch forward of the same net with its weights perturbed by 1e-2 on the observations the actions were
    computed from; vtrace_dev(term_values=) against the fp64 reference at the bars"""
    import torch
    from tests.mlp_ref import forward64
    from tests.test_gpu_policy_ac import LOG_STD, NETS, T, _Net, _ac_bufs, _reset
    from tests.test_gpu_policy_ac import _env as ac_env
    from tests.test_gpu_policy_shapes import _obs_scale
    n = 68
    env = ac_env(n, "alias")
    net = _Net(NETS[0], _obs_scale(env), 0)
    assert net.kind == "mlp" and [W.shape[0] for W, _ in net.layers] == [48, 4]
    pol = net.build(env)
    _, o0 = _reset(env, pol)
    o, r, d, a = _bufs(env, T)
    v, lp = _ac_bufs(env, T)
    tv = torch.full((T, n), float("nan"), device=_dev())
    env.rollout_policy_dev(pol, o, r, d, a, values=v, logp=lp, term_values=tv)
    torch.cuda.synchronize()
    assert bool((d.to(torch.int32).sum(dim=0) >= 1).all())          # every env finished an episode
    rng = np.random.RandomState(5)
    moved = [((W + 1e-2 * rng.randn(*W.shape)).astype(np.float32), (b + 1e-2 * rng.randn(*b.shape)).astype(np.float32)) for W, b in net.layers]
    seen = torch.cat([o0[None], o[:-1]])                            # row t: the observation action t was computed from
    means, _ = forward64(moved, net.act, net.out_tanh, seen)
    target, _ = ac_ref.logp64(a.cpu().numpy(), means.cpu().numpy(), LOG_STD)
    lt = _to_dev(target.astype(np.float32))
    x = (lt - lp).cpu().numpy()
    assert np.isfinite(x).all() and float(np.abs(x).max()) > 1e-3, float(np.abs(x).max())      # off-policy, by a real margin
    inp = dict(T=T, p=float(d.float().mean()), scale=1.0, rew=r.cpu().numpy(), done=d.cpu().numpy(), values=v.cpu().numpy(),
               logp_b=lp.cpu().numpy(), logp_t=lt.cpu().numpy(), term=tv.cpu().numpy())
    worst = np.zeros(2)
    for params in V.PARAMS:
        vs, pg = _run(env, (r, d, v, lp, lt, tv), params, True)
        ref, bar_vs, bar_pg = V.reference(inp, params, True)
        assert np.isfinite(vs).all() and np.isfinite(pg).all() and np.isfinite(ref["vs"]).all()
        fv, fp = V.error_over_bar(vs, ref["vs"], bar_vs), V.error_over_bar(pg, ref["pg"], bar_pg)
        assert fv <= 1.0 and fp <= 1.0, (params, fv, fp)
        worst = np.maximum(worst, (fv, fp))
    print("vtrace end to end: max |x| %.3g, worst error / bar vs %.3g pg %.3g" % (float(np.abs(x).max()), worst[0], worst[1]))
    pol.close(); env.close()
