"""V-trace and advantage standardisation without a GPU.  The inputs tests/test_gpu_vtrace.py feeds the two V-trace kernels are fair to a
correct fp32 kernel and the bars catch a wrong one: the fp32 emulation of tests/vtrace_emul.py over the GPU file's own input generator
stays within the running bars of tests/vtrace_ref.py everywhere, each of six deliberately wrong variants exceeds them wherever it computes
other bits, the bars stand far below the quantity the scan carries, and on-policy the emulation's vs is gae_emul.emulate's ret bit for
bit.  The last test is the interface: the header declares the six new entry points, the binding lists each with the header's argument
count, and QuadrotorEnv.vtrace_dev and norm.AdvNorm exist.

Worst error / bar of the emulation over these cases (numpy's float32 exp standing in for expf): 0.479 on vs, 0.341 on pg_adv -- 0.96
and 0.68 of the first-order bound, which the factor 2 for second-order terms halves."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import gae_emul as G
from tests import vtrace_emul as V

BATCHES = [1, 63, 257]                           # one env, a partial block, a block and an env
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _forms(inp):
    """(the input, the term form?) of every call the GPU file makes on this input"""
    out = [(inp, False), (inp, True)]
    if inp["T"] == 9 and inp["p"] == 0.5:
        out.append((V.with_inf(inp), True))
    return out


@pytest.mark.parametrize("n", BATCHES)
def test_emulation_meets_the_bars_on_the_gpu_files_inputs(n):
    worst, cases, medians = np.zeros(2), 0, []
    for inp in V.inputs(n):
        if n > 1 and inp["p"] == 0.1 and inp["T"] >= 5:
            assert V.rich_dones(inp["done"]), (n, inp["T"], inp["scale"])
        assert np.isnan(inp["term"][inp["done"] == 0]).all() and np.isfinite(inp["term"][inp["done"] != 0]).all()
        assert np.isfinite(inp["logp_b"]).all() and np.isfinite(inp["logp_t"]).all()
        for params in V.PARAMS:
            for x, term in _forms(inp):
                vs, pg = V.emulate(x, params, term)
                ref, bar_vs, bar_pg = V.reference(x, params, term)
                worst = np.maximum(worst, V.check(x, params, term, vs, pg, ref, bar_vs, bar_pg))
                medians.append(V.teeth(ref, bar_vs))
                if n > 1:
                    assert medians[-1] > 100.0, (n, inp["T"], inp["p"], inp["scale"], params, term, medians[-1])
                cases += 1
    # teeth: the quantity the scan carries stands far above its bar (N = 1: a case is T elements, so the cases are pooled)
    assert float(np.median(medians)) > 100.0, (n, float(np.median(medians)))
    print("vtrace emulation n=%d: %d cases, worst error / bar %.3g (vs), %.3g (pg_adv); median |acc| / bar %.3g (least %.3g)"
          % (n, cases, worst[0], worst[1], float(np.median(medians)), min(medians)))


def test_the_ratios_reach_the_overflow_and_both_clips():
    """the draws of x hold what the issue asks for at every N > 1: entries of +20, -20 and +100, whose float32 exp is inf"""
    for n in V.BATCHES[1:]:
        x = np.concatenate([(inp["logp_t"].astype(np.float64) - inp["logp_b"]).ravel() for inp in V.inputs(n)])
        assert (np.abs(x - 20.0) < 1e-4).any() and (np.abs(x + 20.0) < 1e-4).any() and (np.abs(x - 100.0) < 1e-4).any(), n
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(x.astype(np.float32))).any(), n


def _matters(variant, inp, params, term):
    """a sufficient condition for the variant to compute something else than the kernel (None: no simple one)"""
    cut = inp["done"] != 0
    T = inp["T"]
    if variant == "no_cut":
        return True if params[0] * params[1] > 0 and T > 1 and cut[:-1].any() and inp["rew"].shape[1] > 1 else None
    if variant == "term_mul":
        return bool(term and not cut.all())                 # 0 * NaN
    if variant == "drop_tail":
        return T % 4 != 0
    if variant == "pg_rho":
        return None if params[2] != params[4] else False
    return None


@pytest.mark.parametrize("variant", V.VARIANTS)
def test_a_wrong_kernel_exceeds_the_bar(variant):
    """each wrong variant fails a bar in every case in which it computes other bits than the kernel"""
    n, failed, differs = 63, 0, 0
    for inp in V.inputs(n):
        for params in V.PARAMS:
            for term in ((True,) if variant == "term_mul" else (False, True)):
                good = V.emulate(inp, params, term)
                bad = V.emulate(inp, params, term, variant)
                ref, bar_vs, bar_pg = V.reference(inp, params, term)
                assert V.error_over_bar(good[0], ref["vs"], bar_vs) <= 1.0 and V.error_over_bar(good[1], ref["pg"], bar_pg) <= 1.0
                same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(good, bad))
                want = _matters(variant, inp, params, term)
                if want is not None:
                    assert same != want, (variant, inp["T"], inp["p"], params, term)
                if same:
                    continue
                differs += 1
                failed += V.error_over_bar(bad[0], ref["vs"], bar_vs) > 1.0 or V.error_over_bar(bad[1], ref["pg"], bar_pg) > 1.0
    print("%s: %d of the %d cases it differs in exceed a bar" % (variant, failed, differs))
    assert differs > 50 and failed == differs, (variant, failed, differs)


@pytest.mark.parametrize("n", BATCHES)
def test_on_policy_vs_is_gaes_return_bit_for_bit(n):
    """logp_target the bits of logp_behaviour, clips >= 1: vs of the emulation == ret of gae_emul.emulate, both forms, every (gamma,
    lambda) of gae_emul.GAMMA_LAMBDA; the same expressions in the same order, so this pins the ORDER the header promises"""
    for inp in V.inputs(n):
        x = V.on_policy(inp)
        for gamma, lam in G.GAMMA_LAMBDA:
            for term in (False, True):
                _, ret = G.emulate(inp, gamma, lam, term)
                for clips in ((1.0, 1.0, 1.0), (2.0, 1.5, 3.0), (np.inf, np.inf, np.inf)):
                    vs, _ = V.emulate(x, (gamma, lam) + clips, term)
                    assert np.array_equal(vs.view(np.uint32), ret.view(np.uint32)), (n, inp["T"], inp["p"], gamma, lam, term, clips)


def _header_args():
    """{function: number of arguments} of every declaration of include/gaq.h"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaq.h")).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(gaq_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_the_new_entry_points_are_declared_bound_and_wrapped():
    from gym_art_amd import QuadrotorEnv, _lib, norm, policy
    declared = _header_args()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    want = {"gaq_vtrace_dev": 15, "gaq_vtrace_term_dev": 16, "gaq_adv_norm_create": 4, "gaq_adv_norm_apply_dev": 5,
            "gaq_adv_norm_get_stats": 4, "gaq_adv_norm_destroy": 1}
    for name, count in want.items():
        assert declared.get(name) == count, (name, declared.get(name))
        assert name in sig and len(sig[name]) == count, name
    for name in ("gaq_gae_dev", "gaq_gae_term_dev", "gaq_ret_norm_apply_dev"):      # (the parser counts what it should)
        assert declared[name] == len(sig[name]), name
    lib = _lib.load()
    for name in want:
        assert hasattr(lib, name), name
    params = inspect.signature(QuadrotorEnv.vtrace_dev).parameters
    assert list(params)[:9] == ["self", "rew", "done", "values", "logp_behaviour", "logp_target", "gamma", "vs", "pg_adv"]
    assert params["pg_adv"].default is None
    for key, default in (("lam", 1.0), ("rho_bar", 1.0), ("c_bar", 1.0), ("pg_rho_bar", 1.0), ("term_values", None), ("stream", None)):
        assert params[key].kind is inspect.Parameter.KEYWORD_ONLY and params[key].default == default, key
    init = inspect.signature(norm.AdvNorm.__init__).parameters
    assert list(init) == ["self", "env", "eps", "ddof"] and init["eps"].default == 1e-8 and init["ddof"].default == 1
    assert list(inspect.signature(norm.AdvNorm.normalize_dev).parameters) == ["self", "adv", "out", "stream"]
    assert callable(norm.AdvNorm.stats) and callable(norm.AdvNorm.close)
    assert policy.AdvNorm is norm.AdvNorm


def test_the_new_entry_points_refuse_null_arguments():
    import ctypes as C
    from gym_art_amd import _lib
    lib = _lib.load()
    h, d = C.c_void_p(), C.c_double()
    calls = [lambda: lib.gaq_vtrace_dev(None, 4, None, None, None, None, None, 0.99, 1.0, 1.0, 1.0, 1.0, None, None, None),
             lambda: lib.gaq_vtrace_term_dev(None, 4, None, None, None, None, None, None, 0.99, 1.0, 1.0, 1.0, 1.0, None, None, None),
             lambda: lib.gaq_adv_norm_create(None, 1e-8, 1, C.byref(h)),
             lambda: lib.gaq_adv_norm_apply_dev(None, 4, None, None, None),
             lambda: lib.gaq_adv_norm_get_stats(None, C.byref(d), C.byref(d), C.byref(d))]
    for call in calls:
        assert call() == -1 and b"null" in lib.gaq_last_error()
    assert not h.value
    assert lib.gaq_adv_norm_destroy(None) == 0
