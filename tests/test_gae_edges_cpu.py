"""The inputs tests/test_gpu_gae_edges.py feeds the two GAE kernels are fair to a correct fp32 kernel, and the bars catch a wrong one: the
fp32 emulation of tests/gae_emul.py over the GPU file's own input generator stays within the derived bars everywhere, and each of three
deliberately wrong variants of it exceeds them.  No GPU.  Worst error / bar of the emulation over these cases: 0.25."""
import numpy as np
import pytest

from tests import gae_emul as G

BATCHES = [1, 63, 257]                           # one env, a partial block, a block and an env


def _forms(inp):
    """(the input, the term form?) of every call the GPU file makes on this input"""
    out = [(inp, False), (inp, True)]
    if inp["T"] == 9 and inp["p"] == 0.5:
        out.append((G.with_inf(inp), True))
    return out


@pytest.mark.parametrize("n", BATCHES)
def test_emulation_meets_the_bars_on_the_gpu_files_inputs(n):
    worst, cases = 0.0, 0
    for inp in G.inputs(n):
        if n > 1 and inp["p"] == 0.1 and inp["T"] >= 5:
            assert G.rich_dones(inp["done"]), (n, inp["T"], inp["scale"])
        assert set(np.unique(inp["done"])) <= {0, 1, 2, 255}
        assert np.isnan(inp["term"][inp["done"] == 0]).all() and np.isfinite(inp["term"][inp["done"] != 0]).all()
        for gamma, lam in G.GAMMA_LAMBDA:
            for x, term in _forms(inp):
                adv, ret = G.emulate(x, gamma, lam, term)
                aref, bar = G.reference(x, gamma, lam, term)
                worst = max(worst, G.check(x, gamma, lam, term, adv, ret, aref, bar))
                cases += 1
    print("gae emulation n=%d: %d cases, worst error / bar %.3g" % (n, cases, worst))


def test_every_batch_size_has_a_seed_with_rich_dones():
    """the GPU file's batch sizes that the emulation above does not run: the p = 0.1 inputs hold the dones the issue asks for"""
    for n in G.BATCHES:
        seen = {0.0: 0, 1.0: 0}
        for inp in G.inputs(n):
            if n > 1 and inp["p"] == 0.1 and inp["T"] >= 5:
                assert G.rich_dones(inp["done"]), (n, inp["T"], inp["scale"])
            if inp["p"] in seen:
                assert bool((inp["done"] != 0).all()) == (inp["p"] == 1.0) and bool((inp["done"] != 0).any()) == (inp["p"] == 1.0)
                seen[inp["p"]] += 1
        assert seen[0.0] == seen[1.0] == len(G.STEPS) * len(G.SCALES)


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_a_wrong_kernel_exceeds_the_bar(variant):
    """each wrong variant fails the bar in every case in which it computes something else than the kernel"""
    n, failed, differs = 63, 0, 0
    for inp in G.inputs(n):
        cut = inp["done"] != 0
        for gamma, lam in G.GAMMA_LAMBDA:
            term = variant == "term_mul"
            good, _ = G.emulate(inp, gamma, lam, term)
            adv, _ = G.emulate(inp, gamma, lam, term, variant)
            aref, bar = G.reference(inp, gamma, lam, term)
            assert G.error_over_bar(good, aref, bar) <= 1.0
            if variant == "no_cut":
                matters = gamma * lam > 0 and cut[:-1].any() if inp["T"] > 1 else False
            elif variant == "term_mul":
                matters = not cut.all()                     # 0 * NaN
            else:
                matters = inp["T"] % 4 != 0
            if not matters:
                assert np.array_equal(adv, good, equal_nan=True), (variant, inp["T"], inp["p"], gamma, lam)
                continue
            differs += 1
            failed += G.error_over_bar(adv, aref, bar) > 1.0
    print("%s: %d of the %d cases it differs in exceed the bar" % (variant, failed, differs))
    assert differs > 50 and failed == differs, (variant, failed, differs)
