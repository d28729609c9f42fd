"""gae_kernel and gae_term_kernel (gaq.h gaq_gae_dev, gaq_gae_term_dev) on synthetic tensors at the shapes their code branches on: T of
1, 2, 3, 4, 5, 7, 9 and 65 (the t loop is unrolled by 4), N of 1, 63, 255, 256, 257 and 2096 (the block is 256 threads), no done, sparse
and dense dones and all dones (a done at t = 0, at t = T - 1, two in a row), done bytes 1, 2 and 255, rewards and values of scale 1 and
100, seven (gamma, lambda) pairs with 0 and 1 among them, and for the term form NaN -- and once +inf -- in every entry whose done byte is
clear: the kernel's comment says such an entry never reaches a sum.  The env is only a handle of N envs.

Inputs, fp32 emulation and checks are those of tests/gae_emul.py; tests/test_gae_edges_cpu.py shows without a GPU that these inputs are
fair (worst error / bar of the emulation 0.25) and that the bars catch three wrong kernels.  The advantages are held to the derived bars
of tests/ac_ref.py gae_bar and tests/term_ref.py gae_term_bar with no element excluded.

Each case prints the device's worst |A - A_ref| / bar of its N (the bar is 1).
FIGURES: not yet measured on an MI355X; the fp32 emulation's worst is 0.25."""
import numpy as np
import pytest

from tests import gae_emul as G
from tests.policy_util import _dev

pytestmark = pytest.mark.gpu


def _to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _run(env, dev, gamma, lam, term):
    """the call with ret and the adv-only call; (adv, ret) as numpy, after asserting that the two advantages are the same bits"""
    import torch
    r, d, v, tv = dev
    adv, ret, adv_only = (torch.full_like(r, float("nan")) for _ in range(3))
    env.gae_dev(r, d, v, gamma, lam, adv, ret, term_values=tv if term else None)
    env.gae_dev(r, d, v, gamma, lam, adv_only, term_values=tv if term else None)
    torch.cuda.synchronize()
    assert torch.equal(adv.view(torch.int32), adv_only.view(torch.int32)), (gamma, lam, term)
    return adv.cpu().numpy(), ret.cpu().numpy()


@pytest.mark.parametrize("n", G.BATCHES)
def test_gae_kernels_at_their_edge_shapes(n):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(num_envs=n)
    worst, cases = {False: 0.0, True: 0.0}, 0
    for inp in G.inputs(n):
        if n > 1 and inp["p"] == 0.1 and inp["T"] >= 5:
            assert G.rich_dones(inp["done"]), (n, inp["T"], inp["scale"])
        forms = [(inp, False), (inp, True)]
        if inp["T"] == 9 and inp["p"] == 0.5:
            forms.append((G.with_inf(inp), True))               # +inf instead of NaN where done is clear
        for x, term in forms:
            dev = tuple(_to_dev(x[key]) for key in ("rew", "done", "values", "term"))
            for gamma, lam in G.GAMMA_LAMBDA:
                adv, ret = _run(env, dev, gamma, lam, term)
                aref, bar = G.reference(x, gamma, lam, term)
                worst[term] = max(worst[term], G.check(x, gamma, lam, term, adv, ret, aref, bar))
                cases += 1
    print("gae edges n=%d: %d cases, worst error / bar %.3g (gae_kernel), %.3g (gae_term_kernel)" % (n, cases, worst[False], worst[True]))
    env.close()
