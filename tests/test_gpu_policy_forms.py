"""-m gpu: the launches a rollout call chooses (csrc/gaq_policy.hip rollout_plan) against each other, bit for bit: asking for more leaves
what a narrower call writes as it was, the general entry points with their optional arguments null are the narrow ones, the two-launch
critic is the fused one and both are values_dev of the recorded rows, and a window split into calls is the window.  N = 1 and 65, T = 8
at ep_time = 0.05, every actor engine and cell, critics narrower and wider than the actor, normalisers on both nets and on the actor
only.  The scenarios are tests/policy_forms.py.  On an MI355X: 115 cases in under 3 s."""
import numpy as np
import pytest

from tests import policy_forms as pf

pytestmark = pytest.mark.gpu
ROLLOUT = ("obs0", "obs", "rew", "done", "actions")
ident = lambda case: "-".join(str(f) for f in case).replace(" ", "")


def same(a, b, names):
    bad = [k for k in names if a[k].shape != b[k].shape or not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]
    assert not bad, bad


def written(sc, case):
    """every output asked for was written in full; terminal values were gathered for at least one row"""
    assert sc["done"].any() and not sc["done"].all()                 # episodes ended inside the window
    for k in ("values", "logp", "term_values"):
        assert (k in sc) == (k[0] in case.ask) and (k not in sc or np.isfinite(sc[k]).all()), k
    if "t" in case.ask:
        assert sc["term_values"][sc["done"] != 0].any() and not sc["term_values"][sc["done"] == 0].any()


@pytest.mark.parametrize("case", pf.CASES["asked"] + pf.CASES["paired"] + pf.CASES["normed"], ids=ident)
def test_asking_for_more_changes_nothing_else(case):
    """values, logp and / or term_values, from a value head or a critic: obs, rew, done and actions are the plain entry point's"""
    sc, ref = pf.scenario(case), pf.scenario(pf.plain(case))
    written(sc, case)
    same(sc, ref, ROLLOUT + tuple(k for k in ("hidden", "cell") if k in ref))


@pytest.mark.parametrize("case", pf.CASES["wide"], ids=ident)
def test_a_general_entry_point_with_nulls_is_the_narrow_one(case):
    """gaq_step_policy_ac_term_many_dev with a null term_value_out, gaq_step_policy_critic_many_dev with a null critic: every array
    is what the entry point rollout_policy_dev picks for the same outputs wrote"""
    sc, ref = pf.scenario(case), pf.scenario(case._replace(entry="py"))
    written(sc, case)
    assert sorted(sc) == sorted(ref)
    same(sc, ref, sorted(ref))


@pytest.mark.parametrize("case", pf.UNFUSED, ids=ident)
def test_the_two_launch_critic_is_the_fused_one(case):
    """a critic created under GAQ_NO_FUSED_CRITIC=1 (for an MLP actor with the critic's normaliser: another kernel, another LDS size)"""
    sc, ref = pf.scenario(case), pf.scenario(case._replace(fused=True))
    assert sorted(sc) == sorted(ref)
    same(sc, ref, sorted(ref))


@pytest.mark.parametrize("case", [c for c in pf.CASES["paired"] + pf.CASES["normed"] + pf.UNFUSED if c.source in pf.CRITICS], ids=ident)
def test_rollout_values_are_values_dev_of_the_rows_they_were_computed_from(case):
    """rows 0 .. T of `values`: the critic's batch form on the start observation, obs[:-1], and obs[-1] for the bootstrap row"""
    sc = pf.scenario(case)
    assert sc["values"].shape == (pf.T + 1, case.n)
    same(sc, {"values": sc["values_dev"]}, ["values"])


@pytest.mark.parametrize("case", pf.CASES["split"], ids=ident)
def test_a_window_split_into_calls_is_the_window(case):
    """3 + 5 steps against 8: every output, a recurrent policy's states afterwards, and at the seam the first call's bootstrap row is the
    second call's row 0"""
    sc, ref = pf.scenario(case), pf.scenario(case._replace(calls=(pf.T,)))
    names = sorted(ref)
    assert sorted(k for k in sc if not k.startswith("seam_")) == names
    same(sc, ref, names)
    if "v" in case.ask:
        same({"seam": sc["seam_boot"]}, {"seam": sc["seam_next"]}, ["seam"])
