"""-m gpu: the passes of the per-env parameter pipeline (csrc/gaq_params.hip) put side by side at edge sizes -- one env, a ragged second
tile (65), a second workgroup holding one env (257) -- for a RelativeSampler around the Crazyflie and for RandomQuad.  Every pass derives
"the tree of env i at draw k" and the planes of it with its own inlined copy of quad_params_dev.hpp; they have to give the same bits, on
every field of gaq_model.  The scenario (what is done to which handle) is tests/param_passes.py."""
import numpy as np
import pytest

from tests import param_passes as pp

pytestmark = pytest.mark.gpu
CASES = [(n, kind) for n in pp.SIZES for kind in pp.KINDS]


def same_fields(got, want):
    g, w = pp.fields(got), pp.fields(want)
    assert sorted(g) == sorted(w)
    bad = [k for k in w if not np.array_equal(g[k], w[k])]
    assert not bad, bad


@pytest.fixture(params=CASES, ids=["%d-%s" % c for c in CASES])
def sc(request):
    return pp.scenario(*request.param)


def test_the_scenario_reached_the_same_draw_everywhere(sc):
    """every handle compared below stands at the same resample count per env, and it is DRAWS past a fresh handle's"""
    assert np.array_equal(sc["redrawn_resamples"], sc["fresh_resamples"] + pp.DRAWS)
    assert np.array_equal(sc["stepped_resamples"], sc["redrawn_resamples"])
    assert np.array_equal(sc["caught_up_resamples"], sc["redrawn_resamples"]) and not sc["caught_up_done"].any()
    assert np.all(sc["redrawn"][:, 0] > 0) and np.isfinite(sc["redrawn"]).all()


def test_rebuild_from_the_counts_equals_the_redraws(sc):
    """gaq_randomize_dev k times on A; B is given A's counters and resample counts (gaq_set_counters): B holds A's parameters"""
    same_fields(sc["rebuilt"], sc["redrawn"])


def test_promotion_and_refill_equal_the_redraws(sc):
    """dynamics_randomize_every = 1: after k finished episodes per env the parameters (env.models) are those of k redraws"""
    same_fields(sc["stepped_models"], sc["redrawn"])


def test_the_rows_pass_equals_the_redraws_and_is_a_read(sc):
    """gaq_get_params after hot-planes-only promotions (the whole row derived afresh): the redrawn handle's, twice; state and counters
    are untouched"""
    same_fields(sc["stepped"], sc["redrawn"])
    same_fields(sc["stepped_again"], sc["redrawn"])
    for what in ("state", "counters", "episodes", "resamples"):
        assert np.array_equal(sc["stepped_" + what], sc["stepped_%s_after_reads" % what]), what


def test_catch_up_equals_the_redraws(sc):
    """the parameter flags change under the live randomizer; the next step launch first brings the planes that hot-planes-only promotions
    left behind up to date: what is then read (from memory) is still the redrawn handle's"""
    same_fields(sc["caught_up"], sc["redrawn"])


def test_trees_read_back_give_the_same_planes(sc):
    """gaq_get_param_trees of A -> gaq_set_param_trees on a fresh handle (links_by_density as the sampler implies) = A's gaq_get_params"""
    same_fields(sc["from_trees"], sc["redrawn"])


def test_masked_redraw_changes_exactly_the_selected_env(sc):
    """a mask that selects only the last env (env 64 of 65: the one lane of the second tile): exactly that env's parameters change"""
    changed = np.nonzero(np.any(sc["rebuilt_masked_redraw"] != sc["rebuilt"], axis=1))[0]
    assert changed.tolist() == [sc["rebuilt"].shape[0] - 1]
