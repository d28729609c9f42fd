"""tests/test_gpu_policy_critic_shapes.py's case tables against the documented LDS formulas of the separate-critic kernels
(gym_art_amd/csrc/gaq_policy.hip): the tables really contain what that file's docstring claims -- each of the four LDS-sizing regimes,
a launch above 64 KiB for each of the three kernels, all activation mixes, every last width and every GRU H -- and the mixed-activation
cases have teeth: a critic evaluated with the other trunk's activation misses the fp64 reference by far more than the bar.
No device and no torch: the GPU file's tables are plain Python."""
import numpy as np

from tests import test_gpu_policy_critic_shapes as S
from tests.test_gpu_policy_ac import T, _style
from tests.test_gpu_policy_critic import ACTS, _CNet
from tests.test_gpu_policy_shapes import ATOL_FP32, OBS, _batches

LDS_ATTR = 65536                                 # above this the host raises the kernel's dynamic-LDS attribute before it launches


def _kin(D):
    return (D + 3) & ~3


def fused_lds(D, actor, critic):
    """policy_mfma_critic_kernel: the sums' 2 KiB + 256 B x max(in_dim rounded up to 4, every actor width, every critic width)"""
    return 2048 + 256 * max([_kin(D)] + list(actor) + list(critic))


def critic_lds(D, critic):
    """critic_mfma_kernel and critic_mfma_term_kernel: the parts of V, 1 KiB, + 256 B x max(in_dim rounded up to 4, critic widths)"""
    return 1024 + 256 * max([_kin(D)] + list(critic))


def _rollouts():
    """every (D, actor spec, critic widths, fused) the GPU file's rollouts run; all of them ask for values and term_values at least once"""
    out = []
    for obs, _ in S.CASES:
        for kind in ("mlp", "gru"):
            out += [(obs[2], spec, cw, True) for spec, _, cw, _ in S._pairs(kind, obs[2])]
    for _, obs, aw, cw in S.MIX:
        out += [(obs[2], ("mlp", aw), cw, fused) for fused in (True, False)]
    out += [(108, S.BIG_GRU, cw, True) for cw in S.BIG_GRU_CRITICS]
    out += [(18, spec, cw, True) for spec in S.GATHER_NETS for cw in S.GATHER_CRITICS]
    out += [(18, spec, cw, fused) for spec, cw, fused in S.GRAPH_PAIRS + S.SUBSET_PAIRS]
    return out


def test_formulas_at_the_documented_sizes():
    assert fused_lds(18, [256], [16]) == 66 * 1024 and critic_lds(18, [256, 256]) == 65 * 1024          # "66 KiB at width 256", 65 KiB
    assert fused_lds(108, [16], [48]) == 2048 + 256 * 108 and critic_lds(108, [16]) == 1024 + 256 * 108   # in_dim sizes both
    assert fused_lds(13, [16], [16]) == 2048 + 256 * 16 and _kin(13) == 16 and _kin(108) == 108 and _kin(25) == 28


def test_the_four_lds_sizing_regimes_of_the_mixed_cases():
    regimes = {m[0]: m for m in S.MIX}
    assert sorted(regimes) == ["actor", "both", "critic", "in_dim"]
    for name, obs, aw, cw in S.MIX:
        k, a, c = _kin(obs[2]), max(aw), max(cw)
        assert fused_lds(obs[2], aw, cw) == 2048 + 256 * max(k, a, c)
        if name == "in_dim":
            assert k > a and k > c
        elif name == "actor":
            assert a > k and a > c
        elif name == "critic":
            assert c > k and c > a
        else:
            assert a == c and a > k
    assert {m[1][2] for m in S.MIX} == {18, 108}
    assert (regimes["in_dim"][1][2], regimes["in_dim"][2], regimes["in_dim"][3]) == (108, [16], [48])
    assert (regimes["actor"][2], regimes["actor"][3]) == ([256, 256, 256], [16])
    assert (regimes["critic"][2], regimes["critic"][3]) == ([16], [256, 256])
    assert (regimes["both"][1][2], regimes["both"][2], regimes["both"][3]) == (108, [256], [256])
    # N = 64 + q: a tile plus a sliver at both widths
    assert [_batches(m[1][1])[2] for m in S.MIX] == [80, 68, 68, 80]
    # the same critics through term_values put the gathered kernel at 65 KiB
    assert sum(critic_lds(m[1][2], m[3]) == 65 * 1024 for m in S.MIX) == 2


def test_every_kernel_is_launched_above_64_kib():
    runs = _rollouts()
    fused = [fused_lds(D, spec[1], cw) for D, spec, cw, f in runs if spec[0] == "mlp" and f]
    # critic_mfma_term_kernel: the rollouts (each asks for term_values); critic_mfma_kernel: per step where the actor is a GRU or the
    # critic was built for two launches, the bootstrap row of the others (listed apart), and values_dev
    term = [critic_lds(D, cw) for D, _, cw, _ in runs]
    per_step = [critic_lds(D, cw) for D, spec, cw, f in runs if spec[0] == "gru" or not f]
    bootstrap = [critic_lds(D, cw) for D, spec, cw, f in runs if spec[0] == "mlp" and f]
    alone = [critic_lds(obs[2], widths) for obs in OBS for widths in S.VALUE_TRUNKS]
    assert len(per_step) + len(bootstrap) == len(runs)
    for sizes in (per_step, bootstrap, alone):
        assert max(sizes) > LDS_ATTR and min(sizes) <= LDS_ATTR
    batch = per_step + bootstrap + alone
    for name, sizes in (("policy_mfma_critic_kernel", fused), ("critic_mfma_term_kernel", term), ("critic_mfma_kernel", batch)):
        assert max(sizes) > LDS_ATTR and min(sizes) <= LDS_ATTR, name       # both sides of the host's branch
        assert max(sizes) <= 160 * 1024, name
    # the gather test and the captured rollout have one each
    assert any(critic_lds(18, cw) > LDS_ATTR for cw in S.GATHER_CRITICS)
    assert any(critic_lds(18, cw) > LDS_ATTR for _, cw, _ in S.GRAPH_PAIRS)
    # in_dim sizes the critic kernels' LDS too: D = 108 with every width at most 96
    assert any(D == 108 and max(cw) <= 96 and critic_lds(D, cw) == 1024 + 256 * 108 for D, _, cw, _ in runs)
    assert OBS[-1][2] == 108 and any(max(w) <= 96 and critic_lds(108, w) == 1024 + 256 * 108 for w in S.VALUE_TRUNKS)


def test_all_activation_mixes_with_both_output_tanh_settings():
    mixes = {(_style(k)[0], cact, _style(k)[1]) for k in S.MIX_STYLES for cact in ACTS}
    assert mixes == {(a, c, t) for a in ACTS for c in ACTS for t in (True, False)}
    # the rotated pairs of the rollouts mix them too: at every width, for MLP and GRU actors, some pairs share an activation and some
    # do not, and over the file all four combinations occur for both kinds
    for kind in ("mlp", "gru"):
        seen = set()
        for obs, _ in S.CASES:
            here = {(_style(k)[0], ACTS[kc % 2]) for _, k, _, kc in S._pairs(kind, obs[2])}
            assert any(a == c for a, c in here) and any(a != c for a, c in here), (kind, obs[2])
            seen |= here
        assert seen == {(a, c) for a in ACTS for c in ACTS}, kind


def test_every_last_width_and_every_gru_h():
    last, hs, actors = set(), set(), set()
    for obs, _ in S.CASES:
        for kind in ("mlp", "gru"):
            pairs = S._pairs(kind, obs[2])
            assert len(pairs) in (3, 4)
            last |= {cw[-1] for _, _, cw, _ in pairs}
            hs |= {spec[1] for spec, _, _, _ in pairs if spec[0] == "gru"}
            actors |= {tuple(spec[1]) for spec, _, _, _ in pairs if spec[0] == "mlp"}
    assert last == {16, 48, 80, 144, 240, 256}
    assert hs == {48, 80, 240}
    assert len(actors) == 6                                         # every MLP net of tests/test_gpu_policy_ac_shapes.py
    tables = [repr([(spec, cw) for spec, _, cw, _ in S._pairs("mlp", obs[2])]) for obs in OBS]
    assert len(set(tables)) == len(OBS)                             # no two widths share a table
    assert ("mlp", [256, 256, 256]) in [spec for spec, _, _, _ in S._pairs("mlp", 108)]       # in_dim = 108 under the widest actor
    assert [48, 256, 16] in S.CRITICS and [48, 256, 16] in S.VALUE_TRUNKS      # narrow after wide
    assert {w[-1] for w in S.VALUE_TRUNKS} >= {16, 144, 80, 256} and len(OBS) == 11
    assert S.ROWS == (1, 63, 64, 65, 130)
    assert len(S.CASES) == 13 and [_batches(0)[j] for j in range(4)] == [4, 64, 68, 2096]


def test_the_other_trunks_activation_misses_fp64_by_far_more_than_the_bar():
    """the inputs of the mixed cases are the env's observations with _obs_scale folded into the first layer: rows of at most unit RMS
    per input.  The env's rows need the device; unit-variance rows of the same widths and counts stand in for them here (the device
    test itself holds V to fp64 on the real rows): the same weights with the other activation give another V altogether."""
    for name, obs, _, cw in S.MIX:
        D = obs[2]
        x = np.random.RandomState(D).randn(_batches(obs[1])[2] * (T + 1), D)
        for k in S.MIX_STYLES:
            nets = [_CNet(cw, np.ones(D), 40 + k, D, act) for act in ACTS]
            assert [n.act for n in nets] == ACTS
            for a, b in zip(nets[0].layers, nets[1].layers):        # the same weights
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            diff = np.abs(nets[0].ref64(x, name) - nets[1].ref64(x, name))
            assert float(np.mean(diff > 100 * ATOL_FP32)) > 0.9, (name, k, float(np.median(diff)))
            assert float(np.median(diff)) > 1000 * ATOL_FP32, (name, k, float(np.median(diff)))
