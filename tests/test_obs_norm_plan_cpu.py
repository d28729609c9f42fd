"""The batch sizes of tests/test_gpu_obs_norm_sizes.py without a GPU (tests/obs_norm_plan.py): that each size reaches the path its GPU
test names -- proved from the restated split, not assumed --, that the device's order of operations (the numpy emulation) stays inside
the bars the GPU tests use at those sizes while three wrong orders do not, that the two-pass fp64 reference is itself far inside the
bars against np.longdouble, that the bars of the running merge hold against an np.longdouble merge, and that every bar still rejects an
fp32 accumulation by a factor of 100."""
import numpy as np
import pytest

from tests import obs_norm_plan as P
from tests import obs_norm_ref as R
from tests.test_gpu_obs_norm import _stat_bars, _stat_data

EMPTY = lambda D: (0.0, np.zeros(D), np.zeros(D))
CAP_SHAPES = P.cap_shapes(R.WIDTHS)
_ids = lambda shapes: ["d%d-%d" % s for s in shapes]


def _tiles_per_block(p):
    return sorted({len(t) for t in p.tiles})


def _starts(p):
    return {t.a for tiles in p.tiles for t in tiles}


# ---- 1. what each size reaches ----------------------------------------------------------------------------------------------------------
def test_split_matches_the_figures_of_the_existing_sizes():
    """the sizes tests/test_gpu_obs_norm.py runs never iterate the tile loop twice and, below G tile_rows + 1 rows (every size at D <= 20,
    all but 4097 rows from D = 22 on), never merge two partials in one run"""
    for D in R.WIDTHS:
        for rows in (1, 2, 63, 64, 65, 4097):
            p = P.plan(rows, D)
            assert _tiles_per_block(p) == [1] and p.nb == p.nb0 and p.rpb <= p.tile_rows
            assert sum(t.tr for tiles in p.tiles for t in tiles) == rows
            if rows < P.chunk_two(D):
                assert p.chunk == 1
        assert (P.chunk_two(D) > 4097) == (D <= 20)
    assert [P.cap(D) + 1 for D in (13, 18, 108)] == [645121, 465921, 76801]
    assert [P.chunk_two(D) for D in (13, 18, 25)] == [11971, 6371, 3271]


@pytest.mark.parametrize("D", R.WIDTHS)
def test_two_tiles_reach_the_loop_and_a_short_launch(D):
    """rows = 1024 tile_rows + 1: every workgroup runs the tile loop twice, its second tile is ONE row, and the launch has fewer
    workgroups than the plan first asked for (nb < nb0 = 1024); about 32 MiB"""
    rows = P.two_tiles(D)
    p = P.plan(rows, D)
    assert p.nb0 == P.MAX_BLOCKS and p.rpb == p.tile_rows + 1 and p.nb < p.nb0
    assert all([t.tr for t in tiles] == [p.tile_rows, 1] for tiles in p.tiles[:-1])
    last = p.tiles[-1]
    assert 1 <= sum(t.tr for t in last) <= p.tile_rows and len(last) == 1                   # the short workgroup: one partial tile
    assert sum(t.tr for tiles in p.tiles for t in tiles) == rows and 31 * 2 ** 20 < rows * D * 4 < 33 * 2 ** 20
    assert p.chunk > 1 and all(t.lead + 4 * t.nq + t.tail == t.tr * D and t.tail < 4 for tiles in p.tiles for t in tiles)


@pytest.mark.parametrize("D", P.FULL_WIDTHS)
def test_full_cap_has_no_short_workgroup(D):
    p = P.plan(P.two_tiles_full(D), D)
    assert p.nb == p.nb0 == P.MAX_BLOCKS and all([t.tr for t in tiles] == [p.tile_rows, 1] for tiles in p.tiles)


@pytest.mark.parametrize("D", P.THREE_WIDTHS)
def test_three_tiles_take_every_alignment(D):
    """rows = 2 x 1024 tile_rows + 1: tiles of tile_rows, tile_rows and one row, and the tile starts of ONE launch take all four
    offsets a -- hence lead = 0, 3, 2, 1 -- whatever the base's own offset; about 64 MiB"""
    rows = P.three_tiles(D)
    for off in range(4):
        p = P.plan(rows, D, off)
        assert all([t.tr for t in tiles] == [p.tile_rows, p.tile_rows, 1] for tiles in p.tiles[:-1])
        assert _starts(p) == {0, 1, 2, 3}
        assert {t.lead for tiles in p.tiles for t in tiles if t.tr > 1} == {0, 1, 2, 3}
        assert {t.a for tiles in p.tiles for t in tiles[1:]} == {0, 1, 2, 3}                 # ... among the tiles after the first, too
    assert 63 * 2 ** 20 < rows * D * 4 < 65 * 2 ** 20


def test_chunk_two_shapes_leave_row_groups_empty():
    """rows = G tile_rows + 1: single-tile workgroups, more of them than row groups, so chunk = 2, the leading row groups merge TWO
    partials and the trailing ones none; rows = 1024 tile_rows at D = 13: the full cap in one tile each, chunk = 54"""
    for D in P.CHUNK_WIDTHS:
        p = P.plan(P.chunk_two(D), D)
        assert _tiles_per_block(p) == [1] and p.G < p.nb <= 2 * p.G and p.chunk == 2
        runs = [min(2 * (g + 1), p.nb) - min(2 * g, p.nb) for g in range(p.G)]
        assert runs[0] == 2 and runs == sorted(runs, reverse=True) and sum(runs) == p.nb
        assert p.empty_groups == runs.count(0) >= 1
    p = P.plan(P.cap(13), 13)
    assert p.nb == p.nb0 == P.MAX_BLOCKS and _tiles_per_block(p) == [1] and p.rpb == p.tile_rows and p.chunk == 54
    assert p.empty_groups == 0 and p.nb - (p.G - 1) * p.chunk == 52                          # the last row group's run is shorter


def test_small_sizes_take_every_alignment():
    """rows = 1, 2 and 65 at the four base offsets: a = the offset, lead = (4 - a) & 3 cut to the row at rows = 1; offsets 2 and 3 are the
    ones no earlier test takes.  The large batches of case c are the shapes of case a at D = 13, 19 and 25."""
    for D in R.WIDTHS:
        for rows in (1, 2, 65):
            for off in range(4):
                p = P.plan(rows, D, off)
                (t,) = p.tiles[0]
                assert p.nb == 1 and (t.a, t.lead) == (off, min((4 - off) & 3, rows * D)) and t.lead + 4 * t.nq + t.tail == rows * D
    assert set(P.align_shapes()) <= set(P.cap_shapes(P.ALIGN_WIDTHS)) | {(D, P.two_tiles_full(D)) for D in P.ALIGN_WIDTHS}
    assert {D for D, rows in P.align_shapes() if rows == P.three_tiles(D)} == set(P.THREE_WIDTHS)


# ---- 2. the emulation inside the bars, the mutants outside ------------------------------------------------------------------------------
def _inside(got, ref, bars):
    (n, mean, m2), (n_ref, mean_ref, m2_ref) = got, ref
    em, e2 = np.abs(mean - mean_ref), np.abs(m2 - m2_ref)
    return n == n_ref, bool(np.all(em <= bars[0]) and np.all(e2 <= bars[1])), max(P.frac(em, bars[0]), P.frac(e2, bars[1]))


@pytest.mark.parametrize("D,rows", CAP_SHAPES, ids=_ids(CAP_SHAPES))
def test_emulation_inside_the_bars_mutants_outside(D, rows):
    """At every size of case a, on the data of the GPU test (plain, and with the outlier in row 0): the device's order of operations
    is inside _stat_bars with the exact count and an exact constant column.  The three mutants (obs_norm_plan.MUTANTS) are not:
    "cnt_reset" and "drop_last" give another count; "stale_a" leaves the bars wherever some workgroup's later tile starts at another
    offset than its first (tile_rows D % 4 != 0: D = 13, 14, 18, 19 and 25) -- at the other widths a full tile is a whole number of
    16-byte units, every tile of a workgroup has the same a and the mutant IS the kernel, which the plan shows and the test states."""
    x = P.data(D, rows)
    for outlier in (False, True):
        if outlier:
            x[0, P.OUTLIER_COL] = P.OUTLIER
        ref, bars = R.moments(x), _stat_bars(x)
        got = P.emulate_update(x, EMPTY(D))
        count_ok, ok, worst = _inside(got, ref, bars)
        print("d=%d rows=%d outlier=%d: emulation error / bar %.3g" % (D, rows, outlier, worst))
        assert count_ok and ok and got[2][2] == 0.0 and got[1][2] == 1.5
    p = P.plan(rows, D)
    moves = any(t.a != tiles[0].a for tiles in p.tiles for t in tiles[1:])
    assert moves == (p.tile_rows * D % 4 != 0) == (D in (13, 14, 18, 19, 25))
    for mutant in P.MUTANTS:
        bad = P.emulate_update(x, EMPTY(D), mutant=mutant)
        count_ok, ok, worst = _inside(bad, ref, bars)
        print("   %s: count %s, error / bar %.3g" % (mutant, "exact" if count_ok else "WRONG", worst))
        if mutant == "stale_a":
            assert count_ok and ok == (not moves)
            assert moves or all(np.array_equal(u, v) for u, v in zip(bad[1:], got[1:]))
        else:
            assert not count_ok


@pytest.mark.parametrize("D,rows", P.chunk_shapes(), ids=_ids(P.chunk_shapes()))
def test_emulation_inside_the_bars_at_chunk_two(D, rows):
    """case b: inside the bars; a merge that drops the last partial of a run of two loses rows (the count); a merge that read the
    trailing row groups' missing partials would have nothing to read them from (the emulation pads them with n = 0)"""
    x = P.data(D, rows)
    ref, bars = R.moments(x), _stat_bars(x)
    count_ok, ok, _ = _inside(P.emulate_update(x, EMPTY(D)), ref, bars)
    assert count_ok and ok
    assert P.emulate_update(x, EMPTY(D), mutant="drop_last")[0] < ref[0]


def test_emulation_does_not_depend_on_the_base_offset():
    """nothing in the order depends on the pointer: the emulation gives the same bits at the four offsets (what case c asserts of the
    device)"""
    for D, rows in [(13, P.chunk_two(13)), (19, 65), (25, 2)]:
        x = P.data(D, rows)
        runs = [P.emulate_update(x, EMPTY(D), off) for off in range(4)]
        assert all(np.array_equal(r[k], runs[0][k]) for r in runs for k in (1, 2))


# ---- 3. the reference is not what the bars measure -------------------------------------------------------------------------------------
def _moments_ld(x):
    """two-pass moments in np.longdouble, a column at a time"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here: it is no yardstick for fp64"
    mean, m2 = np.zeros(x.shape[1], np.longdouble), np.zeros(x.shape[1], np.longdouble)
    for c in range(x.shape[1]):
        col = x[:, c].astype(np.longdouble)
        mean[c] = col.sum() / np.longdouble(col.size)
        m2[c] = ((col - mean[c]) ** 2).sum()
    return np.longdouble(x.shape[0]), mean, m2


LD_FRACTION = 1e-3


@pytest.mark.parametrize("outlier", [False, True])
def test_reference_against_longdouble_at_the_largest_size(outlier):
    """R.moments (numpy's pairwise fp64 sums) at the largest batch, 2 x 1024 x 630 + 1 rows of 13, against a two-pass in np.longdouble
    (64 bits of mantissa): within LD_FRACTION = 1e-3 of the bars, so the bars measure the device and not the reference"""
    D = 13
    x = P.data(D, P.three_tiles(D), outlier)
    _, mean, m2 = R.moments(x)
    _, mean_ld, m2_ld = _moments_ld(x)
    bars = _stat_bars(x)
    em, e2 = np.abs(mean - mean_ld).astype(np.float64), np.abs(m2 - m2_ld).astype(np.float64)
    print("reference error / bar: mean %.3g, M2 %.3g" % (P.frac(em, bars[0]), P.frac(e2, bars[1])))
    assert np.all(em <= LD_FRACTION * bars[0]) and np.all(e2 <= LD_FRACTION * bars[1])


# ---- 4. the running merge ------------------------------------------------------------------------------------------------------------------
def merge_cases(D):
    """case d's (name, state, batch): the state as (count, mean, M2); tests/test_gpu_obs_norm_sizes.py loads the same"""
    mean, var = R.case_stats(D)
    pinned = mean.copy()
    pinned[2] = 1.5                                        # the constant column: the state agrees with the batch and holds M2 = 0
    m2 = lambda count: np.where(np.arange(D) == 2, 0.0, var * count)
    return [("1e12+1", (1e12, pinned, m2(1e12)), _stat_data(D, 1)[0]),
            ("1+4097", (1.0, pinned, m2(1.0)), _stat_data(D, 4097)[0]),
            ("1e-4+65", (1e-4, np.zeros(D), np.full(D, 1e-4)), _stat_data(D, 65)[0]),
            ("0(mean 7)+65", (0.0, np.full(D, 7.0), np.full(D, 3.0)), _stat_data(D, 65)[0]),
            ("far+4097", (4097.0, np.full(D, 1e3), np.full(D, 4097.0)), R.stand_in_obs(4097, D))]


def _merge_ld(state, x):
    (na, ma, sa), (nb, mb, sb) = state, _moments_ld(x)
    if na == 0:
        return nb, mb, sb
    na, ma, sa = np.longdouble(na), np.asarray(ma, np.longdouble), np.asarray(sa, np.longdouble)
    n = na + nb
    delta = mb - ma
    return n, ma + delta * (nb / n), sa + sb + delta * delta * (na * nb / n)


@pytest.mark.parametrize("D", R.WIDTHS)
def test_merge_bars_against_a_longdouble_merge(D):
    """merge_bars on every pair of case d: the fp64 reference the GPU test compares with (R.chan_merge of R.moments) is within
    HALF the bars of a merge in np.longdouble -- the bars are a handful of fp64 roundings on each side of the comparison, and the
    reference is one side --, and the emulation of the device's order is within the bars of that reference.  The count is the same fp64
    sum on both sides.  The stored mean of a state with count 0 has no effect."""
    for name, state, x in merge_cases(D):
        batch = R.moments(x)
        bars = P.merge_bars(state, batch, _stat_bars(x))
        ref = R.chan_merge(state, batch)
        ld = _merge_ld(state, x)
        em, e2 = np.abs(ref[1] - ld[1]).astype(np.float64), np.abs(ref[2] - ld[2]).astype(np.float64)
        assert np.all(em <= 0.5 * bars[0]) and np.all(e2 <= 0.5 * bars[1]), name
        got = P.emulate_update(x, state)
        count_ok, ok, worst = _inside(got, ref, bars)
        print("d=%d %s: emulation error / bar %.3g, reference error / bar %.3g" % (D, name, worst, max(P.frac(em, bars[0]), P.frac(e2, bars[1]))))
        assert count_ok and ok, (name, worst)
        assert got[0] == state[0] + x.shape[0]
        if name.startswith("0("):
            other = P.emulate_update(x, (0.0, np.full(D, -3.0), np.zeros(D)))
            assert all(np.array_equal(u, v) for u, v in zip(got[1:], other[1:])) and np.array_equal(got[1], P.emulate_update(x, EMPTY(D))[1])
        elif state[2][2] == 0.0 and np.all(x[:, 2] == 1.5):
            assert got[2][2] == 0.0 and got[1][2] == 1.5


@pytest.mark.parametrize("D", [13, 18, 108])
def test_forty_updates_inside_steps_bars(D):
    """40 successive updates of 63 rows in the device's order against one two-pass over the 2520 rows"""
    x = _stat_data(D, 40 * 63)[0]
    state = EMPTY(D)
    for k in range(40):
        state = P.emulate_update(x[63 * k:63 * (k + 1)], state, (63 * k * D) & 3)
    count_ok, ok, worst = _inside(state, R.moments(x), P.steps_bars(x, 40))
    assert count_ok and ok and state[2][2] == 0.0 and state[1][2] == 1.5, worst


# ---- 5. every bar still rejects an fp32 accumulation ---------------------------------------------------------------------------------------
def _fp32_moments(col):
    """(mean, M2) of a column accumulated in sequence in fp32: sum x and sum x^2, unshifted"""
    s32 = np.add.accumulate(col, dtype=np.float32)[-1]
    q32 = np.add.accumulate(col * col, dtype=np.float32)[-1]
    n = np.float32(col.size)
    mean32 = np.float32(s32 / n)
    return mean32, np.float32(q32 - n * mean32 * mean32)


def test_bars_reject_an_fp32_accumulation():
    """the 1e3 +- 1e-2 column summed in fp32 misses _stat_bars at the capped size of D = 13, merge_bars on the 1 + 4097 pair and
    steps_bars on the 40 x 63 rows, each by more than the factor of 100 tests/test_gpu_obs_norm.py demands"""
    D = 13
    col = P.data(D, P.two_tiles(D))[:, 1]
    mean32, m2_32 = _fp32_moments(col)
    _, mref, m2ref = R.moments(col[:, None])
    bm, b2 = _stat_bars(col[:, None])
    print("capped: fp32 accumulation / bar: mean %.3g, M2 %.3g" % (abs(mean32 - mref[0]) / bm[0], abs(m2_32 - m2ref[0]) / b2[0]))
    assert abs(mean32 - mref[0]) > 100 * bm[0] and abs(m2_32 - m2ref[0]) > 100 * b2[0]
    name, state, x = merge_cases(D)[1]
    col = x[:, 1:2]
    state = (state[0], state[1][1:2], state[2][1:2])
    batch = R.moments(col)
    bm, b2 = P.merge_bars(state, batch, _stat_bars(col))
    mean32, m2_32 = _fp32_moments(col[:, 0])
    ref = R.chan_merge(state, batch)
    bad = R.chan_merge(state, (batch[0], np.array([mean32], np.float64), np.array([m2_32], np.float64)))
    assert abs(bad[1][0] - ref[1][0]) > 100 * bm[0] and abs(bad[2][0] - ref[2][0]) > 100 * b2[0], name
    col = _stat_data(D, 40 * 63)[0][:, 1]
    mean32, m2_32 = _fp32_moments(col)
    _, mref, m2ref = R.moments(col[:, None])
    bm, b2 = P.steps_bars(col[:, None], 40)
    assert abs(mean32 - mref[0]) > 100 * bm[0] and abs(m2_32 - m2ref[0]) > 100 * b2[0]
