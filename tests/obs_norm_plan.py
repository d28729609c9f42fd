"""The observation normaliser's update (gaq_learn.hip: gaq_obs_norm_update_dev, obs_norm_partial_kernel, obs_norm_merge_kernel) restated
in numpy: the host's split of a batch into workgroups and tiles (plan), the device's order of fp64 operations (emulate_update), the batch
sizes at which the kernels take another path (cap_shapes, chunk_shapes, align_shapes), the data those sizes are fed (data) and the bars
of the running merge (merge_bars, steps_bars).  tests/test_obs_norm_plan_cpu.py proves from plan what each size reaches and runs the
emulation against the bars without a GPU; tests/test_gpu_obs_norm_sizes.py runs the same sizes on the device.

emulate_update is NOT expected to equal the device bit for bit: the device computes q += d d as one fma, and the compiler may contract
other expressions (sq - sum * sum / cnt, a.mean + delta * (b.n / n)) where numpy rounds twice.  It has the device's ORDER -- which rows a
thread sums, in which sequence the partials merge -- so its distance from a two-pass reference is what the algorithm as written costs, and
its MUTANTS are what a wrong index or a wrong carry would cost."""
import collections

import numpy as np

BLOCK = 256                  # kObsNormBlock
TILE = 8192                  # kObsNormTile
MAX_BLOCKS = 1024            # kObsNormMaxBlocks
U64 = 2.0 ** -52

Plan = collections.namedtuple("Plan", "tile_rows nb0 rpb nb tiles G chunk empty_groups")
Tile = collections.namedtuple("Tile", "t0 tr a lead nq tail")
MUTANTS = ["stale_a", "cnt_reset", "drop_last"]


def plan(rows, D, base_float_offset=0):
    """The split gaq_obs_norm_update_dev makes of `rows` rows of width D whose first float sits `base_float_offset` floats past a 16-byte
    boundary.  tiles[b] lists workgroup b's tiles (t0, tr, a, lead, nq, tail): first row, rows, the tile's offset mod 4 in floats (the
    kernel's `a`), the floats loaded singly before the first 16-byte boundary, the float4 loads, the floats loaded singly after them.
    G = 256 / D row groups; the merge kernel gives row group g the partials [g chunk, min((g + 1) chunk, nb)); empty_groups counts the row
    groups whose run is empty."""
    tile_rows = TILE // D
    want = -(-rows // tile_rows)
    nb0 = min(want, MAX_BLOCKS)
    rpb = -(-rows // nb0)
    nb = -(-rows // rpb)
    tiles = []
    for b in range(nb):
        r0, r1 = b * rpb, min((b + 1) * rpb, rows)
        mine = []
        for t0 in range(r0, r1, tile_rows):
            tr = min(r1 - t0, tile_rows)
            n = tr * D
            a = (base_float_offset + t0 * D) & 3
            lead = min((4 - a) & 3, n)
            nq = (n - lead) >> 2
            mine.append(Tile(t0, tr, a, lead, nq, n - lead - 4 * nq))
        tiles.append(mine)
    G = BLOCK // D
    chunk = -(-nb // G)
    return Plan(tile_rows, nb0, rpb, nb, tiles, G, chunk, sum(1 for g in range(G) if g * chunk >= nb))


# ---- the batch sizes of tests/test_gpu_obs_norm_sizes.py (what each reaches is asserted in tests/test_obs_norm_plan_cpu.py) -----------
def cap(D):
    """the largest batch every workgroup of which still holds one tile: 1024 tile_rows rows, about 32 MiB at every width"""
    return MAX_BLOCKS * (TILE // D)


def two_tiles(D):
    return cap(D) + 1                      # rpb = tile_rows + 1: a second tile of ONE row in every workgroup, nb < 1024


def two_tiles_full(D):
    return cap(D) + MAX_BLOCKS             # the same rpb and nb == 1024: no workgroup is short


def three_tiles(D):
    return 2 * cap(D) + 1                  # rpb = 2 tile_rows + 1: tiles of tile_rows, tile_rows and one row, about 64 MiB


def chunk_two(D):
    return (BLOCK // D) * (TILE // D) + 1  # G + 1 single-tile workgroups: chunk = 2 and trailing row groups without a partial


FULL_WIDTHS = [13, 108]
THREE_WIDTHS = [13, 25]                    # the only widths that run 64 MiB
CHUNK_WIDTHS = [13, 18, 25, 60]
ALIGN_WIDTHS = [13, 19, 25]


def cap_shapes(widths):
    """(D, rows) of case a: every width with two tiles, the full cap at FULL_WIDTHS, three tiles at THREE_WIDTHS"""
    return [(D, two_tiles(D)) for D in widths] + [(D, two_tiles_full(D)) for D in FULL_WIDTHS] + [(D, three_tiles(D)) for D in THREE_WIDTHS]


def chunk_shapes():
    """(D, rows) of case b"""
    return [(D, chunk_two(D)) for D in CHUNK_WIDTHS] + [(13, cap(13))]


def align_shapes():
    """(D, rows) of case c's large batches: the shapes of case a at ALIGN_WIDTHS (three tiles where case a runs them)"""
    return [(D, f(D)) for D in ALIGN_WIDTHS for f in (two_tiles, two_tiles_full)] + [(D, three_tiles(D)) for D in THREE_WIDTHS]


RAMP_COL, OUTLIER_COL, OUTLIER = 0, 3, 1e6


def data(D, rows, outlier=False):
    """fp32 rows [rows, D] with the columns of test_gpu_obs_norm._stat_data -- per-column scales 1 + k % 4, column 1 of mean 1e3 and
    spread 1e-2, column 2 constant 1.5 -- plus a ramp from 0 to 4 over the rows in column 0 (a tile summed twice, or in another tile's
    place, moves that column's mean by a multiple of (4 tile_rows / rows) (tile_rows / rows): 4e-6 at the cap of D = 13, where the bar
    is 1e-8), and with outlier=True 1e6 in row 0 of column 3: row 0 is the shift K, so every other d of that column is about -1e6 and
    q - s^2 / n cancels twelve digits -- the shifted sum's worst case."""
    rng = np.random.default_rng(D * 10007 + rows % 99991)
    x = rng.standard_normal((rows, D), dtype=np.float32)
    x *= (1.0 + np.arange(D) % 4).astype(np.float32)
    x[:, RAMP_COL] += (4.0 * np.arange(rows) / max(rows - 1, 1)).astype(np.float32)
    x[:, 1] = 1e3 + 1e-2 * rng.standard_normal(rows)
    x[:, 2] = 1.5
    if outlier:
        x[0, OUTLIER_COL] = OUTLIER
    return x


# ---- the device's order -----------------------------------------------------------------------------------------------------------------
def _merge(a, b):
    """obs_moments_merge on arrays of moments (n, mean, M2), element by element, with its two early returns"""
    (na, ma, sa), (nb, mb, sb) = a, b
    n = na + nb
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = mb - ma
        mean = ma + delta * (nb / n)
        m2 = sa + sb + delta * delta * (na * nb / n)
    ra, rb = nb == 0, (na == 0) & (nb != 0)
    pick = lambda va, vb, v: np.where(ra, va, np.where(rb, vb, v))
    return pick(na, nb, n), pick(ma, mb, mean), pick(sa, sb, m2)


def _columns(m):
    """obs_moments_column: moments [..., G, D] -> [..., D], merged in ascending row group"""
    acc = tuple(np.zeros_like(v[..., 0, :]) for v in m)
    for g in range(m[0].shape[-2]):
        acc = _merge(acc, tuple(v[..., g, :] for v in m))
    return acc


def emulate_update(x, state, base_float_offset=0, mutant=None):
    """(count, mean [D], M2 [D]) in float64 after gaq_obs_norm_update_dev of the fp32 rows x [rows, D] on the running state
    `state` = (count, mean, M2), in the device's order.  obs_norm_partial_kernel: workgroup b copies each of its tiles into a buffer of
    8192 + 4 floats at the tile's offset a and thread (g, c) adds d = x - K (K = row 0 of the batch), d d and 1 over the tile's rows
    g, g + G, ..., carried from tile to tile; its shifted moments (cnt, s / cnt, max(q - s s / cnt, 0)) merge per column in ascending g.
    obs_norm_merge_kernel: thread (g, c) merges its run of `chunk` partials in ascending b, the columns merge in ascending g, K is added to
    the mean, and the batch merges into the state.
    Not bit-exact with the device (the module's docstring): q + d d is an fma there, and the compiler may contract other expressions.
    mutant -- "stale_a": every tile after a workgroup's first is read at the first tile's a (the offset computed once, not per tile);
    "cnt_reset": cnt starts at 0 in every tile while sum and sq carry; "drop_last": the merge kernel's run of a row group stops one
    partial early where it holds more than one."""
    x = np.ascontiguousarray(x, np.float32)
    rows, D = x.shape
    p = plan(rows, D, base_float_offset)
    G = p.G
    K = x[0].astype(np.float64)
    flat = x.reshape(-1)
    tile = np.zeros(TILE + 4, np.float32)
    gi, ci = np.arange(G)[None, :, None], np.arange(D)[None, None, :]
    cnt, s, q = (np.zeros((p.nb, G, D)) for _ in range(3))
    for b, tiles in enumerate(p.tiles):
        sb, qb, cb = np.zeros((1, G, D)), np.zeros((1, G, D)), np.zeros((G, D))
        for k, t in enumerate(tiles):
            tile[t.a:t.a + t.tr * D] = flat[t.t0 * D:(t.t0 + t.tr) * D]
            a = tiles[0].a if (mutant == "stale_a" and k > 0) else t.a
            r = np.arange(-(-t.tr // G))[:, None, None] * G + gi                # [steps, G, 1]: the row a thread reads in each step
            valid = np.broadcast_to(r < t.tr, r.shape[:2] + (D,))
            d = np.where(valid, tile[np.minimum(a + r * D + ci, TILE + 3)].astype(np.float64) - K, 0.0)
            sb = np.add.accumulate(np.concatenate([sb, d]), axis=0)[-1:]        # in sequence; + 0.0 where a thread has no row
            qb = np.add.accumulate(np.concatenate([qb, d * d]), axis=0)[-1:]
            cb = (0.0 if mutant == "cnt_reset" else cb) + valid.sum(axis=0)
        cnt[b], s[b], q[b] = cb, sb[0], qb[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        some = cnt > 0
        mine = (cnt, np.where(some, s / cnt, 0.0), np.where(some, np.maximum(q - s * s / cnt, 0.0), 0.0))
    part = _columns(mine)                                                       # [nb, D]: part[b][c]
    b = np.arange(G)[:, None] * p.chunk + np.arange(p.chunk)[None, :]           # [G, chunk]: the partial row group g merges j-th
    b1 = np.minimum((np.arange(G)[:, None] + 1) * p.chunk, p.nb)
    if mutant == "drop_last":
        b1 = np.where(b1 - np.arange(G)[:, None] * p.chunk > 1, b1 - 1, b1)
    taken = b < b1
    run = tuple(np.where(taken[:, :, None], v[np.minimum(b, p.nb - 1)], 0.0) for v in part)      # [G, chunk, D]; n = 0: merged as nothing
    mine = tuple(np.zeros((G, D)) for _ in range(3))
    for j in range(p.chunk):
        mine = _merge(mine, tuple(v[:, j, :] for v in run))
    n, mean, m2 = _columns(mine)
    mean = mean + K
    count, smean, sm2 = state
    n, mean, m2 = _merge((np.full(D, float(count)), np.asarray(smean, np.float64), np.asarray(sm2, np.float64)), (n, mean, m2))
    assert np.all(n == n[0])
    return float(n[0]), mean, m2


# ---- bars of the running merge ------------------------------------------------------------------------------------------------------------
def merge_bars(state, batch, batch_bars):
    """Bars for (mean, M2) after ONE update of a state (na, mean_a, M2_a) with a batch whose two-pass moments are `batch` =
    (nb, mean_b, M2_b), against obs_norm_ref.chan_merge(state, batch) in fp64.  The device evaluates the same three expressions on ITS
    batch moments, which are off by at most batch_bars = _stat_bars(x) = (e_mean, e_M2):
      mean = mean_a + delta (nb / n), delta = mean_b - mean_a: four roundings (delta, nb / n, the product, the sum), each relative to a
        quantity <= 2 max(|mean_a|, |mean_b|), on each side of the comparison, contracted or not: 8 u max(|mean_a|, |mean_b|) is taken,
        plus e_mean (nb / n <= 1 scales the batch's own error down, never up);
      M2 = M2_a + M2_b + delta^2 (na nb / n): six roundings relative to the sum S of the three non-negative terms on each side: 8 u S is
        taken, plus e_M2, plus what e_mean does to the last term, 2 |delta| (na nb / n) e_mean (first order: e_mean << |delta| or the
        term is negligible against e_M2).
    With na = 0 the result IS the batch (the stored mean and M2 are not read): the batch's bars alone.  u = 2^-52."""
    (na, ma, sa), (nb, mb, sb) = state, batch
    e_mean, e_m2 = batch_bars
    if na == 0:
        return e_mean, e_m2
    ma, sa = np.asarray(ma, np.float64), np.asarray(sa, np.float64)
    w = na * nb / (na + nb)
    delta = np.abs(mb - ma)
    return (e_mean + 8 * U64 * np.maximum(np.abs(ma), np.abs(mb)),
            e_m2 + 8 * U64 * (sa + sb + delta * delta * w) + 2 * delta * w * e_mean)


def steps_bars(x, updates):
    """Bars for (mean, M2) after `updates` successive updates whose batches concatenate to x [n, D], from an empty state, against ONE
    two-pass over x.  _stat_bars counts 8 u per ADDED TERM relative to max|x| (mean) and to n range^2 (M2); every running merge adds the
    roundings of merge_bars, 8 u, relative to quantities with the same bounds (every running mean lies within the data's range, every
    running M2 and every delta^2 na nb / n is at most n range^2): 8 (n + updates) u times those bounds."""
    n = x.shape[0]
    x64 = np.asarray(x, np.float64)
    rng_ = x64.max(axis=0) - x64.min(axis=0)
    f = 8 * (n + updates) * U64
    return f * np.abs(x64).max(axis=0), f * n * rng_ ** 2


def frac(err, bar):
    """the worst err / bar over the entries with a bar > 0 (an entry with bar 0 has to be exact, which err <= bar asserts)"""
    pos = bar > 0
    return float((err[pos] / bar[pos]).max()) if pos.any() else 0.0
