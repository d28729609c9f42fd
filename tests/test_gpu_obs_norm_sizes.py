"""The observation normaliser's update (gaq.h gaq_obs_norm_update_dev; obs_norm_partial_kernel, obs_norm_merge_kernel, and
obs_norm_apply_kernel for the offsets) at the batch sizes a training rollout feeds it, where the kernels take paths the sizes of
tests/test_gpu_obs_norm.py never reach.  What each size reaches is proved from the restated split in tests/test_obs_norm_plan_cpu.py
(tests/obs_norm_plan.py), which also shows without a GPU that the device's order of operations stays inside every bar used here.

a. the cap and the tile loop: rows = 1024 tile_rows + 1 at every width (two tiles per workgroup, the second ONE row, nb < 1024; about
   32 MiB), + 1024 at D = 13 and 108 (nb == 1024), 2 x 1024 tile_rows + 1 at D = 13 and 25 (three tiles, all four offsets a among the
   tile starts of one launch; about 64 MiB); plain data and with an outlier of 1e6 in row 0, the shift.
b. chunk > 1 in the merge at small widths: rows = (256 / D) tile_rows + 1 at D = 13, 18, 25 and 60 (chunk = 2, trailing row groups with
   no partial) and rows = 1024 tile_rows at D = 13 (full cap, one tile each, chunk = 54).
c. the four offsets 0, 4, 8, 12 bytes past a 16-byte boundary: the shapes of a at D = 13, 19 and 25 (three tiles at 13 and 25 only: the
   64 MiB batches stay at the two widths of a) and rows = 1, 2, 65 at every width: state and table BIT-IDENTICAL across the offsets;
   normalize_dev with its input and its output at each offset, rows = 1, 65, 130, bit for bit the element expression.
d. the running merge: a state loaded with load_state_dict, one update_dev, against obs_norm_ref.chan_merge(state, moments(batch)):
   count 1e12 + one row; count 1 + 4097 rows; the rl_games start (count 1e-4, mean 0, var 1) + 65 rows; count 0 with a stored mean of 7
   and M2 of 3 (neither may have any effect) + 65 rows; a state of mean 1e3 + a batch of mean 0 (delta^2 na nb / n is all of M2); and 40
   successive updates of 63 rows, each a view at its own offset, against one two-pass over the 2520 rows.
e. a rollout's own buffer: update_dev(obs[1:]) of the [T + 1, N, D] observations a closed-loop policy rollout wrote, no copy.  The
   library refuses a T > 1 rollout unless N D % 4 == 0 (every row of its obs [T, N, D] is 16-byte aligned), so obs[1:] of ONE call's
   buffer is always aligned: that is the first case.  With N D % 4 != 0 (asserted; offsets of 8 and 12 bytes) only one-step calls are
   admitted, each into an aligned row, and the rows are gathered on the device into the [T + 1, N, D] buffer whose [1:] view goes to
   update_dev as it is.

Everywhere: the count exact, mean and M2 of EVERY column inside the bars, the published table exactly fp32 of the device's fp64 state
(_table), the worst error printed as a fraction of the bar.  Bars: a, b, c, e use test_gpu_obs_norm._stat_bars as it stands (8 n u per
added term, u = 2^-52); d uses obs_norm_plan.merge_bars / steps_bars, derived there from chan_merge's operations.  Each rejects an fp32
accumulation by more than 100x (tests/test_obs_norm_plan_cpu.py::test_bars_reject_an_fp32_accumulation).

The emulation's mutants (tests/obs_norm_plan.py, run in tests/test_obs_norm_plan_cpu.py at every shape of a) and what each fails:
  stale_a   -- a workgroup's later tiles read at its first tile's offset a: the count is right, mean and M2 leave the bars by 1e7x and
               more at D = 13, 14, 18, 19, 25 (where tile_rows D % 4 != 0; at the other widths a does not change between tiles);
  cnt_reset -- cnt restarts in every tile while sum and sq carry: the count is wrong (and mean, M2 by 1e6x and more);
  drop_last -- the merge kernel's run stops one partial early: the count is wrong (rows are lost).

FIGURES (MI355X): 64 cases, 64 passed, no kernel or host change was needed; 8.8 s for the file, slowest case 0.54 s
(test_three_tiles_per_workgroup[13], 64 MiB twice).  The four-offset runs were bit-identical in state and table at every shape.
Worst device error as a fraction of the bar, per width (a: two tiles, full cap and three tiles, plain and outlier; d: the five pairs
and the 40 updates):
    D      a: mean    a: M2      d: mean    d: M2
    13     9.0e-08    3.6e-06    7.5e-04    1.3e-03
    14     5.3e-08    4.0e-07    1.1e-03    2.2e-03
    18     6.7e-08    9.8e-07    8.8e-04    2.3e-03
    19     1.9e-07    6.7e-07    6.2e-04    2.3e-03
    20     1.6e-07    6.0e-07    7.8e-04    2.3e-03
    22     1.9e-07    9.6e-07    6.4e-04    2.3e-03
    25     2.3e-07    9.9e-07    8.4e-04    2.1e-03
    24     1.4e-07    1.3e-06    4.1e-04    2.4e-03
    36     2.2e-07    1.1e-06    8.6e-04    2.1e-03
    60     7.0e-07    1.3e-05    1.7e-03    2.2e-03
    108    4.4e-06    1.3e-05    7.6e-04    2.3e-03
b: at most 8.8e-05 (mean) and 1.5e-04 (M2), at D = 60; e: at most 2.1e-04 and 1.4e-04.  The bars of a count 8 u per added term for
n in the hundreds of thousands, and the device's errors do not add up in one direction: the margin is the bars' own, not a tuned one.
"""
import numpy as np
import pytest

from tests import obs_norm_plan as P
from tests import obs_norm_ref as R
from tests.policy_util import _bufs, _dev
from tests.test_gpu_obs_norm import _Actor, _env, _stat_bars, _stat_data, _t, _table
from tests.test_gpu_policy_shapes import OBS, OBS_IDS
from tests.test_obs_norm_plan_cpu import merge_cases

pytestmark = pytest.mark.gpu

OBS_OF = {d: o for o in OBS for d in [o[2]]}
_ids = lambda shapes: ["d%d-%d" % s for s in shapes]


def _fresh(env):
    from gym_art_amd.policy import ObsNorm
    return ObsNorm(env, R.EPS, R.CLIP)


def _at_offset(x, off):
    """the rows x on the device in a buffer whose first float is `off` floats past a 16-byte boundary"""
    import torch
    pad = torch.zeros(x.size + 4, device=_dev())
    buf = pad[off:off + x.size].view(x.shape)
    assert buf.data_ptr() % 16 == 4 * off and buf.is_contiguous()
    buf.copy_(torch.from_numpy(x))
    return buf


def _check(norm, ref, bars, what, constant=True):
    """the device's state against (count, mean, M2) within bars = (mean, M2), every column; the table; -> (state, table, fractions)"""
    s = norm.state_dict()
    em, e2 = np.abs(s["mean"] - ref[1]), np.abs(s["m2"] - ref[2])
    fr = (P.frac(em, bars[0]), P.frac(e2, bars[1]))
    assert s["count"] == ref[0], (what, s["count"], ref[0])
    assert s["mean"].shape == ref[1].shape and np.all(em <= bars[0]) and np.all(e2 <= bars[1]), (what,) + fr
    if constant:
        assert s["m2"][2] == 0.0 and s["mean"][2] == 1.5, what
    return s, np.stack(_table(norm)), fr


def _one_update(env, x, off=0):
    norm = _fresh(env)
    norm.update_dev(_at_offset(x, off))
    return norm


def _same_bits(runs, what):
    s0, t0 = runs[0]
    for s, t in runs[1:]:
        assert s["count"] == s0["count"] and all(np.array_equal(s[k].view(np.uint64), s0[k].view(np.uint64)) for k in ("mean", "m2")), what
        assert np.array_equal(t.view(np.uint32), t0.view(np.uint32)), what


def _cap_case(D, rows, offsets, outliers):
    """one data set of (D, rows), one two-pass per variant, one update per offset -> worst (mean, M2) fraction of the bar"""
    env = _env(OBS_OF[D])
    x = P.data(D, rows)
    worst = np.zeros(2)
    for outlier in outliers:
        if outlier:
            x[0, P.OUTLIER_COL] = P.OUTLIER
        ref, bars = R.moments(x), _stat_bars(x)
        runs = []
        for off in offsets:
            norm = _one_update(env, x, off)
            s, tab, fr = _check(norm, ref, bars, (D, rows, off, outlier))
            norm.close()
            runs.append((s, tab))
            worst = np.maximum(worst, fr)
        _same_bits(runs, (D, rows, outlier))
    print("d=%d rows=%d offsets=%s: worst device error / bar: mean %.3g, M2 %.3g" % (D, rows, list(offsets), worst[0], worst[1]))
    env.close()


# ---- a. the cap and the tile loop --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_two_tiles_per_workgroup(obs):
    _cap_case(obs[2], P.two_tiles(obs[2]), (0,), (False, True))


@pytest.mark.parametrize("D", P.FULL_WIDTHS)
def test_two_tiles_full_cap(D):
    _cap_case(D, P.two_tiles_full(D), (0,), (False, True))


@pytest.mark.parametrize("D", P.THREE_WIDTHS)
def test_three_tiles_per_workgroup(D):
    _cap_case(D, P.three_tiles(D), (0,), (False, True))


# ---- b. chunk > 1 in the merge -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,rows", P.chunk_shapes(), ids=_ids(P.chunk_shapes()))
def test_merge_runs_of_more_than_one_partial(D, rows):
    _cap_case(D, rows, (0, 1), (False, True))


# ---- c. the four offsets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,rows", P.align_shapes(), ids=_ids(P.align_shapes()))
def test_four_offsets_same_bits_large(D, rows):
    _cap_case(D, rows, (0, 1, 2, 3), (False,))


@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_four_offsets_same_bits_small(obs):
    env = _env(obs)
    D = env.obs_dim
    for rows in (1, 2, 65):
        x, ref = _stat_data(D, rows)
        bars = _stat_bars(x)
        runs = []
        for off in range(4):
            norm = _one_update(env, x, off)
            s, tab, _ = _check(norm, ref, bars, (D, rows, off))
            norm.close()
            runs.append((s, tab))
        _same_bits(runs, (D, rows))
    env.close()


@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_apply_at_every_offset(obs):
    """normalize_dev with the input at each of the four offsets and the output at each of the four (and in place): bit for bit
    obs_norm_ref.normalize with the published table; the input is left as it was and the floats around the output are not written"""
    import torch
    from gym_art_amd.policy import ObsNorm
    env = _env(obs)
    D = env.obs_dim
    mean, var = R.case_stats(D)
    norm = ObsNorm.from_stats(env, mean, var, 1.0, R.EPS, R.CLIP)
    mean32, inv32 = _table(norm)
    for rows in (1, 65, 130):
        x = R.stand_in_obs(rows, D)
        ref = R.normalize(x, mean32, inv32, R.CLIP).view(np.uint32)
        for off_in in range(4):
            xd = _at_offset(x, off_in)
            for off_out in range(4):
                pad = torch.full((x.size + 4,), 77.0, device=_dev())
                out = pad[off_out:off_out + x.size].view(x.shape)
                assert norm.normalize_dev(xd, out=out) is out
                got = pad.cpu().numpy()
                assert np.array_equal(got[off_out:off_out + x.size].view(np.uint32).reshape(x.shape), ref), (D, rows, off_in, off_out)
                assert np.all(got[:off_out] == 77.0) and np.all(got[off_out + x.size:] == 77.0)
            assert np.array_equal(xd.cpu().numpy(), x)
            norm.normalize_dev(xd, out=xd)
            assert np.array_equal(xd.cpu().numpy().view(np.uint32), ref), (D, rows, off_in)
    norm.close(); env.close()


# ---- d. the running merge ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_running_merge(obs):
    env = _env(obs)
    D = env.obs_dim
    worst = np.zeros(2)
    for name, state, x in merge_cases(D):
        norm = _fresh(env)
        norm.load_state_dict({"count": state[0], "mean": state[1], "m2": state[2]})
        norm.update_dev(_t(x))
        batch = R.moments(x)
        ref = R.chan_merge(state, batch)
        pinned = state[0] == 0 or state[2][2] == 0.0                  # the constant column: exact where the state's M2 was 0 (or unread)
        s, _, fr = _check(norm, ref, P.merge_bars(state, batch, _stat_bars(x)), (D, name), constant=pinned and bool(np.all(x[:, 2] == 1.5)))
        assert s["count"] == state[0] + x.shape[0]
        if state[0] == 0:                                             # ... and the stored mean and M2 of an empty state change no bit
            other = _fresh(env)
            other.update_dev(_t(x))
            _same_bits([(s, np.stack(_table(norm))), (other.state_dict(), np.stack(_table(other)))], (D, name))
            other.close()
        norm.close()
        print("d=%d %s: device error / bar: mean %.3g, M2 %.3g" % (D, name, fr[0], fr[1]))
        worst = np.maximum(worst, fr)
    # 40 successive updates of 63 rows, views of one buffer (the k-th starts 63 k D floats in), against one two-pass
    x, ref = _stat_data(D, 40 * 63)
    xd = _t(x)
    norm = _fresh(env)
    for k in range(40):
        norm.update_dev(xd[63 * k:63 * (k + 1)])
    _, _, fr = _check(norm, ref, P.steps_bars(x, 40), (D, "40x63"))
    norm.close()
    worst = np.maximum(worst, fr)
    print("d=%d 40x63: device error / bar: mean %.3g, M2 %.3g; worst of case d: mean %.3g, M2 %.3g" % (D, fr[0], fr[1], worst[0], worst[1]))
    env.close()


# ---- e. a rollout's own buffer ---------------------------------------------------------------------------------------------------------------
def _from_rollout(norm, buf, what):
    """update_dev of buf[1:] as it is, against numpy on the same rows read back"""
    view = buf[1:]
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * buf[0].numel()
    norm.update_dev(view)
    assert view.data_ptr() == buf[1:].data_ptr()
    x = view.cpu().numpy().reshape(-1, buf.shape[-1])
    assert np.isfinite(x).all() and x.std() > 0
    _, _, fr = _check(norm, R.moments(x), _stat_bars(x), what, constant=False)
    print("%s: device error / bar: mean %.3g, M2 %.3g" % (what, fr[0], fr[1]))


def test_rollout_buffer_one_call():
    """[T + 1, N, D] = the reset observation and the T rows ONE closed-loop call wrote behind it (N D % 4 == 0, as the library demands
    of T > 1): rows 1: start N D 4 bytes past the allocation, 16-byte aligned"""
    import torch
    T, n = 6, 68
    env = _env(OBS[2], n, ep_time=0.03)
    D = env.obs_dim
    pol = _Actor("mfma", [48, 16], D=D, value=False).build(env, None, log_std=None)
    buf = torch.empty((T + 1, n, D), device=_dev())
    env.reset_dev(buf[0])
    _, r, d, a = _bufs(env, T)
    env.rollout_policy_dev(pol, buf[1:], r, d, a)
    torch.cuda.synchronize()
    assert int(d.sum()) > 0 and buf[1:].data_ptr() % 16 == 0
    norm = _fresh(env)
    _from_rollout(norm, buf, "rollout T=%d N=%d D=%d" % (T, n, D))
    pol.close(); norm.close(); env.close()


@pytest.mark.parametrize("k,n", [(2, 65), (0, 131)], ids=["d18-n65", "d13-n131"])
def test_rollout_buffer_off_a_boundary(k, n):
    """N D % 4 != 0 (2 at D = 18, N = 65; 3 at D = 13, N = 131): the library admits one-step closed-loop calls only, each into a
    16-byte-aligned row; the rows are gathered into [T + 1, N, D] on the device and rows 1:, 8 and 12 bytes past a 16-byte boundary, go to
    update_dev with no copy"""
    import torch
    T = 6
    env = _env(OBS[k], n, ep_time=0.03)
    D = env.obs_dim
    assert (n * D) % 4 != 0
    pol = _Actor("mfma", [48, 16], D=D, value=False).build(env, None, log_std=None)
    buf = torch.empty((T + 1, n, D), device=_dev())
    row = torch.empty((n, D), device=_dev())
    env.reset_dev(row)
    buf[0].copy_(row)
    o, r, d, a = _bufs(env, 1)
    dones = 0
    for t in range(T):
        env.rollout_policy_dev(pol, o, r, d, a)
        buf[t + 1].copy_(o[0])
        dones += int(d.sum())
    torch.cuda.synchronize()
    assert dones > 0 and buf[1:].data_ptr() % 16 == 4 * ((n * D) % 4) != 0
    norm = _fresh(env)
    _from_rollout(norm, buf, "one-step rollouts T=%d N=%d D=%d" % (T, n, D))
    pol.close(); norm.close(); env.close()
