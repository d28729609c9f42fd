"""Advantage standardisation on the device (gaq.h gaq_adv_norm; gym_art_amd.norm.AdvNorm): obs_norm_partial_kernel at D = 1,
adv_norm_finish_kernel and adv_norm_apply_kernel.

Counts 1 (ddof = 0), 2, 255, 8191, 8192, 8193 (a tile is 8192 floats), 3 x 8192 + 5 and 2^23 + 8193 (more than kObsNormMaxBlocks = 1024
tiles, so rows_per_block exceeds a tile and is no multiple of 4: every offset a among one launch's tile starts); the base pointer at every
offset 0..3 floats past a 16-byte boundary (slices of a larger tensor); randn, 1e3 + 1e-2 randn, a constant batch and randn with one
outlier of 1e6; ddof 0 and 1 (at the largest count ddof = 1 on the randn batch only).

count, mean and M2 of stats() against numpy's fp64 two-pass values at the bars tests/test_gpu_obs_norm.py _stat_bars derives for the
same pass (8 n u per added term, u = 2^-52; a constant batch: M2 == 0 exactly).  out against fp64 (x - mean) / (std + eps) with numpy's
statistics, no element excluded, at the bar _out_bar derives: the device computes fl(fl(x - m32) i32) with m32 = fl32(mean_dev) and
i32 = fl32(inv_dev), so with u = 2^-24
    |x - m32 - (x - mean)| <= u |mean| + bar_mean              (the rounding of the mean to fp32, the device's mean against numpy's)
    the subtraction rounds once: u (|x - mean| + u |mean| + bar_mean)
    i32 = inv (1 + e), |e| <= u + bar_M2 / (2 M2)              (its rounding to fp32; inv moves by half M2's relative error, times
                                                                  std / (std + eps) <= 1)
    the product rounds once: u |out|
    => |out - ref| <= inv (u |mean| + bar_mean) + |ref| (3 u + bar_M2 / (2 M2)),  first order; times 1 + 2^-20 for the products of these.
The largest count is compared with numpy at one unaligned offset and bit for bit with that run at the other three (the statistics at all
four): the fp64 comparison of 2^23 elements is the slow part, not the device.

Also: in place == out of place, two runs, an [T, N] tensor and its flat view: the same bits; a constant batch gives +0 everywhere; every
refusal leaves a NaN-filled output untouched.

Each case prints its worst error / bar.
FIGURES (MI355X): 10 cases, 4.5 s for the file, slowest case 1.9 s (count 2^23 + 8193).  Worst error / bar per count:
    count  1    2      255      8191     8192     8193     24581    8396801
    mean   0    0      1.3e-04  8.3e-06  7.1e-06  4.7e-06  7.5e-07  4.7e-10
    M2     0    0      3.3e-05  2.9e-07  4.6e-07  6.5e-07  2.0e-07  2.9e-10
    out    0    0.512  0.644    0.792    0.698    0.791    0.608    0.149
The four offsets, in place and the second run gave the first run's bits at every count; the constant batches M2 == 0 and +0."""
import ctypes as C

import numpy as np
import pytest

from tests.policy_util import _dev
from tests.test_gpu_obs_norm import _stat_bars

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 255, 8191, 8192, 8193, 3 * 8192 + 5, (1 << 23) + 8193]
KINDS = ["randn", "offset", "constant", "outlier"]
U24 = 2.0 ** -24


def _data(kind, count):
    z = np.random.default_rng(count % 9973 + KINDS.index(kind)).standard_normal(count, dtype=np.float32)
    if kind == "randn":
        return z
    if kind == "offset":
        return (np.float32(1e3) + np.float32(1e-2) * z).astype(np.float32)
    if kind == "constant":
        return np.full(count, 1.5, np.float32)
    x = z
    x[count // 2] = 1e6
    return x


def _at_offset(x, off):
    """x on the device in a buffer whose first float is `off` floats past a 16-byte boundary, NaN around it"""
    import torch
    pad = torch.full((x.size + 8,), float("nan"), device=_dev())
    assert pad.data_ptr() % 16 == 0
    buf = pad[off:off + x.size]
    assert buf.data_ptr() % 16 == 4 * off and buf.is_contiguous()
    buf.copy_(torch.from_numpy(x))
    return pad, buf


def _moments(x):
    x64 = x.astype(np.float64)
    mean = x64.mean()
    return float(x.size), float(mean), float(((x64 - mean) ** 2).sum())


def _out_bar(x, ref_stats, eps, ddof):
    """(ref [count] f64, bar [count]) of the module docstring"""
    count, mean, m2 = ref_stats
    bar_mean, bar_m2 = (float(b[0]) for b in _stat_bars(x.reshape(-1, 1)))
    inv = 1.0 / (np.sqrt(m2 / (count - ddof)) + eps)
    ref = (x.astype(np.float64) - mean) * inv
    rel_inv = bar_m2 / (2.0 * m2) if m2 > 0 else 0.0
    bar = inv * (U24 * abs(mean) + bar_mean) + np.abs(ref) * (3.0 * U24 + rel_inv)
    return ref, bar * (1.0 + 2.0 ** -20)


def _env():
    from gym_art_amd import QuadrotorEnv
    return QuadrotorEnv(num_envs=64)


def _check_stats(norm, x, ref_stats, what):
    """stats() against numpy within _stat_bars; returns the fractions of the bars"""
    count, mean, m2 = norm._stats()
    bar_mean, bar_m2 = (float(b[0]) for b in _stat_bars(x.reshape(-1, 1)))
    assert count == ref_stats[0], (what, count)
    em, e2 = abs(mean - ref_stats[1]), abs(m2 - ref_stats[2])
    assert em <= bar_mean and e2 <= bar_m2, (what, em, bar_mean, e2, bar_m2)
    c, m, std = norm.stats()
    assert (c, m) == (count, mean) and std == np.sqrt(m2 / (count - norm.ddof)), what
    return em / bar_mean if bar_mean else 0.0, e2 / bar_m2 if bar_m2 else 0.0


@pytest.mark.parametrize("count", COUNTS)
def test_standardisation_against_fp64(count):
    import torch
    from gym_art_amd.norm import AdvNorm
    env = _env()
    big = count > (1 << 20)
    worst = np.zeros(3)
    norms = {ddof: AdvNorm(env, ddof=ddof) for ddof in ((0,) if count == 1 else (0, 1))}
    for kind in KINDS:
        x = _data(kind, count)
        ref_stats = _moments(x)
        for ddof, norm in norms.items():
            if big and ddof == 1 and kind != "randn":
                continue                                            # (the largest count: ddof = 1 on one kind of data)
            ref, bar = _out_bar(x, ref_stats, norm.eps, ddof)
            first = None
            for off in ((1, 0, 2, 3) if big else range(4)):         # (the largest count: numpy sees the run at an unaligned offset)
                what = (count, kind, ddof, off)
                _, xd = _at_offset(x, off)
                pad, out = _at_offset(np.zeros_like(x), off)
                out.fill_(float("nan"))
                assert norm.normalize_dev(xd, out=out) is out
                fm, f2 = _check_stats(norm, x, ref_stats, what)
                if first is None:
                    got = out.cpu().numpy()
                    assert np.isfinite(got).all(), what
                    err = np.abs(got.astype(np.float64) - ref)
                    assert (err <= bar).all(), (what, float((err / bar).max()))
                    worst = np.maximum(worst, (fm, f2, float((err / bar).max())))
                    if kind == "constant":
                        assert ref_stats[2] == 0.0 and norm._stats()[2] == 0.0 and (got.view(np.uint32) == 0).all(), what
                    first = out.clone()
                    second = torch.full_like(first, float("nan"))
                    norm.normalize_dev(xd, out=second)              # two runs: the same bits
                    assert torch.equal(second.view(torch.int32), first.view(torch.int32)), what
                else:
                    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), what
                assert bool(torch.isnan(pad[:off]).all()) and bool(torch.isnan(pad[off + count:]).all()), what
                assert torch.equal(xd, torch.from_numpy(x).to(_dev())), what                    # the input is left as it was
                norm.normalize_dev(xd, out=xd)                      # in place: the same bits
                assert torch.equal(xd.view(torch.int32), first.view(torch.int32)), what
    alloc = norms[0].normalize_dev(xd)                              # out=None allocates
    assert alloc is not xd and alloc.shape == xd.shape
    for norm in norms.values():
        norm.close()
    print("adv_norm count=%d: worst error / bar: mean %.3g, M2 %.3g, out %.3g" % (count, worst[0], worst[1], worst[2]))
    env.close()


def test_a_rollout_shaped_tensor_and_its_flat_view_give_the_same_bits():
    import torch
    from gym_art_amd.policy import AdvNorm
    env = _env()
    T, n = 20, 2096
    x = torch.from_numpy(_data("randn", T * n)).to(_dev()).view(T, n)
    norm = AdvNorm(env)
    a = norm.normalize_dev(x)
    b = norm.normalize_dev(x.view(-1))
    c = norm.normalize_dev(x.view(T, n // 4, 4))
    assert a.shape == x.shape and b.shape == (T * n,) and c.shape == (T, n // 4, 4)
    assert torch.equal(a.view(-1).view(torch.int32), b.view(torch.int32)) and torch.equal(c.view(-1).view(torch.int32), b.view(torch.int32))
    count, mean, std = norm.stats()
    assert count == T * n and abs(mean) < 0.05 and abs(std - 1.0) < 0.05
    got = a.double()
    assert abs(float(got.mean())) < 1e-6 and abs(float(got.std()) - 1.0) < 1e-6
    norm.close(); env.close()


def test_refusals_leave_the_output_untouched():
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.norm import AdvNorm
    env = _env()
    lib = _lib.load()
    for bad in (2, -1, 3):
        with pytest.raises(ValueError):
            AdvNorm(env, ddof=bad)
    with pytest.raises(ValueError):
        AdvNorm(env, ddof=0.5)
    for bad in (float("nan"), float("inf"), -1e-8):
        with pytest.raises(ValueError):
            AdvNorm(env, eps=bad)
    x = torch.from_numpy(_data("randn", 64)).to(_dev())
    out = torch.full_like(x, float("nan"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ddof in (0, 1):
        norm = AdvNorm(env, ddof=ddof)
        with pytest.raises(ValueError):
            norm.normalize_dev(x[:ddof], out=out[:ddof])            # count < 1 + ddof
        with pytest.raises(ValueError):
            norm.normalize_dev(x[:0], out=out[:0])
        h, px, po = norm.handle, x.data_ptr(), out.data_ptr()
        for a, b in ((px + 2, po), (px, po + 2), (px + 1, po + 1)):  # misaligned pointers
            assert lib.gaq_adv_norm_apply_dev(h, 16, C.c_void_p(a), C.c_void_p(b), st) == -1 and b"aligned" in lib.gaq_last_error()
        too_many = ((1 << 31) - 1) * 1024 + 1                       # a count too large for one launch
        assert lib.gaq_adv_norm_apply_dev(h, too_many, C.c_void_p(px), C.c_void_p(po), st) == -1 and b"too large" in lib.gaq_last_error()
        assert lib.gaq_adv_norm_apply_dev(h, 64, None, C.c_void_p(po), st) == -1
        assert lib.gaq_adv_norm_apply_dev(h, 64, C.c_void_p(px), None, st) == -1
        for bad in (x.double(), x.cpu(), x.view(8, 8).t(), None):
            with pytest.raises(ValueError):
                norm.normalize_dev(bad, out=out)
        with pytest.raises(ValueError):
            norm.normalize_dev(x, out=out[:32])
        with pytest.raises(ValueError):
            norm.normalize_dev(x, out=out.double())
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
        assert norm._stats() == (0.0, 0.0, 0.0) and norm.stats() == (0.0, 0.0, 0.0)          # nothing ran
        assert norm.normalize_dev(x, out=out) is out                # ... and after all that the call works
        assert bool(torch.isfinite(out).all())
        out.fill_(float("nan"))
        norm.close()
        with pytest.raises(ValueError):
            norm.normalize_dev(x, out=out)                          # closed
        norm.close()
    env.close()
