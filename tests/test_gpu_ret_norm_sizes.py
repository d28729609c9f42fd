"""The return normaliser's update (gaq.h gaq_ret_norm_update_dev: ret_norm_partial_kernel, then obs_norm_merge_kernel with D = 1) at the
batch sizes a training rollout feeds it and at the limits of its shift K, where tests/test_gpu_ret_norm.py (N = 68 and 2096 only) never
goes.  The cases a to e are the functions of tests/ret_norm_plan.py, driven here through RetNorm; tests/test_ret_norm_plan_cpu.py
drives the same functions through a numpy emulation of the device's order and through six wrong orders, each of which fails an
assertion made here at a named shape, and proves from plan(N) what each size reaches.

a. the merge launch beyond 256 partials: N = 65 537 (nb = 257: 128 runs of two partials, one run of one, 127 empty row groups),
   131 072 (512: every run full) and 196 609 (769: chunk = 4, a trailing run of one), T = 2 and 5; one update (two fresh objects: the
   same bits) and two on top of each other.
b. wave and workgroup edges of the lane tree: N = 1, 63, 64, 65, 255, 256, 257, each at T = 1, 2, 3, 4, 7, 8 with three consecutive
   updates (the carry crosses the calls, K becomes the running mean); N = 1 a second time on rewards of 1e3 + 1e-2.
c. gamma = 0 (the carry is the last reward widened); gamma = 1 over T = 1000 without a done (returns up to 1e3); gamma = 1 with dones.
d. the shift's reach, at N = 2096, T = 5 and N = 68, T = 20: (1) fresh statistics beside a loaded carry of 1e5, K = reward[0, 0] = 1e3:
   inside stat_bars_shifted and OUTSIDE the plain M2 bar -- the documented limit of a one-pass shifted sum; (2) a state stored as
   count 0, mean 7, M2 3 has no effect: M2 == 0.0 on windows of one value, a fresh object's bits on an ordinary one; (3) an outlier of
   1e6 at reward[0, 0]; (4) a jump of the return level from 0 to 1e5 between two updates.
e. the running merge: 200 successive updates against one two-pass over 2 096 000 samples; a prior count of 1e12; SB3's start
   (RetNorm.from_stats(env, 1.0, count=1e-4, mean=0.0)).
f. a captured graph of update_dev, normalize_dev(out=rew) and gae_dev replayed three times beside an eager twin (the first replay
   takes K from reward[0], the later ones from the running mean: chosen on the device); stream= on a side stream; reset_returns
   between two updates without a synchronisation.

Everywhere in a to e (ret_norm_plan.check): the count exact, the carry bit for bit ret_norm_ref.returns, mean and M2 inside the stated
bar, the table read back with test_gpu_ret_norm._inv_std, the worst error printed as a fraction of its bar.  Bars: ret_norm_ref.stat_bars
as it stands wherever K lies inside the samples (a, b, c, d.3, e's batches); ret_norm_ref.stat_bars_shifted where it does not (d.1, d.4);
obs_norm_plan.merge_bars on top of either (d.4, e's priors); obs_norm_plan.steps_bars for the 200 updates.  None is tuned to the device,
and each rejects fp32 arithmetic by more than 100x (tests/test_ret_norm_plan_cpu.py::test_bars_reject_fp32_arithmetic; of the merge on
the prior count of 1e12 the M2 bar does, the mean bar cannot: the batch mean's error arrives scaled by 1e-8).

FIGURES (MI355X): 32 cases, no kernel or host change was needed; 3.2 s for the file, slowest case 0.26 s
(test_merge_runs_of_more_than_one_partial[65537-2], the first to upload).  Two fresh objects gave the same bits at every size of a, and
the replayed graph, the side stream and the eager runs of f agreed bit for bit.  Worst device error as a fraction of its bar:
    group                                   mean       M2
    a  257, 512, 769 partials               4.9e-07    3.8e-07
    b  N = 1 (a bar of 8 u, 1 to 3 samples) 1.5e-02    5.2e-03
    b  N = 63 ... 257                       5.1e-04    1.3e-04
    c  gamma 0, gamma 1                     4.7e-06    2.4e-06
    d  far K (K-aware bar), outlier, jump   6.0e-05    3.1e-05
    e  200 updates                          1.3e-08    2.1e-08
    e  priors 1e12 and SB3's                2.1e-06    0
d.1, relative M2 error of the device next to the numpy emulation of its order (tests/ret_norm_plan.py) and as a multiple of the plain
stat_bars' M2 bar, which it has to exceed:
    N = 2096, T = 5     device 8.2e-05    emulation 2.0e-04    6.0e+04 x the plain bar
    N = 68, T = 20      device 4.7e-04    emulation 3.0e-04    4.0e+06 x the plain bar
The bars count 8 u per added term and the device's errors do not add up in one direction: the margin is the bars' own, not a tuned one.
"""
import numpy as np
import pytest

from tests import ret_norm_plan as P
from tests import ret_norm_ref as R
from tests.policy_util import _dev
from tests.test_gpu_ret_norm import _bits, _env, _inv_std, _t

pytestmark = pytest.mark.gpu

_shape_ids = ["n%d-t%d" % s for s in P.SHIFT_SHAPES]


class Device:
    """RetNorm behind the interface of ret_norm_plan's cases (ret_norm_plan.Emulated is the other one)"""

    def __init__(self, env, N, gamma=R.GAMMA, from_stats=None, norm=None):
        from gym_art_amd.policy import RetNorm
        assert env.num_envs == N
        if norm is not None:
            self.norm = norm
        elif from_stats is not None:
            var, count, mean = from_stats
            self.norm = RetNorm.from_stats(env, var, count=count, mean=mean, gamma=gamma)
        else:
            self.norm = RetNorm(env, gamma=gamma)

    def load(self, count, mean, m2, returns=None):
        self.norm.load_state_dict({"count": count, "mean": mean, "m2": m2, "returns": returns})

    def update(self, rew, done):
        self.norm.update_dev(_t(rew), _t(done))

    def stats(self):
        s = self.norm.state_dict()
        return s["count"], s["mean"], s["m2"]

    def returns(self):
        return self.norm.returns

    def table(self):
        _inv_std(self.norm)

    def close(self):
        self.norm.close()


def _run(case, N, *args, **kw):
    env = _env(N)
    try:
        return case(lambda n, **k: Device(env, n, **k), N, *args, **kw)
    finally:
        env.close()


# ---- a. the merge launch beyond 256 partials -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", P.CHUNK_STEPS)
@pytest.mark.parametrize("N", P.CHUNK_SIZES)
def test_merge_runs_of_more_than_one_partial(N, T):
    p = P.plan(N)
    assert p.chunk > 1 and p == {65537: P.Plan(257, 2, 128, 1, 127, (1, 0, 0, 0)), 131072: P.Plan(512, 2, 256, 0, 0, (64, 64, 64, 64)),
                                 196609: P.Plan(769, 4, 192, 1, 63, (1, 0, 0, 0))}[N]
    _run(P.case_chunks, N, T)


# ---- b. wave and workgroup edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", P.EDGE_SIZES)
def test_wave_and_workgroup_edges(N):
    _run(P.case_edges, N)
    if N == 1:
        _run(P.case_edges, N, big=True)


# ---- c. gamma and long windows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", P.SHIFT_SHAPES, ids=_shape_ids)
def test_gamma_zero(N, T):
    _run(P.case_gamma_zero, N, T)


def test_gamma_one_thousand_steps_without_a_done():
    _run(lambda new, N: P.case_gamma_one_long(new), P.long_rewards()[0].shape[1])


@pytest.mark.parametrize("N", [n for n, _ in P.SHIFT_SHAPES])
def test_gamma_one_with_dones(N):
    _run(P.case_gamma_one_dones, N)


# ---- d. the shift's reach ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", P.SHIFT_SHAPES, ids=_shape_ids)
def test_shift_far_from_the_samples(N, T):
    """d.1.  The numpy emulation of the device's order is 2.0e-4 (N = 2096) and 3.0e-4 (N = 68) relative off in M2, 1.5e5 x and
    2.6e6 x the plain bar: the second assertion of the case (the error EXCEEDS the plain bar) keeps this the documented limit."""
    _run(P.case_shift_far, N, T)


@pytest.mark.parametrize("N,T", P.SHIFT_SHAPES, ids=_shape_ids)
def test_stored_numbers_of_an_empty_state_have_no_effect(N, T):
    _run(P.case_shift_empty_state, N, T)


@pytest.mark.parametrize("N,T", P.SHIFT_SHAPES, ids=_shape_ids)
def test_outlier_at_the_first_reward(N, T):
    _run(P.case_shift_outlier, N, T)


@pytest.mark.parametrize("N,T", P.SHIFT_SHAPES, ids=_shape_ids)
def test_level_jump_between_updates(N, T):
    _run(P.case_shift_jump, N, T)


# ---- e. the running merge ------------------------------------------------------------------------------------------------------------
def test_two_hundred_updates_against_one_two_pass():
    _run(lambda new, N: P.case_long_run(new), P.LONG_N)


@pytest.mark.parametrize("name", sorted(P.PRIORS))
def test_one_window_on_a_prior_state(name):
    _run(lambda new, N: P.case_prior(new, name), P.LONG_N)


# ---- f. graphs and streams -----------------------------------------------------------------------------------------------------------
def _same_state(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    assert all(_bits(np.float64(sa[k])) == _bits(np.float64(sb[k])) for k in ("count", "mean", "m2")), (what, sa, sb)
    assert np.array_equal(_bits(sa["returns"]), _bits(sb["returns"])), what


def test_graph_captured_update_normalize_gae():
    """update_dev, normalize_dev(out=rew) and gae_dev captured on one stream (a linear chain) over static [T, N] buffers and replayed
    three times with fresh contents, beside an eager twin on buffers of its own: state, carry, normalised rewards and advantages
    bit-equal after every replay.  The captured object is EMPTY at the first replay, so the graph's partial kernel takes K from
    reward[0] there and from the running mean afterwards; the statistics after the last replay are checked against numpy as well."""
    import torch
    from gym_art_amd.policy import RetNorm
    N, T = 2096, 5
    env = _env(N)
    windows = P.chain(T, N, (0, 1, 2))
    values = torch.from_numpy(np.random.RandomState(21).randn(T + 1, N).astype(np.float32)).to(_dev())
    graphed, eager = RetNorm(env), RetNorm(env)
    rew_g, done_g = _t(windows[0][0]).clone(), _t(windows[0][1]).clone()
    adv_g, adv_e = torch.empty((T, N), device=_dev()), torch.empty((T, N), device=_dev())

    def chain_of_three(norm, rew, done, adv):
        norm.update_dev(rew, done)
        assert norm.normalize_dev(rew, out=rew) is rew
        env.gae_dev(rew, done, values, 0.99, 0.95, adv)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up on a side stream
        chain_of_three(graphed, rew_g, done_g, adv_g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.load_state_dict({"count": 0.0, "mean": 0.0, "m2": 0.0, "returns": np.zeros(N)})     # ... and forgotten
    _same_state(graphed, eager, "before the capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain_of_three(graphed, rew_g, done_g, adv_g)
    _same_state(graphed, eager, "after the capture: nothing has run")
    for rep, (rew, done, seen, carry) in enumerate(windows):
        rew_g.copy_(_t(rew)); done_g.copy_(_t(done))
        g.replay()
        rew_e, done_e = _t(rew).clone(), _t(done).clone()
        chain_of_three(eager, rew_e, done_e, adv_e)
        torch.cuda.synchronize()
        what = "replay %d" % rep
        _same_state(graphed, eager, what)
        assert graphed.count == (rep + 1) * T * N, what
        assert torch.equal(rew_g.view(torch.int32), rew_e.view(torch.int32)) and torch.equal(adv_g.view(torch.int32), adv_e.view(torch.int32)), what
        assert not np.array_equal(rew_g.cpu().numpy(), rew) and torch.isfinite(adv_g).all() and float(adv_g.abs().max()) > 0, what
    fr = P.check(Device(env, N, norm=graphed), R.moments(seen), R.stat_bars(seen), carry, "three replays")
    print("f three replays: error / bar: mean %.3g, M2 %.3g" % fr)
    for o in (graphed, eager, env):
        o.close()


def test_stream_argument():
    """update_dev and normalize_dev with stream= a side stream's handle while another stream is current: the current stream waits on
    the side stream and reads the result; state, carry and normalised rewards equal the default-stream run's bit for bit.  This pins the
    RESULTS of a call with stream=, not which stream the launches went to: with the waits on both sides either stream is a legal
    order, and a library that ignored the argument would give the same bits."""
    import torch
    from gym_art_amd.policy import RetNorm
    N, T = 2096, 5
    env = _env(N)
    (rew, done, _, _), (rew2, done2, seen, carry) = P.chain(T, N, (0, 1))
    plain, streamed = RetNorm(env), RetNorm(env)
    outs = []
    for r, d in ((rew, done), (rew2, done2)):
        plain.update_dev(_t(r), _t(d))
        outs.append(plain.normalize_dev(_t(r)))
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    for (r, d), ref in zip(((rew, done), (rew2, done2)), outs):
        rd, dd = _t(r), _t(d)
        out = torch.empty_like(rd)
        side.wait_stream(torch.cuda.current_stream())               # the uploads were made on the current stream
        streamed.update_dev(rd, dd, stream=side.cuda_stream)
        assert streamed.normalize_dev(rd, out=out, stream=side.cuda_stream) is out
        torch.cuda.current_stream().wait_stream(side)
        copy = out.clone()                                          # on the current stream, behind the wait
        torch.cuda.synchronize()
        assert torch.equal(copy.view(torch.int32), ref.view(torch.int32)) and np.array_equal(rd.cpu().numpy(), r)
    _same_state(plain, streamed, "stream=")
    fr = P.check(Device(env, N, norm=streamed), R.moments(seen), R.stat_bars(seen), carry, "stream=")
    print("f stream=: error / bar: mean %.3g, M2 %.3g" % fr)
    for o in (plain, streamed, env):
        o.close()


def test_reset_returns_between_updates_without_a_synchronisation():
    """update_dev, reset_returns(mask) with the mask already on the device, update_dev: three enqueues, no host wait in between, and
    the second update starts from the masked carry.  T = 3: R.rollout has no all-done row below T = 4, so the mask reaches the second
    window's last carry as well as its samples (asserted)"""
    import torch
    from gym_art_amd.policy import RetNorm
    N, T = 2096, 3
    env = _env(N)
    (rew, done, s1, c1), (rew2, done2, both, unmasked) = P.chain(T, N, (0, 1))
    mask = np.random.RandomState(9).rand(N) < 0.3
    masked = np.where(mask, 0.0, c1)
    assert np.count_nonzero(masked != c1) > N // 8
    s2, c2 = R.returns(rew2, done2, R.GAMMA, masked)
    assert np.count_nonzero(c2 != unmasked) > N // 8 and np.count_nonzero(s2 != both[T:]) > N // 8
    norm = RetNorm(env)
    bufs = [_t(a) for a in (rew, done, rew2, done2)] + [torch.from_numpy(mask).to(_dev())]
    torch.cuda.synchronize()
    norm.update_dev(bufs[0], bufs[1])
    norm.reset_returns(bufs[4])
    norm.update_dev(bufs[2], bufs[3])
    seen = np.concatenate([s1, s2])
    fr = P.check(Device(env, N, norm=norm), R.moments(seen), R.stat_bars(seen), c2, "update, masked reset, update")
    print("f masked reset: error / bar: mean %.3g, M2 %.3g" % fr)
    norm.close(); env.close()
