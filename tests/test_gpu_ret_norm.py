"""Return normalisation on the device (gaq.h gaq_ret_norm, gym_art_amd.policy.RetNorm): the per-env carry against the numpy fp64 recurrence
bit for bit, split rollouts, the streaming statistics against numpy fp64 within the derived bars, the published table and the element
expression bit for bit, a real actor-critic rollout through update_dev / normalize_dev / gae_dev, masked resets, checkpoints and
refusals.  The reference arithmetic, the bars and the synthetic rollouts are tests/ret_norm_ref.py (checked without a GPU in
tests/test_ret_norm_cpu.py).  The partial kernel's grid is ceil(N / 256) workgroups, never capped, so no shape depends on a cap."""
import functools

import numpy as np
import pytest

from tests import ret_norm_ref as R
from tests.mlp_ref import _scaled_layers
from tests.policy_util import _bufs, _dev
from tests.test_gpu_policy_shapes import OBS, _kw

pytestmark = pytest.mark.gpu

SIZES = [68, 2096]            # one 64-lane wave plus a sliver of the next; 8 workgroups and a 48-env tail
STEPS = [1, 5, 20]            # below, around and well above the loop's unroll of 4
LOG_STD = [-1.0, -0.8, -1.2, -0.9]


def _env(n, **over):
    from gym_art_amd import QuadrotorEnv
    kw = _kw(OBS[2], n)
    kw.update(over)
    return QuadrotorEnv(**kw)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _case(T, N, seed=0):
    """a synthetic rollout and its reference from a zero carry: (rew, done, samples, carry, moments), all read-only"""
    rew, done = R.rollout(T, N, seed)
    samples, carry = R.returns(rew, done, R.GAMMA)
    samples.setflags(write=False); carry.setflags(write=False)
    return rew, done, samples, carry, R.moments(samples)


def _inv_std(norm):
    """The device's published inv_std, READ BACK through normalize_dev and required to equal, exactly, fp32 of the device's own fp64
    statistics: for a power of two p the element is inv_std * p, exact (a power-of-two scaling, no clamp below clip / 2, no underflow at
    these sizes), so z / p is the table's inv_std bit for bit.  The clip is read back with +-FLT_MAX."""
    s = norm.state_dict()
    inv = R.inv_std(s["count"], s["m2"], norm.eps)
    p = next(np.float32(2.0 ** e) for e in range(0, -64, -1) if np.float64(2.0 ** e) * np.float64(inv) < 0.5 * norm.clip)
    big = np.float32(3.0e38)
    z = norm.normalize_dev(_t(np.array([p, -p, big, -big], np.float32))).cpu().numpy()
    assert _bits(z[0] / p) == _bits(inv) and _bits(z[1] / p) == _bits(-inv), "the table's inv_std is not fp32(1 / sqrt(M2 / count + eps))"
    if np.isfinite(norm.clip):
        assert z[2] == np.float32(norm.clip) and z[3] == -np.float32(norm.clip), "the table's clip is not the object's"
    return inv


def _check_stats(norm, samples, what, worst=None):
    """count equal, mean and M2 within the derived bars of the two-pass fp64 moments of `samples`"""
    n, mean, m2 = R.moments(samples)
    bar_mean, bar_m2 = R.stat_bars(samples)
    s = norm.state_dict()
    em, e2 = abs(s["mean"] - mean), abs(s["m2"] - m2)
    print("%s: device error / bar: mean %.3g, M2 %.3g" % (what, em / bar_mean, e2 / bar_m2))
    assert s["count"] == n and em <= bar_mean and e2 <= bar_m2, (what, s["count"], n, em / bar_mean, e2 / bar_m2)
    if worst is not None:
        worst[0], worst[1] = max(worst[0], em / bar_mean), max(worst[1], e2 / bar_m2)


# ---- 1. the carry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("N", SIZES)
def test_carry_is_the_fp64_recurrence_bit_for_bit(N, T):
    """three updates in a row (the carry crosses the calls), then an all-done row and an all-clear row of their own (T = 1 has no room
    for them inside the window)"""
    from gym_art_amd.policy import RetNorm
    env = _env(N)
    norm = RetNorm(env)
    assert np.array_equal(norm.returns, np.zeros(N)) and norm.count == 0.0 and norm.mean == 0.0 and norm.var == 1.0
    carry = None
    windows = [_case(T, N, seed)[:2] for seed in range(3)]
    one = np.ones((1, N), np.uint8)
    windows += [(windows[0][0][:1], one), (windows[1][0][:1], 1 - one)]
    for k, (rew, done) in enumerate(windows):
        _, carry = R.returns(rew, done, R.GAMMA, carry)
        norm.update_dev(_t(rew), _t(done))
        assert np.array_equal(_bits(norm.returns), _bits(carry)), (N, T, k)
        if k == 3:
            assert not carry.any()
    assert norm.count == (3 * T + 2) * N and carry.all()
    norm.close(); env.close()


# ---- 2. split rollouts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_split_rollout(N):
    from gym_art_amd.policy import RetNorm
    rew, done, samples, carry, _ = _case(20, N)
    env = _env(N)
    one, two = RetNorm(env), RetNorm(env)
    one.update_dev(_t(rew), _t(done))
    two.update_dev(_t(rew[:7]), _t(done[:7]))
    assert np.array_equal(_bits(two.returns), _bits(R.returns(rew[:7], done[:7], R.GAMMA)[1]))
    two.update_dev(_t(rew[7:]), _t(done[7:]))
    assert np.array_equal(_bits(one.returns), _bits(carry)) and np.array_equal(_bits(two.returns), _bits(carry))
    assert one.count == two.count == 20 * N
    _check_stats(one, samples, "N=%d T=20 in one update" % N)
    _check_stats(two, samples, "N=%d T=7+13" % N)
    one.close(); two.close(); env.close()


# ---- 3. statistics -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_statistics_against_numpy_fp64(N):
    import torch
    from gym_art_amd.policy import RetNorm
    env = _env(N)
    worst = [0.0, 0.0]
    for T in STEPS:
        rew, done, samples, _, _ = _case(T, N)
        pair = []
        for _ in range(2):                                         # two fresh objects, the same input: the same bits
            norm = RetNorm(env)
            norm.update_dev(_t(rew), _t(done))
            _check_stats(norm, samples, "N=%d T=%d" % (N, T), worst)
            probe = norm.normalize_dev(_t(np.linspace(-40000.0, 40000.0, 257).astype(np.float32)))
            pair.append((norm.state_dict(), probe))
            _inv_std(norm)
            norm.close()
        (a, pa), (b, pb) = pair
        assert all(_bits(np.float64(a[k])) == _bits(np.float64(b[k])) for k in ("count", "mean", "m2")) and torch.equal(pa, pb)
        assert np.array_equal(_bits(a["returns"]), _bits(b["returns"]))
        # a second update on top of the first: the running mean is now the shift
        norm = RetNorm(env)
        norm.update_dev(_t(rew), _t(done))
        rew2, done2 = _case(T, N, 1)[:2]
        norm.update_dev(_t(rew2), _t(done2))
        s1, c1 = R.returns(rew, done, R.GAMMA)
        s2, _ = R.returns(rew2, done2, R.GAMMA, c1)
        _check_stats(norm, np.concatenate([s1, s2]), "N=%d T=%d+%d" % (N, T, T), worst)
        norm.close()
    print("N=%d: worst device error / bar: mean %.3g, M2 %.3g" % (N, worst[0], worst[1]))
    # samples of one value: M2 is exactly 0 -- a constant reward without discounting, and no reward at all
    for gamma, value in ((0.0, 1.7), (0.99, 0.0)):
        norm = RetNorm(env, gamma=gamma)
        norm.update_dev(torch.full((5, N), value, device=_dev()), _t(R.rollout(5, N)[1]))
        s = norm.state_dict()
        assert s["count"] == 5 * N and s["m2"] == 0.0 and s["mean"] == float(np.float32(value)), (gamma, s["mean"], s["m2"])
        assert _inv_std(norm) == np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-8))))
        norm.close()
    env.close()


# ---- 4. the table and the element expression ---------------------------------------------------------------------------------------
def test_table_and_apply_bit_for_bit():
    from gym_art_amd.policy import RetNorm
    N = 68
    env = _env(N)
    rew, done = _case(20, N)[:2]
    updated = RetNorm(env)
    updated.update_dev(_t(rew), _t(done))
    imported = RetNorm.from_stats(env, 0.01, count=100.0, mean=3.0)
    assert _inv_std(imported) == np.float32(1.0 / np.sqrt(0.01 + np.float64(np.float32(1e-8))))
    assert imported.count == 100.0 and imported.mean == 3.0 and imported.var == 0.01 and not imported.returns.any()
    rng = np.random.RandomState(3)
    for norm in (updated, imported):
        inv = _inv_std(norm)
        for shape in ((1,), (1023,), (1024,), (1025,), (4 * 1024 + 3,), (20, N), (3, 5, 7)):
            r = (rng.randn(*shape) * (norm.clip / np.float64(inv))).astype(np.float32)
            ref = R.normalize(r, inv, norm.clip)
            if r.size > 1000:
                hi, lo, inside = int((ref == norm.clip).sum()), int((ref == -norm.clip).sum()), int((np.abs(ref) < norm.clip).sum())
                assert hi > 0 and lo > 0 and inside > 0 and hi + lo + inside == r.size
            rd = _t(r)
            out = norm.normalize_dev(rd)
            assert out.shape == rd.shape and np.array_equal(_bits(out.cpu().numpy()), _bits(ref)) and np.array_equal(rd.cpu().numpy(), r)
            assert norm.normalize_dev(rd, out=rd) is rd            # in place
            assert np.array_equal(_bits(rd.cpu().numpy()), _bits(ref))
    # a slice of a larger buffer that starts 4 bytes past a 16-byte boundary
    pad = _t(rng.randn(1030).astype(np.float32))
    assert pad[1:].data_ptr() % 16 == 4
    inv = _inv_std(imported)
    assert np.array_equal(_bits(imported.normalize_dev(pad[1:]).cpu().numpy()), _bits(R.normalize(pad[1:].cpu().numpy(), inv, imported.clip)))
    # fresh statistics without a clamp: the identity on every fp32 value
    fresh = RetNorm(env, clip=float("inf"))
    x = np.array([0.0, -0.0, 1.0, -1.5, 3.4e38, -3.4e38, 1e-45, -1e-45, 1e-39, -1.1754942e-38, np.inf, -np.inf], np.float32)
    assert np.array_equal(_bits(fresh.normalize_dev(_t(x)).cpu().numpy()), _bits(x))
    for o in (updated, imported, fresh, env):
        o.close()


# ---- 5. with a real rollout ----------------------------------------------------------------------------------------------------------
def _ac_rollout(env, pol, T):
    import torch
    n, dev = env.num_envs, _dev()
    o, r, d, a = _bufs(env, T)
    values, logp = torch.empty((T + 1, n), device=dev), torch.empty((T, n), device=dev)
    env.rollout_policy_dev(pol, o, r, d, a, values=values, logp=logp)
    torch.cuda.synchronize()
    return dict(obs=o, rew=r, done=d, actions=a, values=values, logp=logp)


def _same(a, b):
    """equality of two state_dict trees: dicts, sequences, arrays, plain values"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


@pytest.mark.parametrize("layout", ["alias", "plain"])
@pytest.mark.parametrize("N", SIZES)
def test_with_a_real_rollout(N, layout):
    """an exploring 18-48-4 MFMA policy with a value head, T = 20 and episodes of 15 steps: every env finishes exactly once in the
    window.  update_dev on the recorded tensors against the reference; normalize_dev in place + gae_dev against gae_dev on rewards
    normalised in numpy; and a twin env that never saw a RetNorm ends in the same state and continues with the same bits"""
    import torch
    from gym_art_amd.policy import MLPPolicy, RetNorm
    T = 20
    layers = _scaled_layers([48], 18, 0)
    rng = np.random.RandomState(77)
    value = ((rng.randn(48) / np.sqrt(48)).astype(np.float32), np.float32(0.1))
    runs, states, nexts = [], [], []
    for with_norm in (True, False):
        env = _env(N, alias_obs=True if layout == "alias" else None)
        pol = MLPPolicy.from_arrays(env, layers, "tanh", True, LOG_STD, "mfma", value)
        env.reset_dev(torch.empty((N, 18), device=_dev()))
        run = _ac_rollout(env, pol, T)
        if with_norm:
            norm = RetNorm(env)
            rew, done = run["rew"].cpu().numpy(), run["done"].cpu().numpy()
            assert np.array_equal(done.sum(axis=0), np.ones(N)), "every env must finish exactly once in the window"
            norm.update_dev(run["rew"], run["done"])
            samples, carry = R.returns(rew, done, norm.gamma)
            assert np.array_equal(_bits(norm.returns), _bits(carry))
            _check_stats(norm, samples, "rollout N=%d %s" % (N, layout))
            inv = _inv_std(norm)
            ref_rew = R.normalize(rew, inv, norm.clip)
            assert not np.array_equal(ref_rew, rew)
            adv_ref, adv = torch.empty((T, N), device=_dev()), torch.empty((T, N), device=_dev())
            env.gae_dev(_t(ref_rew), run["done"], run["values"], 0.99, 0.95, adv_ref)
            raw = run["rew"].clone()
            assert norm.normalize_dev(run["rew"], out=run["rew"]) is run["rew"]
            env.gae_dev(run["rew"], run["done"], run["values"], 0.99, 0.95, adv)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(run["rew"].cpu().numpy()), _bits(ref_rew)) and torch.equal(adv, adv_ref)
            assert torch.isfinite(adv).all() and float(adv.abs().max()) > 0
            run["rew"] = raw
            norm.close()
        runs.append(run)
        states.append(env.state_dict())
        nexts.append(_ac_rollout(env, pol, 4))
        pol.close(); env.close()
    assert _same(states[0], states[1])
    for a, b in ((runs[0], runs[1]), (nexts[0], nexts[1])):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


# ---- 6. housekeeping -----------------------------------------------------------------------------------------------------------------
def test_reset_returns():
    import torch
    from gym_art_amd.policy import RetNorm
    N = 2096
    rew, done, _, carry, _ = _case(5, N)
    assert np.count_nonzero(carry) > N // 2
    env = _env(N)
    norm = RetNorm(env)
    mask = np.random.RandomState(9).rand(N) < 0.3
    for m in (mask, torch.from_numpy(mask).to(_dev()), _t(mask.astype(np.uint8)), mask.tolist()):
        norm.load_state_dict({"count": 0.0, "mean": 0.0, "m2": 0.0, "returns": np.zeros(N)})
        norm.update_dev(_t(rew), _t(done))
        stats = norm.state_dict()
        norm.reset_returns(m)
        assert np.array_equal(_bits(norm.returns), _bits(np.where(mask, 0.0, carry)))
        after = norm.state_dict()
        assert all(after[k] == stats[k] for k in ("count", "mean", "m2"))     # the statistics are not the carry's business
    norm.reset_returns()
    assert not norm.returns.any()
    with pytest.raises(ValueError, match="one entry per env"):
        norm.reset_returns(mask[:-1])
    norm.close(); env.close()


def test_checkpoint_round_trip():
    import torch
    from gym_art_amd.policy import RetNorm
    N = 68
    (rew, done), (rew2, done2) = _case(20, N)[:2], _case(5, N, 1)[:2]
    env = _env(N)
    whole = RetNorm(env)
    whole.update_dev(_t(rew), _t(done))
    state = whole.state_dict()
    assert set(state) == {"count", "mean", "m2", "returns", "gamma", "eps", "clip"}
    assert state["gamma"] == float(np.float32(0.99)) and state["eps"] == float(np.float32(1e-8)) and state["clip"] == 10.0
    resumed = RetNorm(env)
    resumed.load_state_dict(state)
    probe = _t(np.linspace(-40000.0, 40000.0, 129).astype(np.float32))
    assert torch.equal(whole.normalize_dev(probe), resumed.normalize_dev(probe))
    for norm in (whole, resumed):
        norm.update_dev(_t(rew2), _t(done2))
    a, b = whole.state_dict(), resumed.state_dict()
    assert all(_bits(np.float64(a[k])) == _bits(np.float64(b[k])) for k in ("count", "mean", "m2"))
    assert np.array_equal(_bits(a["returns"]), _bits(b["returns"]))
    assert torch.equal(whole.normalize_dev(probe), resumed.normalize_dev(probe)) and a["count"] == 25 * N
    for key, other in (("gamma", dict(gamma=0.9)), ("eps", dict(eps=1e-6)), ("clip", dict(clip=5.0))):
        foreign = RetNorm(env, **other)
        with pytest.raises(ValueError, match=key):
            foreign.load_state_dict(state)
        assert foreign.count == 0.0 and not foreign.returns.any()
        foreign.close()
    small = _env(64)
    foreign = RetNorm(small)
    with pytest.raises(ValueError, match="returns must have 64 entries"):
        foreign.load_state_dict(state)
    assert foreign.count == 0.0
    for o in (foreign, small, whole, resumed, env):
        o.close()


def test_refusals_leave_the_object_usable():
    import ctypes as C
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import RetNorm
    lib = _lib.load()
    N, T = 68, 5
    rew, done, _, carry, _ = _case(T, N)
    env = _env(N)
    norm = RetNorm(env)
    r, d = _t(rew), _t(done)
    bad = [(r[:, :-1], d[:, :-1]), (r[:, :-1].contiguous(), d[:, :-1].contiguous()),          # non-contiguous; another N
           (r.double(), d), (r, d.bool()), (r, d.float()), (r, d[:-1]), (r.cpu(), d), (r, d.cpu()),
           (torch.empty((N, T), device=_dev()).t(), d), (r[:0], d[:0]), (r[0], d[0]), (rew, done)]
    for x, y in bad:
        with pytest.raises(ValueError):
            norm.update_dev(x, y)
    for x, out in ((r.double(), None), (r.cpu(), None), (torch.empty((N, T), device=_dev()).t(), None), (r, r[:-1]), (r, r.double()),
                   (r, r.cpu()), (rew, None)):
        with pytest.raises(ValueError):
            norm.normalize_dev(x, out=out)
    # the library's own refusals: GAQ_ERR_INVALID with the argument named, nothing launched
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h, pr, pd = norm.handle, r.data_ptr(), d.data_ptr()
    for call, word in ((lambda: lib.gaq_ret_norm_update_dev(h, 0, C.c_void_p(pr), C.c_void_p(pd), st), b"T"),
                     (lambda: lib.gaq_ret_norm_update_dev(h, -2, C.c_void_p(pr), C.c_void_p(pd), st), b"T"),
                     (lambda: lib.gaq_ret_norm_update_dev(h, T, None, C.c_void_p(pd), st), b"null"),
                     (lambda: lib.gaq_ret_norm_update_dev(h, T, C.c_void_p(pr), None, st), b"null"),
                     (lambda: lib.gaq_ret_norm_update_dev(h, 1, C.c_void_p(pr + 2), C.c_void_p(pd), st), b"aligned"),
                     (lambda: lib.gaq_ret_norm_apply_dev(h, -1, C.c_void_p(pr), C.c_void_p(pr), st), b"count"),
                     (lambda: lib.gaq_ret_norm_apply_dev(h, 4, C.c_void_p(pr), None, st), b"null"),
                     (lambda: lib.gaq_ret_norm_apply_dev(h, 4, C.c_void_p(pr), C.c_void_p(pr + 1), st), b"aligned"),
                     (lambda: lib.gaq_ret_norm_set_stats(h, -1.0, 0.0, 1.0), b"count"),
                     (lambda: lib.gaq_ret_norm_set_stats(h, 1.0, float("nan"), 1.0), b"mean"),
                     (lambda: lib.gaq_ret_norm_set_stats(h, 1.0, 0.0, -1.0), b"M2"),
                     (lambda: lib.gaq_ret_norm_set_returns(h, None), b"null")):
        rc = call()
        assert rc == -1 and word in lib.gaq_last_error(), (rc, word, lib.gaq_last_error())
    out = C.c_void_p()
    for gamma, eps, clip, word in ((1.5, 1e-8, 10.0, b"gamma"), (-0.1, 1e-8, 10.0, b"gamma"), (float("nan"), 1e-8, 10.0, b"gamma"),
                                   (0.99, -1.0, 10.0, b"eps"), (0.99, float("inf"), 10.0, b"eps"), (0.99, 1e-8, 0.0, b"clip"),
                                   (0.99, 1e-8, float("nan"), b"clip")):
        assert lib.gaq_ret_norm_create(env._handle, gamma, eps, clip, C.byref(out)) == -1 and not out.value
        assert word in lib.gaq_last_error()
    with pytest.raises(ValueError, match="gamma"):
        RetNorm(env, gamma=1.01)
    assert lib.gaq_ret_norm_apply_dev(h, 0, C.c_void_p(pr), C.c_void_p(pr), st) == 0       # nothing to do is not an error
    # nothing was launched or changed, and a good update follows
    assert norm.count == 0.0 and not norm.returns.any()
    norm.update_dev(r, d)
    assert np.array_equal(_bits(norm.returns), _bits(carry)) and norm.count == T * N
    assert np.array_equal(r.cpu().numpy(), rew)
    norm.close()
    norm.close()                                                   # closing twice is fine; using a closed object is not
    for call in (lambda: norm.update_dev(r, d), lambda: norm.normalize_dev(r), lambda: norm.reset_returns(), lambda: norm.count,
                 lambda: norm.returns, lambda: norm.state_dict(), lambda: norm.load_state_dict({"count": 0.0, "mean": 0.0, "m2": 0.0})):
        with pytest.raises(ValueError, match="closed"):
            call()
    env.close()


def test_a_closed_obs_norm_says_so():
    """N = 65 (one full tile and one lane): an ObsNorm that has taken one update and was closed twice refuses every use with
    "the ObsNorm is closed", as a RetNorm does, instead of handing the library a null handle"""
    import torch
    from gym_art_amd.policy import MLPPolicy, ObsNorm
    N = 65
    env = _env(N)
    norm = ObsNorm(env)
    obs = _t(np.random.RandomState(3).randn(3, N, 18).astype(np.float32))
    norm.update_dev(obs)
    assert norm.count == 3 * N
    state = norm.state_dict()
    pol = MLPPolicy.from_arrays(env, _scaled_layers([48], 18, 0), "tanh", True, None, "mfma")
    norm.close()
    norm.close()
    for call in (lambda: norm.update_dev(obs), lambda: norm.normalize_dev(obs), lambda: norm.count, lambda: norm.state_dict(),
                 lambda: norm.load_state_dict(state), lambda: pol.set_obs_norm(norm)):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert pol.obs_norm is None
    assert torch.equal(obs.cpu(), _t(np.random.RandomState(3).randn(3, N, 18).astype(np.float32)).cpu())     # nothing was launched on it
    pol.close(); env.close()
