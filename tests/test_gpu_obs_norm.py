"""Observation normalisation on the device (gaq.h gaq_obs_norm, gym_art_amd.policy.ObsNorm): the streaming statistics against numpy fp64,
apply_dev against the element expression bit for bit, the kernels' staging against apply_dev bit for bit, the identity table, actors
against their fp64 references on normalised inputs, actor-critic rollouts, a captured rollout whose table changes between replays,
refusals and checkpoints.  The case table and the reference arithmetic are tests/obs_norm_ref.py (checked without a GPU in
tests/test_obs_norm_cpu.py)."""
import functools

import numpy as np
import pytest

from tests import obs_norm_ref as R
from tests.gru_util import _gru, _head
from tests.gru_util import reference_rollout as gru_reference
from tests.lstm_util import _lstm
from tests.lstm_util import reference_rollout as lstm_reference
from tests.lstm_util import torch_head32, torch_step32
from tests.mlp_ref import _scaled_layers, forward64
from tests.policy_util import _bufs, _dev, environ
from tests.test_gpu_policy_shapes import OBS, OBS_IDS, _kw

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -52
LOG_STD = [-1.0, -0.8, -1.2, -0.9]


def _env(obs=OBS[2], n=None, **over):
    from gym_art_amd import QuadrotorEnv
    kw = _kw(obs, n if n is not None else max(4, obs[1]))
    kw.update(over)
    env = QuadrotorEnv(**kw)
    assert env.obs_dim == obs[2]
    return env


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _case_norm(env, clip=R.CLIP):
    from gym_art_amd.policy import ObsNorm
    mean, var = R.case_stats(env.obs_dim)
    return ObsNorm.from_stats(env, mean, var, 1.0, R.EPS, clip)


def _table(norm):
    """The device's published fp32 table (mean, inv_std), READ BACK through apply_dev and required to equal, exactly, fp32 of the device's
    own fp64 statistics.  mean: (x - mean) * inv_std is 0 iff x == mean (inv_std > 0, no underflow at these sizes), so x = m gives 0 and
    both fp32 neighbours of m do not iff the table holds m.  inv_std: for a power of two p with fl(fl(m + p) - m) == p the element is
    inv_std * p, exact (a power-of-two scaling), so z / p is the table's inv_std bit for bit; p is chosen below the clamp."""
    s = norm.state_dict()
    m, inv = R.table(s["count"], s["mean"], s["m2"], norm.eps)
    p = np.zeros_like(m)
    for e in range(-3, -24, -1):
        q = np.float32(2.0 ** e)
        ok = (p == 0) & ((m + q).astype(np.float32) - m == q) & (q * inv.astype(np.float64) < 0.5 * norm.clip)
        p[ok] = q
    assert np.all(p > 0), (m, inv)
    probe = np.stack([m, np.nextafter(m, np.float32(np.inf)), np.nextafter(m, np.float32(-np.inf)), (m + p).astype(np.float32)])
    z = norm.normalize_dev(_t(probe)).cpu().numpy()
    assert np.all(z[0] == 0.0) and np.all(z[1] > 0.0) and np.all(z[2] < 0.0), "the table's mean is not fp32 of the fp64 mean"
    assert np.array_equal((z[3] / p).view(np.uint32), inv.view(np.uint32)), "the table's inv_std is not fp32(1 / sqrt(var + eps))"
    return m, inv


def _critic_layers(widths, D, seed):
    layers = _scaled_layers(widths, D, seed)
    W, b = layers[-1]
    return layers[:-1] + [(W[:1], b[:1])]


def test_widths_are_the_env_layouts():
    assert [d for _, _, d in OBS] == R.WIDTHS


# ---- 1. statistics ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stat_data(D, rows):
    """rows of fp32 data with a column of mean 1e3 and spread 1e-2 (column 1) and a constant column (column 2); and its fp64 moments"""
    rng = np.random.RandomState(D * 10007 + rows)
    x = (rng.randn(rows, D) * (1.0 + np.arange(D) % 4)).astype(np.float32)
    x[:, 1] = (1e3 + 1e-2 * rng.randn(rows)).astype(np.float32)
    x[:, 2] = 1.5
    x.setflags(write=False)
    return x, R.moments(x)


def _stat_bars(x):
    """Bars for the device's (mean, M2) against numpy's two-pass fp64 values of the same fp32 data.  The device adds, per column, at most
    `rows` terms in fp64 (shifted by a value of the column, so |d| <= the column's range) and then merges partials; a sum of n terms
    carries at most (n - 1) u of relative error on the sum of magnitudes (u = 2^-52), and the merges, the final K + s / n and numpy's own
    pairwise sums add a few more roundings: 8 n u is taken.  mean: magnitudes <= max|x|, so |err| <= 8 n u max|x|.  M2: the terms
    are d^2 <= range^2, n of them, so |err| <= 8 n u (n range^2); a constant column (range 0) must give exactly 0."""
    n = x.shape[0]
    x64 = x.astype(np.float64)
    rng_ = x64.max(axis=0) - x64.min(axis=0)
    return 8 * n * U64 * np.abs(x64).max(axis=0), 8 * n * U64 * n * rng_ ** 2


@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_statistics_against_numpy_fp64(obs):
    import torch
    from gym_art_amd.policy import ObsNorm
    env = _env(obs)
    D = env.obs_dim
    worst = [0.0, 0.0]
    for rows in (1, 2, 63, 64, 65, 4097):
        x, (n_ref, mean_ref, m2_ref) = _stat_data(D, rows)
        bar_mean, bar_m2 = _stat_bars(x)
        pad = torch.zeros(rows * D + 5, device=_dev())
        results = []
        for off in (0, 1, 0):                                      # aligned, 4 bytes past a 16-byte boundary, aligned again (same bits)
            norm = ObsNorm(env, R.EPS, R.CLIP)
            buf = pad[off:off + rows * D].view(rows, D)
            assert (buf.data_ptr() % 16) == 4 * off
            buf.copy_(_t(x))
            norm.update_dev(buf)
            s = norm.state_dict()
            assert s["count"] == n_ref
            em, e2 = np.abs(s["mean"] - mean_ref), np.abs(s["m2"] - m2_ref)
            assert np.all(em <= bar_mean) and np.all(e2 <= bar_m2), (D, rows, off, (em / np.maximum(bar_mean, 1e-300)).max(),
                                                                     (e2 / np.maximum(bar_m2, 1e-300)).max())
            assert s["m2"][2] == 0.0 and s["mean"][2] == 1.5
            if rows > 1:
                worst[0] = max(worst[0], float((em[bar_mean > 0] / bar_mean[bar_mean > 0]).max()))
                worst[1] = max(worst[1], float((e2[bar_m2 > 0] / bar_m2[bar_m2 > 0]).max()))
            # the published table is fp32 of the device's own fp64 statistics, exactly (_table reads it back and asserts it)
            mean32, inv32 = _table(norm)
            results.append((s, np.stack([mean32, inv32])))
            norm.close()
        a, b = results[0], results[2]
        assert all(np.array_equal(a[0][k], b[0][k]) for k in ("mean", "m2")) and np.array_equal(a[1], b[1])   # same bits twice
    # two updates of 65 and 4097 rows against one of their concatenation
    xa, xb = _stat_data(D, 65)[0], _stat_data(D, 4097)[0]
    xc = np.concatenate([xa, xb])
    n_ref, mean_ref, m2_ref = R.moments(xc)
    bar_mean, bar_m2 = _stat_bars(xc)
    two, one = ObsNorm(env, R.EPS, R.CLIP), ObsNorm(env, R.EPS, R.CLIP)
    two.update_dev(_t(xa)); two.update_dev(_t(xb)); one.update_dev(_t(xc))
    for norm in (two, one):
        s = norm.state_dict()
        assert s["count"] == n_ref and np.all(np.abs(s["mean"] - mean_ref) <= bar_mean) and np.all(np.abs(s["m2"] - m2_ref) <= bar_m2)
        assert np.allclose(norm.var, m2_ref / n_ref, rtol=1e-9, atol=1e-300) and norm.count == n_ref
        norm.close()
    # the bar rejects an fp32 accumulation by a wide margin: the 1e3 / 1e-2 column summed in numpy fp32 on the CPU
    col = xb[:, 1]
    s32 = np.float32(0.0)
    q32 = np.float32(0.0)
    for v in col:
        s32 = np.float32(s32 + v)
        q32 = np.float32(q32 + v * v)
    mean32 = np.float32(s32 / np.float32(col.size))
    m2_32 = np.float32(q32 - np.float32(col.size) * mean32 * mean32)
    _, mref, m2ref = R.moments(col[:, None])
    bm, b2 = _stat_bars(col[:, None])
    print("d=%d: worst device error / bar: mean %.3g, M2 %.3g; fp32 accumulation / bar: mean %.3g, M2 %.3g"
          % (D, worst[0], worst[1], abs(mean32 - mref[0]) / bm[0], abs(m2_32 - m2ref[0]) / b2[0]))
    assert abs(mean32 - mref[0]) > 100 * bm[0] and abs(m2_32 - m2ref[0]) > 100 * b2[0]
    env.close()


# ---- 2. apply_dev ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_apply_is_the_expression_bit_for_bit(obs):
    env = _env(obs)
    D = env.obs_dim
    norm = _case_norm(env)
    mean32, inv32 = _table(norm)
    for rows in (1, 64, 65):
        x = R.stand_in_obs(rows, D)
        ref = R.normalize(x, mean32, inv32, R.CLIP)
        xd = _t(x)
        out = norm.normalize_dev(xd)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and np.array_equal(xd.cpu().numpy(), x)
        assert norm.normalize_dev(xd, out=xd) is xd                    # in place
        assert np.array_equal(xd.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        x3 = _t(np.stack([x, x]))                                      # [T, N, D]
        assert np.array_equal(norm.normalize_dev(x3).cpu().numpy()[1].view(np.uint32), ref.view(np.uint32))
    norm.close(); env.close()


# ---- 3. staging == apply_dev -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs", OBS, ids=OBS_IDS)
def test_staging_equals_apply_bit_for_bit(obs):
    import torch
    from gym_art_amd.policy import MLPCritic
    env = _env(obs)
    D = env.obs_dim
    norm = _case_norm(env)
    layers = _critic_layers([48, 16], D, 40 + D)
    with_norm, twin = MLPCritic.from_arrays(env, layers, "tanh"), MLPCritic.from_arrays(env, layers, "tanh")
    with_norm.set_obs_norm(norm)
    for rows in (1, 63, 64, 65, 130):
        x = _t(R.stand_in_obs(rows, D))
        v = with_norm.values_dev(x)
        ref = twin.values_dev(norm.normalize_dev(x))
        raw = twin.values_dev(x)
        assert torch.equal(v, ref), (D, rows)
        assert not torch.equal(v, raw)
    with_norm.set_obs_norm(None)
    assert torch.equal(with_norm.values_dev(x), raw)                   # detached: the plain kernel again
    with_norm.close(); twin.close(); norm.close(); env.close()


# ---- the nets of the rollout tests ---------------------------------------------------------------------------------------------------
class _Actor:
    """kind "mfma" / "bf16": an MLP of `widths`; "gru" / "lstm": a cell of widths[0] units and a bare head"""

    def __init__(self, kind, widths, D=18, seed=0, value=True):
        self.kind, self.widths, self.D = kind, widths, D
        self.act, self.out_tanh = "tanh", True
        if kind in ("mfma", "bf16"):
            self.layers = _scaled_layers(widths, D, seed)
            last = widths[-1]
        else:
            H = widths[0]
            self.cell = (_gru if kind == "gru" else _lstm)(H, D, seed, 1.0 / np.sqrt(D + H))
            self.layers = _head(H, (), seed + 1)
            last = H
        rng = np.random.RandomState(seed + 77)
        self.value = ((rng.randn(last) / np.sqrt(last)).astype(np.float32), np.float32(0.1)) if value and kind != "bf16" else None

    def build(self, env, norm=None, log_std=LOG_STD):
        from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPPolicy
        if self.kind in ("mfma", "bf16"):
            return MLPPolicy.from_arrays(env, self.layers, self.act, self.out_tanh, log_std, self.kind, self.value, norm)
        pol = (GRUPolicy if self.kind == "gru" else LSTMPolicy)(env, self.cell, self.layers, self.act, self.out_tanh, log_std, self.value)
        if norm is not None:
            pol.set_obs_norm(norm)
        return pol


def _rollout(env, pol, T, critic=None, term=True):
    """reset, zero the states, one rollout with everything the policy can give: dict of tensors"""
    import torch
    n, dev = env.num_envs, _dev()
    o0 = torch.empty((n, env.obs_dim), device=dev)
    env.reset_dev(o0)
    out = dict(obs0=o0.clone())
    if hasattr(pol, "reset_hidden"):
        pol.reset_hidden()
    o, r, d, a = _bufs(env, T)
    kw = {}
    if pol.value_head is not None or critic is not None:
        kw["values"] = torch.empty((T + 1, n), device=dev)
        if term:
            kw["term_values"] = torch.empty((T, n), device=dev)
    if pol.log_std is not None and pol.engine == "mfma":
        kw["logp"] = torch.empty((T, n), device=dev)
    if critic is not None:
        kw["critic"] = critic
    env.rollout_policy_dev(pol, o, r, d, a, **kw)
    torch.cuda.synchronize()
    out.update(obs=o, rew=r, done=d, actions=a, **{k: v for k, v in kw.items() if k != "critic"})
    for name in ("hidden", "cell"):
        if hasattr(pol, name):
            out[name] = getattr(pol, name).clone()
    return out


def _assert_same(a, b, what):
    import torch
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


# ---- 4. identity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,widths", [("mfma", [48, 16]), ("bf16", [48, 48]), ("gru", [48]), ("lstm", [48])])
def test_identity_table_changes_no_bit(kind, widths):
    """mean 0, var 1, eps 0, clip inf: the *_norm_kernel twins reproduce the plain kernels' rollout bit for bit -- actions, obs, reward,
    done, values, logp, term_values and the recurrent state; N = 68, T = 6, episodes of 3 steps so that auto-resets happen"""
    from gym_art_amd.policy import ObsNorm
    net = _Actor(kind, widths)
    runs = []
    for attach in (False, True):
        env = _env(OBS[2], 68, ep_time=0.03)
        norm = ObsNorm.from_stats(env, np.zeros(18), np.ones(18), 1.0, 0.0, float("inf")) if attach else None
        pol = net.build(env, norm)
        assert (pol.obs_norm is norm)
        runs.append(_rollout(env, pol, 6))
        pol.close(); env.close()
        if norm is not None:
            norm.close()
    assert int(runs[0]["done"].sum()) > 0
    if "term_values" in runs[0]:
        assert float(runs[0]["term_values"].abs().sum()) > 0
    _assert_same(runs[0], runs[1], kind)


# ---- 5. actors against fp64 ----------------------------------------------------------------------------------------------------------
T5 = 20
MARGIN = 8.0


def _torch_mlp32(layers, act, out_tanh, x32):
    import torch
    y = torch.from_numpy(np.asarray(x32, np.float32))
    with torch.no_grad():
        for k, (W, b) in enumerate(layers):
            y = torch.nn.functional.linear(y, torch.from_numpy(W), torch.from_numpy(b))
            if k < len(layers) - 1:
                y = torch.tanh(y) if act == "tanh" else torch.relu(y)
        return (torch.tanh(y) if out_tanh else y).numpy().astype(np.float64)


def _torch_gru_step32(gru):
    import torch
    W_ih, W_hh, b_ih, b_hh = gru
    cell = torch.nn.GRUCell(W_ih.shape[1], W_hh.shape[1])
    with torch.no_grad():
        for p, a in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), gru):
            p.copy_(torch.from_numpy(np.asarray(a, np.float32)))

    def step(x, h):
        with torch.no_grad():
            return cell(torch.from_numpy(np.asarray(x, np.float32)), torch.from_numpy(np.asarray(h, np.float32))).numpy().astype(np.float64)
    return step


def _gru_rollout32(net, obs0, obs, done):
    """the yardstick's GRU rollout: torch fp32 cell and head on the CPU over the given (normalised) inputs"""
    step, (actions, _) = _torch_gru_step32(net.cell), torch_head32(net.layers, net.act, net.out_tanh)
    h = np.zeros((obs.shape[1], net.widths[0]))
    acts = []
    for t in range(obs.shape[0]):
        h = step(obs0 if t == 0 else obs[t - 1], h)
        acts.append(actions(h))
        h = np.where(done[t][:, None] != 0, 0.0, h)
    return np.stack(acts), h


@pytest.mark.parametrize("layout", ["alias", "plain"])
@pytest.mark.parametrize("n", [68, 130])
@pytest.mark.parametrize("kind,widths", [("mfma", [48]), ("mfma", [256, 256, 256]), ("gru", [16]), ("lstm", [16])],
                         ids=["mfma48", "mfma256x3", "gru16", "lstm16"])
def test_actors_against_fp64_on_normalised_inputs(kind, widths, n, layout):
    """Deterministic actors with the case table attached, T = 20 with every env auto-resetting (episodes of 15 steps): action[t] (and a
    recurrent state) against the project's fp64 references fed the device's recorded observations normalised in fp64 WITH THE PUBLISHED
    fp32 TABLE, so that only the kernel's arithmetic is under test.
    Bar: inputs reach +-clip, so the existing bars do not carry over.  Yardstick = the error of a torch fp32 CPU evaluation of the same
    normalised inputs (rounded to fp32, as torch would be fed them) against the same fp64 reference; bar = MARGIN (8) x the yardstick's
    worst error, because the device sums in another order than torch's GEMM (k-ascending fmaf chains) and a worst case over ~20 x n x 4
    samples of two orders of the same-length sums differs by a small factor, not by an order of magnitude.  The test prints the worst
    device error as a fraction of the bar (the figures of a device run are not recorded yet: DESIGN.md section 4a).
    N = 130 stands for the 129 of two tiles and a sliver: a T > 1 rollout needs N x obs_dim x 4 to be a multiple of 16, so N is even."""
    env = _env(OBS[2], n, alias_obs=True if layout == "alias" else None)
    norm = _case_norm(env)
    mean32, inv32 = _table(norm)
    net = _Actor(kind, widths, value=False)
    pol = net.build(env, norm, log_std=None)
    run = {k: v.cpu().numpy() for k, v in _rollout(env, pol, T5).items()}
    assert int(run["done"][:-1].sum()) >= n
    z0, z = (R.normalize(run[k], mean32, inv32, R.CLIP, np.float64) for k in ("obs0", "obs"))
    hi, lo, inside = R.clip_census(z)
    assert hi > 0 and lo > 0 and inside > 0
    z0_32, z_32 = z0.astype(np.float32), z.astype(np.float32)
    if kind == "mfma":
        prev64, prev32 = np.concatenate([z0[None], z[:-1]]), np.concatenate([z0_32[None], z_32[:-1]])
        ref, _ = forward64(net.layers, net.act, net.out_tanh, prev64)
        ref = np.asarray(ref, np.float64)
        yard = np.abs(_torch_mlp32(net.layers, net.act, net.out_tanh, prev32) - ref).max()
        err = np.abs(run["actions"] - ref).max()
    elif kind == "gru":
        ra, rh = gru_reference(net.cell, net.layers, net.act, net.out_tanh, z0, z, run["done"], np.zeros((n, widths[0])))
        ya, yh = _gru_rollout32(net, z0_32, z_32, run["done"])
        yard = max(np.abs(ya - ra).max(), np.abs(yh - rh).max())
        err = max(np.abs(run["actions"] - ra).max(), np.abs(run["hidden"] - rh).max())
    else:
        zeros = np.zeros((n, widths[0]))
        ref = lstm_reference(net.cell, net.layers, net.act, net.out_tanh, z0, z, run["done"], zeros, zeros)
        y = lstm_reference(net.cell, net.layers, net.act, net.out_tanh, z0_32, z_32, run["done"], zeros, zeros, step=torch_step32(net.cell),
                           head=torch_head32(net.layers, net.act, net.out_tanh))
        yard = max(np.abs(y[k] - ref[k]).max() for k in ("a", "h", "c"))
        err = max(np.abs(run["actions"] - ref["a"]).max(), np.abs(run["hidden"] - ref["h"]).max(), np.abs(run["cell"] - ref["c"]).max())
    bar = MARGIN * yard
    print("%s %s n=%d %s: device error %.3g, torch fp32 yardstick %.3g, error / bar %.3g" % (kind, widths, n, layout, err, yard, err / bar))
    assert yard > 0 and err <= bar, (kind, widths, n, layout, err, yard)
    pol.close(); norm.close(); env.close()


# ---- 6. actor-critic -----------------------------------------------------------------------------------------------------------------
def _prev_obs(run):
    import torch
    return torch.cat([run["obs0"][None], run["obs"][:-1]])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_launches"])
@pytest.mark.parametrize("where", ["both", "actor", "critic", "two"])
@pytest.mark.parametrize("kind,widths", [("mfma", [48, 16]), ("gru", [48])], ids=["mlp", "gru"])
def test_separate_critic_with_a_normaliser(kind, widths, where, fused):
    """values, the bootstrap row and term_values from an MLPCritic with the normaliser on the actor only, the critic only, both, and
    ("two") a normaliser of its own with other statistics on each,
    fused and with GAQ_NO_FUSED_CRITIC=1: every value equals, bit for bit, a twin critic without a normaliser evaluated on
    normalize_dev of the recorded observation (or on the raw one where the critic has none) -- V of a row depends on that row alone;
    the actions equal those of the same actor in a rollout without a critic; row T of one call is row 0 of the next."""
    import torch
    from gym_art_amd.policy import MLPCritic, ObsNorm
    n, T = 129 + 3, 8
    env = _env(OBS[2], n, ep_time=0.03)
    term = torch.zeros((n, 18), device=_dev())
    env.set_terminal_obs(term)
    norm = _case_norm(env)
    net = _Actor(kind, widths, value=False)
    pol = net.build(env, norm if where in ("both", "actor", "two") else None)
    mean, var = R.case_stats(18)
    cnorm = ObsNorm.from_stats(env, mean[::-1].copy(), 2.0 * var, 1.0, R.EPS, 3.0) if where == "two" else norm
    cl = _critic_layers([80, 48], 18, 9)
    with environ(GAQ_NO_FUSED_CRITIC="0" if fused else "1"):
        crit = MLPCritic.from_arrays(env, cl, "tanh")
    twin = MLPCritic.from_arrays(env, cl, "tanh")
    if where in ("both", "critic", "two"):
        crit.set_obs_norm(cnorm)
    seen = (lambda x: cnorm.normalize_dev(x)) if where in ("both", "critic", "two") else (lambda x: x)
    run = _rollout(env, pol, T, critic=crit)
    prev = _prev_obs(run)
    assert torch.equal(run["values"][:T], twin.values_dev(seen(prev)))
    assert torch.equal(run["values"][T], twin.values_dev(seen(run["obs"][T - 1])))
    done = run["done"].bool()
    assert int(done.sum()) > 0 and torch.all(run["term_values"][~done] == 0)
    # the terminal observations of the last step are still in the registered buffer
    last = done[T - 1]
    assert int(last.sum()) == n
    assert torch.equal(run["term_values"][T - 1], twin.values_dev(seen(term)))
    # a second call: its row 0 is the first call's row T
    o, r, d, a = _bufs(env, 2)
    v2 = torch.empty((3, n), device=_dev())
    env.rollout_policy_dev(pol, o, r, d, a, values=v2, critic=crit)
    torch.cuda.synchronize()
    assert torch.equal(v2[0], run["values"][T])
    # the actor does not depend on the critic
    plain_env = _env(OBS[2], n, ep_time=0.03)
    pnorm = _case_norm(plain_env)
    ppol = net.build(plain_env, pnorm if where in ("both", "actor", "two") else None)
    plain = _rollout(plain_env, ppol, T)
    for k in ("actions", "obs", "done", "rew"):
        assert torch.equal(plain[k], run[k]), k
    for x in (pol, ppol, crit, twin, norm, pnorm, env, plain_env) + ((cnorm,) if where == "two" else ()):
        x.close()


@pytest.mark.parametrize("n", [1 * 4, 64, 68, 132])
def test_value_head_with_a_normaliser(n):
    """an MFMA policy's value head with the normaliser attached: values, the bootstrap row and term_values equal, bit for bit, a twin
    critic with the same hidden layers and that head (gaq.h: the same kernel stages) on normalize_dev of the recorded observations,
    terminal observations included (every env finishes in the same step: done counts 4, 64, 68 and 132 for the gathered pass)."""
    import torch
    from gym_art_amd.policy import MLPCritic
    T = 5
    env = _env(OBS[2], n, ep_time=0.03, init_random_state=False)
    term = torch.zeros((n, 18), device=_dev())
    env.set_terminal_obs(term)
    norm = _case_norm(env)
    net = _Actor("mfma", [48, 16])
    pol = net.build(env, norm)
    w, b = net.value
    twin = MLPCritic.from_arrays(env, net.layers[:-1] + [(w[None, :], np.asarray([b], np.float32))], "tanh")
    run = _rollout(env, pol, T)
    assert torch.equal(run["values"][:T], twin.values_dev(norm.normalize_dev(_prev_obs(run))))
    assert torch.equal(run["values"][T], twin.values_dev(norm.normalize_dev(run["obs"][T - 1])))
    done = run["done"].bool()
    counts = sorted(set(int(c) for c in done.sum(dim=1)))
    assert counts[-1] == n, counts                                 # a step in which every env finishes
    t_last = int(torch.nonzero(done.sum(dim=1) > 0)[-1])
    tv = twin.values_dev(norm.normalize_dev(term))
    raw = twin.values_dev(term)
    sel = done[t_last]
    assert torch.equal(run["term_values"][t_last][sel], tv[sel]) and not torch.equal(tv[sel], raw[sel])
    assert torch.all(run["term_values"][~done] == 0)
    for x in (pol, twin, norm, env):
        x.close()


# ---- 6b. value heads against tests/term_ref.py, the gathered pass at done counts 1, 63, 64, 65 and 129 ------------------------------
STAGGER = {"1+129": [0], "63+67": list(range(63)), "64+66": list(range(64)), "65+65": list(range(65))}
HEAD_NETS = [("mlp", [48, 16]), ("gru", 48, (16, 80)), ("lstm", 48)]


def _yard32(kind, net, z0, z, d, h0, c0, zt):
    """the yardstick of test_value_heads_against_fp64: (V [T + 1, N], V_term [T, N] where done) as torch fp32 computes them on the CPU
    from the same normalised inputs rounded to fp32"""
    T_, n = d.shape
    z0, z, zt = (np.asarray(a, np.float32) for a in (z0, z, zt))
    tv = np.zeros((T_, n))
    if kind == "lstm":
        y = lstm_reference(net.cell, net.layers, net.act, net.out_tanh, z0, z, d, h0, c0, value=net.value,
                           term_rows=np.broadcast_to(zt, (T_,) + zt.shape), step=torch_step32(net.cell),
                           head=torch_head32(net.layers, net.act, net.out_tanh, net.value))
        return y["v"], y["tv"]
    if kind == "mlp":
        _, v = torch_head32(net.layers, net.act, net.out_tanh, net.value)      # (its "trunk" is the whole MLP below the output layer)
        vals = np.stack([v(x) for x in np.concatenate([z0[None], z])])
        for t in range(T_):
            sel = d[t] != 0
            if sel.any():
                tv[t, sel] = v(zt[sel])
        return vals, tv
    step, (_, v) = _torch_gru_step32(net.gru), torch_head32(net.layers, net.act, net.out_tanh, net.value)
    h, vals = np.asarray(h0, np.float64), []
    for t in range(T_ + 1):
        hn = step(z0 if t == 0 else z[t - 1], h)
        vals.append(v(hn))
        if t == T_:
            break
        sel = d[t] != 0
        if sel.any():
            tv[t, sel] = v(step(zt[sel], hn[sel]))
        h = np.where(sel[:, None], 0.0, hn)
    return np.stack(vals), tv


@pytest.mark.parametrize("mask_id", list(STAGGER))
@pytest.mark.parametrize("spec", HEAD_NETS, ids=["mlp48-16", "gru48-16-80", "lstm48"])
def test_value_heads_against_fp64(spec, mask_id):
    """A value head on an MFMA, a GRU and an LSTM policy with the case table attached, N = 130, the staggered regime of
    tests/test_gpu_policy_term.py: the masked envs finish in window step 15, the rest in step 10 -- gathered passes of 129 and 1, 67 and
    63, 66 and 64, 65 and 65 rows.  values [T + 1, N] and term_values against the fp64 references (tests/ac_ref.py, tests/term_ref.py;
    the LSTM's is tests/lstm_util.py) fed the recorded observations, terminal rows included, normalised in fp64 with the published
    table; the states start from what the five steps before the window left.  Bar: MARGIN (8) x the worst error of the torch fp32 CPU
    evaluation of the same inputs (_yard32), for the reason given at test_actors_against_fp64_on_normalised_inputs.  Teeth: references
    on the raw terminal rows (the gathered pass skipping the table) and on a table shifted by one column are off by more than 100 bars."""
    import torch
    from tests import ac_ref, term_ref
    from tests.test_gpu_policy_ac import T, _Net
    from tests.test_gpu_policy_term import _one_done_each, _start, _zeros_are_plus_zero
    kind, n = spec[0], 130
    mask = np.zeros(n, bool)
    mask[STAGGER[mask_id]] = True
    env = _env(OBS[2], n)
    norm = _case_norm(env)
    mean32, inv32 = _table(norm)
    if kind == "lstm":
        net = _Actor("lstm", [spec[1]], seed=5)
        pol = net.build(env, norm)
    else:
        net = _Net(spec, np.ones(18), 4)
        pol = net.build(env)
        pol.set_obs_norm(norm)
    o0 = _start(env, pol, "staggered", mask)
    h0 = pol.hidden.cpu().numpy().astype(np.float64) if kind != "mlp" else None
    c0 = pol.cell.cpu().numpy().astype(np.float64) if kind == "lstm" else None
    tt = torch.full((n, 18), float("nan"), device=_dev())
    env.set_terminal_obs(tt)
    o, r, d, a = _bufs(env, T)
    v, tv = torch.full((T + 1, n), float("nan"), device=_dev()), torch.full((T, n), float("nan"), device=_dev())
    env.rollout_policy_dev(pol, o, r, d, a, values=v, term_values=tv)
    torch.cuda.synchronize()
    what = (spec, mask_id)
    at = _one_done_each(d, what).cpu().numpy()
    counts = d.to(torch.int32).sum(dim=1).cpu().numpy()
    assert counts[10] == n - int(mask.sum()) and counts[15] == int(mask.sum()) and counts.sum() == n, (what, counts)
    _zeros_are_plus_zero(tv, d, what)
    o0n, on, dn, rows = (x.cpu().numpy() for x in (o0, o, d, tt))
    assert np.isfinite(rows).all()
    norm64 = lambda x, inv=inv32: R.normalize(x, mean32, inv, R.CLIP, np.float64)
    z0, z, zt = norm64(o0n), norm64(on), norm64(rows)

    def reference(z0, z, zt):
        if kind == "mlp":
            _, vref, _ = ac_ref.mlp_means_values64(net.layers, net.act, net.out_tanh, net.value, np.concatenate([z0[None], z]))
            return np.asarray(vref), np.asarray(term_ref.mlp_term_values64(net, zt))
        if kind == "gru":
            _, vref, _ = ac_ref.gru_means_values64(net.gru, net.layers, net.act, net.out_tanh, net.value, z0, z, dn, h0)
            return vref, term_ref.gru_term_values64(net, z0, z, dn, h0, at, zt)
        y = lstm_reference(net.cell, net.layers, net.act, net.out_tanh, z0, z, dn, h0, c0, value=net.value,
                           term_rows=np.broadcast_to(zt, (T,) + zt.shape))
        return y["v"], y["tv"][at, np.arange(n)]

    vref, tref = reference(z0, z, zt)
    yv, ytv = _yard32(kind, net, z0, z, dn, h0, c0, zt)
    yard = max(np.abs(yv - vref).max(), np.abs(ytv[at, np.arange(n)] - tref).max())
    bar = MARGIN * yard
    verr = np.abs(v.cpu().numpy() - vref).max()
    terr = np.abs(tv.cpu().numpy()[at, np.arange(n)] - tref).max()
    print("%s %s: |V - V_ref| %.3g, |V_term - V_ref| %.3g, torch fp32 yardstick %.3g, worst error / bar %.3g"
          % (spec, mask_id, verr, terr, yard, max(verr, terr) / bar))
    _, t_raw = reference(z0, z, rows.astype(np.float64))
    v_roll, t_roll = reference(norm64(o0n, np.roll(inv32, -1)), norm64(on, np.roll(inv32, -1)), norm64(rows, np.roll(inv32, -1)))
    assert np.abs(t_raw - tref).max() > 100 * bar and np.abs(t_roll - tref).max() > 100 * bar and np.abs(v_roll - vref).max() > 100 * bar
    assert yard > 0 and verr <= bar and terr <= bar, (what, verr, terr, yard)
    for x in (pol, norm, env):
        x.close()


# ---- 5b. the bf16 engine against its contract's reference ---------------------------------------------------------------------------------
def _bf16_forward32(layers, act, out_tanh, x):
    """the yardstick: tests/policy_bf16_ref.py forward with the sums in torch fp32 on the CPU instead of fp64"""
    import torch
    from tests.policy_bf16_ref import bf16_round
    f = torch.tanh if act == "tanh" else torch.relu
    h = x.to(torch.float32)
    for k, (W, b) in enumerate(layers):
        z = torch.nn.functional.linear(bf16_round(h), bf16_round(torch.as_tensor(W)), torch.as_tensor(b).to(torch.float32))
        h = f(z) if k < len(layers) - 1 else (torch.tanh(z) if out_tanh else z)
    return h.to(torch.float64)


@pytest.mark.parametrize("layout", ["alias", "plain"])
@pytest.mark.parametrize("n", [68, 130])
def test_bf16_actor_against_its_reference_on_normalised_inputs(n, layout):
    """bf16 18-240-80-4 with the case table attached, T = 20 with every env auto-resetting: action[t] against
    tests/policy_bf16_ref.py forward on the recorded observations normalised in fp32 with the published table -- the contract: the
    element expression runs in fp32 and its result is what is rounded to bf16 (R.normalize in float32 is that expression bit for bit).
    Bar: MARGIN (8) x the worst error of the same contract evaluated with torch fp32 sums on the CPU (_bf16_forward32): both differ from
    the fp64 sums by units that round to the other bf16 neighbour, a handful per run, each worth one bf16 ulp of a unit times a weight.
    Teeth: the reference with the clamp dropped, and with the table shifted by one column, is off by more than 100 bars."""
    import torch
    from tests.policy_bf16_ref import forward as bf16_forward
    env = _env(OBS[2], n, alias_obs=True if layout == "alias" else None)
    norm = _case_norm(env)
    mean32, inv32 = _table(norm)
    net = _Actor("bf16", [240, 80])
    pol = net.build(env, norm, log_std=None)
    run = {k: v.cpu().numpy() for k, v in _rollout(env, pol, T5).items()}
    assert int(run["done"][:-1].sum()) >= n
    prev = np.concatenate([run["obs0"][None], run["obs"][:-1]]).reshape(-1, 18)
    fwd = lambda z: bf16_forward(net.layers, net.act, net.out_tanh, torch.from_numpy(np.ascontiguousarray(z, np.float32))).numpy()
    z = R.normalize(prev, mean32, inv32, R.CLIP)
    hi, lo, inside = R.clip_census(z)
    assert z.dtype == np.float32 and hi > 0 and lo > 0 and inside > 0
    ref = fwd(z)
    yard = np.abs(_bf16_forward32(net.layers, net.act, net.out_tanh, torch.from_numpy(z)).numpy() - ref).max()
    err = np.abs(run["actions"].reshape(-1, 4) - ref).max()
    bar = MARGIN * yard
    print("bf16 [240, 80] n=%d %s: device error %.3g, torch fp32 yardstick %.3g, error / bar %.3g" % (n, layout, err, yard, err / bar))
    assert np.abs(fwd(R.normalize(prev, mean32, inv32, np.inf)) - ref).max() > 100 * bar
    assert np.abs(fwd(R.normalize(prev, mean32, np.roll(inv32, -1), R.CLIP)) - ref).max() > 100 * bar
    assert yard > 0 and err <= bar, (n, layout, err, yard)
    pol.close(); norm.close(); env.close()


# ---- 7. a captured rollout -----------------------------------------------------------------------------------------------------------
def test_captured_rollout_sees_new_statistics():
    """graph-safe mode: capture a rollout with a normaliser attached, replay, update_dev eagerly on the same stream, replay again: the
    second replay equals an eager rollout on a twin whose normaliser took the same update (the table's address never changes)"""
    import torch
    from gym_art_amd.policy import ObsNorm
    n, T = 68, 6
    envs = [_env(OBS[2], n) for _ in range(2)]
    norms = [ObsNorm(e, R.EPS, R.CLIP) for e in envs]
    net = _Actor("mfma", [48, 16], value=False)
    pols = [net.build(e, nm) for e, nm in zip(envs, norms)]
    bufs = []
    for e in envs:
        e.set_graph_safe(True)
        e.reset_dev(torch.empty((n, 18), device=_dev()))
        bufs.append(_bufs(e, T))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # warm-up on a side stream (torch's capture protocol)
        envs[0].rollout_policy_dev(pols[0], *bufs[0])
    torch.cuda.current_stream().wait_stream(side)
    envs[1].rollout_policy_dev(pols[1], *bufs[1])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*bufs))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        envs[0].rollout_policy_dev(pols[0], *bufs[0])
    g.replay()
    envs[1].rollout_policy_dev(pols[1], *bufs[1])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*bufs))
    before = bufs[0][3].clone()
    fresh = _t(R.stand_in_obs(4097, 18) * np.float32(3.0) + np.float32(0.5))
    for nm in norms:
        nm.update_dev(fresh)                                       # eagerly, on the stream the replay runs on
    g.replay()
    envs[1].rollout_policy_dev(pols[1], *bufs[1])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*bufs))
    assert norms[0].count == 4097 and not torch.equal(bufs[0][3], before)
    for x in pols + norms + envs:
        x.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_usable():
    import ctypes as C
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import MLPCritic, MLPPolicy, ObsNorm
    lib = _lib.load()
    env, other = _env(OBS[2], 68), _env(OBS[2], 68)
    norm, foreign = _case_norm(env), _case_norm(other)
    net = _Actor("mfma", [48, 16], value=False)
    valu = MLPPolicy.from_arrays(env, net.layers, "tanh", True, None, "valu")
    with pytest.raises(ValueError, match="VALU engine"):
        valu.set_obs_norm(norm)
    assert valu.obs_norm is None
    with pytest.raises(ValueError, match="mfma|valu|engine"):
        MLPPolicy.from_arrays(env, net.layers, "tanh", True, None, "valu", None, norm).close()
    pol = net.build(env, None, None)
    crit = MLPCritic.from_arrays(env, _critic_layers([48], 18, 3), "tanh")
    for owner in (pol, crit):
        with pytest.raises(ValueError, match="another env"):
            owner.set_obs_norm(foreign)
        assert owner.obs_norm is None
    x = _t(R.stand_in_obs(8, 18))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h, p = norm.handle, x.data_ptr()
    assert lib.gaq_obs_norm_update_dev(h, 0, C.c_void_p(p), st) == -1
    assert lib.gaq_obs_norm_update_dev(h, -3, C.c_void_p(p), st) == -1
    assert lib.gaq_obs_norm_update_dev(h, 8, None, st) == -1
    assert lib.gaq_obs_norm_update_dev(h, 4, C.c_void_p(p + 2), st) == -1
    assert lib.gaq_obs_norm_update_dev(None, 8, C.c_void_p(p), st) == -1
    assert lib.gaq_obs_norm_apply_dev(h, 8, C.c_void_p(p), None, st) == -1
    assert lib.gaq_obs_norm_apply_dev(h, 4, C.c_void_p(p), C.c_void_p(p + 1), st) == -1
    assert lib.gaq_obs_norm_apply_dev(h, 0, C.c_void_p(p), C.c_void_p(p), st) == -1
    out = C.c_void_p()
    assert lib.gaq_obs_norm_create(env._handle, C.c_float(-1.0), C.c_float(5.0), C.byref(out)) == -1 and not out.value
    assert lib.gaq_obs_norm_create(env._handle, C.c_float(1e-5), C.c_float(0.0), C.byref(out)) == -1 and not out.value
    with pytest.raises(ValueError):
        norm.update_dev(x[:, :17])
    # nothing was launched or changed, and good calls follow
    assert norm.count == 1.0
    norm.update_dev(x)
    assert norm.count == 9.0
    pol.set_obs_norm(norm); crit.set_obs_norm(norm)
    run = _rollout(env, pol, 3, critic=crit, term=False)
    assert torch.isfinite(run["values"]).all()
    _rollout(env, valu, 2)
    for o in (pol, crit, valu, norm, foreign, env, other):
        o.close()


# ---- 9. checkpoint -----------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip():
    import torch
    from gym_art_amd.policy import ObsNorm
    net = _Actor("gru", [48])
    data = _t(R.stand_in_obs(4097, 18) * np.float32(2.0))
    runs, tables = [], []
    state = None
    for restored in (False, True):
        env = _env(OBS[2], 68, ep_time=0.03)
        norm = ObsNorm(env, R.EPS, R.CLIP)
        if restored:
            norm.load_state_dict(state)
        else:
            norm.update_dev(data)
            state = norm.state_dict()
            with pytest.raises(ValueError, match="clip"):
                ObsNorm(env, R.EPS, 3.0).load_state_dict(state)
        probe = _t(R.stand_in_obs(2, 18))
        tables.append(norm.normalize_dev(probe))
        assert all(np.array_equal(norm.state_dict()[k], state[k]) for k in ("mean", "m2")) and norm.count == state["count"]
        pol = net.build(env, norm)
        runs.append(_rollout(env, pol, 6))
        pol.close(); norm.close(); env.close()
    assert torch.equal(tables[0], tables[1])
    _assert_same(runs[0], runs[1], "checkpoint")
