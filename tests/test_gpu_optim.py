"""Adam on the device (gaq.h "the optimiser on the device", gym_art_amd.policy.AdamDev) against the fp64 reference of
tests/optim_ref.py: the case matrix under the bound 8 x torch fp32's committed error, the weights stepped in place where the rollout
and gradient kernels read them, the skip rule, determinism, a captured gradient + step, two closed loops beside torch, the state round
trip and the refusals.  Every figure a test bounds is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import optim_ref as R
from tests import policy_grad_ac_ref as A
from tests import policy_grad_seq_ref as S
from tests.gru_util import _gru, _head
from tests.lstm_util import _lstm
from tests.policy_util import _bufs, _dev, _layers

G = A.G
pytestmark = pytest.mark.gpu

REPR = {18: "xyz_vxyz_R_omega", 19: "xyz_vxyz_R_omega_h"}


def _make_env(D=18, n=64):
    from gym_art_amd import QuadrotorEnv
    env = QuadrotorEnv(num_envs=n, ep_time=0.15, seed=7, init_random_state=True, auto_reset=True, alias_obs=True, obs_repr=REPR[D])
    assert env.obs_dim == D
    return env


@pytest.fixture(scope="module")
def envs():
    made = {}

    def get(D=18, n=64, twin=0):
        if (D, n, twin) not in made:
            made[(D, n, twin)] = _make_env(D, n)
        return made[(D, n, twin)]
    yield get
    for e in made.values():
        e.close()


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=_dev())


def _np(t):
    return t.detach().cpu().numpy()


def _build(case, env, theta=None, explore=True):
    """the case's handle with theta (default: the case's theta0) as its packed weights, value head and log_std"""
    from gym_art_amd import _lib
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPCritic, MLPPolicy
    th = R.theta0(case) if theta is None else theta
    log_std = th[2] if case.log_std and explore else None
    value = (th[1][:-1], th[1][-1]) if case.head else None
    if case.kind == "critic":
        layers = _layers(case.widths, case.D)
        net = MLPCritic.from_arrays(env, layers[:-1] + [(layers[-1][0][:1], layers[-1][1][:1])])
        _lib.check(net._lib.gaq_critic_set_weights(net.handle, _lib.ptr(th[0])))
        return net
    if case.kind == "mlp":
        net = MLPPolicy.from_arrays(env, _layers(case.widths, case.D), "tanh", True, log_std=log_std, engine=case.engine, value=value)
    elif case.kind == "gru":
        net = GRUPolicy(env, _gru(case.widths[0], case.D), _head(case.widths[0], case.widths[1:]), "tanh", True, log_std=log_std, value=value)
    else:
        net = LSTMPolicy(env, _lstm(case.widths[0], case.D), _head(case.widths[0], case.widths[1:]), "tanh", True, log_std=log_std,
                         value=value)
    assert net._count == case.weight_count
    _lib.check(net._lib.gaq_policy_set_weights(net.handle, _lib.ptr(th[0])))     # (the step is elementwise: any packed contents do)
    return net


def _optim(case, net, **kw):
    from gym_art_amd.policy import AdamDev
    return AdamDev(net, **dict(case.hp, **kw))


def _grads(case, k):
    """step k's gradients on the device as step() takes them: (grad, grad_value or None, grad_log_std or None)"""
    g = R.gradients(case, k)
    return _t(g[0]), _t(g[1]) if case.head else None, _t(g[2]) if case.log_std else None


def _read(case, net, opt):
    """(theta, m, v) per group, read back from the handle and the optimiser, then (step, skipped)"""
    sd = opt.state_dict()
    theta = [net.get_packed(), np.zeros(0, np.float32), np.zeros(0, np.float32)]
    if case.head:
        w, b = net.get_value_head()
        theta[1] = np.concatenate([w, [b]]).astype(np.float32)
    if opt.steps_log_std:
        opt.sync_log_std()
        theta[2] = np.asarray(net.log_std, np.float32).copy()
    n = np.cumsum([0] + [x.size for x in theta])
    assert n[-1] == sd["m"].size == sd["v"].size == opt._count
    m = [sd["m"][n[k]:n[k + 1]] for k in range(3)]
    v = [sd["v"][n[k]:n[k + 1]] for k in range(3)]
    return theta, m, v, (sd["step"], sd["skipped"])


def _bits(x):
    return [np.asarray(a, np.float32).view(np.uint32).copy() for part in x[:3] for a in part] + [x[3]]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _check_against_reference(case, got, ref, steps, what):
    worst = 0.0
    for i, name in enumerate(("theta", "m", "v")):
        for gidx in range(3):
            e, b = R.rel(got[i][gidx], ref[i][gidx]), R.bound(case.name, steps, name, gidx)
            print("%s %s after %d steps: %s of %s differs by %.3g (bound %.3g)" % (case.name, what, steps, name, R.GROUPS[gidx], e, b))
            assert got[i][gidx].size == ref[i][gidx].size and e <= b, (case.name, what, steps, name, gidx, e, b)
            worst = max(worst, e / b)
    return worst


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case_matrix(case, envs):
    """theta, m and v of every group after 1, 2 and 10 steps with changing gradients within 8 x torch fp32's error (never
    below k x 2^-24); every step's norm and coef to 1e-6 relative, the step count and the skipped count exact"""
    import torch
    net = _build(case, envs(case.D))
    opt = _optim(case, net)
    assert [g[2] for g in opt.groups] == [s for s in case.sizes if s]
    ref = R.reference(case.name)
    stats = torch.zeros(4, dtype=torch.float64, device=_dev())
    coefs = []
    for k in range(R.STEPS):
        opt.step(*_grads(case, k), stats=stats, sync_log_std=(k % 2 == 0))
        st, want = _np(stats), ref[k][3]
        e_norm, e_coef = R.rel(st[0], want[0]), R.rel(st[1], want[1])
        print("%s step %d: norm %.9g (off by %.3g) coef %.9g (off by %.3g) t %d skipped %d" % (case.name, k + 1, st[0], e_norm, st[1], e_coef,
                                                                                             st[2], st[3]))
        assert e_norm <= 1e-6 and e_coef <= 1e-6 and st[2] == k + 1 and st[3] == 0.0
        coefs.append(st[1])
        if k + 1 in R.AT:
            got = _read(case, net, opt)
            _check_against_reference(case, got, ref[k], k + 1, "default")
            assert got[3] == (k + 1, 0)
    if case.clip == "above":
        assert max(coefs) < 0.05
    if case.clip == "below":
        assert min(coefs) == 1.0
    if case.hp["max_grad_norm"] is None:
        assert min(coefs) == 1.0
    assert net.packed is None
    opt.close()
    net.close()


def test_the_one_launch_form_meets_the_same_bounds(envs):
    """GAQ_OPTIM_LAUNCHES=1 (read at creation): the single-workgroup form on the largest case and on the three-group smallest"""
    from tests.policy_util import environ
    for name in ("mlp128x128x128", "mlp16-head-logstd"):
        case = R.BY_NAME[name]
        net = _build(case, envs(case.D))
        with environ(GAQ_OPTIM_LAUNCHES="1"):
            opt = _optim(case, net)
        ref = R.reference(name)
        for k in range(R.STEPS):
            opt.step(*_grads(case, k), sync_log_std=False)
        got = _read(case, net, opt)
        _check_against_reference(case, got, ref[R.STEPS - 1], R.STEPS, "one launch")
        assert got[3] == (R.STEPS, 0)
        opt.close()
        net.close()


def test_the_handle_flies_with_the_stepped_weights(envs):
    """after a step, logp_dev and the mean from the stepped handle equal, bit for bit, those of a fresh handle built from
    get_weights(), and so does a deterministic 3-step rollout at N = 65"""
    import torch
    from gym_art_amd.policy import MLPPolicy
    case = R.BY_NAME["mlp16-head-logstd"]
    env_a, env_b = envs(18, 65, 0), envs(18, 65, 1)
    net = _build(case, env_a)
    opt = _optim(case, net)
    before = net.get_packed()
    opt.step(*_grads(case, 0))
    layers = net.get_weights()
    assert not np.array_equal(before, net.get_packed())
    w, b = net.get_value_head()
    fresh = MLPPolicy.from_arrays(env_b, layers, "tanh", True, log_std=net.log_std, engine="mfma", value=(w, b))
    assert np.array_equal(fresh.packed, net.get_packed())
    rng = np.random.RandomState(5)
    obs, act = _t(rng.randn(65, 18).astype(np.float32)), _t(rng.randn(65, 4).astype(np.float32))
    m1, m2 = (torch.full((65, 4), float("nan"), device=_dev()) for _ in range(2))
    lp1, lp2 = net.logp_dev(obs, act, mean=m1), fresh.logp_dev(obs, act, mean=m2)
    torch.cuda.synchronize()
    assert torch.equal(lp1.view(torch.int32), lp2.view(torch.int32)) and torch.equal(m1.view(torch.int32), m2.view(torch.int32))
    ls = np.asarray(net.log_std).copy()
    net.set_log_std(None)                                        # the deterministic rollout
    fresh.set_log_std(None)
    # (three calls of one step each: a call of T > 1 needs N * obs_dim * 4 bytes to be a multiple of 16, which 65 x 18 floats are not)
    runs = []
    for env, pol in ((env_a, net), (env_b, fresh)):
        o0 = torch.empty((65, 18), device=_dev())
        env.reset_dev(o0)
        out = [o0.clone()]
        for _ in range(3):
            bufs = _bufs(env, 1)
            env.rollout_policy_dev(pol, *bufs)
            out += [x.clone() for x in bufs]
        torch.cuda.synchronize()
        runs.append(out)
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert float(runs[0][4].abs().sum()) > 0.0                  # (the first step's actions)
    net.set_log_std(ls)
    opt.close()
    net.close()
    fresh.close()


@pytest.mark.parametrize("name", ["valu64x64-d19", "gru16", "gru64x64x64-head", "lstm16", "critic16"])
def test_every_kind_of_handle_flies_with_the_stepped_weights(name, envs):
    """the same for the other kinds of handle: after two steps a VALU, GRU or LSTM policy's deterministic 3-step rollout at N = 65
    (recurrent state included), and a critic's values, equal bit for bit those of a fresh handle built from get_weights()"""
    import torch
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy, MLPCritic, MLPPolicy
    case = R.BY_NAME[name]
    env_a, env_b = envs(case.D, 65, 0), envs(case.D, 65, 1)
    net = _build(case, env_a)
    opt = _optim(case, net)
    before = net.get_packed()
    for k in range(2):
        opt.step(*_grads(case, k))
    assert not np.array_equal(before, net.get_packed())
    if case.kind == "critic":
        fresh = MLPCritic.from_arrays(env_b, net.get_weights())
        obs = _t(np.random.RandomState(5).randn(65, case.D).astype(np.float32))
        va, vb = net.values_dev(obs), fresh.values_dev(obs)
        torch.cuda.synchronize()
        assert torch.equal(va.view(torch.int32), vb.view(torch.int32)) and float(va.abs().sum()) > 0.0
    else:
        value = net.get_value_head() if case.head else None
        if case.kind == "mlp":
            fresh = MLPPolicy.from_arrays(env_b, net.get_weights(), "tanh", True, engine=case.engine)
        else:
            cell, head = net.get_weights()
            fresh = (GRUPolicy if case.kind == "gru" else LSTMPolicy)(env_b, cell, head, "tanh", True, value=value)
        assert np.array_equal(fresh.packed, net.get_packed())
        opt.close()                                              # (the optimiser owns log_std while it lives)
        net.set_log_std(None)                                    # the deterministic rollout
        runs = []
        for env, pol in ((env_a, net), (env_b, fresh)):
            o0 = torch.empty((65, case.D), device=_dev())
            env.reset_dev(o0)
            out = [o0.clone()]
            for _ in range(3):                                   # (one step per call: 65 x D floats are no multiple of 16 bytes)
                bufs = _bufs(env, 1)
                if case.head:
                    v = torch.empty((2, 65), device=_dev())
                    env.rollout_policy_dev(pol, *bufs, values=v)
                    out.append(v.clone())
                else:
                    env.rollout_policy_dev(pol, *bufs)
                out += [x.clone() for x in bufs]
            out += [getattr(pol, s).clone() for s in getattr(pol, "CELL", None).states] if case.kind != "mlp" else []
            torch.cuda.synchronize()
            runs.append(out)
        for x, y in zip(*runs):
            assert torch.equal(x, y)
        assert float(bufs[3].abs().sum()) > 0.0                  # (the last step's actions)
    opt.close()
    net.close()
    fresh.close()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_gradient_skips_the_step(bad, envs):
    """one NaN, and separately one Inf, in each group in turn: theta, m, v and t keep their bits, the skipped counter and stats[3]
    are 1, and the next finite step leaves exactly the bits of a twin that never saw the bad call and matches the reference"""
    import torch
    case = R.BY_NAME["mlp16-head-logstd"]
    ref = R.reference(case.name)[1]                              # after the finite steps 0 and 1: the skipped call leaves no trace
    twin = _build(case, envs(case.D))
    topt = _optim(case, twin)
    topt.step(*_grads(case, 0))
    topt.step(*_grads(case, 1))
    want = _read(case, twin, topt)
    stats = torch.zeros(4, dtype=torch.float64, device=_dev())
    for group in range(3):
        net = _build(case, envs(case.D))
        opt = _optim(case, net)
        opt.step(*_grads(case, 0))
        before = _read(case, net, opt)
        g = [x.clone() for x in _grads(case, 1)]
        g[group][g[group].numel() // 2] = bad
        opt.step(*g, stats=stats)
        after = _read(case, net, opt)
        st = _np(stats)
        print("group %s with %r: stats %s, step %d skipped %d" % (R.GROUPS[group], bad, st, after[3][0], after[3][1]))
        assert all(np.array_equal(x, y) for x, y in zip(_bits(before)[:-1], _bits(after)[:-1]))
        assert before[3] == (1, 0) and after[3] == (1, 1) and st[3] == 1.0 and st[2] == 1.0 and st[1] == 0.0 and not np.isfinite(st[0])
        assert opt.skipped == 1 and opt.step_count == 1
        opt.step(*_grads(case, 1), stats=stats)                  # the same gradients without the bad element
        got = _read(case, net, opt)
        assert got[3] == (2, 1) and _np(stats)[3] == 0.0
        assert all(np.array_equal(x, y) for x, y in zip(_bits(got)[:-1], _bits(want)[:-1]))
        for i, name in enumerate(("theta", "m", "v")):
            for gi in range(3):
                e, b = R.rel(got[i][gi], ref[i][gi]), R.bound(case.name, 2, name, gi)
                print("after the skipped call: %s of %s differs by %.3g (bound %.3g)" % (name, R.GROUPS[gi], e, b))
                assert e <= b
        assert np.isfinite(net.get_packed()).all()
        opt.close()
        net.close()
    topt.close()
    twin.close()


def _loaded_step(case, env, stream=None):
    """a fresh handle and optimiser, a loaded state (t = 3, seeded moments), one step: everything read back"""
    import torch
    net = _build(case, env)
    opt = _optim(case, net)
    rng = np.random.RandomState(11)
    state = {"step": 3, "skipped": 2, "m": rng.uniform(-1, 1, opt._count).astype(np.float32),
             "v": rng.uniform(0, 1, opt._count).astype(np.float32)}
    opt.load_state_dict(state)
    g = _grads(case, 4)
    stats = torch.zeros(4, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    if stream is None:
        opt.step(*g, stats=stats)
    else:
        with torch.cuda.stream(stream):
            opt.step(*g, stats=stats)
        stream.synchronize()
    out = _read(case, net, opt)
    st = _np(stats).copy()
    opt.close()
    net.close()
    return out, st


def test_determinism(envs):
    """the same step twice from the same loaded state, and once on another stream: equal bits, statistics included"""
    import torch
    for name in ("mlp128x128x128", "mlp16-head-logstd"):
        case = R.BY_NAME[name]
        a, sa = _loaded_step(case, envs(case.D))
        b, sb = _loaded_step(case, envs(case.D))
        c, sc = _loaded_step(case, envs(case.D), torch.cuda.Stream(device=_dev()))
        assert a[3] == (4, 2) and sa[2] == 4.0
        assert _same(a, b) and _same(a, c) and np.array_equal(sa, sb) and np.array_equal(sa, sc)


def _ac_pieces(envs, name="ac-64x64-tanh-vclip"):
    from tests.test_gpu_policy_grad_ac import _call, _dev_inputs, _policy
    case, inp = A.case_inputs(name)
    return case, inp, _call, _dev_inputs(inp), (lambda: _policy(envs(), case, inp)[0])


def test_a_captured_gradient_and_step_replays_with_the_eager_bits(envs):
    """ppo_ac_grad_dev + step at 453 rows, captured on a side stream after one warm-up, with sync_log_std=False and
    learn_log_std=False: 5 replays equal 5 eager iterations bit for bit -- weights, head, moments and t = 5 -- with set_lr between
    iterations 2 and 3 on both sides"""
    import torch
    case, inp, call, d, make = _ac_pieces(envs)
    hp = dict(lr=3e-4, max_grad_norm=0.5, weight_decay=1e-2, learn_log_std=False)
    from gym_art_amd.policy import AdamDev

    def read(pol, opt):
        sd = opt.state_dict()
        w, b = pol.get_value_head()
        return [pol.get_packed(), w, np.float32(b), sd["m"], sd["v"]], (sd["step"], sd["skipped"])

    eager, eopt = make(), None
    eopt = AdamDev(eager, **hp)
    for k in range(5):
        if k == 2:
            eopt.set_lr(1e-3)
        g, gv, gls, st = call(eager, case, d)
        eopt.step(g, gv, gls, sync_log_std=False)
    want = read(eager, eopt)
    assert want[1] == (5, 0)

    pol = make()
    opt = AdamDev(pol, **hp)
    start = read(pol, opt)
    out = [torch.empty_like(x) for x in call(pol, case, d)]      # the warm-up of the gradient call (it sizes the handle's scratch)
    opt.step(out[0], out[1], out[2], sync_log_std=False)          # ... and of the step, undone below
    pol._lib.gaq_policy_set_weights(pol.handle, C.c_void_p(start[0][0].ctypes.data))
    pol.set_value_head(start[0][1], start[0][2])
    opt.load_state_dict({"step": 0, "skipped": 0, "m": start[0][3], "v": start[0][4]})
    assert all(np.array_equal(x, y) for x, y in zip(read(pol, opt)[0], start[0]))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(pol, case, d, grad=out[0], grad_value=out[1], grad_log_std=out[2], stats=out[3])
        opt.step(out[0], out[1], out[2], sync_log_std=False)
    assert opt.step_count == 0                                    # capturing ran nothing
    for k in range(5):
        if k == 2:
            opt.set_lr(1e-3)
        graph.replay()
        torch.cuda.synchronize()
    got = read(pol, opt)
    assert got[1] == (5, 0)
    for x, y in zip(got[0], want[0]):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert not np.array_equal(got[0][0], start[0][0])
    for x in (opt, pol, eopt, eager):
        x.close()


def test_closed_loop_on_the_shared_trunk_case(envs):
    """Ten steps (lr 3e-4, max_grad_norm 0.5) on the 453 rows: ppo_ac_grad_dev -> AdamDev.step, beside torch fp32 autograd +
    clip_grad_norm_ + torch.optim.Adam on the twin module.  Each parameter tensor ends within 100 x the single-step gradient bound
    (tests/test_gpu_policy_grad_ac.py's rule) and both losses fall."""
    import torch
    from gym_art_amd.policy import AdamDev
    case, inp, call, d, make = _ac_pieces(envs)
    pol = make()
    lr, steps, mgn = 3e-4, 10, 0.5
    ent_const = float(A.ENT_COEF * 2.0 * (1.0 + np.log(2.0 * np.pi)))
    opt = AdamDev(pol, lr=lr, max_grad_norm=mgn)
    assert [g[0] for g in opt.groups] == ["weights", "value_head", "log_std"]
    stats = torch.zeros(4, dtype=torch.float64, device=_dev())
    loss_dev, coefs = [], []
    for _ in range(steps):
        ls = np.asarray(pol.log_std, np.float64)
        g, gv, gls, st = call(pol, case, d)
        opt.step(g, gv, gls, stats=stats)
        loss_dev.append((float(st[0]) + A.VF_COEF * float(st[3])) / A.R - A.ENT_COEF * float(ls.sum()) - ent_const)
        coefs.append(float(stats[1]))
    model = A.torch_model(case, inp, torch.float32)
    trunk, actor, critic, ls = model
    leaves = list(trunk.parameters()) + list(actor.parameters()) + list(critic.parameters()) + [ls]
    topt = torch.optim.Adam(leaves, lr=lr)
    loss_ref = []
    for _ in range(steps):
        topt.zero_grad()
        loss = A.torch_loss(case, inp, A.R, torch.float32, model)[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, mgn)
        loss_ref.append(float(loss.detach()))
        topt.step()
    print("closed loop: loss %s on the device, %s in torch; coef %s" % (["%.6f" % x for x in loss_dev], ["%.6f" % x for x in loss_ref],
                                                                      ["%.4f" % c for c in coefs]))
    bound = 100.0 * A.bounds(case.name, A.R)[0]
    lins = [m for m in trunk if hasattr(m, "weight")] + [actor]
    w, b = pol.get_value_head()
    got = [x for Wb in pol.get_weights() for x in Wb] + [np.concatenate([w, [b]]), np.asarray(pol.log_std)]
    want = [_np(p) for m in lins for p in (m.weight, m.bias)] + [np.concatenate([_np(critic.weight).reshape(-1), _np(critic.bias).reshape(-1)]),
                                                                   _np(ls)]
    errs = [G.rel(a, b_) for a, b_ in zip(got, want)]
    print("closed loop: parameters after %d steps differ by %.3g at most (bound %.3g)" % (steps, max(errs), bound))
    assert max(errs) <= bound, (errs, bound)
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    assert opt.step_count == steps and opt.skipped == 0
    opt.close()
    pol.close()


def test_closed_loop_on_the_gru_case(envs):
    """Ten steps at (T, S) = (6, 130): ppo_seq_grad_dev -> AdamDev.step, beside torch fp32 autograd + clip_grad_norm_ + Adam on the
    twin module (tests/test_gpu_policy_grad_seq.py's).  Each parameter tensor ends within 100 x the single-step gradient bound and both
    losses fall."""
    import torch
    from gym_art_amd.policy import AdamDev
    from tests.test_gpu_policy_grad_seq import _call, _dev_inputs, _policy
    case, inp = S.case_inputs("gru64x16x48-tanh-vclip")
    pol, _ = _policy(envs(), case, inp)
    T, Sq = S.TMAX, S.SMAX
    assert (T, Sq) == (6, 130)
    d = _dev_inputs(inp, T, Sq)
    lr, steps, mgn = 3e-4, 10, 0.5
    ent_const = float(S.ENT_COEF * 2.0 * (1.0 + np.log(2.0 * np.pi)))
    opt = AdamDev(pol, lr=lr, max_grad_norm=mgn)
    loss_dev = []
    for _ in range(steps):
        ls = np.asarray(pol.log_std, np.float64)
        g, gv, gls, st = _call(pol, case, d)
        opt.step(g, gv, gls)
        loss_dev.append((float(st[0]) + S.VF_COEF * float(st[3])) / (T * Sq) - S.ENT_COEF * float(ls.sum()) - ent_const)
    model = S.torch_model(case, inp, torch.float32)
    cell, lins, critic, ls = model
    tens = S.torch_tensors(inp, T, Sq, torch.float32)
    leaves = list(cell.parameters()) + [p for l in lins for p in l.parameters()] + list(critic.parameters()) + [ls]
    topt = torch.optim.Adam(leaves, lr=lr)
    loss_ref = []
    for _ in range(steps):
        topt.zero_grad()
        loss = S.torch_loss(case, tens, T, Sq, model)[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, mgn)
        loss_ref.append(float(loss.detach()))
        topt.step()
    print("closed loop (GRU): loss %s on the device, %s in torch" % (["%.6f" % x for x in loss_dev], ["%.6f" % x for x in loss_ref]))
    bound = 100.0 * S.bounds(case.name, T, Sq)[0]
    gru, head = pol.get_weights()
    w, b = pol.get_value_head()
    got = [gru[0], gru[2], gru[1], gru[3]] + [x for Wb in head for x in Wb] + [np.concatenate([w, [b]]), np.asarray(pol.log_std)]
    want = [_np(p) for p in (cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh)] + [_np(p) for l in lins for p in (l.weight, l.bias)] + \
           [np.concatenate([_np(critic.weight).reshape(-1), _np(critic.bias).reshape(-1)]), _np(ls)]
    errs = [G.rel(a, b_) for a, b_ in zip(got, want)]
    print("closed loop (GRU): parameters after %d steps differ by %.3g at most (bound %.3g)" % (steps, max(errs), bound))
    assert max(errs) <= bound, (errs, bound)
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    opt.close()
    pol.close()


def test_state_round_trip(envs):
    """state_dict after 3 steps, loaded into a fresh optimiser on a twin handle built from get_weights(): 2 more steps on each leave
    equal bits.  A state of the wrong size is refused."""
    case = R.BY_NAME["gru64x64x64-head"]
    net = _build(case, envs(case.D))
    opt = _optim(case, net)
    for k in range(3):
        opt.step(*_grads(case, k))
    sd = opt.state_dict()
    assert sd["step"] == 3 and sd["m"].size == sum(case.sizes)
    w, b = net.get_value_head()
    twin = _build(case, envs(case.D), theta=[net.get_packed(), np.concatenate([w, [b]]).astype(np.float32), np.asarray(net.log_std)])
    topt = _optim(case, twin, lr=1.0)                            # (the state brings the learning rate)
    topt.load_state_dict(sd)
    assert topt.lr == case.hp["lr"]
    for k in (3, 4):
        opt.step(*_grads(case, k))
        topt.step(*_grads(case, k))
    a, b_ = _read(case, net, opt), _read(case, twin, topt)
    assert a[3] == b_[3] == (5, 0) and _same(a, b_)
    other = _build(R.BY_NAME["gru16"], envs())
    oopt = _optim(R.BY_NAME["gru16"], other)
    with pytest.raises(ValueError, match="floats"):
        oopt.load_state_dict(sd)
    for x in (oopt, other, topt, twin, opt, net):
        x.close()


def test_refusals(envs):
    """each launches nothing and leaves the handle usable: afterwards the weights have their bits, t is 0, and one step gives a
    twin's bits"""
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import ENGINES, AdamDev, MLPPolicy, _DescEx, _fill_desc, optim_desc
    lib = _lib.load()
    env = envs()
    err = lib.gaq_last_error
    cs = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    # the bf16 engine: refused, the text names the engine
    bf = MLPPolicy.from_arrays(env, _layers([32, 32]), "tanh", True, engine="bf16")
    with pytest.raises(ValueError, match="bf16 engine"):
        AdamDev(bf)
    bf.close()
    # weights never set
    d = _fill_desc(_DescEx(), 18, [16], "tanh", out_tanh=1, engine=ENGINES["mfma"])
    h, o = C.c_void_p(), C.c_void_p()
    assert lib.gaq_policy_create_ex(env._handle, C.byref(d), C.byref(h)) == 0
    desc = optim_desc()
    assert lib.gaq_optim_create_policy(h, C.byref(desc), C.byref(o)) == -1 and b"weights not set" in err() and o.value is None
    lib.gaq_policy_destroy(h)
    # hyper-parameters
    case = R.BY_NAME["mlp16-head-logstd"]
    net = _build(case, env)
    for kw in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.5)), dict(eps=0.0), dict(lr=-1.0), dict(lr=float("nan")),
               dict(weight_decay=-1.0), dict(weight_decay=float("nan")), dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError):
            AdamDev(net, **kw)
    opt = _optim(case, net)
    before = _read(case, net, opt)
    g, gv, gls = _grads(case, 0)

    def raw(grad=g, grad_value=gv, grad_ls=gls, stats=None):
        return lib.gaq_optim_step_dev(opt.handle, _lib.ptr(grad), _lib.ptr(grad_value), _lib.ptr(grad_ls), _lib.ptr(stats), cs)
    assert raw(grad=None) == -1 and b"null" in err()
    assert raw(grad=g.data_ptr() + 2) == -1 and b"aligned" in err()
    assert raw(grad_value=gv.data_ptr() + 1) == -1 and b"aligned" in err()
    assert raw(stats=torch.zeros(4, dtype=torch.float64, device=_dev()).data_ptr() + 4) == -1 and b"aligned" in err()
    assert raw(grad_value=None) == -1 and b"grad_value is required" in err()
    assert raw(grad_ls=None) == -1 and b"grad_log_std is required" in err()
    with pytest.raises(ValueError, match="grad_value is required"):
        opt.step(g, None, gls)
    with pytest.raises(ValueError, match="lr"):
        opt.set_lr(-1.0)
    assert lib.gaq_optim_set_lr_dev(opt.handle, float("nan"), cs) == -1 and b"lr" in err()
    # the head removed since creation: GAQ_ERR_STATE; put back: usable again
    net.set_value_head(None)
    assert raw() == -4 and b"value head" in err()
    net.set_value_head(before[0][1][:-1], before[0][1][-1])
    # log_std set behind the optimiser that steps it, or exploration switched off: GAQ_ERR_STATE from step and sync, nothing
    # overwritten; the optimiser's own values put back: usable again
    mine = np.asarray(net.log_std, np.float32).copy()
    net.set_log_std(mine + 0.25)
    assert raw() == -4 and b"log_std was set on the policy" in err()
    assert lib.gaq_optim_sync_log_std(opt.handle, cs) == -4 and b"log_std was set on the policy" in err()
    with pytest.raises(_lib.GaqError, match="log_std"):
        opt.sync_log_std()
    assert np.array_equal(net.log_std, mine + 0.25)
    net.set_log_std(None)
    assert raw() == -4 and b"deterministic" in err()
    assert lib.gaq_optim_sync_log_std(opt.handle, cs) == -4 and b"deterministic" in err()
    assert net.log_std is None
    got_ls = np.empty(4, np.float32)
    assert lib.gaq_optim_get_log_std(opt.handle, _lib.ptr(got_ls)) == 0 and np.array_equal(got_ls, mine)
    net.set_log_std(got_ls)
    # an optimiser without a head: grad_value given is refused, a head added later is GAQ_ERR_STATE
    nohead = R.BY_NAME["mlp48x80x32"]
    net2 = _build(nohead, env)
    opt2 = _optim(nohead, net2)
    g2 = _grads(nohead, 0)
    start2 = net2.get_packed()
    assert lib.gaq_optim_step_dev(opt2.handle, _lib.ptr(g2[0]), _lib.ptr(g2[0]), _lib.ptr(g2[2]), None, cs) == -1 and b"no value head" in err()
    net2.set_value_head(np.zeros(32, np.float32), 0.0)
    assert lib.gaq_optim_step_dev(opt2.handle, _lib.ptr(g2[0]), None, _lib.ptr(g2[2]), None, cs) == -4 and b"gained a value head" in err()
    with pytest.raises(_lib.GaqError, match="value head"):
        opt2.step(g2[0], None, g2[2])
    net2.set_value_head(None)
    assert opt2.step_count == 0 and np.array_equal(start2, net2.get_packed())
    # a closed handle, a closed optimiser
    opt2.close()
    with pytest.raises(ValueError, match="closed"):
        opt2.step(*g2)
    net2.close()
    # nothing was launched: the bits and t are what they were, and a step gives a twin's bits
    after = _read(case, net, opt)
    assert after[3] == (0, 0) and _same(before, after)
    twin = _build(case, env)
    topt = _optim(case, twin)
    opt.step(g, gv, gls)
    topt.step(g, gv, gls)
    assert _same(_read(case, net, opt), _read(case, twin, topt))
    net.close()
    with pytest.raises(ValueError, match="closed"):
        opt.step(g, gv, gls)
    for x in (opt, topt, twin):
        x.close()
