"""AdamEncDev (gaq.h gaq_optim_create_policy_enc, gaq_optim_step_enc_dev): the optimiser of a recurrent policy with an encoder, whose
fourth group -- the encoder's block, after log_std -- is stepped in place where the rollout's encoder kernel reads it.

1. one step against the fp64 reference of tests/optim_ref.py on the four groups with the joint norm and clip (the reference has three
   group slots and treats slots 0 and 1 alike, so the encoder's block rides behind the weights in slot 0: the same arithmetic per
   element, the same joint norm).  Bound, by that module's rule: 8 x the error of torch fp32 (AdamW + clip_grad_norm_, foreach=False, on
   the CPU, computed here on the same inputs) and never below 2^-24, one rounding of the value; every figure is printed first;
2. a non-finite encoder gradient skips the step: weights, encoder block, moments and step count keep their bits;
3. three eager iterations of ppo_enc_seq_grad_idx_dev + step on a device-mode policy equal three replays of one captured graph of the
   two -- weights, encoder block, value head, the exploration table, both moments, the step count -- which also shows that a graph
   captured after the largest gradient call keeps valid pointers into the scratch behind the tape;
4. after steps a rollout uses the new encoder weights: bit for bit a fresh handle given get_encoder_weights() and the other weights;
5. refusals by text."""
import ctypes as C

import numpy as np
import pytest

from gym_art_amd import _lib
from tests import optim_ref as O
from tests import policy_grad_enc_ref as R
from tests.policy_util import _bufs, _dev
from tests.test_gpu_policy_grad_enc import _call_idx, _dev_inputs, _policy, envs  # noqa: F401  (envs: the module's fixture)

pytestmark = pytest.mark.gpu
HP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=0.5)
CASES = ["enc80-gru64x64-tanh-vclip", "enc32x64-lstm16-relu-norm"]


def _enc_packed(pol):
    out = np.empty(pol._enc_count, np.float32)
    _lib.check(_lib.load().gaq_policy_get_encoder_weights(pol.handle, _lib.ptr(out)))
    return out


def _theta(pol):
    """the four groups as they stand on the device: weights, value head, log_std, encoder"""
    w, b = pol.get_value_head()
    return [pol.get_packed(), np.concatenate([np.asarray(w, np.float32).reshape(-1), [np.float32(b)]]).astype(np.float32),
            np.asarray(pol.get_log_std(), np.float32), _enc_packed(pol)]


def _synthetic(sizes, seed):
    """optim_ref.gradients' recipe: magnitudes log-uniform over [1e-6, 10], random signs, about 5 % exact zeros"""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        g = 10.0 ** rng.uniform(-6.0, 1.0, n) * rng.choice([-1.0, 1.0], n)
        g[rng.uniform(size=n) < 0.05] = 0.0
        out.append(g.astype(np.float32))
    return out


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=_dev())


def _split(opt, flat):
    return {name: flat[off:off + n] for name, off, n in opt.groups}


@pytest.mark.parametrize("name", CASES)
def test_one_step_is_the_reference_on_four_groups(name, envs):
    import torch
    from gym_art_amd.policy import AdamEncDev
    case, inp = R.case_inputs(name)
    pol, norm = _policy(envs(case.D), case, inp)
    opt = AdamEncDev(pol, **HP)
    assert [g[0] for g in opt.groups] == ["weights", "value_head", "log_std", "encoder"]
    assert opt.groups[3][1] == pol._count + pol.widths[-1] + 1 + 4 and opt.groups[3][2] == pol._enc_count
    th0 = _theta(pol)
    g = _synthetic([t.size for t in th0], 4242)
    stats = torch.zeros(4, dtype=torch.float64, device=_dev())
    opt.step(_t(g[0]), _t(g[3]), _t(g[1]), _t(g[2]), stats=stats)
    torch.cuda.synchronize()
    th1, sd = _theta(pol), opt.state_dict()
    m, v = _split(opt, sd["m"]), _split(opt, sd["v"])
    # the reference: slot 0 = weights then encoder, slot 1 the head, slot 2 log_std
    nw = th0[0].size
    st = O.State([np.concatenate([th0[0], th0[3]]), th0[1], th0[2]])
    rstats = O.step(st, [np.concatenate([g[0], g[3]]), g[1], g[2]], **HP)
    ref = lambda x: {"weights": x[0][:nw], "encoder": x[0][nw:], "value_head": x[1], "log_std": x[2]}
    # the yardstick: torch fp32 on the CPU on the same inputs
    params = [torch.tensor(t, dtype=torch.float32, requires_grad=True) for t in th0]
    topt = torch.optim.AdamW([{"params": [params[0], params[1], params[3]], "weight_decay": HP["weight_decay"]},
                              {"params": [params[2]], "weight_decay": 0.0}], lr=HP["lr"], betas=HP["betas"], eps=HP["eps"], foreach=False)
    for p, x in zip(params, g):
        p.grad = torch.tensor(x)
    torch.nn.utils.clip_grad_norm_(params, HP["max_grad_norm"], foreach=False)
    topt.step()
    names = ("weights", "value_head", "log_std", "encoder")
    yard = {"theta": dict(zip(names, [p.detach().numpy() for p in params])),
            "m": dict(zip(names, [topt.state[p]["exp_avg"].numpy() for p in params])),
            "v": dict(zip(names, [topt.state[p]["exp_avg_sq"].numpy() for p in params]))}
    got = {"theta": dict(zip(names, th1)), "m": m, "v": v}
    want = {"theta": ref(st.theta), "m": ref(st.m), "v": ref(st.v)}
    for what in ("theta", "m", "v"):
        for n in names:
            e, y = O.rel(got[what][n], want[what][n]), O.rel(yard[what][n], want[what][n])
            bound = max(O.FACTOR * y, 2.0 ** -24)
            print("%s %s %s: device %.3g torch fp32 %.3g bound %.3g" % (name, what, n, e, y, bound))
            assert e <= bound, (name, what, n, e, bound)
    s = stats.cpu().numpy()
    print("%s: norm %.9g (ref %.9g) coef %.9g (ref %.9g)" % (name, s[0], rstats[0], s[1], rstats[1]))
    assert O.rel(s[0], rstats[0]) <= 1e-12 and O.rel(s[1], rstats[1]) <= 1e-12 and s[2] == 1.0 and s[3] == 0.0
    assert s[1] < 1.0                                              # the clip binds: the norm is joint over the four groups
    assert not np.array_equal(th1[3], th0[3]) and opt.step_count == 1 and pol.encoder_packed is None
    # a state_dict round trip covers the fourth group
    opt.load_state_dict(dict(sd, step=7))
    sd2 = opt.state_dict()
    assert sd2["step"] == 7 and np.array_equal(sd2["m"], sd["m"]) and np.array_equal(sd2["v"], sd["v"]) and sd["m"].size == opt.groups[3][1] + opt.groups[3][2]
    opt.close(); pol.close()
    if norm is not None:
        norm.close()


def test_a_non_finite_encoder_gradient_skips_the_step(envs):
    import torch
    from gym_art_amd.policy import AdamEncDev
    case, inp = R.case_inputs(CASES[0])
    pol, _ = _policy(envs(case.D), case, inp)
    opt = AdamEncDev(pol, **HP)
    th0 = _theta(pol)
    g = _synthetic([t.size for t in th0], 5)
    opt.step(_t(g[0]), _t(g[3]), _t(g[1]), _t(g[2]))
    th1, sd1 = _theta(pol), opt.state_dict()
    bad = g[3].copy()
    bad[3] = np.inf
    stats = torch.zeros(4, dtype=torch.float64, device=_dev())
    opt.step(_t(g[0]), _t(bad), _t(g[1]), _t(g[2]), stats=stats)
    torch.cuda.synchronize()
    th2, sd2 = _theta(pol), opt.state_dict()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(th1, th2))
    assert np.array_equal(sd1["m"].view(np.uint32), sd2["m"].view(np.uint32)) and np.array_equal(sd1["v"].view(np.uint32), sd2["v"].view(np.uint32))
    assert sd2["step"] == 1 and sd2["skipped"] == 1 and opt.skipped == 1 and stats.cpu().numpy()[3] == 1.0
    opt.close(); pol.close()


def _loop_case(env, case, inp):
    """a device-mode policy, its optimiser, the source tensors, three index slices and the output tensors of one minibatch"""
    import torch
    from gym_art_amd.policy import AdamEncDev, perm_dev
    pol, norm = _policy(env, case, inp)
    pol.log_std_to_device()
    d = _dev_inputs(case, inp, R.TMAX, R.SMAX)
    perm = perm_dev(R.SMAX, 99, device=_dev())
    slices = [perm[k * 43:(k + 1) * 43].clone() for k in range(3)]
    idx = slices[0].clone()
    outs = [torch.empty_like(x) for x in _call_idx(pol, case, idx, d)]   # the warm-up call: the scratch is allocated, nothing is stepped
    ostats = torch.zeros(4, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    return pol, AdamEncDev(pol, lr=1e-2, max_grad_norm=0.5, learn_log_std=True), d, slices, idx, outs, ostats, norm


def _minibatch(case, c):
    pol, opt, d, _, idx, outs, ostats, _ = c
    _call_idx(pol, case, idx, d, grad=outs[0], grad_encoder=outs[1], grad_value=outs[2], grad_log_std=outs[3], stats=outs[4])
    opt.step(outs[0], outs[1], outs[2], outs[3], stats=ostats)


def _read(c):
    import torch
    torch.cuda.synchronize()
    sd = c[1].state_dict()
    return _theta(c[0]) + [sd["m"], sd["v"], c[5][4].cpu().numpy(), c[6].cpu().numpy()], sd["step"]


@pytest.mark.parametrize("name", CASES)
def test_three_eager_iterations_are_three_replays_of_one_graph(name, envs):
    import torch
    case, inp = R.case_inputs(name)
    env = envs(case.D)
    eager, cap = _loop_case(env, case, inp), _loop_case(env, case, inp)
    start = _theta(cap[0])
    want = []
    for k in range(3):
        eager[4].copy_(eager[3][k])
        _minibatch(case, eager)
        want.append(_read(eager))
    side = torch.cuda.Stream(device=_dev())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _minibatch(case, cap)
    assert cap[1].step_count == 0 and all(np.array_equal(a, b) for a, b in zip(_theta(cap[0]), start))     # capturing ran nothing
    for k in range(3):
        cap[4].copy_(cap[3][k])
        torch.cuda.synchronize()
        graph.replay()
        got = _read(cap)
        assert got[1] == want[k][1] == k + 1
        for j, (x, y) in enumerate(zip(got[0], want[k][0])):
            assert np.all(np.isfinite(x)) and np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(y).view(np.uint8)), (name, k, j)
    end = _theta(cap[0])
    print("%s: log_std %s -> %s; encoder block moved in %d of %d words" % (name, start[2], end[2], int((end[3] != start[3]).sum()), end[3].size))
    assert np.all(end[2] != start[2]) and np.mean(end[3] != start[3]) > 0.9 and np.mean(end[0] != start[0]) > 0.9
    for c in (eager, cap):
        c[1].close(); c[0].close()
        if c[7] is not None:
            c[7].close()


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_a_rollout_uses_the_stepped_encoder(cell):
    """two steps, then a rollout: observations, rewards, dones, actions, values and the states are bit for bit those of a fresh handle
    built from get_encoder_weights() and the stepped cell, head and value head -- and not those of the handle before the steps"""
    import torch
    from gym_art_amd.policy import AdamEncDev, GRUPolicy, LSTMPolicy
    from tests.enc_util import _cell, _encoder
    from tests.gru_util import _head
    from tests.test_gpu_policy_encoder import _env
    n, D, H, T = 130, 18, 16, 4
    cls = GRUPolicy if cell == "gru" else LSTMPolicy
    value = ((np.arange(H) / H - 0.5).astype(np.float32), np.float32(0.1))
    runs = []
    stepped = None
    for how in ("before", "stepped", "fresh"):
        env = _env(D, n)
        if how == "fresh":
            pol = cls.with_encoder(env, stepped[0], *stepped[1], "tanh", True, log_std=None, value=stepped[2])
        else:
            pol = cls.with_encoder(env, _encoder(D, (32, 48), 3), _cell(cell, H, 48, 4), _head(H, (), 5), "tanh", True, log_std=None, value=value)
        if how == "stepped":
            opt = AdamEncDev(pol, lr=5e-2)
            assert [g[0] for g in opt.groups] == ["weights", "value_head", "encoder"]
            for k in range(2):
                g = _synthetic([pol._count, H + 1, pol._enc_count], 70 + k)
                opt.step(_t(g[0]), _t(g[2]), _t(g[1]))
            opt.close()
            stepped = (pol.get_encoder_weights(), pol.get_weights(), pol.get_value_head())
        o0 = torch.empty((n, D), device=_dev())
        env.reset_dev(o0)
        o, r, d, a = _bufs(env, T)
        v = torch.empty((T + 1, n), device=_dev())
        env.rollout_policy_dev(pol, o, r, d, a, values=v)
        torch.cuda.synchronize()
        runs.append([o.clone(), r.clone(), d.clone(), a.clone(), v.clone(), pol.hidden.clone()] + ([pol.cell.clone()] if cell == "lstm" else []))
        pol.close(); env.close()
    for x, y in zip(runs[1], runs[2]):
        assert bool(torch.isfinite(x.float()).all()) and torch.equal(x, y)
    assert not torch.equal(runs[0][3], runs[1][3])


def test_refusals(envs):
    import torch
    from gym_art_amd.policy import AdamDev, AdamEncDev, GRUPolicy, optim_desc
    from tests.enc_util import _cell
    from tests.gru_util import _head
    lib = _lib.load()
    err = lambda: lib.gaq_last_error().decode()
    case, inp = R.case_inputs("enc16-gru16-tanh")
    env = envs(18)
    pol, _ = _policy(env, case, inp)
    plain = GRUPolicy(env, _cell("gru", 16, 18), _head(16), log_std=R.LOG_STD)
    with pytest.raises(ValueError, match="encoder"):
        AdamEncDev(plain)
    with pytest.raises(ValueError, match="encoder"):
        AdamDev(pol)                                                # the parent class keeps refusing the handle
    d, h = optim_desc(), C.c_void_p()
    assert lib.gaq_optim_create_policy_enc(plain.handle, C.byref(d), C.byref(h)) == -1 and "encoder" in err() and not h.value
    assert lib.gaq_optim_create_policy_enc(None, C.byref(d), C.byref(h)) == -1 and "null" in err()
    opt, popt = AdamEncDev(pol), AdamDev(plain)
    before = pol.get_packed()
    g = [torch.zeros(n, device=_dev()) for n in (pol._count, pol._enc_count, pol.widths[-1] + 1, 4)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gaq_optim_step_dev(opt.handle, _lib.ptr(g[0]), _lib.ptr(g[2]), _lib.ptr(g[3]), None, st) == -1 and "gaq_optim_step_enc_dev" in err()
    assert lib.gaq_optim_step_enc_dev(popt.handle, _lib.ptr(g[0]), _lib.ptr(g[1]), None, _lib.ptr(g[3]), None, st) == -1
    assert "gaq_optim_create_policy_enc" in err()
    assert lib.gaq_optim_step_enc_dev(opt.handle, _lib.ptr(g[0]), None, _lib.ptr(g[2]), _lib.ptr(g[3]), None, st) == -1 and "null" in err()
    with pytest.raises(ValueError, match="grad_encoder"):
        opt.step(g[0], g[1][:-1].contiguous(), g[2], g[3])
    torch.cuda.synchronize()
    assert np.array_equal(before, pol.get_packed()) and opt.step_count == 0
    for x in (opt, popt, plain, pol):
        x.close()
