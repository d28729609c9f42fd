"""Gradients on the device (gaq.h gaq_policy_logp_dev, gaq_policy_backward_dev, gaq_policy_grad_ppo_dev, gaq_critic_backward_dev,
gaq_critic_grad_mse_dev) against the fp64 reference of tests/policy_grad_ref.py: the case matrix under the bound 8 x torch fp32's error,
the forward pass's bits against the rollout's, recorded log-probabilities, determinism, partial tiles, the fused calls against the
caller-given-delta ones, a closed Adam loop, and the refusals.  Every figure a test bounds is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_grad_ref as G
from tests.policy_util import _bufs, _dev, environ

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

    def get(D=18):
        if D not in made:
            made[D] = _make_env(D)
        return made[D]
    yield get
    for e in made.values():
        e.close()


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=_dev()) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=_dev())


def _net(env, case, inp, log_std=G.LOG_STD):
    """the case's policy or critic on the device, and the normaliser it keeps alive"""
    from gym_art_amd.policy import MLPCritic, MLPPolicy, ObsNorm
    if case.n_out == 1:
        return MLPCritic.from_arrays(env, inp["layers"], case.act), None
    norm = None
    if case.norm:
        mean, var, eps, clip = G.norm_stats(case.D)
        norm = ObsNorm.from_stats(env, mean, var, 1.0, eps, clip)
    return MLPPolicy.from_arrays(env, inp["layers"], case.act, case.out_tanh, log_std=log_std, engine="mfma", obs_norm=norm), norm


def _dev_inputs(inp):
    return {k: _t(v) for k, v in inp.items() if k != "layers" and k != "x"}


def _np(t):
    return t.detach().cpu().numpy()


def _check_ppo(case, inp, d, pol, rows, what):
    ref = G.ppo(case, inp, rows)
    bg, bl, bloss, bkl = G.bounds(case.name, rows)
    g, gls, st = pol.ppo_grad_dev(d["obs"][:rows], d["actions"][:rows], d["logp_old"][:rows], d["adv"][:rows], clip=G.CLIP)
    lp = pol.logp_dev(d["obs"][:rows], d["actions"][:rows])
    errs = G.grad_errors(pol.unpack(_np(g)), _np(gls), ref)
    st = _np(st)
    e_lp, e_loss, e_kl = G.rel(_np(lp), ref["logp"]), G.rel(st[0], ref["stats"][0]), G.rel(st[2], ref["stats"][2])
    print("%s %s rows=%d: grad %.3g (bound %.3g) logp %.3g (%.3g) loss %.3g (%.3g) kl %.3g (%.3g)"
          % (case.name, what, rows, max(errs), bg, e_lp, bl, e_loss, bloss, e_kl, bkl))
    assert max(errs) <= bg, (case.name, what, rows, errs, bg)
    assert e_lp <= bl and e_loss <= bloss and e_kl <= bkl, (case.name, what, rows, e_lp, bl, e_loss, bloss, e_kl, bkl)
    assert st[1] == ref["stats"][1] and st[3] == rows, (st, ref["stats"])         # the clipped-row count and rows are exact
    return max(errs), g


def _check_mse(case, inp, d, crit, rows, what):
    ref = G.mse(case, inp, rows)
    bg, bv, bloss, _ = G.bounds(case.name, rows)
    g, st = crit.mse_grad_dev(d["obs"][:rows], d["target"][:rows])
    v = crit.values_dev(d["obs"][:rows])
    errs = G.grad_errors(crit.unpack(_np(g)), None, ref)
    st = _np(st)
    e_v, e_loss = G.rel(_np(v), ref["value"]), G.rel(st[0], ref["stats"][0])
    print("%s %s rows=%d: grad %.3g (bound %.3g) V %.3g (%.3g) loss %.3g (%.3g)" % (case.name, what, rows, max(errs), bg, e_v, bv, e_loss, bloss))
    assert max(errs) <= bg, (case.name, what, rows, errs, bg)
    assert e_v <= bv and e_loss <= bloss and st[1] == rows, (case.name, what, rows, e_v, bv, e_loss, bloss, st)
    return max(errs), g


@pytest.mark.parametrize("case", G.POLICY_CASES + G.CRITIC_CASES, ids=[c.name for c in G.POLICY_CASES + G.CRITIC_CASES])
def test_case_matrix(case, envs):
    """every net x style x observation form at 1, 63, 64, 65 and 453 rows, and 453 = 64 * 7 + 5 rows over 3 workgroups (several tiles per
    workgroup, an uneven split, a partial last tile): each parameter tensor, grad_log_std, logp and the sums within 8 x torch fp32's error"""
    _, inp = G.case_inputs(case.name)
    assert G.conditions(case, inp) is None
    net, norm = _net(envs(case.D), case, inp)
    d = _dev_inputs(inp)
    check = _check_ppo if case.n_out == 4 else _check_mse
    worst = 0.0
    for rows in G.ROWS:
        worst = max(worst, check(case, inp, d, net, rows, "default")[0])
    with environ(GAQ_GRAD_GROUPS="3"):
        worst = max(worst, check(case, inp, d, net, G.R, "3 groups")[0])
    print("%s: worst gradient error %.3g" % (case.name, worst))
    net.close()
    if norm is not None:
        norm.close()


@pytest.mark.parametrize("n", [65, 453])
def test_mean_is_the_rollouts_action_bit_for_bit(n):
    """mean from logp_dev on an observation == the action of a one-step deterministic rollout from that observation"""
    import torch
    from gym_art_amd.policy import MLPPolicy
    env = _make_env(18, n)
    for name in ("policy-128x128-tanh", "policy-48x80x32-relu", "policy-16-tanh"):
        case, inp = G.case_inputs(name)
        pol = MLPPolicy.from_arrays(env, inp["layers"], case.act, case.out_tanh, engine="mfma")
        o0 = torch.empty((n, 18), device=_dev())
        env.reset_dev(o0)
        obs0 = o0.clone()
        o, r, dn, a = _bufs(env, 1)
        env.rollout_policy_dev(pol, o, r, dn, a)
        pol.set_log_std(G.LOG_STD)
        mean = torch.full((n, 4), float("nan"), device=_dev())
        pol.logp_dev(obs0, a[0], mean=mean)
        torch.cuda.synchronize()
        assert torch.equal(mean.view(torch.int32), a[0].view(torch.int32)), name
        pol.close()
    env.close()


def test_recorded_log_probabilities():
    """logp_dev(obs_{t-1}, actions_t) against the logp an exploring T = 4 rollout recorded: the means are bit-equal, so only z is recomputed
    from the rounded action; with log_std >= -1 and |a| <= 8, dz <~ 2.5e-6 and dlogp <~ 4 * 6 * 2.5e-6 < 1e-4"""
    import torch
    from gym_art_amd.policy import MLPPolicy
    n, T = 454, 4                                                # (a T-step rollout needs N * obs_dim * 4 bytes to be a multiple of 16)
    env = _make_env(18, n)
    case, inp = G.case_inputs("policy-64x64-tanh")
    assert float(G.LOG_STD.min()) >= -1.0
    pol = MLPPolicy.from_arrays(env, inp["layers"], case.act, case.out_tanh, log_std=G.LOG_STD, engine="mfma")
    o0 = torch.empty((n, 18), device=_dev())
    env.reset_dev(o0)
    obs0 = o0.clone()
    o, r, dn, a = _bufs(env, T)
    lp = torch.empty((T, n), device=_dev())
    env.rollout_policy_dev(pol, o, r, dn, a, logp=lp)
    prev = torch.cat([obs0[None], o[:-1]]).contiguous()
    got = pol.logp_dev(prev, a)
    torch.cuda.synchronize()
    assert float(a.abs().max()) <= 8.0
    err = float((got - lp).abs().max())
    print("recorded logp: max |logp_dev - recorded| = %.3g" % err)
    assert err <= 1e-4, err
    pol.close()
    env.close()


def test_determinism(envs):
    """the same call twice, and once on another stream: equal bits; 3 workgroups against the default: within the bound (not equal)"""
    import torch
    case, inp = G.case_inputs("policy-128x128-tanh")
    pol, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    args = (d["obs"], d["actions"], d["logp_old"], d["adv"])
    first = [x.clone() for x in pol.ppo_grad_dev(*args)]
    again = [x.clone() for x in pol.ppo_grad_dev(*args)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        other = [x.clone() for x in pol.ppo_grad_dev(*args)]
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    with environ(GAQ_GRAD_GROUPS="3"):
        three = pol.ppo_grad_dev(*args)
    torch.cuda.synchronize()
    ref = G.ppo(case, inp, G.R)
    for got in (first, three):
        assert max(G.grad_errors(pol.unpack(_np(got[0])), _np(got[1]), ref)) <= G.bounds(case.name, G.R)[0]
    pol.close()


def test_partial_tiles(envs):
    """65 rows = the references of rows 0-63 and of row 64 added up; NaN in every buffer past `rows` changes no output bit"""
    import torch
    case, inp = G.case_inputs("policy-48x80x32-relu")
    pol, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    sc = 1.0 / 65
    lo = G.ppo(case, {k: (v[:64] if k != "layers" else v) for k, v in inp.items()}, 64, scale=sc)
    hi = G.ppo(case, {k: (v[64:65] if k != "layers" else v) for k, v in inp.items()}, 1, scale=sc)
    want = dict(grads=[(a + c, b + e) for (a, b), (c, e) in zip(lo["grads"], hi["grads"])], glogstd=lo["glogstd"] + hi["glogstd"])
    g, gls, st = pol.ppo_grad_dev(d["obs"][:65], d["actions"][:65], d["logp_old"][:65], d["adv"][:65], clip=G.CLIP)
    errs = G.grad_errors(pol.unpack(_np(g)), _np(gls), want)
    print("partial tile: %.3g (bound %.3g)" % (max(errs), G.bounds(case.name, 65)[0]))
    assert max(errs) <= G.bounds(case.name, 65)[0]
    lp = pol.logp_dev(d["obs"][:65], d["actions"][:65])
    nan = {k: v.clone() for k, v in d.items()}
    for v in nan.values():
        v[65:] = float("nan")
    g2, gls2, st2 = pol.ppo_grad_dev(nan["obs"][:65], nan["actions"][:65], nan["logp_old"][:65], nan["adv"][:65], clip=G.CLIP)
    lp2 = pol.logp_dev(nan["obs"][:65], nan["actions"][:65])
    torch.cuda.synchronize()
    for a, b in ((g, g2), (gls, gls2), (st, st2), (lp, lp2)):
        assert torch.equal(a, b)
    pol.close()


def test_fused_calls_agree_with_the_caller_given_delta(envs):
    """ppo_grad_dev == backward_dev fed the reference's dL/dmean in fp32, mse_grad_dev == the critic's backward_dev, within the bound"""
    case, inp = G.case_inputs("policy-64x64-tanh")
    pol, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    ref = G.ppo(case, inp, G.R)
    g = pol.backward_dev(d["obs"], _t(ref["dmean"].astype(np.float32)), scale=1.0)
    errs = G.grad_errors(pol.unpack(_np(g)), None, ref)
    print("backward_dev against the reference: %.3g" % max(errs))
    assert max(errs) <= G.bounds(case.name, G.R)[0]
    fused = pol.ppo_grad_dev(d["obs"], d["actions"], d["logp_old"], d["adv"], clip=G.CLIP)[0]
    ref_b = dict(grads=[(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in pol.unpack(_np(g))])
    assert max(G.grad_errors(pol.unpack(_np(fused)), None, ref_b)) <= G.bounds(case.name, G.R)[0]
    pol.close()
    case, inp = G.case_inputs("critic-48x80x32-relu")
    crit, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    ref = G.mse(case, inp, G.R)
    g = crit.backward_dev(d["obs"], _t(ref["dv"][:, 0].astype(np.float32)), scale=1.0)
    errs = G.grad_errors(crit.unpack(_np(g)), None, ref)
    print("critic backward_dev against the reference: %.3g" % max(errs))
    assert max(errs) <= G.bounds(case.name, G.R)[0]
    fused = crit.mse_grad_dev(d["obs"], d["target"])[0]
    ref_b = dict(grads=[(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in crit.unpack(_np(g))])
    errs = G.grad_errors(crit.unpack(_np(fused)), None, ref_b)
    print("mse_grad_dev against the critic's backward_dev: %.3g" % max(errs))
    assert max(errs) <= G.bounds(case.name, G.R)[0]
    crit.close()


def test_captured_in_a_graph_after_one_warm_up_call(envs):
    """ppo_grad_dev and mse_grad_dev captured in a graph after one warm-up call replay with the eager call's bits, also after an eager
    call of another size on the same handle in between (the scratch does not move) and on new contents of the same buffers"""
    import torch
    case, inp = G.case_inputs("policy-128x128-tanh")            # (more than 64 KiB of LDS: the launch raises the kernel's limit)
    ccase, cinp = G.case_inputs("critic-64x64-tanh")
    pol, _ = _net(envs(), case, inp)
    crit, _ = _net(envs(), ccase, cinp)
    d, dc = _dev_inputs(inp), _dev_inputs(cinp)
    args = (d["obs"], d["actions"], d["logp_old"], d["adv"])
    eager = [x.clone() for x in pol.ppo_grad_dev(*args[:3], args[3].clone())] + [x.clone() for x in crit.mse_grad_dev(dc["obs"], dc["target"])]
    pol.ppo_grad_dev(*(x[:65] for x in args))                     # the warm-up may be of any size
    out = [torch.empty_like(x) for x in eager]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pol.ppo_grad_dev(*args, grad=out[0], grad_log_std=out[1], stats=out[2])
        crit.mse_grad_dev(dc["obs"], dc["target"], grad=out[3], stats=out[4])
    for x in out:
        x.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    pol.ppo_grad_dev(*(x[:129] for x in args))                    # another size in between
    flipped = [x.clone() for x in pol.ppo_grad_dev(*args[:3], -args[3])]
    args[3].neg_()                                                # new contents, the same buffers
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out[:3], flipped):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], eager[0])
    pol.close(); crit.close()


def _pack_torch(layers):
    import torch
    out = []
    for W, b in layers[:-1]:
        o, i = W.shape
        out += [W.reshape(o // 16, 16, i).permute(0, 2, 1).reshape(-1), b]
    out += [layers[-1][0].T.reshape(-1), layers[-1][1]]
    return torch.cat(out).contiguous()


def test_closed_loop_of_ten_adam_steps(envs):
    """ten Adam steps on the 453 rows with device gradients -> unpack_weights -> param.grad -> set_weights_dev, beside the same ten steps
    with torch fp32 autograd: the surrogate decreases in both, and each parameter tensor ends within 100 x the single-step bound
    (max|a - b| / max|b|; Adam's division by sqrt(v) can turn a last-bit difference in a small gradient into a full step's)"""
    import torch
    case, inp = G.case_inputs("policy-64x64-tanh")
    pol, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    lr, steps = 3e-4, 10
    # the device path
    params = [(_t(W).clone().requires_grad_(True), _t(b).clone().requires_grad_(True)) for W, b in inp["layers"]]
    log_std = _t(G.LOG_STD).clone().requires_grad_(True)
    leaves = [p for Wb in params for p in Wb] + [log_std]
    opt = torch.optim.Adam(leaves, lr=lr)
    loss_dev = []
    for _ in range(steps):
        with torch.no_grad():
            pol.set_weights_dev(_pack_torch(params))
        pol.set_log_std(_np(log_std))
        g, gls, st = pol.ppo_grad_dev(d["obs"], d["actions"], d["logp_old"], d["adv"], clip=G.CLIP)
        for (W, b), (gW, gb) in zip(params, pol.unpack(g)):
            W.grad, b.grad = gW.contiguous(), gb.contiguous()
        log_std.grad = gls.clone()
        loss_dev.append(float(st[0]) / G.R)
        opt.step()
    # torch autograd, fp32, on the CPU
    layers, ls, fwd = G.torch_net(case, inp, torch.float32)
    opt = torch.optim.Adam([p for Wb in layers for p in Wb] + [ls], lr=lr)
    loss_ref = []
    for _ in range(steps):
        opt.zero_grad()
        loss = G.torch_loss(case, inp, G.R, torch.float32, layers, ls, fwd)[0]
        loss.backward()
        loss_ref.append(float(loss.detach()))
        opt.step()
    print("closed loop: surrogate %.6f -> %.6f on the device, %.6f -> %.6f in torch" % (loss_dev[0], loss_dev[-1], loss_ref[0], loss_ref[-1]))
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    bound = 100.0 * G.bounds(case.name, G.R)[0]
    got = [p for Wb in params for p in Wb] + [log_std]
    want = [p for Wb in layers for p in Wb] + [ls]
    errs = [G.rel(_np(a), _np(b)) for a, b in zip(got, want)]
    print("closed loop: parameters after %d steps differ by %.3g at most (bound %.3g)" % (steps, max(errs), bound))
    assert max(errs) <= bound, (errs, bound)
    pol.close()


def test_rows_zero_gives_zeros(envs):
    import torch
    case, inp = G.case_inputs("policy-16-tanh")
    pol, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    g, gls, st = (torch.full_like(x, 7.0) for x in pol.ppo_grad_dev(d["obs"], d["actions"], d["logp_old"], d["adv"]))
    pol.ppo_grad_dev(d["obs"][:0], d["actions"][:0], d["logp_old"][:0], d["adv"][:0], grad=g, grad_log_std=gls, stats=st)
    g2 = pol.backward_dev(d["obs"][:0], d["actions"][:0], grad=torch.full_like(g, 7.0))
    assert pol.logp_dev(d["obs"][:0], d["actions"][:0]).shape == (0,)
    torch.cuda.synchronize()
    assert not g.any() and not gls.any() and not st.any() and not g2.any()
    pol.close()
    case, inp = G.case_inputs("critic-16-relu")
    crit, _ = _net(envs(), case, inp)
    d = _dev_inputs(inp)
    g, st = (torch.full_like(x, 7.0) for x in crit.mse_grad_dev(d["obs"], d["target"]))
    crit.mse_grad_dev(d["obs"][:0], d["target"][:0], grad=g, stats=st)
    g2 = crit.backward_dev(d["obs"][:0], d["target"][:0], grad=torch.full_like(g, 7.0))
    torch.cuda.synchronize()
    assert not g.any() and not st.any() and not g2.any()
    crit.close()


def test_refusals(envs):
    """each returns the stated code with the named text, launches nothing, and a valid call afterwards still works"""
    import torch
    from gym_art_amd import _lib
    from gym_art_amd.policy import GRUPolicy, MLPCritic, MLPPolicy
    from tests.gru_util import _gru, _head
    from tests.mlp_ref import _scaled_layers
    env = envs()
    lib = _lib.load()
    case, inp = G.case_inputs("policy-16-tanh")
    d = _dev_inputs(inp)
    o, a, lo, adv = d["obs"][:65], d["actions"][:65], d["logp_old"][:65], d["adv"][:65]

    def refused(pol, match, exc=ValueError):
        with pytest.raises(exc, match=match):
            pol.ppo_grad_dev(o, a, lo, adv)
        with pytest.raises(exc, match=match):
            pol.logp_dev(o, a)

    small = _scaled_layers([16], 18, 0)
    for engine, text in (("valu", "VALU engine"), ("bf16", "bf16 engine")):
        pol = MLPPolicy.from_arrays(env, small, "tanh", True, log_std=G.LOG_STD, engine=engine)
        refused(pol, text)
        with pytest.raises(ValueError, match=text):
            pol.backward_dev(o, a)
        pol.close()
    gru = GRUPolicy(env, _gru(16, 18, 3), _head(16), "tanh", True, log_std=G.LOG_STD)
    with pytest.raises(ValueError, match="GRU"):
        _lib.check(lib.gaq_policy_logp_dev(gru.handle, 65, _lib.ptr(o), _lib.ptr(a), _lib.ptr(lo.clone()), None, None))
    gru.close()
    wide = MLPPolicy.from_arrays(env, _scaled_layers([256], 18, 0), "tanh", True, log_std=G.LOG_STD, engine="mfma")
    refused(wide, "width")
    wide.close()
    wl = _scaled_layers([256], 18, 0)
    crit = MLPCritic.from_arrays(env, wl[:-1] + [(wl[-1][0][:1], wl[-1][1][:1])], "tanh")
    with pytest.raises(ValueError, match="width"):
        crit.mse_grad_dev(o, lo)
    crit.close()

    pol, _ = _net(env, case, inp, log_std=None)
    refused(pol, "log_std", _lib.GaqError)                         # GAQ_ERR_STATE
    assert lib.gaq_policy_logp_dev(pol.handle, 65, _lib.ptr(o), _lib.ptr(a), _lib.ptr(lo.clone()), None, None) == -4
    pol.backward_dev(o, a)                                        # needs no log_std
    pol.set_log_std(G.LOG_STD)
    for clip in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="clip_eps"):
            pol.ppo_grad_dev(o, a, lo, adv, clip=clip)
    with pytest.raises(ValueError, match="NaN"):
        pol.ppo_grad_dev(o, a, lo, adv, scale=float("nan"))
    g, gls, st = pol.ppo_grad_dev(o, a, lo, adv)
    st_ptr, cs = _lib.ptr(st), C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)

    def raw(rows=65, obs=o, logp_old=lo, grad=g, grad_ls=gls):
        return lib.gaq_policy_grad_ppo_dev(pol.handle, rows, _lib.ptr(obs), _lib.ptr(a), _lib.ptr(logp_old), _lib.ptr(adv), 0.2, 1.0,
                                           _lib.ptr(grad), _lib.ptr(grad_ls), st_ptr, cs)
    assert raw(rows=-1) == -1 and b"rows" in lib.gaq_last_error()
    assert raw(obs=None) == -1 and b"null" in lib.gaq_last_error()
    assert raw(grad=o.view(-1)[:g.numel()]) == -1 and b"overlap" in lib.gaq_last_error()          # an output over an input
    assert raw(grad_ls=g[4:8]) == -1 and b"overlap" in lib.gaq_last_error()                        # two outputs
    assert raw(logp_old=lo.data_ptr() + 2) == -1 and b"aligned" in lib.gaq_last_error()
    from gym_art_amd.policy import ENGINES, _DescEx              # weights never set: a handle straight from the C ABI
    dsc = _DescEx()
    dsc.struct_size, dsc.in_dim, dsc.n_hidden, dsc.engine = C.sizeof(_DescEx), 18, 1, ENGINES["mfma"]
    dsc.width[0] = 16
    h = C.c_void_p()
    _lib.check(lib.gaq_policy_create_ex(env._handle, C.byref(dsc), C.byref(h)))
    assert lib.gaq_policy_backward_dev(h, 65, _lib.ptr(o), _lib.ptr(a), 1.0, _lib.ptr(g.clone()), cs) == -1
    assert b"weights not set" in lib.gaq_last_error()
    lib.gaq_policy_destroy(h)
    # the handle is as usable as before: the same bits as the call before the refusals
    g2, gls2, st2 = pol.ppo_grad_dev(o, a, lo, adv)
    torch.cuda.synchronize()
    assert torch.equal(g, g2) and torch.equal(gls, gls2) and torch.equal(st, st2)
    pol.close()
