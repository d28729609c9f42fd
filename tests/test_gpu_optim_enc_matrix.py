"""AdamEncDev (gaq.h gaq_optim_create_policy_enc, gaq_optim_step_enc_dev) over the case matrix of tests/optim_enc_ref.py: layouts with
empty groups, group and chunk boundaries in every position, both launch forms (GAQ_OPTIM_LAUNCHES, read at creation -- the one-launch
form is optim_step_one_kernel<4>), ten steps with changing gradients against the fp64 reference under max(8 x torch fp32's committed
error, k x 2^-24); the exploration table a device-mode policy's step publishes; and a closed loop of ten ppo_enc_seq_grad_dev ->
AdamEncDev.step beside torch fp32 autograd + Adam on the twin module, which takes the device's own grad_encoder through the optimiser.
Every figure a test bounds is printed before it is asserted."""
import numpy as np
import pytest

from gym_art_amd import _lib
from tests import optim_enc_ref as R
from tests import optim_ref as O
from tests import policy_grad_enc_edges as E
from tests import policy_grad_enc_ref as PR
from tests.policy_util import _dev, environ
from tests.test_gpu_policy_grad_enc import _call, _dev_inputs, _policy, envs  # noqa: F401  (envs: the module's fixture)

pytestmark = pytest.mark.gpu
LAUNCHES = ["2", "1"]


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=_dev())


def _build(case, env, device_mode=False):
    """the case's policy with theta0 as its packed weights, value head, log_std and encoder block (the step is elementwise: any packed
    contents do)"""
    from gym_art_amd.policy import GRUPolicy, LSTMPolicy
    from tests.enc_util import _cell, _encoder
    from tests.gru_util import _head
    th = R.theta0(case)
    log_std = {"learn": th[2], "frozen": R.FROZEN_LOG_STD, None: None}[case.log_std]
    value = (th[1][:-1], th[1][-1]) if case.head else None
    H = case.widths[0]
    cls = GRUPolicy if case.cell == "gru" else LSTMPolicy
    pol = cls.with_encoder(env, _encoder(case.D, case.enc), _cell(case.cell, H, case.enc[-1]), _head(H, case.widths[1:]), "tanh", True,
                           log_std=log_std, value=value)
    assert (pol._count, pol._enc_count) == (case.sizes[0], case.sizes[3])
    _lib.check(pol._lib.gaq_policy_set_weights(pol.handle, _lib.ptr(th[0])))
    _lib.check(pol._lib.gaq_policy_set_encoder_weights(pol.handle, _lib.ptr(th[3])))
    if device_mode:
        pol.log_std_to_device()
    return pol


def _optim(case, pol, launches):
    from gym_art_amd.policy import AdamEncDev
    with environ(GAQ_OPTIM_LAUNCHES=launches):
        return AdamEncDev(pol, learn_log_std=case.log_std == "learn", **case.hp)


def _grads(case, k):
    """step k's gradients on the device as step() takes them: (grad, grad_encoder, grad_value or None, grad_log_std or None)"""
    g = R.gradients(case, k)
    return _t(g[0]), _t(g[3]), _t(g[1]) if case.head else None, _t(g[2]) if case.log_std == "learn" else None


def _read(case, pol, opt):
    """(theta, m, v) per group -- weights, value head, log_std, encoder -- read back from the handle and the optimiser, then
    (step, skipped)"""
    sd = opt.state_dict()
    zero = np.zeros(0, np.float32)
    theta = [pol.get_packed(), zero, zero, np.empty(pol._enc_count, np.float32)]
    _lib.check(pol._lib.gaq_policy_get_encoder_weights(pol.handle, _lib.ptr(theta[3])))
    if case.head:
        w, b = pol.get_value_head()
        theta[1] = np.concatenate([w, [b]]).astype(np.float32)
    if case.log_std == "learn":
        opt.sync_log_std()
        theta[2] = pol.get_log_std()
    n = np.cumsum([0] + [x.size for x in theta])
    assert tuple(n[1:]) == case.ends and n[-1] == sd["m"].size == sd["v"].size == opt._count
    # the moments: the groups concatenated as .groups says, the encoder's last
    assert [(g[0], g[1], g[2]) for g in opt.groups] == [(name, int(n[k]), int(n[k + 1] - n[k])) for k, name in enumerate(R.GROUPS)
                                                        if n[k + 1] > n[k]]
    m = [sd["m"][n[k]:n[k + 1]] for k in range(4)]
    v = [sd["v"][n[k]:n[k + 1]] for k in range(4)]
    return theta, m, v, (sd["step"], sd["skipped"])


def _check_against_reference(case, got, ref, steps, what):
    worst = 0.0
    for i, name in enumerate(("theta", "m", "v")):
        for gidx in range(4):
            e, b = O.rel(got[i][gidx], ref[i][gidx]), R.bound(case.name, steps, name, gidx)
            print("%s %s after %d steps: %s of %s differs by %.3g (bound %.3g)" % (case.name, what, steps, name, R.GROUPS[gidx], e, b))
            assert got[i][gidx].size == ref[i][gidx].size == case.sizes[gidx] and e <= b, (case.name, what, steps, name, gidx, e, b)
            worst = max(worst, e / b)
    return worst


def _table_is_published(pol, what):
    """a device-mode policy's table log_std[4] | std[4] | inv_std[4]: std and inv_std are float32(exp(+-float64(log_std))) bit for bit"""
    tab = pol._explore_table.cpu().numpy()
    x = tab[:4].astype(np.float64)
    want = np.concatenate([tab[:4], np.exp(x).astype(np.float32), np.exp(-x).astype(np.float32)])
    assert np.array_equal(tab.view(np.uint32), want.view(np.uint32)), (what, tab, want)


def _run(case, env, launches, device_mode=False):
    import torch
    pol = _build(case, env, device_mode)
    opt = _optim(case, pol, launches)
    what = "%s launch(es)%s" % (launches, ", device-mode log_std" if device_mode else "")
    ref = R.reference(case.name)
    stats = torch.zeros(4, dtype=torch.float64, device=_dev())
    coefs, worst = [], 0.0
    for k in range(R.STEPS):
        g = _grads(case, k)
        opt.step(g[0], g[1], g[2], g[3], stats=stats, sync_log_std=(k % 2 == 0))
        st, want = stats.cpu().numpy(), ref[k][3]
        e_norm, e_coef = O.rel(st[0], want[0]), O.rel(st[1], want[1])
        print("%s %s step %d: norm %.9g (off by %.3g) coef %.9g (off by %.3g) t %d skipped %d" % (case.name, what, k + 1, st[0], e_norm, st[1],
                                                                                                e_coef, st[2], st[3]))
        assert e_norm <= 1e-6 and e_coef <= 1e-6 and st[2] == k + 1 and st[3] == 0.0
        coefs.append(st[1])
        if device_mode:
            _table_is_published(pol, (case.name, what, k))
        if k + 1 in R.AT:
            got = _read(case, pol, opt)
            worst = max(worst, _check_against_reference(case, got, ref[k], k + 1, what))
            assert got[3] == (k + 1, 0)
    if case.clip == "above":
        assert max(coefs) < 0.05
    if case.clip == "below" or case.hp["max_grad_norm"] is None:
        assert min(coefs) == 1.0
    assert pol.packed is None and pol.encoder_packed is None and opt.step_count == R.STEPS and opt.skipped == 0
    print("%s %s: worst error / bound %.3f" % (case.name, what, worst))
    opt.close()
    pol.close()


@pytest.mark.parametrize("launches", LAUNCHES, ids=["two-launch", "one-launch"])
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case_matrix(case, launches, envs):
    """theta, m and v of every group after 1, 2 and 10 steps with changing gradients within max(8 x torch fp32's error, k x 2^-24);
    every step's norm and coef to 1e-6 relative, the step and skipped counts exact, the state's sizes and group offsets the case's"""
    _run(case, envs(case.D), launches)


@pytest.mark.parametrize("launches", LAUNCHES, ids=["two-launch", "one-launch"])
def test_a_device_mode_policy_gets_its_table_published(launches, envs):
    """the four-group case across the chunk boundary on a policy after log_std_to_device(): the step writes log_std in the policy's
    table, and after every step std and inv_std beside it are float32(exp(float64(x))) and float32(exp(-float64(x))) bit for bit"""
    case = R.BY_NAME["enc16x16-gru16-head-logstd"]
    _run(case, envs(case.D), launches, device_mode=True)


LOOP = [("enc80-gru64x64-tanh-vclip", PR), ("enc64x32-lstm48x32-tanh-vclip-d19", E)]    # a GRU; an LSTM behind two encoder layers


@pytest.mark.parametrize("name,mod", LOOP, ids=[n for n, _ in LOOP])
def test_closed_loop_of_ten_adam_steps(name, mod, envs):
    """Ten steps at (T, S) = (6, 130) with lr 3e-4, max_grad_norm 0.5 and log_std learned: ppo_enc_seq_grad_dev -> AdamEncDev.step, beside
    torch fp32 autograd + clip_grad_norm_ + Adam on the twin module (policy_grad_enc_ref.torch_errors' construction: the encoder's
    Linears, the parent's cell loop, head and value Linear).  Both losses fall; every parameter tensor of the cell, the head, the value
    head and log_std ends within 100 x the case's single-step gradient bound, every tensor of the encoder within 100 x its encoder
    bound (the parents' rule, test_gpu_optim.py's closed loops)."""
    import torch
    import torch.nn as nn
    from gym_art_amd.policy import AdamEncDev
    case, inp = mod.case_inputs(name)
    pol, norm = _policy(envs(case.D), case, inp)
    assert norm is None and case.value
    T, S = PR.TMAX, PR.SMAX
    assert (T, S) == (6, 130)
    d = _dev_inputs(case, inp, T, S)
    lr, steps, mgn = 3e-4, 10, 0.5
    ent_const = float(PR.ENT_COEF * 2.0 * (1.0 + np.log(2.0 * np.pi)))
    opt = AdamEncDev(pol, lr=lr, max_grad_norm=mgn)
    assert [g[0] for g in opt.groups] == ["weights", "value_head", "log_std", "encoder"]
    stats = torch.zeros(4, dtype=torch.float64, device=_dev())
    loss_dev, coefs = [], []
    for _ in range(steps):
        ls = np.asarray(pol.log_std, np.float64)
        g, ge, gv, gls, st = _call(pol, case, d)
        opt.step(g, ge, gv, gls, stats=stats)
        loss_dev.append((float(st[0]) + PR.VF_COEF * float(st[3])) / (T * S) - PR.ENT_COEF * float(ls.sum()) - ent_const)
        coefs.append(float(stats[1]))
    # the twin
    Rm, inner = PR.REF[case.cell], case.inner
    model = Rm.torch_model(inner, inp, torch.float32)
    cell, lins, critic, ls = model
    enc = []
    for W, b in inp["enc"]:
        lin = nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data, lin.bias.data = torch.tensor(W), torch.tensor(b)
        enc.append(lin)
    tens = Rm.torch_tensors(dict(inp, x=np.zeros((T, S, 1), np.float32)), T, S, torch.float32)
    obs = torch.tensor(inp["obs"][:T, :S])
    leaves = [p for l in enc for p in l.parameters()] + list(cell.parameters()) + [p for l in lins for p in l.parameters()] + \
        list(critic.parameters()) + [ls]
    topt = torch.optim.Adam(leaves, lr=lr)
    loss_ref = []
    for _ in range(steps):
        topt.zero_grad()
        y = obs
        for lin in enc:
            y = lin(y)
            y = torch.tanh(y) if case.act == "tanh" else torch.relu(y)
        loss = Rm.torch_loss(inner, dict(tens, x=y), T, S, model)[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, mgn)
        loss_ref.append(float(loss.detach()))
        topt.step()
    print("closed loop %s: loss %s on the device, %s in torch; coef %s" % (name, ["%.6f" % x for x in loss_dev], ["%.6f" % x for x in loss_ref],
                                                                         ["%.4f" % c for c in coefs]))
    bg, be = mod.bounds(name, T, S)[:2]
    n = lambda p: p.detach().numpy()
    cw, head = pol.get_weights()
    w, b = pol.get_value_head()
    got = [cw[0], cw[2], cw[1], cw[3]] + [x for Wb in head for x in Wb] + [np.concatenate([w, [b]]), np.asarray(pol.log_std)]
    want = [n(p) for p in (cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh)] + [n(p) for l in lins for p in (l.weight, l.bias)] + \
        [np.concatenate([n(critic.weight).reshape(-1), n(critic.bias).reshape(-1)]), n(ls)]
    errs = [PR.G.rel(a, b_) for a, b_ in zip(got, want)]
    eerrs = [PR.G.rel(a, n(p)) for (W, b_), l in zip(pol.get_encoder_weights(), enc) for a, p in ((W, l.weight), (b_, l.bias))]
    print("closed loop %s: parameters after %d steps differ by %.3g at most (bound %.3g), the encoder's by %.3g (bound %.3g) [%s]"
          % (name, steps, max(errs), 100.0 * bg, max(eerrs), 100.0 * be, " ".join("%.3g" % e for e in eerrs)))
    assert len(got) == len(want) == len(errs) and len(eerrs) == 2 * len(case.enc)
    assert max(errs) <= 100.0 * bg, (errs, bg)
    assert max(eerrs) <= 100.0 * be, (eerrs, be)
    assert loss_dev[-1] < loss_dev[0] and loss_ref[-1] < loss_ref[0]
    assert opt.step_count == steps and opt.skipped == 0
    # (a condition on the twin, not a measurement of the device: torch moved every encoder tensor by more than the bound, so a step
    # that never reached one, or reached it with another group's gradient, does not pass)
    moved = [PR.G.rel(n(p), p0) for l, (W0, b0) in zip(enc, inp["enc"]) for p, p0 in ((l.weight, W0), (l.bias, b0))]
    assert min(moved) > 100.0 * be, (moved, be)
    opt.close()
    pol.close()
