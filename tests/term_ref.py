"""fp64 references of time-limit bootstrapping (gaq.h gaq_step_policy_ac_term_many_dev, gaq_gae_term_dev): advantages that bootstrap from
the terminal observation's value at a done, their error bar, and the value of a terminal row for an MLP and for a closed-loop GRU."""
import numpy as np

from tests import ac_ref
from tests.gru_util import gru_step64


def gae_term64(rew, done, values, term_values, gamma, lam):
    """rew [T, N], done [T, N], values [T + 1, N], term_values [T, N] -> (adv [T, N], ret [T, N]) in float64; d = done[t] != 0:
    V' = d ? term_values[t] : V_{t+1},  delta_t = r_t + gamma V' - V_t,  A_t = delta_t + (d ? 0 : gamma lam) A_{t+1} (A_T = 0),
    ret_t = A_t + V_t.  term_values is selected, not multiplied: what it holds where done is clear (NaN included) is never used."""
    rew, values, term = (np.asarray(x, np.float64) for x in (rew, values, term_values))
    d = np.asarray(done) != 0
    T = rew.shape[0]
    adv = np.zeros_like(rew)
    nxt = np.zeros(rew.shape[1:])
    for t in range(T - 1, -1, -1):
        delta = rew[t] + gamma * np.where(d[t], term[t], values[t + 1]) - values[t]
        nxt = delta + np.where(d[t], 0.0, gamma * lam * nxt)
        adv[t] = nxt
    return adv, adv + values[:T]


def gae_term_bar(rew, done, values, term_values, adv_ref, gamma, lam):
    """Per env, the bound on |A - A_ref| of the fp32 evaluation: ac_ref.gae_bar with |term_value| added to M.
    Derivation.  A step of the device's recursion is delta = fl(fl(gamma V' + r_t) - V_t), A_t = fl(c A_{t+1} + delta) with c = fl(gamma
    lam) (or 0 at a done): two fused multiply-adds, one subtraction and the rounding of c, i.e. at most four roundings, each of a quantity
    no larger than |r_t| + |V_t| + |V'| + |A_t|.  V' is V_{t+1} where done is clear and term_value[t] where it is set, so M = max_t (|r_t|
    + |V_t| + |V_{t+1}| + |A_t| + [done_t] |term_value_t|) bounds that quantity in both cases (gae_bar's M is this without the last term:
    there V' is V_{t+1} or nothing).  An error made at step t reaches A_s, s < t, multiplied by at most c^(t - s) -- a done multiplies
    it by 0, which is smaller still -- so the errors sum to at most 4 2^-24 M / (1 - c), and to 4 2^-24 M T at c = 1: gae_bar's formula.
    |term_value| enters through gae_bar's |r| term (it takes |rew| itself), so the formula is gae_bar's own code."""
    term = np.where(np.asarray(done) != 0, np.abs(np.asarray(term_values, np.float64)), 0.0)
    return ac_ref.gae_bar(np.abs(np.asarray(rew, np.float64)) + term, values, adv_ref, gamma, lam)


def mlp_term_values64(net, term_rows):
    """V64 of terminal rows [K, D] for a tests/test_gpu_policy_ac.py _Net of kind "mlp"; the pre-activations go to `hidden` if given"""
    _, v, _ = ac_ref.mlp_means_values64(net.layers, net.act, net.out_tanh, net.value, np.asarray(term_rows, np.float64))
    return v


def gru_head_value64(net, hn):
    """V64(head(h')) for a _Net of kind "gru": ac_ref.gru_means_values64's head on given h' [K, H]"""
    y = hn
    for W, b in net.layers[:-1]:
        y = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        y = np.tanh(y) if net.act == "tanh" else np.maximum(y, 0.0)
    return y @ np.asarray(net.value[0], np.float64).reshape(-1) + np.float64(net.value[1])


def gru_term_values64(net, obs0, obs, done, h0, term_at, term_rows):
    """For a _Net of kind "gru": V64(head(GRU64(term row, h_t))) of each env's terminal row, h_t from the fp64 recurrence on the recorded
    observations and dones stepped as ac_ref.gru_means_values64 steps it (h zeroed in the rows of done[t] after step t): h_t is the state
    action t used, i.e. GRU(obs_{t-1}, h) before that zeroing.  term_at [N]: the step each env finished in; term_rows [N, D].
    Returns [N]."""
    obs0, obs, done = (np.asarray(a) for a in (obs0, obs, done))
    h = np.asarray(h0, np.float64)
    T, N = obs.shape[0], obs.shape[1]
    out = np.full(N, np.nan)
    rows = np.asarray(term_rows, np.float64)
    for t in range(T):
        x = np.asarray(obs0 if t == 0 else obs[t - 1], np.float64)
        hn = gru_step64(net.gru, x, h)                              # the state action t used
        sel = np.nonzero(np.asarray(term_at) == t)[0]
        if sel.size:
            out[sel] = gru_head_value64(net, gru_step64(net.gru, rows[sel], hn[sel]))
        h = np.where(done[t][..., None] != 0, 0.0, hn)
    return out
