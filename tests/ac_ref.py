"""fp64 references of the actor-critic rollout outputs (gaq.h gaq_step_policy_ac_many_dev, gaq_gae_dev): generalised advantage estimation,
the value head on an MLP and on a closed-loop GRU rollout, and the log-probability of an applied action with the error bars the tests
derive from the number formats."""
import numpy as np

from tests.gru_util import gru_step64
from tests.mlp_ref import forward64

TWO_LN_2PI = 2.0 * np.log(2.0 * np.pi)
U24 = 2.0 ** -24                 # half an ulp of an fp32 value, relative


def gae64(rew, done, values, gamma, lam):
    """rew [T, N], done [T, N], values [T + 1, N] -> (adv [T, N], ret [T, N]) in float64, vectorised over the envs:
    delta_t = r_t + gamma nd_t V_{t+1} - V_t,  A_t = delta_t + gamma lam nd_t A_{t+1} (A_T = 0),  ret_t = A_t + V_t,  nd = 1 - done."""
    rew, values = np.asarray(rew, np.float64), np.asarray(values, np.float64)
    nd = 1.0 - (np.asarray(done) != 0).astype(np.float64)
    T = rew.shape[0]
    adv = np.zeros_like(rew)
    nxt = np.zeros(rew.shape[1:])
    for t in range(T - 1, -1, -1):
        delta = rew[t] + gamma * nd[t] * values[t + 1] - values[t]
        nxt = delta + gamma * lam * nd[t] * nxt
        adv[t] = nxt
    return adv, adv + values[:T]


def gae_bar(rew, values, adv_ref, gamma, lam):
    """Per env, the bound on |A - A_ref| of an fp32 evaluation: the recursion contracts by c = gamma lam and each step adds at most four
    roundings of terms no larger than M = max_t (|r_t| + |V_t| + |V_{t+1}| + |A_t|), so 4 2^-24 M / (1 - c); for c = 1, 4 2^-24 M T."""
    rew, values, adv_ref = (np.asarray(x, np.float64) for x in (rew, values, adv_ref))
    T = rew.shape[0]
    M = (np.abs(rew) + np.abs(values[:T]) + np.abs(values[1:]) + np.abs(adv_ref)).max(axis=0)
    c = gamma * lam
    return 4.0 * U24 * M * (T if c >= 1.0 else 1.0 / (1.0 - c))


def value_head(W, seed):
    """(w [W], b) drawn like an output unit of tests/mlp_ref.py _scaled_layers / tests/gru_util.py _head: randn / sqrt(fan_in), 0.1 randn"""
    rng = np.random.RandomState(seed)
    return (rng.randn(W) / np.sqrt(W)).astype(np.float32), np.float32(0.1 * rng.randn())


def with_value(layers, value):
    """the layers with the value head as a fifth output unit of the last layer: forward64(with_value(...), act, False, x)[1] is
    [..., 0:4] the output sums and [..., 4] V"""
    W, b = layers[-1]
    w, bv = value
    return list(layers[:-1]) + [(np.vstack([W, np.asarray(w, np.float32).reshape(1, -1)]),
                                 np.concatenate([b, np.asarray(bv, np.float32).reshape(1)]))]


def mlp_means_values64(layers, act, out_tanh, value, x, hidden=None):
    """forward64 extended with the head: x [..., D] -> (means [..., 4] (after the output tanh), V [...], output sums [..., 4])"""
    _, z = forward64(with_value(layers, value), act, False, x, hidden)
    zz = z[..., :4]
    tanh = np.tanh if isinstance(zz, np.ndarray) else __import__("torch").tanh
    return (tanh(zz) if out_tanh else zz), z[..., 4], zz


def gru_means_values64(gru, layers, act, out_tanh, value, obs0, obs, done, h0, hidden=None):
    """tests/gru_util.py reference_rollout with the value head: (means [T, N, 4], values [T + 1, N], output sums [T, N, 4]).  h is zeroed
    in the rows of done[t] after step t; row T of the values is V of GRU(obs[T - 1], that h), which is not kept."""
    obs0, obs, done = (np.asarray(a) for a in (obs0, obs, done))
    h = np.asarray(h0, np.float64)
    T = obs.shape[0]
    means, values, sums = [], [], []
    for t in range(T + 1):
        x = np.asarray(obs0 if t == 0 else obs[t - 1], np.float64)
        hn = gru_step64(gru, x, h)
        # the head on h': a first "layer" that is the identity is not expressible in forward64, so its layers run here
        y = hn
        for W, b in layers[:-1]:
            y = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
            if hidden is not None:
                hidden.append(y)
            y = np.tanh(y) if act == "tanh" else np.maximum(y, 0.0)
        values.append(y @ np.asarray(value[0], np.float64).reshape(-1) + np.float64(value[1]))
        if t == T:
            break
        W, b = layers[-1]
        z = y @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        sums.append(z)
        means.append(np.tanh(z) if out_tanh else z)
        h = np.where(done[t][..., None] != 0, 0.0, hn)
    return np.stack(means), np.stack(values), np.stack(sums)


def std_of(log_std):
    """exp(log_std) as the library computes it: float32(exp(float64(log_std)))"""
    return np.exp(np.asarray(log_std, np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)


def logp64(actions, means, log_std, mean_atol=0.0):
    """actions [..., 4] (fp32, as applied), means [..., 4] -> (ref [...], bar [...]): the log-probability with z' = (a - m) / std in float64,
    and the derived bound on |device - ref|.  With the means exact (the deterministic twin's bits) z' is the device's z to half an ulp of
    a: dz_k = 2^-24 |a_k| / std_k, which moves sum z^2 / 2 by at most sum (|z'_k| dz_k + dz_k^2 / 2); the device's own fp32 evaluation
    (four fmas, five sums) adds 16 2^-24 max(1, |ref| + sum z'_k^2 / 2).  Means known only to mean_atol add sum |z'_k| mean_atol / std_k."""
    a, m = np.asarray(actions, np.float64), np.asarray(means, np.float64)
    ls = np.asarray(log_std, np.float32).astype(np.float64)
    std = std_of(log_std)
    z = (a - m) / std
    ref = (-0.5 * z * z - ls).sum(axis=-1) - TWO_LN_2PI
    dz = U24 * np.abs(a) / std
    bar = (np.abs(z) * dz + 0.5 * dz * dz).sum(axis=-1) + 16.0 * U24 * np.maximum(1.0, np.abs(ref) + (0.5 * z * z).sum(axis=-1))
    bar = bar + (np.abs(z) * mean_atol / std).sum(axis=-1)
    return ref, bar


def logp32(z, log_std):
    """the device's formula in float32 on given draws z [..., 4]: fma(-z/2, z, -log_std) summed k ascending from 0, then - 2 ln 2 pi
    (each fma is emulated as the float32 rounding of the float64 result, which is exact for these magnitudes' products)"""
    z = np.asarray(z, np.float32)
    ls = np.asarray(log_std, np.float32)
    acc = np.zeros(z.shape[:-1], np.float32)
    for k in range(4):
        term = (np.float64(-0.5) * z[..., k].astype(np.float64) * z[..., k].astype(np.float64) - np.float64(ls[k])).astype(np.float32)
        acc = (acc + term).astype(np.float32)
    return (acc - np.float32(TWO_LN_2PI)).astype(np.float32)
