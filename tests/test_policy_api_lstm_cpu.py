"""The public surface of LSTMPolicy's learner methods in gym_art_amd/policy.py, pinned as tests/test_policy_api_cpu.py pins the other
classes': the signature of each method, a docstring on each, the thin pair over one private body, and the names the class must not
have (the GRU's: the signatures differ by c0).  No library load."""
import inspect

import pytest

from gym_art_amd import policy

GRAD_TAIL = ("logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5, ent_coef=0.0, scale=None, grad=None, grad_value=None, "
             "grad_log_std=None, stats=None, stream=None)")
SURFACE = [
    ("evaluate_seq_dev", "(self, obs, actions, done, h0, c0, logp=None, value=None, mean=None, h_out=None, c_out=None, stream=None)"),
    ("ppo_bptt_grad_dev", "(self, obs, actions, done, h0, c0, " + GRAD_TAIL),
    ("ppo_bptt_grad_idx_dev", "(self, idx, obs, actions, done, h0, c0, " + GRAD_TAIL),
    ("set_weights", "(self, lstm, head_layers)"),
    ("set_weights_dev", "(self, packed)"),
    ("unpack", "(self, packed)"),
]


@pytest.mark.parametrize("name,signature", SURFACE, ids=[n for n, _ in SURFACE])
def test_lstm_policy_surface(name, signature):
    method = getattr(policy.LSTMPolicy, name)
    assert str(inspect.signature(method)) == signature
    assert method.__doc__ and method.__doc__.strip()


def test_lstm_policy_is_a_device_grad_class_with_names_of_its_own():
    assert issubclass(policy.LSTMPolicy, policy._DeviceGrad) and policy.LSTMPolicy.N_OUT == 4
    for name in ("ppo_seq_grad_dev", "ppo_seq_grad_idx_dev"):
        assert not hasattr(policy.LSTMPolicy, name), name
    for name in ("ppo_bptt_grad_dev", "ppo_bptt_grad_idx_dev"):
        assert not hasattr(policy.GRUPolicy, name), name
    # the public pair are thin methods over one private body
    for name in ("ppo_bptt_grad_dev", "ppo_bptt_grad_idx_dev"):
        src = inspect.getsource(getattr(policy.LSTMPolicy, name))
        assert "_ppo_bptt_grad(" in src and "gaq_policy_grad_ppo_lstm" not in src.split('"""')[2]
    body = inspect.getsource(policy.LSTMPolicy._ppo_bptt_grad)
    assert "gaq_policy_grad_ppo_lstm_seq_dev" in body and "gaq_policy_grad_ppo_lstm_seq_idx_dev" in body


def test_the_gru_surface_is_untouched():
    sig = lambda f: str(inspect.signature(f))
    assert sig(policy.GRUPolicy.evaluate_seq_dev) == "(self, obs, actions, done, h0, logp=None, value=None, mean=None, h_out=None, stream=None)"
    assert sig(policy.GRUPolicy.ppo_seq_grad_dev) == "(self, obs, actions, done, h0, " + GRAD_TAIL
