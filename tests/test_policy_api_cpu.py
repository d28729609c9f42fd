"""The public surface of the learner's methods in gym_art_amd/policy.py, pinned: the signature and the docstring of each of the
contiguous / index-gathered gradient pairs and of the forward passes beside them.  The pairs are thin methods over one private body
each; this is what keeps a change to a body from moving a public name, a default or a documented contract.  No library load."""
import hashlib
import inspect

import pytest

from gym_art_amd import policy

# (class, method, str(inspect.signature(method)), md5 of its docstring)
SURFACE = [
    ("MLPPolicy", "logp_dev",
     "(self, obs, actions, out=None, mean=None, stream=None)",
     "e0ccbf0534e2ea6889a38bb1b68d0574"),
    ("MLPPolicy", "backward_dev",
     "(self, obs, dout, scale=1.0, grad=None, stream=None)",
     "42c3844953cac4389d97e242d52c9e74"),
    ("MLPPolicy", "ppo_grad_dev",
     "(self, obs, actions, logp_old, adv, clip=0.2, scale=None, grad=None, grad_log_std=None, stats=None, stream=None)",
     "c9177081a4b0ccad7a14a17ad63609a0"),
    ("MLPPolicy", "ppo_grad_idx_dev",
     "(self, idx, obs, actions, logp_old, adv, clip=0.2, scale=None, grad=None, grad_log_std=None, stats=None, stream=None)",
     "92635363abd520dc9ed3a024c9f7a5c3"),
    ("MLPPolicy", "evaluate_dev",
     "(self, obs, actions, logp=None, value=None, mean=None, stream=None)",
     "c20b2bf9d3b7515d2d18d709c1535e96"),
    ("MLPPolicy", "ppo_ac_grad_dev",
     "(self, obs, actions, logp_old, adv, ret, v_old=None, clip=0.2, vclip=None, vf_coef=0.5, ent_coef=0.0, scale=None, grad=None, "
     "grad_value=None, grad_log_std=None, stats=None, stream=None)",
     "1de826a5c712c2b3b2161670069a6292"),
    ("MLPPolicy", "ppo_ac_grad_idx_dev",
     "(self, idx, obs, actions, logp_old, adv, ret, v_old=None, clip=0.2, vclip=None, vf_coef=0.5, ent_coef=0.0, scale=None, grad=None, "
     "grad_value=None, grad_log_std=None, stats=None, stream=None)",
     "df3cf40e6d31d160e66d2774a3c444ad"),
    ("GRUPolicy", "evaluate_seq_dev",
     "(self, obs, actions, done, h0, logp=None, value=None, mean=None, h_out=None, stream=None)",
     "87a8e7b0464db524b3673076e4d27ec1"),
    ("GRUPolicy", "ppo_seq_grad_dev",
     "(self, obs, actions, done, h0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5, ent_coef=0.0, scale=None, "
     "grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None)",
     "a7b16ea4fed2b2e396e61996951e648f"),
    ("GRUPolicy", "ppo_seq_grad_idx_dev",
     "(self, idx, obs, actions, done, h0, logp_old, adv, ret=None, v_old=None, clip=0.2, vclip=None, vf_coef=0.5, ent_coef=0.0, "
     "scale=None, grad=None, grad_value=None, grad_log_std=None, stats=None, stream=None)",
     "0cce92583bcc5001f579d9f7fef42baa"),
    ("MLPCritic", "backward_dev",
     "(self, obs, dout, scale=1.0, grad=None, stream=None)",
     "1d7ac26bad7057377f8864ab5997feff"),
    ("MLPCritic", "mse_grad_dev",
     "(self, obs, target, scale=None, grad=None, stats=None, stream=None)",
     "51701de100de8ed356584f1f444e1218"),
    ("MLPCritic", "mse_grad_idx_dev",
     "(self, idx, obs, target, scale=None, grad=None, stats=None, stream=None)",
     "51c9f8568b731b09ac57a8e44e14f2d6"),
]


@pytest.mark.parametrize("cls,name,signature,doc_md5", SURFACE, ids=["%s.%s" % (c, m) for c, m, _, _ in SURFACE])
def test_public_surface(cls, name, signature, doc_md5):
    method = getattr(getattr(policy, cls), name)
    assert str(inspect.signature(method)) == signature
    assert hashlib.md5(method.__doc__.encode()).hexdigest() == doc_md5
