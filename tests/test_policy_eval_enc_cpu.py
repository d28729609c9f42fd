"""The learner's forward pass for a recurrent policy with an encoder (gaq.h "sequences through an encoder";
GRUPolicy / LSTMPolicy.evaluate_enc_seq_dev): the surface of the new entry point, the LDS figures of the family it states, and that the
calls it stands beside keep the names, signatures and refusals they had -- no GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

from gym_art_amd import _lib
from gym_art_amd import policy as P

HEADER = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gaq.h")).read()
CAP = 160 * 1024


def fwd_lds(in_dim, H, head):
    """gaq.h's formula for the forward call: 8.25 KiB + 272 B x (in_dim rounded up to 16 + 2 H + the head widths)"""
    return 8448 + 272 * (((in_dim + 15) & ~15) + 2 * H + sum(head))


def test_the_entry_point_is_declared_bound_and_refuses_a_null_handle():
    lib = _lib.load()
    sig = {n: a for n, _, a in _lib.SYMBOLS}
    name = "gaq_policy_eval_enc_seq_dev"
    # gaq_policy_eval_lstm_seq_dev's arguments: both cells through one call
    assert sig[name] == sig["gaq_policy_eval_lstm_seq_dev"] and len(sig[name]) == 14
    assert sig[name][1] is C.c_int32 and sig[name][2] is C.c_int64 and "int " + name + "(" in HEADER
    assert hasattr(lib, name)
    assert lib.gaq_abi_version() == 5 and "#define GAQ_ABI_VERSION 5" in HEADER    # additive: the ABI version stays
    assert getattr(lib, name)(None, 2, 4, *[None] * 11) == -1 and b"null" in lib.gaq_last_error()


def test_the_header_states_the_family_and_the_scratch():
    decl = HEADER[HEADER.index("sequences through an encoder"):HEADER.index("int gaq_policy_eval_enc_seq_dev(")]
    for words in ("encoder widths <= 128", "H and head widths <= 64", "must be NULL for a GRU", "2^31 - 1", "GAQ_ABI_VERSION stays 5",
                  "8.25 KiB + 272 B x (E + 2 H + the head widths)", "only when a call needs more than every call"):
        assert words in decl, words
    m = re.search(r"#define GAQ_ENC_FEAT_BYTES\(T, S, E\) \(\(size_t\)\(T\) \* \(size_t\)\(S\) \* \(size_t\)\(E\) \* 4u\)", HEADER)
    assert m, "the scratch's size is a macro of gaq.h"


def test_every_forward_call_of_the_family_fits_the_lds():
    """E <= 128 and H, head <= 64: the widest forward call is 110.25 KiB, so the sequence kernel's LDS refusal (kept, with its text) is
    never what bounds the forward pass of the family; the source still makes it"""
    assert fwd_lds(128, 64, (64, 64)) == 110.25 * 1024 <= CAP
    assert fwd_lds(64, 64, (64, 64)) == 93.25 * 1024
    assert max(fwd_lds(E, H, hd) for E in range(16, 129, 16) for H in (16, 32, 48, 64) for hd in ((), (64,), (64, 64))) <= CAP
    src = open(os.path.join(_lib._HERE, "csrc", "gaq_policy_grad_seq.hip")).read()
    assert "in_dim too large for the sequence kernel's LDS" in src


SURFACE = [
    ("GRUPolicy", "(self, obs, actions, done, h0, logp=None, value=None, mean=None, h_out=None, stream=None)", "evaluate_seq_dev"),
    ("LSTMPolicy", "(self, obs, actions, done, h0, c0, logp=None, value=None, mean=None, h_out=None, c_out=None, stream=None)",
     "evaluate_seq_dev"),
]


@pytest.mark.parametrize("cls,signature,parent", SURFACE, ids=[s[0] for s in SURFACE])
def test_the_python_surface(cls, signature, parent):
    """evaluate_enc_seq_dev takes the parameters of the class's evaluate_seq_dev, which keeps its own; it is a thin method over the
    shared private body"""
    klass = getattr(P, cls)
    new = klass.evaluate_enc_seq_dev
    assert str(inspect.signature(new)) == signature == str(inspect.signature(getattr(klass, parent)))
    assert "gaq_policy_eval_enc_seq_dev" in new.__doc__ and "bit for bit" in new.__doc__
    assert len(inspect.getsource(new).split('"""')[2].strip().splitlines()) == 1     # one statement behind the docstring
    assert "_evaluate_enc_seq" in inspect.getsource(new) and hasattr(P._RecurrentPolicy, "_evaluate_enc_seq")


def test_the_refusals_of_the_existing_calls_are_the_source_they_were():
    """the texts tests/test_gpu_policy_encoder.py pins on the device stand in the source unchanged, and the new view has its own"""
    src = open(os.path.join(_lib._HERE, "csrc", "gaq_policy.hip")).read()
    assert "policy: no sequence passes on a policy with an encoder yet (gaq_policy_eval_seq_dev, gaq_policy_grad_ppo_seq_dev, " in src
    assert "optim: no step in place on a policy with an encoder yet" in src
    view = src[src.index("int policy_grad_enc_seq_view("):src.index("int policy_encode_rows(")]
    for words in ("null argument", "this one on the", "has none", "must be NULL for a policy on the GRU engine", "encoder weights not set",
                  "weights not set", "of width up to"):
        assert words in view, words
