"""log_std on the device (gaq.h "log_std on the device: the exploration table"): what needs no GPU -- the new entry points are
declared, exported and bound, the Python methods exist with their signatures, the null refusals, and the condition the GPU tests
(tests/test_gpu_explore_dev.py) rest on: exp(+-x) of their two constant sets is nowhere near an fp32 rounding midpoint."""
import inspect
import os
import re

import numpy as np

from gym_art_amd import _lib
from gym_art_amd import policy as P

NEW = ("gaq_policy_set_explore_dev", "gaq_policy_get_log_std", "gaq_policy_explore_mode")
LOG_STD_A = (-1.0, -0.5, 0.25, -2.0)
LOG_STD_B = (-1.25, 0.5, -0.75, -1.5)
MARGIN = 1e-9


def midpoint_margin(x):
    """exp(x) in fp64: its distance from the nearer of the two fp32 rounding midpoints around it, relative to it"""
    y = np.exp(np.float64(x))
    f = np.float32(y)
    mids = [(np.float64(f) + np.float64(np.nextafter(f, np.float32(s) * np.float32(np.inf)))) / 2.0 for s in (-1.0, 1.0)]
    return min(abs(y - m) for m in mids) / y


def test_the_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "gaq.h")).read()
    lib = _lib.load()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in bound and getattr(lib, name) is not None, name
    assert bound["gaq_policy_set_explore_dev"][2] == [_lib._P] * 3 and bound["gaq_policy_get_log_std"][2] == [_lib._P] * 2
    assert all("GAQ_EXPLORE_%s %d" % (w, k) in header for k, w in enumerate(("NONE", "HOST", "DEVICE")))
    assert lib.gaq_abi_version() == 5


def test_null_handles_are_refused():
    lib = _lib.load()
    out = np.zeros(4, np.float32)
    assert lib.gaq_policy_set_explore_dev(None, None, None) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_get_log_std(None, _lib.ptr(out)) == -1 and b"null" in lib.gaq_last_error()
    assert lib.gaq_policy_explore_mode(None) == -1 and b"null" in lib.gaq_last_error()


def test_python_surface():
    def sig(f):
        return str(inspect.signature(f))
    for cls in (P.MLPPolicy, P.GRUPolicy, P.LSTMPolicy):
        for name in ("log_std_to_device", "log_std_to_host", "get_log_std"):
            assert sig(getattr(cls, name)) == "(self)" and getattr(cls, name).__doc__, (cls.__name__, name)
        assert cls.log_std_dev is None
    # what was there stays what it was
    assert sig(P.AdamDev.step) == "(self, grad, grad_value=None, grad_log_std=None, stats=None, stream=None, sync_log_std=True)"
    assert sig(P.AdamDev.sync_log_std) == "(self, stream=None)" and sig(P.MLPPolicy.set_log_std) == "(self, log_std=None)"


def test_the_constants_of_the_gpu_tests_keep_clear_of_every_rounding_midpoint():
    """a condition, not a measurement: for all 16 values of exp(+-x) the fp64 result lies at least 1e-9 (relative) from an fp32
    rounding midpoint, so a device exp that differs from the host's by many ulps of a double still rounds to the same float"""
    margins = [midpoint_margin(s * x) for x in LOG_STD_A + LOG_STD_B for s in (1.0, -1.0)]
    print("smallest margin %.3g" % min(margins))
    assert len(margins) == 16 and min(margins) >= MARGIN
    # (the helper itself: a midpoint has margin 0, a float sits half an ulp -- about 2^-24 relative -- from both)
    f = np.float32(1.2345)
    mid = (np.float64(f) + np.float64(np.nextafter(f, np.float32(2)))) / 2.0
    assert midpoint_margin(np.log(mid)) < 1e-15 and 2.0 ** -26 < midpoint_margin(np.log(np.float64(f))) < 2.0 ** -23
