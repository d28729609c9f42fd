"""-m gpu: a handle keeps the kernel-selection overrides (GAQ_FORCE_GENERIC, GAQ_NO_AUXP, GAQ_PREDRAW, GAQ_NT) it was created under."""
import ctypes as C
import os

import numpy as np
import pytest

from gym_art_amd import _lib

pytestmark = pytest.mark.gpu
F_AUXP = 65536


@pytest.mark.parametrize("n", [64, 65])
def test_a_parameter_upload_selects_under_the_overrides_of_gaq_create(n):
    """A per-env RawControl handle with the info dict's aux row on a split layout is an F_AUXP handle when GAQ_NO_AUXP is unset at
    gaq_create.  Setting GAQ_NO_AUXP=1 afterwards and uploading the same parameters again leaves gaq_kernel_variant where it was, and the
    handle steps: the refresh behind the upload uses the handle's snapshot of the overrides, not the environment of the moment.
    (Before the snapshot the refresh re-read the variable: the variant lost F_AUXP, the split-state handle found itself "needing the
    generic kernel", and the step was refused with GAQ_ERR_STATE.)  One tile, and a second tile of one lane."""
    import torch
    from tests.test_plan_cpu import base_cfg
    assert "GAQ_NO_AUXP" not in os.environ
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    cfg = base_cfg(n, per_env_params=1, control=1, obs_state_alias=1, aux_outputs=1, auto_reset=1)
    rows = np.tile(np.frombuffer(bytes(cfg.model), dtype=np.float64), (n, 1))
    h = C.c_void_p()
    _lib.check(lib.gaq_create(C.byref(cfg), C.byref(h)))
    try:
        _lib.check(lib.gaq_set_params(h, _lib.ptr(rows), 0, n))
        variant = lib.gaq_kernel_variant(h)
        assert variant & F_AUXP and lib.gaq_state_layout(h) != 0, variant
        os.environ["GAQ_NO_AUXP"] = "1"
        try:
            _lib.check(lib.gaq_set_params(h, _lib.ptr(rows), 0, n))
            assert lib.gaq_kernel_variant(h) == variant
            D = lib.gaq_obs_dim(h)
            obs = torch.zeros((n, D), device=dev); rew = torch.zeros(n, device=dev); done = torch.zeros(n, dtype=torch.uint8, device=dev)
            act = torch.zeros((n, 4), device=dev)
            _lib.check(lib.gaq_reset_dev(h, None, _lib.ptr(obs), None))
            _lib.check(lib.gaq_step_dev(h, _lib.ptr(act), _lib.ptr(obs), _lib.ptr(rew), _lib.ptr(done), None))
            torch.cuda.synchronize()
            assert lib.gaq_launch_variant(h) == variant
            assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
        finally:
            del os.environ["GAQ_NO_AUXP"]
    finally:
        lib.gaq_destroy(h)
