"""Helper (collects no tests): a fixed list of configurations walked through `gaq_plan`, one SHA-256 per group.

The kernel selection of libgaq (gaq.hip: config_traits / plan_kernel) is pure host code, so "the library still answers what it answered
before" can be shown over the whole configuration space on a GPU-less host.  A row is gaq_plan's return code and the fourteen
gaq_plan_info fields; a group is one (per_env_params, control, noise) triple under one setting of the overrides that take part in the
choice (GAQ_FORCE_GENERIC, GAQ_NO_AUXP, GAQ_PREDRAW, GAQ_NT), so a digest that moves points at a corner of the space.

    python tests/plan_sweep.py --full [--out FILE]      the acceptance sweep of a change to the selection code: ~1e7 rows, minutes.
                                                        Run it on the library of the parent commit (GAQ_LIB=...) and on the new one.
    python tests/plan_sweep.py --write-golden           tests/golden/plan_sweep_digests.json from the library in use (the committed subset)

tests/test_plan_sweep_cpu.py asserts the committed subset against the recorded digests.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gym_art_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_sweep_digests.json")
OVERRIDE_VARS = ("GAQ_FORCE_GENERIC", "GAQ_NO_AUXP", "GAQ_PREDRAW", "GAQ_NT")
OVERRIDES = {"none": {}, "no_auxp": {"GAQ_NO_AUXP": "1"}, "force_generic": {"GAQ_FORCE_GENERIC": "1"},
             "predraw0_nt0": {"GAQ_PREDRAW": "0", "GAQ_NT": "0"}, "predraw1_nt1": {"GAQ_PREDRAW": "1", "GAQ_NT": "1"}}
COMMITTED_OVERRIDES = ("none", "no_auxp")

HUMMINGBIRD = dict(mass=0.816, inertia=(3.746575e-3, 3.746575e-3, 6.149342e-3), thrust_max=(5.603472,) * 4, torque_max=(0.2801736,) * 4,
                   prop_pos=(0.12, -0.12, 7.174e-3, -0.12, -0.12, 7.174e-3, -0.12, 0.12, 7.174e-3, 0.12, 0.12, 7.174e-3),
                   damp_time_up=0.0, damp_time_down=0.0, linearity=1.0, arm=0.169706, ou_sigma=0.01)
# the 16 observation-flag sets and the seven (envs, randomize_every, CUs, sub-steps) tuples of
# tests/test_plan_cpu.py::test_every_reachable_configuration_has_its_kernel
OBS_SETS = (0, 1, 2, 3, 4, 8, 12, 14, 15, 16, 18, 32, 64, 96, 33, 97)
SEVEN = ((1, 0, 256, 2), (65536, 0, 256, 2), (131072, 1, 256, 2), (131072, 0, 256, 1), (1 << 20, 0, 256, 2), (1 << 20, 0, 256, 4),
         (65536, 0, 64, 2))
TWO = ((65536, 0, 256, 2), (131072, 1, 256, 2))
EXTRAS = ("", "aux", "sense_input", "resample_goal", "excite", "swarm", "action_change")
LAYOUTS = ((0, 0), (1, 0), (2, 0), (1, 1), (0, 1))      # (obs_state_alias, fp32_state) as requested
# the parts of a sweep: (observation-flag sets, size tuples)
FULL = ((tuple(range(128)), TWO), (OBS_SETS, SEVEN))
COMMITTED = ((OBS_SETS, SEVEN),)

_LDS, _LAUNCHABLE = 8, 5      # positions of lds_per_wave / launchable among gaq_plan_info's fields


def _base_cfg():
    cfg = _lib.GaqConfig()
    cfg.struct_size, cfg.abi_version = C.sizeof(cfg), _lib.ABI_VERSION
    cfg.num_envs, cfg.sim_freq, cfg.sim_steps, cfg.ep_len = 4096, 200.0, 2, 500
    cfg.room_size, cfg.gravity, cfg.auto_reset = 10.0, 9.81, 1
    cfg.rew.pos, cfg.rew.effort, cfg.rew.crash, cfg.rew.orient, cfg.rew.spin = 1.0, 0.05, 1.0, 1.0, 0.1
    for k, v in HUMMINGBIRD.items():
        if isinstance(v, tuple):
            getattr(cfg.model, k)[:] = v
        else:
            setattr(cfg.model, k, v)
    return cfg


def _set_sense(cfg, sense):
    s = cfg.sense
    s.enabled = 1 if sense else 0
    s.pos_norm_std, s.gyro_noise_density = (0.005, 0.000175) if sense else (0.0, 0.0)
    s.gyro_norm_std = 0.01 if sense == 2 else 0.0
    s.gyro_bias_correlation_time = 1000.0 if sense else 0.0


def _set_extra(cfg, extra):
    cfg.aux_outputs = int(extra == "aux")
    cfg.sense_input = int(extra == "sense_input")
    cfg.resample_goal = int(extra == "resample_goal")
    cfg.excite = int(extra == "excite")
    sw = cfg.swarm
    sw.agents, sw.goal_radius, sw.collision_dist, sw.prox_dist = (8, 0.5, 0.3, 1.2) if extra == "swarm" else (0, 0.0, 0.0, 0.0)
    cfg.rew.action_change = 0.1 if extra == "action_change" else 0.0


class Sweep:
    """Digests of one walk: `digests[setting][group]` over whole rows, `digests_lds_free` with lds_per_wave blanked on the rows whose
    `launchable` is 0 (a handle that gaq_create refuses never hands that size to a kernel)."""

    def __init__(self):
        self.rows = self.accepted = 0
        self.distinct = set()
        self.digests, self.digests_lds_free = {}, {}

    def total(self, which="digests"):
        h = hashlib.sha256()
        for setting in sorted(getattr(self, which)):
            for group, d in sorted(getattr(self, which)[setting].items()):
                h.update(("%s %s %s\n" % (setting, group, d)).encode())
        return h.hexdigest()


def _walk_group(lib, cfg, parts, per_env, out, add):
    ref = C.byref(cfg)
    oref = C.byref(out)
    plan = lib.gaq_plan
    zeros = bytes(C.sizeof(out))
    for lag, drag in itertools.product((0, 1), (0, 1)):
        cfg.model.damp_time_up = cfg.model.damp_time_down = 0.15 if (lag and not per_env) else 0.0
        cfg.model.c_drag = 0.1 if (drag and not per_env) else 0.0
        a_lag, a_drag = (lag, drag) if per_env else (-1, -1)
        for obs_sets, sizes in parts:
            for obs_flags in obs_sets:
                cfg.obs_flags = obs_flags
                for sense in (0, 1, 2):
                    _set_sense(cfg, sense)
                    for extra in EXTRAS:
                        _set_extra(cfg, extra)
                        for alias, fp32 in LAYOUTS:
                            cfg.obs_state_alias, cfg.fp32_state = alias, fp32
                            for n, every, cus, sim_steps in sizes:
                                cfg.num_envs, cfg.sim_steps = n, sim_steps
                                rc = plan(ref, a_lag, a_drag, every if per_env else 0, cus, oref)
                                add(rc, bytes(out) if rc == 0 else zeros)


def sweep(parts, settings, lib=None):
    """Walk `parts` under each override setting of `settings` (names of OVERRIDES); the environment is put back afterwards."""
    lib = lib or _lib.load()
    res = Sweep()
    saved = {k: os.environ.get(k) for k in OVERRIDE_VARS}
    try:
        for setting in settings:
            for k in OVERRIDE_VARS:
                os.environ.pop(k, None)
            os.environ.update(OVERRIDES[setting])
            res.digests[setting], res.digests_lds_free[setting] = {}, {}
            for per_env, control, noise in itertools.product((0, 1), (0, 1, 2), (0, 1, 2)):
                cfg, out = _base_cfg(), _lib.GaqPlanInfo()
                cfg.per_env_params, cfg.control, cfg.noise = per_env, control, noise
                h, h_free = hashlib.sha256(), hashlib.sha256()

                def add(rc, fields, h=h, h_free=h_free):
                    row = struct.pack("<i", rc) + fields
                    res.rows += 1
                    res.accepted += rc == 0
                    res.distinct.add(row)
                    h.update(row)
                    if rc == 0 and fields[4 * _LAUNCHABLE:4 * _LAUNCHABLE + 4] == b"\0\0\0\0":
                        row = row[:4 + 4 * _LDS] + b"\0\0\0\0" + row[8 + 4 * _LDS:]
                    h_free.update(row)

                _walk_group(lib, cfg, parts, per_env, out, add)
                group = "per_env=%d control=%d noise=%d" % (per_env, control, noise)
                res.digests[setting][group], res.digests_lds_free[setting][group] = h.hexdigest(), h_free.hexdigest()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res


def committed(lib=None):
    """The digests of tests/golden/plan_sweep_digests.json.  lds_per_wave is hashed as 0 on the rows whose `launchable` is 0: gaq_create
    refuses such a handle, so the number never reaches a kernel, and it did move on the refused fp32_state rows when the size became
    tile_image<F>'s (4096 B: the host had branched on the fp32 request, the kernels on F_FP32).  Every other field of every row, and the
    size on every launchable row, is pinned."""
    return sweep(COMMITTED, COMMITTED_OVERRIDES, lib).digests_lds_free


def main(argv):
    if "--write-golden" in argv:
        json.dump(committed(), open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("wrote", GOLDEN)
        return 0
    if "--full" not in argv:
        sys.exit(__doc__)
    res = sweep(FULL, tuple(OVERRIDES))
    text = ["library %s" % _lib.LIB_PATH,
            "rows %d, accepted by gaq_plan %d, distinct rows %d" % (res.rows, res.accepted, len(res.distinct)),
            "digest of all group digests, whole rows                                  %s" % res.total(),
            "digest of all group digests, lds_per_wave blanked where launchable == 0  %s" % res.total("digests_lds_free")]
    for setting in OVERRIDES:
        for group in sorted(res.digests[setting]):
            text.append("%-14s %s  %s  %s" % (setting, group, res.digests[setting][group][:16], res.digests_lds_free[setting][group][:16]))
    print("\n".join(text))
    if "--out" in argv:
        open(argv[argv.index("--out") + 1], "w").write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
