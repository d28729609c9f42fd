"""GPU: EVERY step kernel a `sense_noise` configuration can select, against the fp64 oracle on the device's OWN draws.

The fixture tests (G10 / G16 / G15) need injected draws, and injected draws force the full generic kernel on fp64 planes; the kernels a
user gets with QuadrotorEnv(sense_noise=...) -- the split-state F_PACK / F_AUXP / F_ENVX / F_BIAS forms, Mellinger + noise, the per-env
twins, the plain-layout specialised kernels -- were compared with the generic kernel only.  Here tests/sense_replay.py rebuilds, on the
host, the standard draws the device makes for each env and step (a pure function of seed, global env index, key and stream) in the
oracle's slot layout, and oracle/quad_oracle.py -- NumPy fp64, pinned to the reference's recorded draws at 1e-12 -- flies beside the
kernel: the oracle's own add_noise / observe / reward arithmetic, shared with the device only through the Philox / Box-Muller generator.

A case is one instantiated feature mask: the constructor arguments that select it (`launch_variant` has to agree), 2088 envs (32 wave
tiles and one of 40 lanes) at a non-zero global index, random full-scale states written with set_state, random actions, 40 steps
without resets.  A reset observation and an observe() call (one add_noise call each) are checked first; then observations, rewards
and dones every step, the info dict's aux row where there is one, the gyro-bias plane at the end.  Teeth: with the draws of env i + 1
given to env i, or with the noise left out, the same comparison misses the bound by more than 100 x.  The last test compares the flown
masks with everything gaq_plan can return for a configuration with sensor noise."""
import contextlib
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import sense_replay as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_ENV, LAG, NOISE, GENERIC, ALIAS, FP32, LITE, PREDRAW, NT, DIAG, PACK, RZ, ROWS, CTR, MELL, SWARM, AUXP, ENVX, BIAS = (1 << k for k in range(19))
SAMPLER = {"class": "RelativeSampler", "noise_ratio": 0.2, "sampler": "normal"}
WALK = {"gyro_norm_std": 0.01, "quat_norm_std": 0.01, "pos_unif_range": 0.01, "vel_unif_range": 0.02, "quat_unif_range": 0.005}
N, STEPS, OFFSET, SEED = 2088, 40, (1 << 20) + 192, 57
TEETH_STEPS = 2

# ---- tolerances: against the ORACLE, never against another kernel ---------------------------------------------------------------------
# Observations: the project's parity tolerance, 1e-6 of max(|oracle|, 1) (tests/test_gpu_parity.py).  One cause beyond those tests
# enters: the device's Box-Muller uses the hardware log / sin / cos, 1e-6 of a normal (tests/test_gpu_round2.py), times a noise scale of
# at most 0.02 here.  The rule: 1e-6 wherever the worst measured on the MI355X is at most 5e-7; a case above that gets 2 x its measured
# worst, never above the 3e-6 the host-build stream test grants for the same cause.
# Rewards: 3e-7 absolute (the fixture tests' bound) where the measured worst is at most 1.5e-7.  Gyro bias: 2e-7 (test_gpu_round2.py).
# Measured worst over all 95 flights (MI355X; every case prints its own line):  observations 2.66e-6 (75 of the 95 at most 5e-7)
#                                              rewards 6.8e-9      gyro bias 1.7e-8      aux row 4.5e-7 (of its allowance, see AUX_TOL)
OBS_TOL = 1e-6
# The cases whose measured worst is above 5e-7; the word is omega (15 .. 17) in every one.  All but two have Philox thrust noise ON
# (F_NOISE): the OU thrust-noise normals go through the device's fast Box-Muller, and a thrust difference reaches omega through arm /
# inertia (largest on the Crazyflie's 1e-5 kg m^2, and under Mellinger's feedback: gain 200 on the attitude error, 50 on omega).  The two
# without thrust noise, <214032> and <214034>, are Mellinger on per-env goals (F_MELL | F_ENVX): omega under the controller's feedback on
# tumbling full-scale states; what makes them larger than Mellinger on the default goal (<17424> ..., <82960> ...: at most 5e-7) is NOT
# isolated yet.  mask -> measured worst; the bound is min(3e-6, 2 x measured).
OBS_MEASURED_ABOVE_5E7 = {5: 5.60e-7, 6: 7.00e-7, 7: 9.08e-7, 1046: 6.60e-7, 1047: 8.44e-7, 2055: 1.15e-6, 3095: 7.78e-7, 17431: 7.07e-7,
                          19479: 2.66e-6, 66582: 5.33e-7, 66583: 6.89e-7, 68631: 7.34e-7, 197654: 6.11e-7, 197655: 1.40e-6, 199703: 9.85e-7,
                          214032: 1.09e-6, 214034: 8.77e-7, 214036: 7.29e-7, 214038: 2.41e-6, 459798: 5.88e-7}
OBS_TOL_CAP = 3e-6      # what test_device_sensor_noise_streams_against_the_host_build grants for the same cause
REW_TOL = 3e-7
BIAS_TOL = 2e-7
AUX_TOL = 1e-6          # the aux row's words (accelerometer, omega_dot, torque, controller output, filtered commands): fp32 roundings of the
#                         fp64 quantities like the observation's, same scale rule; omega_dot with thrust noise on gets Oracle.omega_dot_slack
#                         on top (measured without it: up to 7.5e-6 of max(|omega_dot|, 1), <82966>; thrust noise off: 6e-8)
EPS_NORMAL = 1e-6       # the device's Box-Muller (hardware log / sin / cos) against libm's: "1e-6 of a normal" (tests/test_gpu_round2.py)
TEETH = 100.0
QUAT_FACTOR_DROPPED = 55.0        # 1 / (4 w) + 1 / (8 w^2) at w = 0.05: the rows the HIP-vs-HIP tests drop
OBS_PACK = ["xyz_vxyz_R_omega", "xyz_vxyz_R_omega_h", "xyzr_vxyzr_R_omega_h", "xyz_vxyz_R_omega_acc_act", "xyzr_vxyzr_R_omega", "xyz_vxyz_R_omega_act"]
OBS_AUXP = ["xyz_vxyz_quat_omega", "xyz_vxyz_R_omega_t2w_t2t", "xyz_vxyz_R_omega_acc_act", "xyzr_vxyzr_quat_omega_h", "xyz_vxyz_R_omega_t2w",
            "xyzr_vxyzr_R_omega_t2w", "xyzr_vxyzr_quat_omega", "xyz_vxyz_R_omega_h"]
FLOWN = set()
WORST_AT = []                     # (excess, observation word) of every comparison of the running case: the log names the word


@contextlib.contextmanager
def environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: v for k, v in kv.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def instantiated():
    src = open(os.path.join(ROOT, "gym_art_amd", "csrc", "gaq_kernels.hpp")).read()
    out = set()
    for m in re.finditer(r"#define GAQ_STEP_PART\d\(X\)(.*)", src):
        out |= {int(x) for x in re.findall(r"X\((\d+)u\)", m.group(1))}
    return out


def noise_capable_masks():
    """Every step-kernel mask gaq_plan returns for a configuration with sense.enabled and device-drawn noise: the option space of
    tests/test_plan_cpu.py (models x lag x controller x thrust noise x observation flags x both gyro models x the extras that pick a
    tier x layouts x fp32 x per-episode re-randomisation), the F_ROWS / F_CTR twins a launch can switch to included."""
    from tests.test_plan_cpu import base_cfg, plan
    seen = set()
    for per_env, lag, control, noise in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1)):
        for obs_flags, sense, extra in itertools.product([0, 1, 2, 3, 4, 8, 12, 14, 15, 16, 18, 32, 64, 96, 33, 97], (1, 2),
                                                         ("", "aux", "resample_goal", "excite", "swarm", "action_change")):
            if extra == "swarm" and (obs_flags & 16):
                continue
            for (alias, fp32), every in itertools.product(((0, 0), (1, 0), (2, 0), (1, 1)), (0, 1)):
                if every and not per_env:
                    continue
                kw = {"per_env_params": per_env, "control": control, "noise": noise, "obs_flags": obs_flags, "obs_state_alias": alias,
                      "fp32_state": fp32, "auto_reset": 1, "sense.enabled": 1, "sense.pos_norm_std": 0.005, "sense.gyro_noise_density": 0.000175,
                      "sense.gyro_norm_std": 0.0 if sense == 1 else 0.01, "sense.gyro_bias_correlation_time": 1000.0}
                if not per_env:
                    kw["model.damp_time_up"] = kw["model.damp_time_down"] = 0.15 if lag else 0.0
                if extra == "aux":
                    kw["aux_outputs"] = 1
                elif extra in ("resample_goal", "excite"):
                    kw[extra] = 1
                elif extra == "swarm":
                    kw.update({"swarm.agents": 8, "swarm.goal_radius": 0.5, "swarm.collision_dist": 0.3, "swarm.prox_dist": 1.2})
                elif extra == "action_change":
                    kw["rew.action_change"] = 0.1
                p = plan(base_cfg(N, **kw), lag if per_env else -1, 0 if per_env else -1, every, 256)
                if p.launchable:
                    seen |= {v for v in (p.step_variant, p.rows_variant, p.ctr_variant) if v >= 0}
    return seen


def recipe(mask, k=0):
    """Constructor arguments (and creation environment) of a sensor-noise configuration that selects step_kernel<mask>: the inverse of
    gaq.hip select_kernel on the noisy part of its domain.  `k` rotates the observation variant."""
    kw, env = {}, {}
    if mask & PER_ENV:
        kw["dyn_sampler_1"] = dict(SAMPLER)
    if mask & RZ:
        kw["dynamics_randomize_every"] = 1
    if mask & GENERIC:
        lite, diag = bool(mask & LITE), bool(mask & DIAG)
        kw["alias_obs"] = False
        if lite:                                             # the light tier: per-env goals, or (F_DIAG) the aux row on a uniform model
            kw["sense_noise"] = "default"
            kw.update(dict(info=True, obs_repr="xyz_vxyz_R_omega_acc_act") if diag else dict(resample_goal=True, obs_repr=OBS_PACK[k % 6]))
        elif diag:                                           # the full tier with the aux row: the bias walk (uniform) / per-env models
            kw.update(info=True, sense_noise="default" if mask & PER_ENV else dict(WALK), obs_repr=OBS_AUXP[k % 8])
        else:                                                # <8>, <9>, <2057>: the device-drawn generic kernel, the reference of the
            kw.update(sense_noise=dict(WALK), obs_repr=OBS_PACK[k % 6])      # HIP-vs-HIP tests
            env["GAQ_FORCE_GENERIC"] = "1"
        return kw, env
    if mask & LAG:
        kw["dynamics_params"] = "Crazyflie"
    kw["thrust_noise"] = "philox" if mask & NOISE else "off"
    if mask & MELL:
        kw["raw_control"] = False
    kw["sense_noise"] = dict(WALK) if mask & BIAS else "default"
    if mask & ENVX:
        kw.update(obs_repr=OBS_AUXP[k % 8] if mask & BIAS else OBS_PACK[k % 6])
        if not mask & BIAS:
            kw["resample_goal"] = True
    elif mask & AUXP:
        kw.update(info=True, obs_repr=OBS_AUXP[k % 8] if not (mask & PER_ENV and mask & MELL) else OBS_PACK[k % 6])
    elif mask & PACK:
        kw["obs_repr"] = OBS_PACK[k % 6]
    else:
        kw.update(alias_obs=False, obs_repr="xyz_vxyz_R_omega")      # the plain-layout specialised kernels: the 18-word observation only
    return kw, env


def random_state(n, rng, walk, goals):
    """Full-scale initial states as in test_device_sensor_noise_streams_against_the_host_build: [42, n] planes."""
    st = np.zeros((42, n))
    st[0:3] = (rng.uniform(-2, 2, (n, 3)) + [0, 0, 2]).astype(np.float32).T
    st[2] = np.maximum(st[2], 0.3)
    st[3:6] = rng.uniform(-1, 1, (3, n)).astype(np.float32)
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    q[np.linalg.det(q) < 0, :, 0] *= -1
    st[6:15] = q.astype(np.float32).reshape(n, 9).T
    st[15:18] = rng.uniform(-3, 3, (3, n)).astype(np.float32)
    st[34:37] = np.array([[0.], [0.], [2.]])
    if goals:
        st[34:37] += rng.uniform(-0.5, 0.5, (3, n)).astype(np.float32)
    if walk:
        st[39:42] = rng.uniform(-0.01, 0.01, (3, n)).astype(np.float32)
    return st


class Oracle(object):
    """The oracle twin of one env object: parameters read back from the device, the configuration from the constructor arguments."""

    def __init__(self, env, kw):
        from gym_art_amd import _lib
        from gym_art_amd.quadrotor import OBS_FLAGS
        from oracle import quad_oracle as qo
        self.qo, self.env, n = qo, env, env.num_envs
        self.n = n
        rows = np.empty((n, _lib.MODEL_DOUBLES), dtype=np.float64)
        if env._per_env:
            _lib.check(env._lib.gaq_get_params(env._handle, _lib.ptr(rows), 0, n))       # what the device flies with
        else:
            rows[:] = _lib.models_to_rows(env.models)[0]
        m = _lib.rows_to_models(rows)
        self.thrust_noise = kw.get("thrust_noise", "philox") == "philox" and bool(np.any(m["ou_sigma"] != 0))
        self.p = qo.Params(n, mass=m["mass"], inertia=m["inertia"], thrust_max=m["thrust_max"], torque_max=m["torque_max"],
                           prop_pos=m["prop_pos"].reshape(n, 4, 3), damp_time_up=m["damp_time_up"], damp_time_down=m["damp_time_down"],
                           linearity=m["linearity"], arm=m["arm"], ou_sigma=m["ou_sigma"], vel_damp=m["vel_damp"],
                           damp_omega_quadratic=m["damp_omega_quadratic"], C_drag=m["c_drag"], C_roll=m["c_roll"])
        control = "raw_zero_middle" if kw.get("raw_control", True) else "mellinger"
        if control == "mellinger":
            self.p.jacobian_inverse()
        self.cfg = qo.Config(sim_freq=env.sim_freq, sim_steps=env.sim_steps, ep_time=env.ep_time, control=control, obs_repr=env.obs_repr)
        self.cfg.action_f32 = True
        self.cfg.t2w_std, self.cfg.t2t_std = env.t2w_std, env.t2t_std
        assert self.cfg.ep_len == env.ep_len
        self.flags = OBS_FLAGS[env.obs_repr]
        self.prm = {k: v for k, v in env._sense.items() if k != "bypass"}
        self.walk = self.prm["gyro_norm_std"] != 0.0
        self.seed, self.off = env._seed_value, env.env_id_offset

    def twin(self, st, mode):
        """(state, SenseNoise) at the device state `st` [42, n]; mode: "replay", "next env" (the draws of env i + 1), "no noise"."""
        qo, n = self.qo, self.n
        s = qo.State(n)
        s.goal[:] = st[34:37].T
        s.set_state(st[0:3].T, st[3:6].T, st[6:15].T.reshape(n, 3, 3), st[15:18].T)
        s.since_last_svd[:] = st[38] * self.cfg.dt
        sn = None
        if mode != "no noise":
            sn = qo.SenseNoise(n, **self.prm)
            sn.gyro_bias[:] = st[39:42].T
        return s, sn, self.off + (1 if mode == "next env" else 0)

    def w(self, s, quat):
        return np.abs(self.qo._R2quat(s.rot)[:, 0]) if quat else None

    def observe(self, s, sn, off, key):
        z = sr.call_draws(self.seed, off, self.n, key, self.prm, self.flags)
        return self.qo.observe(s, self.cfg, np.zeros((self.n, 4)), sn, None if sn is None else z, self.p)

    def omega_dot_slack(self):
        """What the device's fast Box-Muller may add to omega_dot [n, 3], the one aux word that is a torque divided by an inertia of 1e-5 ..
        1e-2 kg m^2: every OU normal within EPS_NORMAL of libm's, the OU state (theta = 0.15) therefore within EPS_NORMAL sigma / 0.15,
        each thrust within thrust_max (2 - linearity) times that (the command's slope), each arm |prop_pos| long, the yaw term torque_max."""
        if not self.thrust_noise:
            return 0.0
        p = self.p
        dc = EPS_NORMAL * p.ou_sigma / 0.15
        dthrust = p.thrust_max * ((2.0 - p.linearity) * dc)[:, None]                     # [n, 4]
        dtq = np.stack([np.sum(dthrust * np.abs(p.prop_pos[:, :, 1]), axis=1), np.sum(dthrust * np.abs(p.prop_pos[:, :, 0]), axis=1),
                        np.sum(p.torque_max * ((2.0 - p.linearity) * dc)[:, None], axis=1)], axis=1)
        return dtq / p.inertia

    def step(self, s, sn, off, key, a):
        z = sr.step_draws(self.seed, off, self.n, key, self.prm, self.cfg.dt, self.flags)
        nz = sr.ou_normals(self.seed, self.off, self.n, key, self.cfg.sim_steps) if self.thrust_noise else None
        return self.qo.env_step(s, self.p, self.cfg, a.astype(np.float64), nz, sense=sn, sense_draws=None if sn is None else z)


def counters(env):
    from gym_art_amd import _lib
    ctr = _lib.GaqCounters()
    _lib.check(env._lib.gaq_get_counters(env._handle, C.byref(ctr), None, None))
    return int(ctr.step_index), int(ctr.reset_calls)


def obs_excess(obs, ref, w=None, record=False):
    """max over rows and words of |device - oracle| / (max(|oracle|, 1) x the word's conditioning): 1 everywhere but the quaternion words
    (columns 6:10, `w` given), where R2quat's division by 4 w turns an attitude difference d into d (1 / (4 w) + 1 / (8 w^2)).  `w` is
    the ORACLE's: the w of R2quat(true attitude), the number the division is by -- which IS the oracle row's w unless the configuration
    perturbs the quaternion (quat_norm_std / quat_unif_range != 0): there the row holds w after the perturbation, up to 0.02 away from the
    divisor (measured with the row's w on <520>, body-frame quaternion + attitude noise: 5.65e-6 at word 9, a row with a divisor of a few
    1e-3 and a perturbed w several times that).  No row is dropped; the rows the old mask dropped (factor > 55, w < 0.05) may be at most
    a tenth of the batch."""
    scale = np.maximum(np.abs(ref), 1.0)
    if w is not None:
        with np.errstate(divide="ignore"):
            f = np.maximum(1.0, 1.0 / (4.0 * w) + 1.0 / (8.0 * w * w))
        assert np.mean(f > QUAT_FACTOR_DROPPED) <= 0.10, float(np.mean(f > QUAT_FACTOR_DROPPED))
        scale = scale.copy()
        scale[:, 6:10] *= f[:, None]
    e = np.abs(obs - ref) / scale
    if record:
        WORST_AT.append((float(e.max()), int(np.argmax(e.max(axis=0)))))
    return float(e.max())


AUX_KEYS = ("acc", "omega_dot", "torque", "act_clipped", "act_filtered")


def fly_case(mask, kw, env_vars, n=N, stepper="step"):
    from gym_art_amd import QuadrotorEnv
    rng = np.random.RandomState(1000 + mask % 9973)
    with environ(**env_vars):
        # (per-episode re-randomisation inside the step launch exists with auto-reset only; no episode ends within the 40 steps either way)
        env = QuadrotorEnv(num_envs=n, env_id_offset=OFFSET, seed=SEED + mask % 101, ep_time=50, auto_reset=bool(mask & RZ), **kw)
    try:
        assert env.launch_variant == mask, "step_kernel<%d>: the recipe %r launched <%d>" % (mask, kw, env.launch_variant)
        quat = "quat" in env.obs_repr
        worst = dict(obs=0.0, rew=0.0, bias=0.0, aux=0.0)
        del WORST_AT[:]
        aux_by_key = {}
        teeth = {"next env": 0.0, "no noise": 0.0}
        # (1) a reset observation: one add_noise call on the state the reset left, keyed step index + (reset calls << 44)
        before = env.get_state()
        o_dev = env.reset()
        step_index, reset_calls = counters(env)
        after = env.get_state()
        orc = Oracle(env, kw)                              # (parameters read back AFTER the reset: what the flight below flies with)
        st = after.copy()
        st[39:42] = before[39:42]                          # the bias the call started from
        s, sn, off = orc.twin(st, "replay")
        worst["obs"] = max(worst["obs"], obs_excess(o_dev, orc.observe(s, sn, off, step_index + (reset_calls << 44)), orc.w(s, quat), True))
        if orc.walk:
            worst["bias"] = max(worst["bias"], float(np.max(np.abs(after[39:42].T - sn.gyro_bias))))
        # (2) observe() on random full-scale states: keyed by the step index alone
        st = random_state(n, rng, orc.walk, bool(kw.get("resample_goal")))
        env.set_state(st)
        o_dev = env.observe()
        flights = {}
        for mode in ("replay", "next env", "no noise"):
            s, sn, off = orc.twin(st, mode)
            e = obs_excess(o_dev, orc.observe(s, sn, off, step_index), orc.w(s, quat), mode == "replay")
            if mode == "replay":
                worst["obs"] = max(worst["obs"], e)
                bias1 = sn.gyro_bias.copy()
            else:
                teeth[mode] = max(teeth[mode], e)
        if orc.walk:
            worst["bias"] = max(worst["bias"], float(np.max(np.abs(env.get_state()[39:42].T - bias1))))
        # (3) the flight: three add_noise calls per step on the device's draws of (seed, global env index, step index)
        st1 = st.copy()
        st1[39:42] = bias1.T
        for mode in ("replay", "next env", "no noise"):
            flights[mode] = orc.twin(st1, mode)
        acts = rng.uniform(-1, 1, (STEPS, n, 4)).astype(np.float32)
        if stepper == "step":
            outs = (env.step(acts[t]) for t in range(STEPS))
        else:
            outs = iter(stepper(env, acts))
        for t in range(STEPS):
            o_dev, r_dev, d_dev, info = next(outs)
            a = acts[t] if stepper == "step" else info.pop("applied_action")
            for mode in ("replay", "next env", "no noise") if t < TEETH_STEPS else ("replay",):
                s, sn, off = flights[mode]
                o, r, d = orc.step(s, sn, off, step_index + t, a)
                e = obs_excess(np.asarray(o_dev), o, orc.w(s, quat), mode == "replay")
                if mode != "replay":
                    teeth[mode] = max(teeth[mode], e)
                    continue
                worst["obs"] = max(worst["obs"], e)
                worst["rew"] = max(worst["rew"], float(np.max(np.abs(np.asarray(r_dev) - r))))
                assert np.array_equal(np.asarray(d_dev).astype(bool), d), (mask, t)
                if info.get("obs_comp"):
                    oc = orc.qo.info_obs_comp(s, a)
                    for key in AUX_KEYS:
                        ref = oc[key]
                        allowed = AUX_TOL * np.maximum(np.abs(ref), 1.0) + (orc.omega_dot_slack() if key == "omega_dot" else 0.0)
                        e = AUX_TOL * float(np.max(np.abs(np.asarray(info["obs_comp"][key][0]).reshape(n, -1) - ref) / allowed))
                        aux_by_key[key] = max(aux_by_key.get(key, 0.0), e)
                    worst["aux"] = max(aux_by_key.values())
        if orc.walk:
            worst["bias"] = max(worst["bias"], float(np.max(np.abs(env.get_state()[39:42].T - flights["replay"][1].gyro_bias))))
            assert np.abs(flights["replay"][1].gyro_bias).max() > 0
        env.check_finite()
    finally:
        env.close()
    print("step_kernel<%d> %s n=%d %s: worst obs %.3g  reward %.3g  gyro bias %.3g  aux %.3g | teeth: next env %.3g  no noise %.3g"
          % (mask, stepper if isinstance(stepper, str) else stepper.__name__, n, env.obs_repr, worst["obs"], worst["rew"], worst["bias"],
             worst["aux"], teeth["next env"], teeth["no noise"]))
    print("    worst observation word of the replay comparisons: %r   aux by key: %r" % (max(WORST_AT)[1], aux_by_key))
    obs_tol = min(OBS_TOL_CAP, 2.0 * OBS_MEASURED_ABOVE_5E7[mask]) if mask in OBS_MEASURED_ABOVE_5E7 else OBS_TOL
    assert worst["obs"] <= obs_tol, (mask, kw, worst, obs_tol)
    assert worst["rew"] <= REW_TOL, (mask, kw, worst)
    assert worst["bias"] <= BIAS_TOL, (mask, kw, worst)
    assert worst["aux"] <= AUX_TOL, (mask, kw, worst)
    assert min(teeth.values()) > TEETH * OBS_TOL, (mask, kw, teeth)      # the noise term is alive and keyed by the env
    return worst


# every mask test_every_noise_capable_step_kernel_was_flown finds reachable with sensor noise on (it compares this list with gaq_plan's answer)
MASKS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 72, 73, 520, 521, 584, 1040, 1041, 1042, 1043, 1044, 1045, 1046, 1047, 2049, 2051, 2053, 2055, 2057, 2121,
         2569, 3089, 3091, 3093, 3095, 17424, 17425, 17426, 17427, 17428, 17429, 17430, 17431, 19473, 19475, 19477, 19479, 66576, 66577, 66578,
         66579, 66580, 66581, 66582, 66583, 68625, 68627, 68629, 68631, 82960, 82962, 82964, 82966, 197648, 197649, 197650, 197651, 197652,
         197653, 197654, 197655, 199697, 199699, 199701, 199703, 214032, 214034, 214036, 214038, 459792, 459794, 459796, 459798]


@pytest.mark.parametrize("mask", MASKS, ids=["k%d" % m for m in MASKS])
def test_noisy_step_kernel_against_the_oracle_on_the_device_draws(mask):
    kw, env_vars = recipe(mask, k=bin(mask).count("1") + (mask >> 1))
    fly_case(mask, kw, env_vars)
    FLOWN.add(mask)


# ---- the configurations the issue names, whatever mask they land on (asserted), and the shapes besides 2088 ------------------------------
NAMED = [
    ("default_hummingbird_18", dict(sense_noise="default"), 1044, N),
    ("default_hummingbird_h", dict(sense_noise="default", obs_repr="xyz_vxyz_R_omega_h"), 1044, N),
    ("default_crazyflie_h", dict(sense_noise="default", obs_repr="xyz_vxyz_R_omega_h", dynamics_params="Crazyflie"), 1046, N),
    ("bias_walk", dict(sense_noise=dict(WALK)), 459796, N),
    ("bias_walk_one_partial_tile", dict(sense_noise=dict(WALK), obs_repr="xyz_vxyz_R_omega_h"), 459796, 40),
    ("quaternion_info", dict(sense_noise="default", obs_repr="xyz_vxyz_quat_omega", info=True), 66580, N),
    ("t2w_t2t_info", dict(sense_noise="default", obs_repr="xyz_vxyz_R_omega_t2w_t2t", info=True), 66580, N),
    ("acc_act_info", dict(sense_noise="default", obs_repr="xyz_vxyz_R_omega_acc_act", info=True), 66580, N),
    ("mellinger_default", dict(sense_noise="default", raw_control=False), 17428, N),
    ("per_env_default", dict(sense_noise="default", dyn_sampler_1=dict(SAMPLER)), 1045, N),
    ("plain_layout_white_gyro", dict(sense_noise="default", alias_obs=False), 4, N),
]


@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_sensor_noise_configurations_against_the_oracle(case):
    label, kw, mask, n = case
    fly_case(mask, kw, {}, n=n)
    FLOWN.add(mask)


def _launched(kind):
    from gym_art_amd import _lib
    buf = (C.c_uint32 * 1024)()
    k = _lib.load().gaq_launched_variants(kind, buf, 1024)
    return {int(buf[i]) for i in range(k)}


def step_many(env, acts):
    """step_many_dev on a sensor-noise env: no fused rollout kernel holds the packed observation, so the T steps are T launches of the
    handle's step kernel (asserted: no rollout kernel is recorded by the call)."""
    import torch
    dev = torch.device("cuda", 0)
    T, n, D = acts.shape[0], env.num_envs, env.obs_dim
    o = torch.empty((T, n, D), device=dev); r = torch.empty((T, n), device=dev); d = torch.empty((T, n), dtype=torch.uint8, device=dev)
    rolled = _launched(1)
    env.step_many_dev(torch.tensor(acts, device=dev), o, r, d)
    torch.cuda.synchronize()
    assert _launched(1) == rolled and env.launch_variant in _launched(0)
    o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
    return [(o[t], r[t], d[t], {"applied_action": acts[t]}) for t in range(T)]


def rollout_policy(env, acts):
    """rollout_policy_dev: a device MLP closes the loop on the NOISY observation; the oracle flies the actions the policy applied
    (returned by the call), so the env kernel is what is compared.  Per-step path (asserted: no policy rollout kernel is recorded)."""
    import torch
    from gym_art_amd.policy import MLPPolicy
    from tests.policy_util import _net
    dev = torch.device("cuda", 0)
    T, n, D = acts.shape[0], env.num_envs, env.obs_dim
    pol = MLPPolicy.from_torch(_net([32, 32], D=D, seed=3), env, log_std=[-1.0, -1.0, -1.0, -1.0])
    o0 = torch.empty((n, D), device=dev)
    r0 = torch.empty(n, device=dev); d0 = torch.empty(n, dtype=torch.uint8, device=dev)
    o = torch.empty((T, n, D), device=dev); r = torch.empty((T, n), device=dev); d = torch.empty((T, n), dtype=torch.uint8, device=dev)
    a = torch.empty((T, n, 4), device=dev)
    rolled = _launched(2)
    env.step_dev(torch.tensor(acts[0], device=dev), o0, r0, d0)          # the current observation on the device: the policy's first input
    env.rollout_policy_dev(pol, o[1:], r[1:], d[1:], a[1:])
    torch.cuda.synchronize()
    assert _launched(2) == rolled and env.launch_variant in _launched(0)
    o[0], r[0], d[0], a[0] = o0, r0, d0, torch.tensor(acts[0], device=dev)
    o, r, d, a = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), a.cpu().numpy()
    assert np.abs(a[1:]).max() > 0.1 and np.abs(a[1:] - a[1]).max() > 0      # a policy that acts, and not the same action every step
    return [(o[t], r[t], d[t], {"applied_action": a[t]}) for t in range(T)]


@pytest.mark.parametrize("stepper", [step_many, rollout_policy], ids=["step_many_dev", "rollout_policy_dev"])
def test_fused_api_paths_of_a_sensor_noise_env_against_the_oracle(stepper):
    fly_case(1044, dict(sense_noise="default", obs_repr="xyz_vxyz_R_omega_h"), {}, stepper=stepper)


def test_every_noise_capable_step_kernel_was_flown():
    """Runs last in this file: the masks flown above against everything gaq_plan can return with sensor noise on -- a future noisy
    instantiation cannot arrive untested.  (Each mask is a test case of its own, so a deselected or failed case shows here too.)"""
    capable = noise_capable_masks()
    assert capable <= instantiated(), sorted(capable - instantiated())
    assert capable == set(MASKS), (sorted(capable - set(MASKS)), sorted(set(MASKS) - capable))
    assert FLOWN >= capable, "noise-capable step kernels not flown against the oracle: %r" % sorted(capable - FLOWN)
