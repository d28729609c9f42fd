"""The sensor-noise draws the DEVICE makes, rebuilt on the host and laid out the way oracle/quad_oracle.py takes them.

Test infrastructure only.  The device's draws are a pure function of (seed, global env index, key, stream): Philox streams
RNG_SENSE0 + 0 .. 9 (quad_core.hpp sense_noise / pack_obs) and RNG_OU0 + sub-step for the thrust noise (env_step).  The generator itself
-- Philox4x32-10 and the fp32 Box-Muller -- comes from the host build of the arithmetic header (tests/host_harness: hh_philox_n,
hh_normals_n, hh_normals10; pinned by tests/test_core_host.py and the KS tests).  What is restated HERE, in NumPy and from the reading
of sense_noise(), is which draw goes where: the map from the device's 24 normals and three uniform blocks to the slots of the
reference's call order (quad_core.hpp above `struct NoSense`; oracle SenseNoise):
  0 pos n, 1 pos u, 2 vel n, 3 vel u, 4 gyro n (bias model: the bias increment), 5 gyro white n (bias model), 6 quat n, 7 quat u,
  8 acc static n, 9 acc proportional n, 10 / 11 (first column) the t2w / t2t normals.
With these the fp64 oracle flies beside ANY kernel on the device's own draws, and the arithmetic of the noise -- scales, the
small-angle quaternion, the bias walk, the clip of t2w -- is the oracle's, not the header's.

`key` of an observation (pack_obs' `noise_key`): the handle's step index for the observation of a step and for gaq_observe, the step
index + (reset calls << 44) for the observation of a reset (gaq.hip launch_reset; both counters: gaq_get_counters)."""
import ctypes as C

import numpy as np

from tests import hh

RNG_OU0, RNG_SENSE0 = 0, 100             # quad_core.hpp enum RngStream
OBS_APPEND_ACC, OBS_APPEND_T2W, OBS_APPEND_T2T = 4, 32, 64
DEFAULTS = dict(pos_norm_std=0.005, pos_unif_range=0., vel_norm_std=0.01, vel_unif_range=0., quat_norm_std=0., quat_unif_range=0.,
                gyro_norm_std=0., gyro_noise_density=0.000175, gyro_random_walk=0.0105, gyro_bias_correlation_time=1000.,
                acc_static_noise_std=0.002, acc_dynamic_noise_ratio=0.005)      # SensorNoise.__init__ (sensor_noise.py:58-63)


def _call(name, out, seed, env0, key, stream, n):
    fn = getattr(hh.lib(), name)
    fn.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int64, C.c_void_p]
    fn.restype = None
    fn(int(seed) & (2 ** 64 - 1), int(env0), int(key) & (2 ** 64 - 1), int(stream), int(n), out.ctypes.data_as(C.c_void_p))
    return out


def philox(seed, env0, n, key, stream):
    """The four 32-bit words of Philox(seed, env0 + i, key, stream), i < n -> uint32 [n, 4]."""
    return _call("hh_philox_n", np.empty((n, 4), np.uint32), seed, env0, key, stream, n)


def normals4(seed, env0, n, key, stream):
    """The four Box-Muller normals of that block -> float64 [n, 4] (values of the fp32 draws)."""
    return _call("hh_normals_n", np.empty((n, 4), np.float32), seed, env0, key, stream, n).astype(np.float64)


def normals10(seed, env0, n, key, stream):
    """The ten normals out of the blocks `stream` and `stream + 1` -> float64 [n, 10]."""
    return _call("hh_normals10", np.empty((n, 10), np.float32), seed, env0, key, stream, n).astype(np.float64)


def uniform01(words):
    """uni_pm's 24 top bits, centred, as the U(0, 1) draw u of the oracle's `low + (high - low) u`: uni_pm = (2 u - 1) range."""
    return ((words >> np.uint32(8)).astype(np.float64) + 0.5) / 16777216.0


def bias_step_scale(prm, dt):
    """sqrt(1 + pi^2 + pi^4): three steps b <- pi b + sigma z of the bias walk are ONE step (pi^3, sigma sqrt(1 + pi^2 + pi^4)) in
    distribution; the device takes that one step per env step (gaq.hip fill_step_cfg: gyro_pi_step / gyro_sigma_step)."""
    pi = np.exp(-dt / float(prm["gyro_bias_correlation_time"]))
    return float(np.sqrt(1.0 + pi ** 2 + pi ** 4))


def call_draws(seed, env_id_offset, n, key, prm, obs_flags):
    """The standard draws of ONE add_noise call (+ the t2w / t2t normals of that observation) as the device makes them for the envs
    env_id_offset .. + n - 1 under `key` -> [n, 12, 3].  This is the form of a reset observation and of observe()."""
    prm = dict(DEFAULTS, **prm)
    z = np.zeros((n, 12, 3))
    z[:, [1, 3, 7]] = 0.5                                                # a range of zero: any u gives zero
    walk = prm["gyro_norm_std"] != 0.0
    t = normals10(seed, env_id_offset, n, key, RNG_SENSE0)               # blocks 0, 1: position, velocity, gyro white noise
    z[:, 0], z[:, 2] = t[:, 0:3], t[:, 3:6]
    z[:, 5 if walk else 4] = t[:, 6:9]
    if prm["quat_norm_std"] != 0.0:                                      # block 2: its first normal is overwritten by the ninth of the ten
        z[:, 6] = normals4(seed, env_id_offset, n, key, RNG_SENSE0 + 2)[:, 1:4]
    if (obs_flags & OBS_APPEND_ACC) or walk:                             # blocks 3 .. 5: twelve normals in a row, nine of them used
        w = np.concatenate([normals4(seed, env_id_offset, n, key, RNG_SENSE0 + j) for j in (3, 4, 5)], axis=1)
        z[:, 8], z[:, 9] = w[:, 0:3], w[:, 3:6]
        if walk:
            z[:, 4] = w[:, 6:9]
    for slot, name, stream in ((1, "pos_unif_range", 6), (3, "vel_unif_range", 7), (7, "quat_unif_range", 8)):
        if prm[name] != 0.0:
            z[:, slot] = uniform01(philox(seed, env_id_offset, n, key, RNG_SENSE0 + stream)[:, 0:3])
    if obs_flags & (OBS_APPEND_T2W | OBS_APPEND_T2T):
        w = normals4(seed, env_id_offset, n, key, RNG_SENSE0 + 9)
        z[:, 10, 0], z[:, 11, 0] = w[:, 0], w[:, 1]
    return z


def step_draws(seed, env_id_offset, n, key, prm, dt, obs_flags):
    """... and of the three add_noise calls of an env step (key = the step index) -> [3, n, 12, 3] for oracle env_step.  The device
    draws once per step: calls 0 and 1 (whose results the reference discards) get a zero bias increment -- they only decay the bias --
    and call 2 the step's increment scaled by bias_step_scale, which makes the oracle's three single steps the device's composite one."""
    z = np.zeros((3, n, 12, 3))
    z[2] = call_draws(seed, env_id_offset, n, key, prm, obs_flags)
    if dict(DEFAULTS, **prm)["gyro_norm_std"] != 0.0:
        z[2, :, 4] *= bias_step_scale(dict(DEFAULTS, **prm), dt)
    return z


def ou_normals(seed, env_id_offset, n, step_index, sim_steps):
    """The thrust-noise normals of one env step (RNG_OU0 + sub-step, key = the step index) -> [sim_steps, n, 4] for oracle env_step."""
    return np.stack([normals4(seed, env_id_offset, n, step_index, RNG_OU0 + k) for k in range(sim_steps)])
