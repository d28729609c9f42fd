"""CPU: tests/sense_replay.py rebuilds the draws of the DEVICE-DRAWN sensor-noise branch (quad_core.hpp sense_noise, cfg.sense_input == 0)
in the oracle's slot layout.  Proven here without a GPU: the kernel arithmetic compiled for the host (tests/host_harness, the generic
instantiation) draws its own noise from Philox, the pinned fp64 oracle flies beside it on the replayed draws.  tests/test_core_host.py
does the same with INJECTED draws on both sides (test_sensor_noise_random_parameter_sets_against_the_oracle); the bounds are that test's."""
import os

import numpy as np

from tests import golden_util as gu
from tests import hh
from tests import sense_replay as sr

OBS_TOL, BIAS_TOL = 3e-7, 2e-7        # tests/test_core_host.py:360, :362 (both sides use libm: nothing new enters)
REW_TOL = 3e-7                        # the absolute reward bound of the fixture tests (tests/test_gpu_round2.py)
TEETH = 100.0                         # wrong draws / no draws have to break the bound by this factor


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


def test_device_drawn_sensor_noise_on_the_host_against_the_oracle_on_replayed_draws():
    """Random SensorNoise parameter sets in the ranges of the injected-draw twin -- any subset of the Gaussian / uniform terms, both gyro
    models, correlation times 0.5 / 10 / 1000, the six working observation variants, three rates, thrust noise (Philox OU) on in half the
    cases -- three envs each at global indices that are non-zero and, in a third of the cases, above 2^32, from a non-zero step index.
    Teeth: the draws of env i + 1 given to env i, or the noise left out, miss the bound by more than 100 x wherever a noise term is alive."""
    from oracle import quad_oracle as qo
    rng = np.random.RandomState(int(os.environ.get("GAQ_FUZZ_SEED", "78")))
    const = dict(gu.sub(gu.load("g2_hummingbird_raw"), "const_"))
    T, n = 8, 3
    worst = dict(obs=0.0, rew=0.0, bias=0.0)
    bitten = 0
    for c in range(int(os.environ.get("GAQ_FUZZ_CONFIGS", "40"))):
        freq, steps = [(200.0, 2), (100.0, 4), (400.0, 1)][rng.randint(3)]
        dt = 1.0 / freq
        obs_repr = list(hh.OBS_FLAGS)[rng.randint(len(hh.OBS_FLAGS))]
        flags = hh.OBS_FLAGS[obs_repr]
        prm = {}
        for k, hi in (("pos_norm_std", 0.02), ("pos_unif_range", 0.02), ("vel_norm_std", 0.05), ("vel_unif_range", 0.05), ("quat_norm_std", 0.03),
                      ("quat_unif_range", 0.02), ("gyro_noise_density", 0.002), ("acc_static_noise_std", 0.01), ("acc_dynamic_noise_ratio", 0.02),
                      ("gyro_random_walk", 0.02)):
            prm[k] = float(rng.uniform(0, hi)) if rng.rand() < 0.6 else 0.0
        walk = bool(rng.randint(2))
        prm["gyro_norm_std"] = float(rng.uniform(0.001, 0.02)) if walk else 0.0
        prm["gyro_bias_correlation_time"] = float(rng.choice([0.5, 10.0, 1000.0]))
        thrust_noise = bool(c % 2)
        seed = int(rng.randint(1, 2 ** 31))
        off = [1, 4097, (1 << 32) + 5][c % 3] + int(rng.randint(0, 1000))
        step0 = int(rng.randint(1, 100000))
        model = hh.make_model(dict(const, thrust_noise_sigma=np.float64(0.01 if thrust_noise else 0.0)))
        cfg = hh.make_cfg(dt, steps, 500, model, obs_repr=obs_repr, noise=1 if thrust_noise else 0)
        cfg.sense_input, cfg.sense.enabled, cfg.seed, cfg.step_index = 0, 1, seed, step0
        for k, v in prm.items():
            setattr(cfg.sense, k, v)
        bias0 = rng.uniform(-0.01, 0.01, (n, 3)).astype(np.float32) if walk else np.zeros((n, 3), np.float32)
        if walk:
            sb, pi = qo.SenseNoise(1, **prm).gyro_constants(dt)
            cfg.gyro_bias, cfg.gyro_pi, cfg.gyro_sigma = 1, pi, sb
            cfg.gyro_pi_step, cfg.gyro_sigma_step = pi ** 3, sb * np.sqrt(1 + pi ** 2 + pi ** 4)
        pos = (rng.uniform(-2, 2, (n, 3)) + [0, 0, 2]).astype(np.float32).astype(np.float64)
        pos[:, 2] = np.maximum(pos[:, 2], 0.3)
        vel = rng.uniform(-1, 1, (n, 3)).astype(np.float32).astype(np.float64)
        q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
        q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
        q[np.linalg.det(q) < 0, :, 0] *= -1
        rot = q.astype(np.float32).astype(np.float64)
        om = rng.uniform(-3, 3, (n, 3)).astype(np.float32).astype(np.float64)
        acts = rng.uniform(-1, 1, (T, n, 4)).astype(np.float32)
        host = []
        for i in range(n):
            cfg.env_offset = off + i
            host.append(hh.rollout(cfg, model, hh.pack_state(pos[i], vel[i], rot[i], om[i], [0, 0, 2.0]), acts[:, i], variant=8,
                                   want_traj=False, gyro_bias=bias0[i].copy()))        # (rollout hands the final bias back in place)
        h_obs = np.stack([o["obs"] for o in host], axis=1)                      # [T, n, D]
        h_rew = np.stack([o["reward"] for o in host], axis=1)
        h_bias = np.stack([o["gyro_bias"] for o in host])
        p = qo.Params(n, mass=const["mass"], inertia=const["inertia"], thrust_max=const["thrust_max"], torque_max=const["torque_max"],
                      prop_pos=np.asarray(const["prop_pos"]).reshape(4, 3), damp_time_up=const["damp_time_up"], damp_time_down=const["damp_time_down"],
                      linearity=const["motor_linearity"], arm=const["arm"], ou_sigma=0.01 if thrust_noise else 0., vel_damp=const["vel_damp"],
                      damp_omega_quadratic=const["damp_omega_quadratic"], C_drag=0., C_roll=0.)
        ocfg = qo.Config(sim_freq=freq, sim_steps=steps, ep_time=500 * dt * steps + 1e-9, obs_repr=obs_repr)

        def fly(mode):
            sn = None if mode == "no noise" else qo.SenseNoise(n, **prm)
            if sn is not None:
                sn.gyro_bias[:] = bias0.astype(np.float64)
            s = qo.State(n)
            s.set_state(pos, vel, rot, om)
            e_obs, e_rew = 0.0, 0.0
            for t in range(T):
                z = sr.step_draws(seed, off + (1 if mode == "next env" else 0), n, step0 + t, prm, dt, flags)
                nz = sr.ou_normals(seed, off, n, step0 + t, steps) if thrust_noise else None
                o, rwd, dn = qo.env_step(s, p, ocfg, acts[t].astype(np.float64), nz, sense=sn, sense_draws=None if sn is None else z)
                e_obs = max(e_obs, _rel(h_obs[t], o))
                e_rew = max(e_rew, float(np.max(np.abs(h_rew[t] - rwd))))
                assert not dn.any()
            e_bias = float(np.max(np.abs(h_bias - sn.gyro_bias))) if (walk and sn is not None) else 0.0
            return e_obs, e_rew, e_bias

        e_obs, e_rew, e_bias = fly("replay")
        worst = dict(obs=max(worst["obs"], e_obs), rew=max(worst["rew"], e_rew), bias=max(worst["bias"], e_bias))
        assert e_obs <= OBS_TOL, (c, obs_repr, prm, thrust_noise, e_obs)
        assert e_rew <= REW_TOL, (c, e_rew)
        assert e_bias <= BIAS_TOL, (c, prm, e_bias)
        # a term of scale s moves an observation word by ~2.5 s at the largest of its T x n x 3 draws (uniform terms: by up to s): "alive"
        # = some term that reaches this observation variant has a scale of 1e-3 or more, 30 x above the 3e-5 the teeth ask for
        scales = [prm["pos_norm_std"], prm["pos_unif_range"], prm["vel_norm_std"], prm["vel_unif_range"], prm["quat_norm_std"], prm["quat_unif_range"],
                  prm["gyro_random_walk"] if walk else prm["gyro_noise_density"]]
        if flags & sr.OBS_APPEND_ACC:
            scales.append(prm["acc_static_noise_std"])
        if max(scales) >= 1e-3:
            for mode in ("next env", "no noise"):
                assert fly(mode)[0] > TEETH * OBS_TOL, (c, mode, prm)
            bitten += 1
    print("sense replay on the host: worst obs %.3g  reward %.3g  gyro bias %.3g  (%d cases with teeth)" % (worst["obs"], worst["rew"], worst["bias"], bitten))
    assert bitten >= 30 or int(os.environ.get("GAQ_FUZZ_CONFIGS", "40")) < 40


def test_slot_map_of_one_call():
    """The map itself on one call: the ninth normal of the first two blocks is the third gyro draw whether or not the attitude block
    is drawn (the device splices it back after normals4 overwrote it), the attitude normals are words 1 .. 3 of block 2, the bias increment
    starts at the third normal of block 4, uniforms are the centred top 24 bits, t2w / t2t are the first two normals of block 9."""
    seed, off, n, key = 12345, (1 << 33) + 7, 5, 99
    prm = dict(gyro_norm_std=0.01, quat_norm_std=0.02, pos_unif_range=0.01, vel_unif_range=0.0, quat_unif_range=0.003)
    z = sr.call_draws(seed, off, n, key, prm, sr.OBS_APPEND_T2W | sr.OBS_APPEND_T2T)
    t = sr.normals10(seed, off, n, key, 100)
    assert np.array_equal(z[:, 0], t[:, 0:3]) and np.array_equal(z[:, 2], t[:, 3:6]) and np.array_equal(z[:, 5], t[:, 6:9])
    assert np.array_equal(z[:, 6], sr.normals4(seed, off, n, key, 102)[:, 1:4])
    b4, b5 = sr.normals4(seed, off, n, key, 104), sr.normals4(seed, off, n, key, 105)
    assert np.array_equal(z[:, 4], np.concatenate([b4[:, 2:4], b5[:, 0:1]], axis=1))
    w = sr.philox(seed, off, n, key, 106)
    assert np.array_equal(z[:, 1], ((w[:, :3] >> 8) + 0.5) / 2.0 ** 24) and z[:, 1].min() > 0 and z[:, 1].max() < 1
    assert np.all(z[:, 3] == 0.5)                                    # a term that is off draws nothing
    assert np.any(z[:, 7] != 0.5)
    nine = sr.normals4(seed, off, n, key, 109)
    assert np.array_equal(z[:, 10, 0], nine[:, 0]) and np.array_equal(z[:, 11, 0], nine[:, 1])
    # white-noise gyro: slot 4 is the white noise, nothing in slot 5; other envs, keys and seeds give other draws
    z0 = sr.call_draws(seed, off, n, key, {}, 0)
    assert np.array_equal(z0[:, 4], t[:, 6:9]) and not z0[:, 5].any() and not z0[:, 6].any() and not z0[:, 8].any()
    assert np.array_equal(sr.call_draws(seed, off + 1, n - 1, key, {}, 0), z0[1:])
    assert not np.array_equal(sr.call_draws(seed, off, n, key + 1, {}, 0)[:, 0], z0[:, 0])
    assert not np.array_equal(sr.call_draws(seed + 1, off, n, key, {}, 0)[:, 0], z0[:, 0])
    # the composite bias step: calls 0 and 1 carry nothing, call 2 the increment times sqrt(1 + pi^2 + pi^4)
    s3 = sr.step_draws(seed, off, n, key, prm, 0.005, 0)
    assert not s3[:2].any()
    pi = np.exp(-0.005 / 1000.0)
    assert np.allclose(s3[2, :, 4], sr.call_draws(seed, off, n, key, prm, 0)[:, 4] * np.sqrt(1 + pi ** 2 + pi ** 4), rtol=1e-15)
