/* gaq.h -- C ABI of libgaq.so: the MI355X-native batched quadrotor simulator.
 *
 * Drop-in boundary for ONE path of amolchanov86/gym_art: what `QuadrotorEnv.step()` /
 * `reset()` do per call (gym_art/quadrotor/quadrotor.py:942-1028, :1059-1144), i.e.
 * controller -> QuadrotorDynamics.step (step1 x sim_steps, :261-436) -> crash test ->
 * compute_reward_weighted (:544-638) -> tick/done -> state_<obs_repr> (get_state.py),
 * for a batch of N independent environments held in device memory (struct of arrays).
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes.  No torch types.
 * The reference has no FFI of its own (it is pure Python); each entry point below names
 * the reference call it stands in for.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns 0 on success, a negative gaq_status on error; the message
 *     is available (thread-local) from gaq_last_error().
 *   - host-pointer variants (gaq_step, gaq_reset, ...) synchronise before returning;
 *     *_dev variants take device pointers and are asynchronous on `stream`, a hipStream_t passed
 *     as void* with HIP's own meaning of NULL (the legacy default stream, which is also what
 *     torch.cuda.current_stream().cuda_stream is unless the caller switched streams).  The
 *     host-pointer variants run on the handle's private stream, gaq_stream().
 *   - the caller owns every in/out buffer; the library owns the handle and its device
 *     state and allocates nothing per step.
 *   - a handle is not thread-safe; distinct handles are independent.
 *   - actions are [N,4] float32 row-major, 16-byte aligned; obs is [N,obs_dim] float32
 *     row-major; reward [N] float32; done [N] uint8.
 */
#ifndef GAQ_H
#define GAQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAQ_ABI_VERSION 5

typedef struct gaq_env gaq_env;

typedef enum gaq_status {
  GAQ_OK = 0,
  GAQ_ERR_INVALID = -1,   /* bad argument / unsupported configuration (reference: ValueError / assert) */
  GAQ_ERR_DEVICE = -2,    /* HIP runtime error, no device */
  GAQ_ERR_NAN = -3,       /* non-finite reward seen (reference: ValueError, quadrotor.py:633-636) */
  GAQ_ERR_STATE = -4      /* call sequence error */
} gaq_status;

/* RawControl zero-middle / RawControl [0,1] / Mellinger (quadrotor_control.py:72-92, :315-362) */
enum { GAQ_CTRL_RAW_ZERO_MIDDLE = 0, GAQ_CTRL_RAW = 1, GAQ_CTRL_MELLINGER = 2 };
/* thrust (OU) noise source: off / on-device Philox4x32-10 / caller-supplied normals */
enum { GAQ_NOISE_OFF = 0, GAQ_NOISE_PHILOX = 1, GAQ_NOISE_INPUT = 2 };
/* reward of quadrotor.py:544-638 / log-distance variant of quadrotor_multi.py:550-650 */
enum { GAQ_REW_QUADROTOR = 0, GAQ_REW_MULTI_LOG = 1 };
/* observation layout flags (get_state.py): base is [pos-goal, vel, R row-major, omega] = 18 */
enum { GAQ_OBS_BODY_FRAME = 1, GAQ_OBS_APPEND_H = 2, GAQ_OBS_APPEND_ACC = 4, GAQ_OBS_APPEND_ACT = 8,
       /* variants whose code is complete in the reference but raises NameError as shipped (get_state.py lacks the imports of
        * `normal` / `R2quat`); pinned by the patched-import fixture G15: the quaternion R2quat(rot) in place of the 9 words of R
        * (get_state.py:276-322; 13-word base block), the noisy normalised thrust-to-weight / torque-to-thrust ratio appended
        * (:325-384) */
       GAQ_OBS_QUAT = 16, GAQ_OBS_APPEND_T2W = 32, GAQ_OBS_APPEND_T2T = 64 };

/* Derived model constants: what QuadrotorDynamics.update_model computes (quadrotor.py:142-208). */
typedef struct gaq_model {
  double mass;
  double inertia[3];        /* diagonal of I_com (:152) */
  double thrust_max[4];     /* g*m*t2w*asym/4 (:175) */
  double torque_max[4];     /* t2t*thrust_max (:176) */
  double prop_pos[12];      /* [4][3], COM-corrected (:179) */
  double damp_time_up;      /* motor time constants, seconds (:159-160) */
  double damp_time_down;
  double linearity;         /* (:156) */
  double arm;               /* |motor_xy| (:200): crash height */
  double ou_sigma;          /* 0.2 * thrust_noise_ratio (:198) */
  double vel_damp;          /* (:163) */
  double damp_omega_quadratic; /* (:164) */
  double c_drag, c_roll;    /* (:157-158) */
} gaq_model;

#define GAQ_MODEL_NUM_DOUBLES 33  /* sizeof(gaq_model)/8: row length of gaq_set_params */

/* Reward weights (quadrotor.py:799-806; multi: quadrotor_multi.py:811-818). */
typedef struct gaq_rew_coeff {
  float pos, effort, crash, orient, yaw, rot, attitude, spin, action_change, vel;
  float pos_offset, pos_log_weight, pos_linear_weight;
} gaq_rew_coeff;

/* SensorNoise (sensor_noise.py:57-99); enabled = 0 is the reference's `sense_noise=None` (bypass).
 * gyro_norm_std == 0: white gyro noise of std gyro_noise_density (:130-131); != 0: the per-env gyro-bias random
 * walk of add_noise_to_omega (:160-168) with gyro_random_walk / gyro_bias_correlation_time. */
typedef struct gaq_sense_noise {
  int32_t enabled;
  float pos_norm_std, pos_unif_range, vel_norm_std, vel_unif_range, quat_norm_std, quat_unif_range;
  float gyro_noise_density, acc_static_noise_std, acc_dynamic_noise_ratio;
  float gyro_norm_std, gyro_random_walk, gyro_bias_correlation_time;
} gaq_sense_noise;

/* Swarm layer (BASELINE config 5: "8-agent swarm x 131072 worlds with neighbour-distance reward").  The reference
 * snapshot contains no multi-agent code (its quadrotor_multi fork is a single-agent env with a log-distance reward),
 * so this is the library's own specification -- parity-unpinned, see DESIGN.md "Swarm layer":
 *   world w = envs [w*agents, (w+1)*agents); agents is a power of two <= 16 and divides num_envs and env_id_offset;
 *   goal of agent a = (0,0,2) + goal_radius * (cos, sin, 0)(2 pi a / agents);
 *   reward_i -= dt * sum_{j != i} ( w_collision * [d_ij < collision_dist] + w_prox * max(0, 1 - d_ij / prox_dist) );
 *   optional collision response (gaq_swarm.response): colliding, approaching pairs exchange their normal relative velocity;
 *   observation = the configured self block + (pos_j - pos_i, vel_j - vel_i) for j = a+1 .. a+agents-1 (mod agents), as fp32
 *   differences of the fp32-rounded positions / velocities (exact to an ulp of the position, not of the difference). */
typedef struct gaq_swarm {
  int32_t agents;           /* 0 or 1: off */
  float goal_radius;
  float collision_dist;
  float prox_dist;
  float w_collision, w_prox;
  int32_t response;         /* 1: collision RESPONSE -- a pair closer than collision_dist that is still approaching exchanges the normal
                               component of its relative velocity (elastic collision of equal masses: v_i -= ((v_i - v_j) . n) n with
                               n = (p_i - p_j) / d_ij, summed over the colliding neighbours), applied to the integrated state before
                               reward and observation; 0: collisions are a reward term only (agents pass through each other) */
} gaq_swarm;

/* Everything QuadrotorEnv.__init__ fixes for the life of the env (quadrotor.py:653-827). */
typedef struct gaq_config {
  uint32_t struct_size;     /* = sizeof(gaq_config), ABI check */
  uint32_t abi_version;     /* = GAQ_ABI_VERSION */
  int64_t num_envs;         /* N envs held by this handle (this GPU's shard) */
  int64_t env_id_offset;    /* global index of env 0: RNG streams are keyed by global id, so results
                               do not depend on how a batch is sharded over GPUs */
  int32_t device;           /* HIP device ordinal */
  uint64_t seed;
  double sim_freq;          /* dt = 1/sim_freq (:790) */
  int32_t sim_steps;        /* step1 calls per env step (:261-262) */
  int32_t ep_len;           /* int(ep_time/(dt*sim_steps)) (:792); done = tick > ep_len (:987) */
  double room_size;         /* room box [[-s,-s,0],[s,s,s]] (:723) */
  double gravity;           /* used by the accelerometer only (:436) */
  double t2w_std, t2t_std;  /* relative noise of the t2w / t2t observation components (ctor arguments, :658; clip and scaling
                               ranges [1.5, 10] and [0.005, 1] are the reference's constants, :707-712) */
  int32_t control;          /* GAQ_CTRL_* */
  int32_t noise;            /* GAQ_NOISE_* */
  int32_t reward_mode;      /* GAQ_REW_* */
  int32_t obs_flags;        /* GAQ_OBS_* */
  int32_t auto_reset;       /* 1: an env that reports done is re-initialised inside the same launch and
                               its returned obs is the first of the new episode; 0: reference behaviour
                               (caller resets) */
  int32_t init_random_state;/* (:1100-1115) */
  int32_t resample_goal;    /* (:1078-1081) */
  int32_t per_env_params;   /* 1: model constants come from gaq_set_params, one row per env */
  int32_t compact_done;     /* 1: keep a per-step compacted list of done env indices */
  int32_t obs_state_alias;  /* How the 18 integrator words are stored (18-word world-frame observation with RawControl and the
                               default reward terms only -- see gaq_obs_is_state; otherwise 0 is used whatever is asked):
                               0: fp64 planes, the observation tensor is write-only (the caller owns it, like the reference).
                               1: split state whose fp32 head IS the caller's observation tensor (value = obs word + residual
                                  bits held by the library).  Least traffic (277 B/env-step).  CONTRACT: the buffer written by
                                  step k (or reset) is step k+1's INPUT -- it must still hold those bytes and stay allocated
                                  when step k+1 runs; the same buffer may be passed again (in place) or another one (rollout
                                  storage [T,N,D]).  Do not modify or free it in between.  GAQ_CHECK_ALIAS=1 in the environment
                                  makes every call verify a checksum of those rows and fail with GAQ_ERR_STATE if they changed.
                               2: the same split state with LIBRARY-owned heads; the caller's tensor receives a copy (+72 B/env-
                                  step of writes).  No contract: the caller may do anything with the observation.  This is what
                                  gym_art_amd.QuadrotorEnv uses unless told otherwise. */
  int32_t fp32_state;       /* 1: fp32 arithmetic and state -- the 18-word observation tensor IS the whole state (implies the
                               obs_state_alias contract).  Throughput-first: trajectories drift 1e-5..3e-4 (relative) from
                               the reference over 500 steps, i.e. OUTSIDE the 1e-5 parity bar that the default fp64 path
                               meets.  Refused (GAQ_ERR_INVALID) for configurations that need the generic kernel. */
  int32_t excite;           /* 1: a new goal ~ U(-0.5,0.5)^2 x U(1.5,2.5) whenever tick % 5 == 0 (:957-963) */
  int32_t aux_outputs;      /* 1: keep what the info dict's obs_comp needs beyond the state (quadrotor.py:994-1006): the last
                               sub-step's accelerometer, omega_dot and torque, the controller output and thrust_cmds_damp,
                               GAQ_AUX_WORDS floats per env, read with gaq_get_aux.  Runs the generic kernel. */
  int32_t action_f32;       /* RawControl arithmetic when the CALLER's action array is float32 (what action_space.sample() and most
                               policies produce): the reference then forms 0.5*(a+1) in float32 (quadrotor_control.py:88-92);
                               0 = the caller's array is float64 holding float32-representable values (sum exact).  The two differ
                               by <= 6e-8 in the command.  Can be switched per call with gaq_set_action_dtype. */
  int32_t sense_input;      /* 1: sensor-noise (and t2w / t2t observation) draws come from gaq_set_sense_input_dev (parity tests)
                               instead of the device RNG */
  gaq_swarm swarm;
  gaq_rew_coeff rew;
  gaq_sense_noise sense;    /* observation noise; forces the generic kernel and the plain state layout */
  gaq_model model;          /* used when per_env_params == 0 */
} gaq_config;

/* number of visible HIP devices (0 when none / no driver) */
int gaq_num_devices(void);
const char* gaq_last_error(void);
int gaq_abi_version(void);

/* 1 if this library is a MEASUREMENT build (-DGAQ_DIAG_BUILD): only such a build honours the timing-only ablations of GAQ_ABLATE
 * (which give wrong physics by construction); the product library refuses a non-zero GAQ_ABLATE at gaq_create. */
int gaq_is_diag_build(void);

/* Which kernel would gaq_create pick?  Pure host logic (no device needed): the configuration -> feature mask -> instantiation map
 * of the library, so that every reachable combination can be enumerated on a GPU-less host (tests/test_plan_cpu.py) -- a mask
 * without an instantiation is a test failure there, not a runtime GAQ_ERR_STATE.  `motor_lag` / `rotor_drag`: what the per-env
 * parameters (gaq_set_params / the randomizer) bring, -1 = derive from cfg->model (uniform model) or gaq_create's assumption before
 * parameters arrive; `randomize_every`: gaq_randomizer.every; `num_cus`: compute units of the device (the small-batch size rule counts
 * waves per SIMD; hipDeviceProp_t::multiProcessorCount, 256 on a whole MI355X).  No reference counterpart. */
typedef struct gaq_plan_info {
  int32_t obs_dim;
  int32_t state_layout;         /* as gaq_state_layout: 0 fp64 planes, 1 heads in the caller's tensor, 2 library-owned heads */
  int32_t fp32;                 /* fp32_state in effect */
  int32_t step_variant;         /* feature mask of the step kernel (csrc/quad_core.hpp: enum Feature) */
  int32_t step_instantiated;    /* 1 if the library holds that instantiation */
  int32_t launchable;           /* 1 if a step would launch (0 also for rotor drag arriving on a split-state handle: refused loudly) */
  int32_t rollout_variant;      /* mask of the fused kernel gaq_step_many_dev would launch, -1 = one launch per step */
  int32_t rollout_instantiated;
  int32_t lds_per_wave;         /* bytes of LDS per wave of the step launch */
  int32_t rows_variant;         /* the instantiation a step launches while packed rows are registered (gaq_set_packed_rows_dev: the rows are
                                   written by the step launch itself), -1 = the pack launch follows the step */
  int32_t ctr_variant;          /* the instantiation a step launches in graph-safe mode when it advances the step counter itself, -1 = a
                                   one-thread launch follows the step */
  /* graph-safe step counter of a handle of cfg->num_envs envs (gaq_set_graph_safe): the device words sum to step_index << ctr_shift; a
   * self-counting step launch has ctr_waves waves, every one adds 1 except the first, which adds ctr_inc0: 2^ctr_shift per launch */
  int32_t ctr_waves, ctr_shift, ctr_inc0;
} gaq_plan_info;
int gaq_plan(const gaq_config* cfg, int32_t motor_lag, int32_t rotor_drag, int32_t randomize_every, int32_t num_cus,
             gaq_plan_info* out);

/* QuadrotorEnv.__init__ (quadrotor.py:653-827): allocate device state for cfg->num_envs envs. */
int gaq_create(const gaq_config* cfg, gaq_env** out);
int gaq_destroy(gaq_env* env);
int gaq_obs_dim(const gaq_env* env);
/* 1 if this handle runs with obs_state_alias == 1 in effect (the caller's observation tensor is the state head) */
int gaq_obs_is_state(const gaq_env* env);
/* the obs_state_alias value in effect: 0 fp64 planes, 1 heads in the caller's tensor, 2 library-owned heads */
int gaq_state_layout(const gaq_env* env);
int64_t gaq_num_envs(const gaq_env* env);
/* feature mask of the step kernel this handle currently launches (gaq_plan_info.step_variant; changes when parameters arrive) */
int gaq_kernel_variant(const gaq_env* env);
/* ... and of the instantiation the NEXT gaq_step_dev launches: that kernel, or its twin that also writes the registered packed rows
 * (gaq_plan_info.rows_variant) / advances the graph-safe step counter itself (gaq_plan_info.ctr_variant) */
int gaq_launch_variant(const gaq_env* env);
/* test infrastructure: the distinct feature masks of the step (kind 0) / fused rollout (kind 1) instantiations THIS PROCESS has launched so
 * far, ascending; writes min(count, capacity) of them and returns the count (tools/kernel_coverage.py: which kernels a test run reached) */
int gaq_launched_variants(int kind, uint32_t* out, int capacity);

/* update_dynamics / resample_dynamics (quadrotor.py:852-894, :1030-1056) for per-env models:
 * `models` = `count` rows of gaq_model for envs [first, first+count).  Clears the SVD counter
 * and OU state of those envs like constructing a new QuadrotorDynamics does (:104, :198). */
int gaq_set_params(gaq_env* env, const gaq_model* models, int64_t first, int64_t count);
/* The same for a scattered set: models[k] goes to env env_idx[k] (per-episode re-randomisation of the envs that just
 * finished, dynamics_randomize_every, quadrotor.py:1063-1066) -- one call, one upload. */
int gaq_set_params_indexed(gaq_env* env, const gaq_model* models, const int64_t* env_idx, int64_t count);

/* ---- parameter pipeline on the device (SURVEY 8f.3 "or move it on device") -------------------------------------------
 * One quadrotor's parameter tree: the reference's nested dict (quad_models.py:1-176: geom / damp / noise / motor), flat,
 * in the dict's own order.  Shape of the shipped models (every link has a mass, the arms a length); RandomQuad's
 * density-based trees and dynamics_simplification stay on the host path (gaq_set_params). */
#define GAQ_TREE_DOUBLES 40
typedef struct gaq_quad_params {
  double body[4];        /* geom.body      l, w, h, m */
  double payload[4];     /* geom.payload   l, w, h, m */
  double arms[4];        /* geom.arms      l, w, h, m */
  double motors[3];      /* geom.motors    h, r, m */
  double propellers[3];  /* geom.propellers h, r, m */
  double motor_pos[3];   /* geom.motor_pos.xyz */
  double arms_pos[2];    /* geom.arms_pos  angle (deg), z */
  double payload_pos[3]; /* geom.payload_pos xy[2], z_sign */
  double damp[2];        /* damp.vel, damp.omega_quadratic */
  double noise[1];       /* noise.thrust_noise_ratio */
  double motor[11];      /* motor.thrust_to_weight, assymetry[4], torque_to_thrust, linearity, C_drag, C_roll, damp_time_up,
                            damp_time_down */
} gaq_quad_params;

/* RelativeSampler (quadrotor_randomization.py:345-358 -> perturb_dyn_parameters :70-104 -> check_quad_param_limits :16-46)
 * around `base`, per env, ON THE DEVICE, followed by QuadLink (inertia.py:182-310) and update_model (quadrotor.py:142-208).
 * every > 0: an env that reports done and whose finished-episode count k satisfies (k + 1) % every == 0 gets new
 * parameters INSIDE that step launch (dynamics_randomize_every, quadrotor.py:1063-1066), its SVD counter and OU state
 * cleared like a new QuadrotorDynamics (:104, :198): every env's next draw is derived ahead of time into a second set of
 * parameter planes (+360 B per env) and the step kernel only switches the env over.  Draws are Philox streams keyed by
 * (seed, global env index, resample count): the distribution of the reference's numpy draws, not its stream. */
typedef struct gaq_randomizer {
  int32_t sampler;                 /* 0: normal(loc = v, scale = |ratio/2 v|), 1: uniform(v - v ratio, v + v ratio);
                                      2: RandomQuad -- randomquad_parameters (quadrotor_randomization.py:142-243): a random
                                      quadrotor per draw; `ratio` and `base` are not used */
  int32_t every;                   /* dynamics_randomize_every (needs auto_reset = 1); 0 = only when gaq_randomize_dev is called */
  double ratio[GAQ_TREE_DOUBLES];  /* noise ratio per leaf (RelativeSampler noise_ratio / noise_ratio_custom), gaq_quad_params order */
  gaq_quad_params base;            /* the nominal model, dynamics_change already applied; C_drag = C_roll = 0 */
} gaq_randomizer;

/* Install the sampler on a per_env_params handle (RawControl, or Mellinger: the per-env inverse jacobians, quadrotor_control.py:290-291, are
 * rebuilt on the device whenever parameter planes change).  From here on the handle's parameters live on the device:
 * gaq_set_params is refused, gaq_get_params / gaq_get_param_trees read them back. */
int gaq_set_randomizer(gaq_env* env, const gaq_randomizer* rz);
/* resample_dynamics() now for the envs whose mask byte is non-zero (NULL = all): one launch, asynchronous on `stream`. */
int gaq_randomize_dev(gaq_env* env, const uint8_t* mask_dev_or_null, void* stream);
/* Caller-chosen trees for envs [first, first+count), derived on the device (QuadLink + update_model; the limits are NOT
 * applied): the device-side counterpart of gaq_set_params.  links_by_density != 0: RandomQuad's form of the tree -- the five `m`
 * leaves hold densities (mass = density x volume, inertia.py:96-97, :155-156) and arms.l is derived (:223-224). */
int gaq_set_param_trees(gaq_env* env, const gaq_quad_params* trees, int32_t links_by_density, int64_t first, int64_t count);
/* Read back: the derived constants (what update_model computed) / the sampled trees of envs [first, first+count). */
int gaq_get_params(gaq_env* env, gaq_model* models_out, int64_t first, int64_t count);
int gaq_get_param_trees(gaq_env* env, gaq_quad_params* trees_out, int64_t first, int64_t count);

/* ---- checkpoint / resume ----------------------------------------------------------------------------------------------
 * What a bit-exact continuation needs besides the state planes (gaq_get_state / gaq_set_state) and the parameters: the counters
 * behind the RNG keys (steps launched, reset calls) and, per env, the finished-episode and resample counts of the device
 * randomizer (NULL where not wanted / not a per_env_params handle).  gaq_set_counters on a handle with a randomizer installed
 * rebuilds every env's parameters from its resample count: they are a function of (seed, global env index, count).
 * No reference counterpart: the reference pickles its constructor arguments only (quadrotor.py:688). */
typedef struct gaq_counters {
  uint64_t step_index;    /* step launches so far: third word of the Philox keys of thrust noise and in-kernel resets */
  uint64_t reset_calls;   /* gaq_reset / gaq_reset_dev calls so far: keys the reset draws apart from the steps */
} gaq_counters;
int gaq_get_counters(gaq_env* env, gaq_counters* out, uint32_t* episodes_out_or_null, uint32_t* resamples_out_or_null);
int gaq_set_counters(gaq_env* env, const gaq_counters* in, const uint32_t* episodes_or_null, const uint32_t* resamples_or_null);

/* QuadrotorEnv.reset (quadrotor.py:1149 -> :1059-1144) for the envs whose mask byte is non-zero
 * (NULL = all).  Writes the [N,obs_dim] observation (rows of un-reset envs = current obs).  A masked reset leaves every bit of the
 * unmasked envs alone: with the gyro-bias random walk on, their rows are a peek (one add_noise call of sensor_noise.py:166 applied to the
 * row, not kept), whereas gaq_observe -- the reference's state_vector() -- advances the walk of every env like the reference does. */
int gaq_reset(gaq_env* env, const uint8_t* mask_or_null, float* obs_out);
int gaq_reset_dev(gaq_env* env, const uint8_t* mask_dev_or_null, float* obs_dev, void* stream);

/* QuadrotorEnv.step (quadrotor.py:1155 -> :942-1028). */
int gaq_step(gaq_env* env, const float* actions, float* obs, float* reward, uint8_t* done);
/* NB obs_state_alias == 1: obs_dev is ALSO the state head that the next gaq_step_dev / gaq_step_many_dev / gaq_reset_dev
 * reads -- keep it allocated and unmodified until then (see gaq_config.obs_state_alias). */
int gaq_step_dev(gaq_env* env, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                 void* stream);

/* T consecutive env steps with actions [T,N,4] and outputs [T,N,obs_dim], [T,N], [T,N]
 * resident on the device (the rollout loops of quadrotor.py:1278-1305, :1424-1428). */
int gaq_step_many_dev(gaq_env* env, int32_t T, const float* actions_dev, float* obs_dev, float* reward_dev,
                      uint8_t* done_dev, void* stream);

/* ---- device MLP policy: closed-loop rollouts --------------------------------------------------------------------------------
 * A deterministic MLP obs (in_dim = the env's obs_dim) -> [Linear -> act] x n_hidden -> Linear -> 4 (-> tanh), fp32, evaluated on the
 * device inside the rollout.  n_hidden in 1..3, every width a multiple of 16 in [16, 128], hidden_act GAQ_POLICY_TANH / _RELU (every
 * hidden layer), out_tanh 0/1.  Observation normalisation is folded into the first layer by the caller, or (not the VALU engine) is a
 * gaq_obs_norm attached with gaq_policy_set_obs_norm.
 * Packed weight layout (fp32, contiguous), for each hidden layer l with I inputs and O = width[l] outputs:
 *     W'[O/16][I][16] with W'[c][k][j] = W[16c + j][k]   (torch Linear.weight is W[O][I]),   then bias[O];
 * then the output layer (I = width[n_hidden-1]):  W'[I][4] with W'[k][o] = W[o][k],   then bias[4].
 * gaq_policy_weight_count gives the number of floats. */
typedef struct gaq_policy gaq_policy;
enum { GAQ_POLICY_TANH = 0, GAQ_POLICY_RELU = 1 };
typedef struct {
  uint32_t struct_size;       /* sizeof(gaq_policy_desc) */
  int32_t in_dim, n_hidden, width[3], hidden_act, out_tanh;
} gaq_policy_desc;
/* validates the description against the env (obs_dim; RawControl only: the Mellinger controller is refused) */
int gaq_policy_create(gaq_env* env, const gaq_policy_desc* desc, gaq_policy** out);
int64_t gaq_policy_weight_count(const gaq_policy_desc* desc);      /* floats of the packed layout, or GAQ_ERR_INVALID */
/* Policy engines.  GAQ_POLICY_ENGINE_VALU is what gaq_policy_create builds: per-lane VALU FMAs, widths up to 128 (above).
 * GAQ_POLICY_ENGINE_MFMA evaluates the hidden layers on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, 4 waves per 64-env tile, the
 * activations in LDS) and accepts 1-3 hidden layers of widths that are multiples of 16 in [16, 256].  Both use the packed layout above
 * and the same weight count, and on every net both accept they give the same bits: each unit is bias + its inputs in ascending order as
 * one fmaf chain, the 4 outputs sum the last hidden layer's units in ascending order.  An MFMA policy always runs as one policy launch +
 * one step launch per step (every layout; the fused closed-loop launch is VALU only).  MFMA is the faster engine on every net measured,
 * 64-64 included; VALU stays what gaq_policy_create builds, so that existing callers keep their paths. */
enum { GAQ_POLICY_ENGINE_VALU = 0, GAQ_POLICY_ENGINE_MFMA = 1, GAQ_POLICY_ENGINE_MFMA_BF16 = 3 };
/* (2 is not an engine: the MFMA engine's release refused it as unknown, and callers may rely on that; it stays GAQ_ERR_INVALID) */
/* GAQ_POLICY_ENGINE_MFMA_BF16 evaluates the same MLP family (1-3 hidden layers, widths multiples of 16 in [16, 256], tanh or relu) on the
 * bf16 matrix cores (v_mfma_f32_16x16x32_bf16), with this numerical contract:
 *   weights      the caller passes the fp32 packed layout above (same weight count, same set_weights calls); the library rounds every
 *                hidden- and output-layer weight to bf16 (round to nearest even) when the weights are set and repacks them for the
 *                kernel.  Biases stay fp32.  A net whose weights are already bf16 values (a bf16 torch module widened by .float())
 *                loses nothing.
 *   activations  the input of every layer (the observation, each hidden activation) is rounded once to bf16 (RNE); the activation
 *                function runs in fp32 and only its result is rounded.
 *   accumulation each unit starts at its fp32 bias and accumulates bf16 x bf16 products in fp32; the 4 outputs likewise.  The order of
 *                the fp32 sums is the matrix core's, not a k-ordered chain: results are deterministic but need not match the other
 *                engines bit for bit.
 *   outputs      the output tanh and the exploration term are the other engines' (same Philox keys: seed, global env id, step).
 * K is padded to the MFMA's 32 with +0 weights against -0 inputs, which cannot change any sum.  The engine never joins the fused
 * closed-loop launch: one policy launch + one step launch per step, in every layout. */
typedef struct {
  uint32_t struct_size;       /* sizeof(gaq_policy_desc_ex) */
  int32_t in_dim, n_hidden, width[3], hidden_act, out_tanh;
  int32_t engine;             /* GAQ_POLICY_ENGINE_* */
} gaq_policy_desc_ex;
/* as gaq_policy_create / gaq_policy_weight_count, for the engine named in the description (GAQ_ERR_INVALID for an unknown engine,
 * a wrong struct_size or widths that engine does not take) */
int gaq_policy_create_ex(gaq_env* env, const gaq_policy_desc_ex* desc, gaq_policy** out);
int64_t gaq_policy_weight_count_ex(const gaq_policy_desc_ex* desc);
int gaq_policy_engine(const gaq_policy* p);                        /* GAQ_POLICY_ENGINE_* the policy was built with */
/* copy the packed weights (device pointer on the env's device / host pointer) into the policy; synchronous */
int gaq_policy_set_weights_dev(gaq_policy* p, const float* packed_dev);
int gaq_policy_set_weights(gaq_policy* p, const float* packed_host);
/* Gaussian exploration a = mean + exp(log_std[k]) * z_k, z from Philox keyed by (seed, global env id, step index, stream 130):
 * independent of sharding and of how a rollout is split into calls.  NULL = deterministic. */
int gaq_policy_set_explore(gaq_policy* p, const float* log_std4_or_null);
/* ---- log_std on the device: the exploration table -------------------------------------------------------------------------------
 * Additive (GAQ_ABI_VERSION stays 5).  An exploring policy has two modes.
 * HOST mode (the default, everything above and below as it was): log_std lives in the handle on the host, every rollout, log-prob and
 * gradient launch takes it, exp(log_std) and exp(-log_std) by value in its kernel arguments when it is enqueued, and a CAPTURED launch
 * keeps those.
 * DEVICE mode: the policy reads a TABLE of 12 fp32 words in device memory, log_std[4] | std[4] | inv_std[4] (std = exp(log_std),
 * inv_std = exp(-log_std)).  The table is a caller-owned buffer, 16-byte aligned, on the policy's device, registered under the contract
 * of gaq_policy_set_hidden_dev: its address is fixed while it is registered, NULL unregisters it, the library never frees it.  No
 * launch of a device-mode policy carries a value of log_std: each passes the table's address, and the kernels -- the rollout kernels'
 * draw and log-probabilities, the row stages of gaq_policy_logp_dev, gaq_policy_eval_ac_dev, the gaq_policy_grad_ppo* calls and the
 * sequence calls -- load the words they use, wave-uniformly, where they use them.  Whatever wrote the table in an earlier launch or
 * copy on the stream (an optimiser's step, a copy of the caller's) is what the next launch sees, eagerly and in a replayed graph: A
 * CAPTURED LAUNCH OF A DEVICE-MODE POLICY FOLLOWS THE TABLE.  A writer of the table keeps its three parts consistent.
 * gaq_policy_set_explore_dev(p, table, stream): fp32 MFMA, GRU and LSTM policies; GAQ_ERR_INVALID (the text names the engine) for the
 * VALU and bf16 engines, for a misaligned table and for one that is not device memory on the policy's device; GAQ_ERR_STATE for a
 * deterministic policy.  It copies the handle's current log_std, std and inv_std -- the host-computed (float)exp((double)x) and
 * (float)exp(-(double)x), not recomputed ones -- into the table on `stream`, waits for it, and the handle is in device mode: every
 * kernel sees the bits it saw in host mode.  table = NULL leaves device mode: it waits for the device, reads log_std[4] back and takes
 * the path of gaq_policy_set_explore with those values (GAQ_OK and nothing done in host mode).
 * gaq_policy_set_explore(p, log_std) in device mode computes the 12 words on the host as ever and copies them into the table
 * (synchronous: after everything enqueued on the device); NULL makes the policy deterministic as ever (the table stays registered,
 * and values set later go to it).
 * gaq_policy_get_log_std: the current values in either mode; in device mode it waits for the device and reads the table.
 * GAQ_ERR_STATE for a deterministic policy.
 * gaq_policy_explore_mode: GAQ_EXPLORE_NONE for a deterministic policy (with or without a table registered), else _HOST or _DEVICE. */
#define GAQ_EXPLORE_NONE 0
#define GAQ_EXPLORE_HOST 1
#define GAQ_EXPLORE_DEVICE 2
int gaq_policy_set_explore_dev(gaq_policy* p, float* table12_dev_or_null, void* stream);
int gaq_policy_get_log_std(const gaq_policy* p, float* log_std4_host);
int gaq_policy_explore_mode(const gaq_policy* p);
int gaq_policy_destroy(gaq_policy* p);
/* T closed-loop steps: the action of step t is the policy on the observation of step t - 1 (t = 0: the current observation -- what the
 * last reset / step wrote), plus exploration.  Outputs as gaq_step_many_dev: obs [T,N,obs_dim], reward [T,N], done [T,N];
 * actions_out [T,N,4] (or NULL) records the applied actions (before the env clips them).  Counters, auto-resets and random streams
 * advance exactly as in T gaq_step_dev calls fed those actions.  Fused into one launch for the layouts gaq_step_many_dev fuses
 * (unless GAQ_NO_FUSED=1); otherwise one policy launch + one step launch per step.  In the layouts whose observation is not the state
 * head (obs_state_alias off, packed observations) the current observation is the device buffer the last gaq_step_dev / gaq_reset_dev /
 * gaq_step_many_dev / gaq_step_policy_many_dev wrote: keep it alive until this call (GAQ_ERR_STATE if there is none). */
int gaq_step_policy_many_dev(gaq_env* env, gaq_policy* p, int32_t T, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                             float* actions_out_dev_or_null, void* stream);

/* ---- recurrent device policies: a GRU cell in front of the MLP head ---------------------------------------------------------
 * gaq_policy_desc_rnn with cell = GAQ_POLICY_CELL_GRU: hidden layer 0 is a GRU cell of H = width[0] units (torch nn.GRUCell:
 *     r = sigmoid(W_ir x + b_ir + W_hr h + b_hr),  z = sigmoid(W_iz x + b_iz + W_hz h + b_hz),
 *     n = tanh(W_in x + b_in + r (W_hn h + b_hn)),  h' = (1 - z) n + z h   (computed as n + z (h - n))),
 * layers 1 .. n_hidden-1 (if any) are ordinary Linear -> hidden_act layers on h', then the 4-output layer (optional output tanh).
 * engine must be GAQ_POLICY_ENGINE_MFMA (fp32): the cell runs on v_mfma_f32_16x16x4_f32 (policy_gru_kernel), each sum an ascending fmaf
 * chain, r and z starting at b_i + b_h; sigmoid and tanh are the accurate expf / tanhf.  Any other engine, an unknown cell (NONE
 * included: gaq_policy_desc_ex builds feed-forward nets), a wrong struct_size, or widths outside the multiples of 16 in [16, 256] give
 * GAQ_ERR_INVALID.  Packed weights (fp32, I = in_dim; gaq_policy_set_weights[_dev] as above):
 *     W_ih' [3H/16][I][16] (W_ih' [c][k][j] = W_ih[16c + j][k], torch GRUCell.weight_ih [3H][I], gate rows r, z, n), then b_ih [3H];
 *     W_hh' [3H/16][H][16] likewise from weight_hh [3H][H], then b_hh [3H];
 *     then the head layers and the output layer exactly as for the MLP, with H as the first head input.
 * gaq_policy_weight_count_rnn = 3H (I + H) + 6H + the head's count.  gaq_policy_engine() of a GRU policy is GAQ_POLICY_ENGINE_MFMA and
 * gaq_policy_cell() GAQ_POLICY_CELL_GRU (GAQ_POLICY_CELL_NONE for every feed-forward policy). */
enum { GAQ_POLICY_CELL_NONE = 0, GAQ_POLICY_CELL_GRU = 1, GAQ_POLICY_CELL_LSTM = 3 };
/* (2 is not a cell: the GRU engine's release refused it as unknown, and callers may rely on that; it stays GAQ_ERR_INVALID) */
/* cell = GAQ_POLICY_CELL_LSTM: hidden layer 0 is an LSTM cell of H = width[0] units (torch nn.LSTMCell, gate rows i, f, g, o):
 *     i = sigmoid(W_ii x + b_ii + W_hi h + b_hi),  f = sigmoid(W_if x + b_if + W_hf h + b_hf),
 *     g = tanh(W_ig x + b_ig + W_hg h + b_hg),     o = sigmoid(W_io x + b_io + W_ho h + b_ho),
 *     c' = f c + i g  (computed as fmaf(f, c, i * g)),   h' = o tanh(c'),
 * followed by the head a GRU policy has (layers 1 .. n_hidden-1 on h', the 4-output layer, optional output tanh, the same exploration
 * draws).  Same engine rule (GAQ_POLICY_ENGINE_MFMA, fp32, v_mfma_f32_16x16x4_f32: policy_lstm_kernel), same widths.  Each of the four
 * gate sums starts at b_i + b_h (one fp32 add) and takes the x products, then the h products, each as an ascending fmaf chain; sigmoid
 * and tanh are those of the GRU cell (1 / (1 + expf(-v)), tanhf).  Deterministic; no bit promise against torch.  Packed weights:
 *     W_ih' [4H/16][I][16] (from torch LSTMCell.weight_ih [4H][I] as for the GRU), then b_ih [4H];
 *     W_hh' [4H/16][H][16] from weight_hh [4H][H], then b_hh [4H];   then the head as for the GRU.
 * gaq_policy_weight_count_rnn = 4H (I + H) + 8H + the head's count; gaq_policy_cell() is GAQ_POLICY_CELL_LSTM.
 * State: TWO caller-owned [N, H] fp32 buffers, h (gaq_policy_set_hidden_dev) and c (gaq_policy_set_cell_dev), both under the contract
 * stated for the GRU's h below: for t = 0 .. T-1  (h, c) <- LSTM(obs_{t-1}, h, c); act on h'; step the env; rows that reported done[t]
 * start launch t + 1 from h = c = 0 (applied inside that launch), and one masked zero of both buffers follows done[T-1].  After any call
 * the buffers hold exactly the state the next action uses, splitting a rollout into calls changes no bit, and a checkpoint is the env's
 * state plus copies of both.  The value head, gaq_step_policy_ac_many_dev, ..._ac_term_many_dev and ..._critic_many_dev work for an LSTM
 * policy exactly as for a GRU one (the bootstrap launch writes neither h' nor c'; terminal values use the h and c rows the episode
 * ended on, unmasked; a separate critic sees the observation only).
 * These are additive: GAQ_ABI_VERSION guards gaq_config and the existing signatures, none of which changes, so it stays as it is (as
 * it did for every entry point added since the sharded handle). */
typedef struct {
  uint32_t struct_size;       /* sizeof(gaq_policy_desc_rnn) */
  int32_t in_dim, n_hidden, width[3], hidden_act, out_tanh;
  int32_t engine;             /* GAQ_POLICY_ENGINE_MFMA */
  int32_t cell;               /* GAQ_POLICY_CELL_GRU or GAQ_POLICY_CELL_LSTM */
} gaq_policy_desc_rnn;
int gaq_policy_create_rnn(gaq_env* env, const gaq_policy_desc_rnn* desc, gaq_policy** out);
int64_t gaq_policy_weight_count_rnn(const gaq_policy_desc_rnn* desc);
int gaq_policy_cell(const gaq_policy* p);
/* The hidden state is the caller's: a [N, H] fp32 row-major device buffer, 16-byte aligned, registered here (NULL unregisters); its
 * contents are the state.  GAQ_ERR_INVALID for a feed-forward policy or a misaligned buffer.  A rollout with a GRU policy and no
 * registered buffer is GAQ_ERR_STATE and launches nothing. */
int gaq_policy_set_hidden_dev(gaq_policy* p, float* hidden_dev);
/* the same for an LSTM policy's second state c ([N, H] fp32, 16-byte aligned; NULL unregisters).  GAQ_ERR_INVALID on a policy that is
 * not an LSTM (GRU and feed-forward policies have no cell state) or for a misaligned buffer.  A rollout with an LSTM policy and either
 * buffer unregistered is GAQ_ERR_STATE and launches nothing. */
int gaq_policy_set_cell_dev(gaq_policy* p, float* cell_dev);
/* zero the rows of the registered state (an LSTM's h and c: both must be registered) whose mask byte is non-zero (every row for NULL),
 * enqueued on `stream` */
int gaq_policy_reset_hidden_dev(gaq_policy* p, const uint8_t* mask_dev_or_null, void* stream);
/* gaq_step_policy_many_dev with a GRU policy, h the registered state and m the head (head layers, output layer, output tanh,
 * exploration -- the same draws as the MLP engines): for t = 0 .. T-1
 *     h <- GRU(obs_{t-1}, h);  a_t = m(h) + exploration;  step the env with a_t;  then h <- 0 in the rows that reported done[t]
 * (obs_{-1} = the current observation, as for an MLP).  So after every call the buffer holds exactly the state the next action will
 * use: splitting a rollout into calls changes nothing, and a checkpoint is the env's state plus a copy of the buffer.  One policy launch
 * + one step launch per step in every layout (the done mask of step t-1 is applied inside the GRU launch of step t), then one masked-
 * zero launch for done[T-1]; no host synchronisation (graph-capturable).  gaq_step_dev / gaq_reset_dev and the other entry points never
 * touch h: the caller resets the rows of envs it resets itself (gaq_policy_reset_hidden_dev). */

/* ---- recurrent device policies: an MLP encoder in front of the cell ----------------------------------------------------------
 * obs -> [Linear -> hidden_act] x enc_layers -> GRU / LSTM cell -> head: the recurrent actor-critic of sample-factory and rl_games.
 * gaq_policy_desc_rnn_enc is gaq_policy_desc_rnn followed by the encoder: enc_in_dim inputs (the env's obs_dim; any value, a partial
 * k-step such as 19 included), enc_layers = 1 or 2 layers of widths enc_width[] (multiples of 16 in [16, 256]) whose activation is
 * hidden_act.  The cell's in_dim is the encoder's last width E: the cell takes the features where it took the observation, and
 * everything behind it -- head layers, the 4-output layer, out_tanh, the exploration draws, the value head -- is gaq_policy_desc_rnn's.
 * Arithmetic: every encoder layer is the fp32 MFMA engine's hidden layer (each accumulator starts at the bias, the k-steps ascend,
 * each an fmaf chain, then tanhf / max(., 0)), so the features are bit for bit the hidden activations a GAQ_POLICY_ENGINE_MFMA policy
 * computes from the same weights.  Deterministic; no bit promise against torch.  An attached normaliser (gaq_policy_set_obs_norm) is
 * applied where the ENCODER stages the observation; the cell sees the features as they are.
 * Launches: policy_encode_kernel (one workgroup of 4 waves per 64-env tile) writes the features [N, E] fp32 to a buffer the handle owns,
 * then the cell's kernel of the form reads them: one more launch per step, and 8 E bytes per env and step written and read again.  The
 * bootstrap launch of the actor-critic forms is preceded by one too.  Terminal values (gaq_step_policy_ac_term_many_dev): a gathered
 * form of the encoder's kernel runs on the terminal observations of the envs that finished and writes THEIR rows of the same buffer --
 * the step's features have been consumed by then and the next step's launch rewrites every row -- so terminal values add no second
 * buffer and cost one launch that works on about N / episode-length rows.  A separate critic (gaq_step_policy_critic_many_dev) sees the
 * raw observation, as ever, and its terminal pass needs no encoder launch.
 * The feature buffer is N * E * 4 bytes, allocated at create (a captured graph keeps valid pointers) and freed at destroy: 1 GiB at
 * N = 2^20, E = 256; GAQ_ERR_DEVICE if it cannot be had.
 * State contract: gaq_policy_desc_rnn's, word for word -- the hidden buffers hold the next action's state after any call, splitting a
 * rollout into calls changes no bit, the calls are capturable in a graph, nothing synchronises with the host.
 * Weights: the cell and the head keep their packed layout (gaq_policy_weight_count_rnn of the same fields with in_dim = E;
 * gaq_policy_set_weights[_dev], gaq_policy_get_weights).  The encoder's weights are a block of their own in the MLP's hidden-layer
 * layout: per layer W' [W/16][in][16] (W'[c][k][j] = W[16c + j][k]) then bias [W]; gaq_policy_encoder_weight_count floats;
 * gaq_policy_set_encoder_weights (host pointer) / _dev (device pointer), synchronous like gaq_policy_set_weights;
 * gaq_policy_get_encoder_weights reads them back.  A rollout before they were set is GAQ_ERR_INVALID "encoder weights not set" and
 * launches nothing.  gaq_policy_encoder_width is E, and 0 for every policy without an encoder; the three weight calls are
 * GAQ_ERR_INVALID on such a policy.
 * GAQ_ERR_INVALID, with the word "encoder" in the text: a wrong struct_size, enc_layers outside 1..2, a width outside the family,
 * enc_in_dim != the env's obs_dim, in_dim != the encoder's last width, rows that pass the CU's LDS.  gaq_policy_desc_rnn's refusals
 * (engine, cell, H and head widths) are checked after the encoder's fields, with their own texts.
 * Refused with "encoder" in the text: the sequence passes (gaq_policy_eval_seq_dev, gaq_policy_grad_ppo_seq_dev,
 * gaq_policy_grad_ppo_seq_idx_dev and their LSTM forms) and gaq_optim_create_policy on such a policy.  Its learner has entry points of
 * its own: "sequences through an encoder" below and gaq_optim_create_policy_enc.  (The refusals' texts still say that the learner is
 * not built: they are kept word for word.)  Additive: GAQ_ABI_VERSION stays. */
typedef struct {
  uint32_t struct_size;       /* sizeof(gaq_policy_desc_rnn_enc) */
  int32_t in_dim, n_hidden, width[3], hidden_act, out_tanh;   /* in_dim = the encoder's last width */
  int32_t engine;             /* GAQ_POLICY_ENGINE_MFMA */
  int32_t cell;               /* GAQ_POLICY_CELL_GRU or GAQ_POLICY_CELL_LSTM */
  int32_t enc_in_dim;         /* the env's obs_dim */
  int32_t enc_layers;         /* 1 or 2 */
  int32_t enc_width[2];
} gaq_policy_desc_rnn_enc;
int gaq_policy_create_rnn_enc(gaq_env* env, const gaq_policy_desc_rnn_enc* desc, gaq_policy** out);
int64_t gaq_policy_encoder_weight_count(const gaq_policy_desc_rnn_enc* desc);
int gaq_policy_set_encoder_weights(gaq_policy* p, const float* weights_host);
int gaq_policy_set_encoder_weights_dev(gaq_policy* p, const float* weights_dev);
int gaq_policy_get_encoder_weights(gaq_policy* p, float* weights_host);
int gaq_policy_encoder_width(const gaq_policy* p);

/* ---- actor-critic rollouts: value head, log-probabilities, advantages -------------------------------------------------------
 * What an on-policy learner needs beside (obs, reward, done, actions), from the work the policy launch has already done.
 * Value head: a linear critic on the shared trunk, V = w_v . y + b_v (fp32, never through tanh), y = the activations the 4-output
 * layer reads (the last hidden layer; h' for a GRU without head layers).  `wb` = gaq_policy_value_width(p) weights then the bias, host
 * or device pointer; NULL removes the head; synchronous like gaq_policy_set_weights.  It is a buffer of its own: the packed weight
 * layout, the weight counts and the descriptions are untouched.  fp32 MFMA and GRU policies only: GAQ_ERR_INVALID on a VALU or bf16
 * policy (the text names the engine).  V is deterministic; the order of its sum is the library's and carries no bit-compatibility
 * promise (each of 4 waves sums a quarter of the units in ascending order, then (s0 + s1) + (s2 + s3) + b_v). */
int gaq_policy_set_value_head(gaq_policy* p, const float* wb_host_or_null);
int gaq_policy_set_value_head_dev(gaq_policy* p, const float* wb_dev_or_null);
int gaq_policy_value_width(const gaq_policy* p);                   /* width of the last hidden layer, or GAQ_ERR_INVALID */
/* gaq_step_policy_many_dev that also writes
 *   value_out [T + 1, N]  row t = V of the observation action t was computed from (row 0: the current observation; for a GRU, of the h
 *                         that action used).  Row T = V of the observation the call ends on, i.e. row 0 of the next call, bit for bit: one
 *                         extra policy launch that writes V alone -- no action, no exploration draw, no h' (it reads h with the rows of
 *                         done[T-1] as 0, as the next call's first launch will) and does not advance the step counter.
 *   logp_out  [T, N]      log N(a_t; mean_t, exp(log_std)) = sum_k (-z_k^2 / 2 - log_std_k) - 2 ln 2 pi (fp32, k ascending) from the z the
 *                         device drew for a_t.  No Jacobian term: the noise is added after the output tanh.
 * Either may be NULL; with both NULL this IS gaq_step_policy_many_dev.  Asking for them changes nothing else: obs, reward, done, actions,
 * the GRU state and the env's state are the bits of the plain call (same draws, same Philox keys).  value_out without a value head, or
 * logp_out on a deterministic policy: GAQ_ERR_STATE.  Either on a VALU or bf16 policy: GAQ_ERR_INVALID.  Both 16-byte aligned, like obs.
 * Nothing synchronises with the host; graph-safe mode works.
 * Episode ends: where done[t] is set, the env auto-resets and value_out[t + 1] is the value of the NEXT episode's first observation.
 * gaq_gae_dev cuts there (no bootstrap across a done): it treats every episode end as absorbing.  Every done of this environment is a
 * time-limit truncation; gaq_step_policy_ac_term_many_dev and gaq_gae_term_dev below bootstrap from V of the terminal observation. */
int gaq_step_policy_ac_many_dev(gaq_env* env, gaq_policy* p, int32_t T, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                                float* actions_out_dev_or_null, float* value_out_dev_or_null, float* logp_out_dev_or_null, void* stream);
/* Generalised advantage estimation on the device, fp32, one launch: reward [T,N], done [T,N], value [T+1,N] as written above;
 *   nd = 1 - done[t];  delta = r_t + gamma nd V_{t+1} - V_t;  A_t = delta + gamma lambda nd A_{t+1} (A_T = 0);  ret_t = A_t + V_t
 * -> adv_out [T,N], ret_out [T,N] (or NULL).  N is the env's.  gamma or lambda outside [0, 1], or an output that overlaps an input or
 * the other output: GAQ_ERR_INVALID.  Enqueued on `stream`, no host synchronisation. */
int gaq_gae_dev(gaq_env* env, int32_t T, const float* reward_dev, const uint8_t* done_dev, const float* value_dev, float gamma, float lambda,
                float* adv_out_dev, float* ret_out_dev_or_null, void* stream);
/* Time-limit bootstrapping.  gaq_step_policy_ac_many_dev that also writes
 *   term_value_out [T, N] where done[t, i] is set: V (the value head) of the LAST observation of the episode that ended in step t -- the row
 *                         the step launch writes to the terminal-observation buffer (gaq_set_terminal_obs_dev).  MLP: V(trunk(term_obs)).
 *                         GRU: V(head(GRU(term_obs, h))) with h the env's row of the registered state as step t left it (the state action t
 *                         used, not yet zeroed): exactly what value_out[t + 1, i] would have been had the episode not been cut.
 *                         Where done[t, i] is clear: +0.0f.  Every element is written, every call.
 * fp32, 16-byte aligned; with term_value_out NULL this IS gaq_step_policy_ac_many_dev (same launches, same bits).  Asking for it changes
 * nothing else: obs, reward, done, actions, value_out, logp_out, the GRU state, the step counter and the env's state are the bits of the
 * plain call; no exploration draw, no host synchronisation, capturable under the rules of the plain call (the first call allocates: warm
 * up before capturing).  After each step launch one small launch compacts the envs with done[t] into a device list (and zeroes row t) and
 * a value-only policy launch runs on those rows alone, before the next policy launch resets the finished rows of a GRU's h: the cost is
 * proportional to the envs that finished plus two small launches per step.  The order of the list is not deterministic; the values are (V
 * of an env depends on its own row only).  If a terminal-observation buffer is registered it is used in place and stays registered;
 * otherwise the library uses an [N, obs_dim] scratch of its own (allocated on first use) and the env is left unregistered as it was.
 * Rows of envs that did not finish in step t are never read.  value_out may be NULL while term_value_out is not.
 * term_value_out without a value head: GAQ_ERR_STATE.  On a handle created with auto_reset = 0: GAQ_ERR_STATE (there value_out[t + 1]
 * already is the value of the terminal observation).  On a VALU or bf16 policy: GAQ_ERR_INVALID (the text names the engine).  Misaligned:
 * GAQ_ERR_INVALID.  Each refusal launches nothing and leaves env and policy usable. */
int gaq_step_policy_ac_term_many_dev(gaq_env* env, gaq_policy* p, int32_t T, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                                     float* actions_out_dev_or_null, float* value_out_dev_or_null, float* logp_out_dev_or_null,
                                     float* term_value_out_dev_or_null, void* stream);
/* gaq_gae_dev with term_value [T,N] as written above; d = done[t] != 0:
 *   V' = d ? term_value[t] : V_{t+1};  delta = fmaf(gamma, V', r_t) - V_t;  A_t = fmaf(d ? 0 : gamma lambda, A_{t+1}, delta);  ret_t = A_t + V_t
 * (the advantage chain still cuts at a done; only the one-step target looks past it).  term_value entries where done is clear are never
 * used.  With term_value NULL it returns gaq_gae_dev's bits.  term_value joins the overlap checks.  One launch, no host synchronisation. */
int gaq_gae_term_dev(gaq_env* env, int32_t T, const float* reward_dev, const uint8_t* done_dev, const float* value_dev,
                     const float* term_value_dev_or_null, float gamma, float lambda, float* adv_out_dev, float* ret_out_dev_or_null,
                     void* stream);
/* V-trace targets (Espeholt et al. 2018, the IMPALA / APPO off-policy correction) on the device, fp32, one launch: reward [T,N],
 * done [T,N], value [T+1,N] as above, logp_behaviour [T,N] as logp_out wrote it, logp_target [T,N] from the learner's forward pass.
 * For one env, t descending; at t = T - 1 the "next" quantities are V_T, vs_T = V_T and acc_T = 0; d = done[t] != 0:
 *   x   = logp_target[t] - logp_behaviour[t]                  (one fp32 subtraction)
 *   w   = expf(x)                                             (the accurate expf)
 *   rho = fminf(rho_bar, w);  c = lambda * fminf(c_bar, w);  rho_pg = fminf(pg_rho_bar, w)
 *   Vn  = d ? 0 : V[t+1];  VSn = d ? 0 : vs[t+1]              (selected, never multiplied by a mask)
 *   td  = fmaf(gamma, Vn, r[t]) - V[t]
 *   acc = fmaf(d ? 0 : gamma * c, acc, rho * td)
 *   vs[t] = V[t] + acc                                        -> vs_out [T,N]
 *   pg[t] = rho_pg * (fmaf(gamma, VSn, r[t]) - V[t])          -> pg_adv_out [T,N] (or NULL)
 * The order of the operations is part of the contract: when logp_target holds the bits of logp_behaviour and rho_bar, c_bar >= 1,
 * expf(0) is 1, gamma * c is the fp32 product gaq_gae_dev uses, acc is its advantage and vs_out is its ret_out BIT FOR BIT for the same
 * gamma and lambda: on-policy V-trace is the GAE(lambda) return.  w = +inf (expf overflowed) clips to the bars like any large ratio.
 * Refused with GAQ_ERR_INVALID, nothing launched: a null argument other than pg_adv_out; T <= 0; gamma or lambda outside [0, 1];
 * rho_bar, c_bar or pg_rho_bar not > 0 (NaN included; +inf is allowed: no clipping); an output that overlaps an input or the other
 * output.  25 bytes per env-step (21 without pg_adv_out).  Enqueued on `stream`, no host synchronisation. */
int gaq_vtrace_dev(gaq_env* env, int32_t T, const float* reward_dev, const uint8_t* done_dev, const float* value_dev,
                   const float* logp_behaviour_dev, const float* logp_target_dev, float gamma, float lambda, float rho_bar, float c_bar,
                   float pg_rho_bar, float* vs_out_dev, float* pg_adv_out_dev_or_null, void* stream);
/* gaq_vtrace_dev with time-limit bootstrapping: Vn = d ? term_value[t] : V[t+1] and VSn = d ? term_value[t] : vs[t+1], term_value [T,N]
 * as gaq_step_policy_ac_term_many_dev wrote it; the acc chain still cuts at a done.  Entries where done is clear never reach a sum.
 * On-policy, vs_out is gaq_gae_term_dev's ret_out bit for bit.  With term_value NULL it returns gaq_vtrace_dev's bits.  term_value joins
 * the overlap checks.  4 bytes per env-step more. */
int gaq_vtrace_term_dev(gaq_env* env, int32_t T, const float* reward_dev, const uint8_t* done_dev, const float* value_dev,
                        const float* logp_behaviour_dev, const float* logp_target_dev, const float* term_value_dev_or_null, float gamma,
                        float lambda, float rho_bar, float c_bar, float pg_rho_bar, float* vs_out_dev, float* pg_adv_out_dev_or_null,
                        void* stream);

/* ---- separate critic: a value network of its own ----------------------------------------------------------------------------
 * For learners that do not share a trunk between policy and value function.  A critic is an MLP obs (in_dim = the env's obs_dim) ->
 * [Linear -> act] x n_hidden -> Linear -> 1, fp32 on v_mfma_f32_16x16x4_f32: n_hidden in 1..3, every width a multiple of 16 in
 * [16, 256], hidden_act GAQ_POLICY_TANH / _RELU.  It is feed-forward and sees the observation only -- with a GRU actor too: it never
 * reads the actor's hidden state h.  Packed weights (fp32, contiguous): the hidden layers exactly as gaq_policy packs them
 * (W'[O/16][I][16], then bias[O]), then the 1-output layer as a value head is laid out: w[width[n_hidden-1]], then the bias.
 * gaq_critic_weight_count gives the number of floats.  V of a row is, bit for bit, what an fp32 MFMA policy with the same hidden layers
 * and that value head computes (the same kernel stages): each unit bias + its inputs in ascending order as one fmaf chain, V as
 * described at gaq_policy_set_value_head.
 * A wrong struct_size, n_hidden outside 1..3, a width[l] that is not a multiple of 16 in [16, 256], an unknown hidden_act or an in_dim
 * that is not the env's obs_dim: GAQ_ERR_INVALID, the text names the field, nothing is created. */
typedef struct gaq_critic gaq_critic;
typedef struct {
  uint32_t struct_size;       /* sizeof(gaq_critic_desc) */
  int32_t in_dim, n_hidden, width[3], hidden_act;
} gaq_critic_desc;
int gaq_critic_create(gaq_env* env, const gaq_critic_desc* desc, gaq_critic** out);
int64_t gaq_critic_weight_count(const gaq_critic_desc* desc);      /* floats of the packed layout, or GAQ_ERR_INVALID */
/* copy the packed weights (host pointer / device pointer on the env's device) into the critic; synchronous */
int gaq_critic_set_weights(gaq_critic* c, const float* packed_host);
int gaq_critic_set_weights_dev(gaq_critic* c, const float* packed_dev);
int gaq_critic_destroy(gaq_critic* c);
/* V of arbitrary observation rows: obs [rows, in_dim] -> value_out [rows] (fp32, row-major, on the critic's device), e.g. a learner
 * re-evaluating stored observations.  One launch on `stream`, no host synchronisation; rows == 0 is a no-op.  Both pointers need only a
 * float's alignment (4 bytes: a slice of a larger buffer is fine); a misaligned pointer, rows < 0 or weights never set: GAQ_ERR_INVALID. */
int gaq_critic_eval_dev(gaq_critic* c, int64_t rows, const float* obs_dev, float* value_out_dev, void* stream);
/* gaq_step_policy_ac_term_many_dev with V taken from `critic`:
 *   value_out [T + 1, N]  row t = critic(the observation action t was computed from); row T = critic(the observation the call ends on),
 *                         i.e. row 0 of the next call.  For a GRU actor too V is a function of the observation alone.
 *   logp_out  [T, N]      as before: it is the actor's, and does not depend on where V comes from (the policy must explore).
 *   term_value_out [T, N] critic(terminal observation of env i) where done[t, i] is set, +0.0f elsewhere; every element is written
 *                         (auto_reset must be on).
 * With critic NULL this IS gaq_step_policy_ac_term_many_dev: the same launches, the same bits.  With a critic the policy needs no value
 * head, and one that has a value head is refused (GAQ_ERR_STATE, the text says which to remove): the library does not pick one silently.
 * The policy must be an fp32 MFMA MLP policy or a GRU policy (VALU, bf16: GAQ_ERR_INVALID, the text names the engine); a critic created
 * for another env, or without weights: GAQ_ERR_INVALID.  Alignment rules are those of gaq_step_policy_ac_term_many_dev.  Each refusal
 * launches nothing and leaves env, policy and critic usable.  Asking for a critic changes nothing else: obs, reward, done, actions, the
 * GRU state, the step counter and the env's state are the bits of the plain call.
 * Launches: for an MLP actor one fused launch per step evaluates the actor and then the critic on the same tile (GAQ_NO_FUSED_CRITIC=1
 * when the critic is created: the actor's launch, then a critic launch; the same bits); for a GRU actor the GRU launch writes the action
 * and the log-probability and a critic launch writes value_out[t].  The bootstrap row and the terminal values are critic launches (the
 * latter on the gathered rows, in the place the policy's terminal pass has).  No host synchronisation; graph-safe mode works. */
int gaq_step_policy_critic_many_dev(gaq_env* env, gaq_policy* p, gaq_critic* critic_or_null, int32_t T, float* obs_dev, float* reward_dev,
                                    uint8_t* done_dev, float* actions_out_dev_or_null, float* value_out_dev_or_null,
                                    float* logp_out_dev_or_null, float* term_value_out_dev_or_null, void* stream);

/* ---- observation normalisation: running statistics and a clamp, on the device -------------------------------------------------
 * What rl_games (normalize_input), sample-factory and SB3's VecNormalize put in front of actor and critic: (x - mean) / sqrt(var + eps),
 * clamped to +-clip, with running mean / variance.  A normaliser belongs to one env (dim = its obs_dim, at most 256) and is attached to
 * that env's policies and critics; their kernels then normalise each observation where they stage it, so rollouts need no host loop.
 * State (device, fp64): count, mean[D], M2[D]; the population variance is M2 / count; before any update count = 0, mean = 0 and the
 *   variance is defined as 1.
 * Published table (device, fp32, what the kernels read): mean[D], inv_std[D] = 1 / sqrt(var + eps) computed in fp64 and rounded once,
 *   and clip.  Only the last launch of gaq_obs_norm_update_dev and gaq_obs_norm_set_stats write it, so work queued on the same stream
 *   sees a consistent table, and its address never changes: a captured rollout replays with whatever statistics are current.
 * One element, in every place (gaq_obs_norm_apply_dev and the staging of every kernel): fminf(fmaxf((x - mean[k]) * inv_std[k], -clip),
 *   clip) in fp32, the subtraction and the product rounded separately (no fma) -- so apply_dev and the kernels agree to the bit, and with
 *   mean = 0, inv_std = 1, clip = +inf it is the identity on every fp32 value, -0 included.  The bf16 engine rounds that fp32 result.
 *   Statistics stay fixed for a whole rollout: nothing inside gaq_step_policy_*_many_dev updates them.
 * LIFETIME: a normaliser must outlive every policy and critic it is attached to (detach with NULL, or destroy those first); the library
 *   keeps the pointer and does not count references.  A handle is not thread-safe: one update at a time (they share partial sums).
 * Every refusal below is GAQ_ERR_INVALID, launches nothing and leaves env, policy, critic and normaliser usable. */
typedef struct gaq_obs_norm gaq_obs_norm;
/* eps >= 0 (finite); clip > 0, +inf allowed (no clamp) */
int gaq_obs_norm_create(gaq_env* env, float eps, float clip, gaq_obs_norm** out);
/* Merge the rows of obs [rows, D] (fp32 row-major, device, 4-byte aligned: any slice of a larger buffer; rows >= 1) into the running
 * statistics and publish the table: one streaming pass (fp64 sums and partial means shifted by the batch's first row, so a feature with a large
 * mean and a small spread keeps its variance), Chan's parallel merge in a fixed order, no atomics -- the same input gives the same bits.
 * Two launches on `stream`, no host synchronisation. */
int gaq_obs_norm_update_dev(gaq_obs_norm* n, int64_t rows, const float* obs_dev, void* stream);
/* out[r][k] = the element expression of obs[r][k] with the published table; out may be obs (in place), but may not overlap it otherwise.
 * What a learner feeds its torch net: exactly what the device policy saw.  One launch on `stream`. */
int gaq_obs_norm_apply_dev(gaq_obs_norm* n, int64_t rows, const float* obs_dev, float* out_dev, void* stream);
/* synchronous (they wait for the device): read / replace the state; set_stats republishes the table (count >= 0, M2 >= 0, all finite) */
int gaq_obs_norm_get_stats(gaq_obs_norm* n, double* count, double* mean_D, double* m2_D);
int gaq_obs_norm_set_stats(gaq_obs_norm* n, double count, const double* mean_D, const double* m2_D);
int gaq_obs_norm_destroy(gaq_obs_norm* n);
/* Attach (NULL: detach).  From then on every launch that evaluates the policy -- rollout steps, the bootstrap row, the gathered terminal
 * pass, which normalises the terminal observations it gathers -- stages its observations through the table; the observations a rollout
 * RETURNS stay raw.  Without a normaliser every kernel launched is the one launched before this existed, bit for bit.  Refused: a
 * normaliser of another env; a VALU policy (the text names the engine; the fused closed-loop launch has no normalising form). */
int gaq_policy_set_obs_norm(gaq_policy* p, gaq_obs_norm* n_or_null);
/* The same for a separate critic (gaq_critic_eval_dev included).  Actor and critic each use their own attachment; the usual case is one
 * object on both.  The fused actor+critic launch needs the SAME normaliser (or none) on both; otherwise the rollout takes the
 * two-launch path (the bits are the same either way). */
int gaq_critic_set_obs_norm(gaq_critic* c, gaq_obs_norm* n_or_null);

/* ---- gradients on the device: the learner's forward-on-stored-rows and backward passes -----------------------------------------
 * For feed-forward fp32 MFMA nets: a policy created with GAQ_POLICY_ENGINE_MFMA, and a gaq_critic; 1 to 3 hidden layers of tanh or
 * relu, every hidden width a multiple of 16 in [16, 128].  The limit of 128 belongs to these five calls only (rollouts keep 256): a
 * wider net, and a VALU, bf16 or recurrent policy, is refused with GAQ_ERR_INVALID and a text that names the engine or the width.  A
 * value head on the policy's trunk takes no part in these five; the two shared-trunk forms below (gaq_policy_eval_ac_dev,
 * gaq_policy_grad_ppo_ac_dev) are the ones that use it, under the same limits.  An attached gaq_obs_norm is honoured where the observation is staged; its statistics
 * are frozen and take no gradient.
 * `rows` is any count >= 0 of row-major fp32 rows on the handle's device -- e.g. a [t0:t1] slice of a rollout's [T, N] buffers (rows
 * picked by an index vector: the *_idx_dev forms, "shuffled minibatches" below).  Pointers
 * need only a float's alignment (stats_out a double's).  Every gradient is in the packed weight layout of gaq_policy_set_weights /
 * gaq_critic_set_weights: weights and biases sit where the weights and biases are, weight_count floats.
 * Each call is enqueued on `stream` with no host synchronisation: one launch over the tiles and, for the gradient calls, one small
 * reduction.  The gradient calls keep a library-owned scratch on the handle (the workgroups' partial gradients), allocated by the first
 * gradient call of any form for the default number of workgroups (and the widest form's stride) and never moved by a later call of any `rows`, so a call is capturable in a graph
 * after one warm-up gradient call on that handle (only a call under a GAQ_GRAD_GROUPS above the default, larger than any before, frees
 * and re-allocates it, which invalidates graphs captured earlier).  The scratch is the handle's one: gradient calls on one handle must
 * be ordered -- on one stream, or with events between streams -- never concurrent; handles are independent of each other.
 * Determinism: every output is a function of the inputs alone -- not of the device's CU count, the stream or timing.  The number of
 * workgroups G = min(tiles of 64 rows, 512) and the tiles of each depend on `rows` only; each workgroup adds up its tiles in ascending
 * order, and the G partial gradients (and partial statistics) are summed in ascending order in fp64 and rounded once.  No floating-point
 * atomics.  GAQ_GRAD_GROUPS=<n> in the environment, read at the call, replaces the 512 (for tests).
 * rows == 0: zeros to every gradient and statistic, no tile work.  Refused with GAQ_ERR_INVALID, nothing launched, the handle stays
 * usable: a null required pointer, rows < 0, weights never set, clip_eps outside (0, 1), a NaN scale, a misaligned pointer, an output
 * that overlaps an input or another output. */
/* logp_out [rows] = log N(actions; mean, exp(log_std)) with mean = the net's output after the optional output tanh:
 * z_k = (a_k - mean_k) * exp(-log_std_k), logp = sum_k (-z_k^2 / 2 - log_std_k) - 2 ln 2 pi, k ascending (gaq_step_policy_ac_many_dev's
 * formula).  mean_out [rows, 4] (or NULL) is bit for bit what the rollout's policy launch computes for a deterministic policy on the same
 * observation.  A policy without log_std (gaq_policy_set_explore): GAQ_ERR_STATE. */
int gaq_policy_logp_dev(gaq_policy* p, int64_t rows, const float* obs_dev, const float* actions_dev, float* logp_out_dev,
                        float* mean_out_dev_or_null, void* stream);
/* grad_out [weight_count] = sum_i scale * dout[i] . d mean_i / d theta for a caller-given dout [rows, 4] (the gradient with respect to mean) */
int gaq_policy_backward_dev(gaq_policy* p, int64_t rows, const float* obs_dev, const float* dout_dev, float scale, float* grad_out_dev,
                            void* stream);
/* The clipped PPO surrogate, fused.  Per row: x = logp - logp_old, r = expf(x), s1 = r A, s2 = clamp(r, 1 - eps, 1 + eps) A,
 * L = -min(s1, s2); dL/dlogp = -A r where s1 <= s2, else 0; dlogp/dmean_k = z_k exp(-log_std_k) (times 1 - mean_k^2 under out_tanh);
 * dlogp/dlog_std_k = z_k^2 - 1.  grad_out [weight_count] and grad_log_std_out [4] are sum_i scale * dL_i (pass scale = 1 / rows for the
 * mean).  stats_out: 4 doubles -- sum_i L_i (unscaled), the number of rows with s2 < s1, sum_i (r - 1 - x) (the k3 estimate of the KL
 * divergence, for early stopping), rows.  APPO passes gaq_vtrace_dev's pg_adv as adv.  No entropy term: for a state-independent
 * log_std its gradient is a constant the caller adds.  A policy without log_std: GAQ_ERR_STATE. */
int gaq_policy_grad_ppo_dev(gaq_policy* p, int64_t rows, const float* obs_dev, const float* actions_dev, const float* logp_old_dev,
                            const float* adv_dev, float clip_eps, float scale, float* grad_out_dev, float* grad_log_std_out_dev,
                            double* stats_out_dev, void* stream);
/* The critic's forms: dout [rows] is the gradient with respect to V; the loss of grad_mse is L = (V - target)^2 / 2, its stats_out 2
 * doubles: sum_i L_i (unscaled) and rows. */
int gaq_critic_backward_dev(gaq_critic* c, int64_t rows, const float* obs_dev, const float* dout_dev, float scale, float* grad_out_dev,
                            void* stream);
int gaq_critic_grad_mse_dev(gaq_critic* c, int64_t rows, const float* obs_dev, const float* target_dev, float scale, float* grad_out_dev,
                            double* stats_out_dev, void* stream);
/* Shared-trunk actor-critic: a policy with a value head (gaq_policy_set_value_head) V = wv . y + bv on its last hidden layer.  Both
 * calls are one pass of the same kernel family, under everything said above (limits, scratch, determinism, refusals); without a value
 * head they return GAQ_ERR_STATE with a text that names the value head, without log_std GAQ_ERR_STATE as gaq_policy_logp_dev.
 * gaq_policy_eval_ac_dev: the learner's forward pass on stored rows.  logp_out [rows] and mean_out [rows, 4] (or NULL) are
 * gaq_policy_logp_dev's bits; value_out [rows] is bit for bit the V gaq_step_policy_ac_many_dev records on the same observation: each
 * of four parts sums its quarter of the units from 0 in ascending order, V = ((p0 + p1) + (p2 + p3)) + bv. */
int gaq_policy_eval_ac_dev(gaq_policy* p, int64_t rows, const float* obs_dev, const float* actions_dev, float* logp_out_dev,
                           float* value_out_dev, float* mean_out_dev_or_null, void* stream);
/* The combined PPO loss, fused: per row L = L_clip + vf_coef L_V - ent_coef H, times scale, summed over the rows.  L_clip is
 * gaq_policy_grad_ppo_dev's surrogate (the same branch rule s1 <= s2).  L_V = (V - ret)^2 / 2 when vclip == 0 (v_old may be NULL); when
 * vclip > 0, L_V = max(e1^2, e2^2) / 2 with e1 = V - ret, e2 = v_old + clamp(V - v_old, +-vclip) - ret, and dL_V/dV = e1 where
 * e1^2 >= e2^2, else 0 (the PPO2 clipped value loss).  H is the diagonal Gaussian's entropy: state-independent, it adds
 * -ent_coef * scale * rows to every component of grad_log_std, in fp64 before the one rounding.  The two losses' deltas meet in the trunk:
 * one forward, one backward.  grad_out [weight_count]: the packed trunk and 4-output layer, gaq_policy_grad_ppo_dev's layout;
 * grad_value_out [W + 1]: gaq_policy_set_value_head's layout (weights, bias), W = gaq_policy_value_width; grad_log_std_out [4].
 * stats_out: 6 doubles -- sum L_clip, rows with the ratio clipped, sum (r - 1 - x), sum L_V (unweighted, unscaled), rows whose value
 * gradient the clip cut, rows.  With vf_coef == 0 and ent_coef == 0, grad_out, grad_log_std_out and the first three statistics are
 * gaq_policy_grad_ppo_dev's bits.  Refused with GAQ_ERR_INVALID besides the above: vclip negative or NaN; vf_coef, ent_coef or scale NaN;
 * vclip > 0 with a NULL v_old. */
int gaq_policy_grad_ppo_ac_dev(gaq_policy* p, int64_t rows, const float* obs_dev, const float* actions_dev, const float* logp_old_dev,
                               const float* adv_dev, const float* ret_dev, const float* v_old_dev_or_null, float clip_eps, float vclip,
                               float vf_coef, float ent_coef, float scale, float* grad_out_dev, float* grad_value_out_dev,
                               float* grad_log_std_out_dev, double* stats_out_dev, void* stream);

/* ---- gradients of a recurrent policy: the learner's passes over stored sequences, for a GRU policy -----------------------------
 * For a policy created with gaq_policy_create_rnn and GAQ_POLICY_CELL_GRU: a cell of H in {16, 32, 48, 64}, 0 to 2 head layers of
 * width <= 64 (tanh or relu), out_tanh 0 or 1, any in_dim that fits the kernel's LDS.  The limit of 64 belongs to these two calls only
 * (rollouts keep 256): a backward step holds the observation, hin, the carried dh and four delta planes of H rows of a 64-sequence
 * tile in LDS at once, 8.25 KiB + 272 B x (in_dim rounded up to 16 + 2 H + max(4 H, H + the head widths)) -- 118.75 KiB at
 * 18-GRU64-64-64, over 200 KiB at H = 128, against 160 KiB.  A feed-forward policy (the text says a recurrent cell is required), an
 * LSTM policy (the text names the LSTM: gaq_policy_eval_lstm_seq_dev and gaq_policy_grad_ppo_lstm_seq_dev below take it), a wider net
 * (the text names the width) and weights never set: GAQ_ERR_INVALID.
 * Inputs are T >= 1 steps of S >= 0 independent sequences (S need not be the env's N): obs [T, S, D], where row t is the observation
 * action t was computed from -- of a rollout: obs0, then obs_out[:-1]; actions [T, S, 4]; done [T, S] (uint8); h0 [S, H], the
 * registered hidden state as it stood before the rollout call.  With h_{-1} = h0, for t = 0 .. T-1:
 *   hin_t = (t > 0 and done[t-1]) ? 0 : h_{t-1}   (a select), h_t = GRU(obs_t, hin_t) in the rollout kernel's arithmetic,
 *   y_t = the head's layers on h_t, mean_t = the 4 outputs (after the optional tanh), V_t = wv . y_t + bv, logp_t = gaq_policy_logp_dev's
 *   formula -- so mean, V and h are bit for bit what gaq_step_policy_ac_many_dev computed.  An attached gaq_obs_norm is honoured where
 *   the observation is staged; it is frozen and takes no gradient.
 * Both calls are enqueued on `stream` with no host synchronisation.  S == 0 writes zeros to the gradient outputs and the statistics
 * and launches nothing.  Refused with GAQ_ERR_INVALID, nothing launched, the handle stays usable: T < 1, S < 0, a null required
 * pointer, a misaligned pointer (h0 and h_out 16 bytes, stats_out 8, the others a float's), an output that overlaps an input or another
 * output, clip_eps outside (0, 1), vclip negative or NaN, vclip > 0 with a NULL v_old, a NaN coefficient or scale.
 * gaq_policy_eval_seq_dev: logp_out [T, S], value_out [T, S], mean_out [T, S, 4] and h_out [S, H] are each optional (NULL).  h_out is
 * h_{T-1} with the rows of done[T-1] zeroed: the state the next action uses, what the rollout leaves in the registered buffer.
 * value_out without a value head and logp_out without log_std: GAQ_ERR_STATE (gaq_policy_eval_ac_dev's texts).  With logp_out NULL,
 * actions may be NULL.  One launch. */
int gaq_policy_eval_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs_dev, const float* actions_dev_or_null,
                            const uint8_t* done_dev, const float* h0_dev, float* logp_out_dev_or_null, float* value_out_dev_or_null,
                            float* mean_out_dev_or_null, float* h_out_dev_or_null, void* stream);
/* The truncated-BPTT gradient of gaq_policy_grad_ppo_ac_dev's loss, per (t, sequence) scale * (L_clip + vf_coef L_V - ent_coef H),
 * summed: the same branch rules (s1 <= s2; e2 taken as e1 where the clamp does not bind; the tie to e1), the entropy term formed in
 * fp64 by the host and added in the reduction, and the same six statistics -- sum L_clip, rows with the ratio clipped, sum (r - 1 - x),
 * sum L_V, rows the value clip cut, T S.  The gradient is truncated at the call's first step -- nothing flows into h0, there is no
 * grad_h0 -- and flows through time exactly where done[t-1] is clear.
 * grad_out [gaq_policy_weight_count_rnn] is in the packed GRU layout: W_ih', b_ih, W_hh', b_hh, then the head.  b_ih and b_hh are
 * separate words: for the r and z gates they receive the same sum, for n those of da_n and of da_n r.  grad_value_out [W + 1]
 * (gaq_policy_set_value_head's layout), grad_log_std_out [4], stats_out: 6 doubles.
 * Without a value head ret, v_old and grad_value_out must be NULL (else GAQ_ERR_STATE, the text names the value head); vf_coef and
 * vclip are then ignored and the statistics 3 and 4 are exactly 0.  With one, ret and grad_value_out are required.  No log_std:
 * GAQ_ERR_STATE.
 * Determinism: G = min(tiles of 64 sequences, 512 or GAQ_GRAD_GROUPS) workgroups; workgroup g takes the tiles [g nt / G, (g + 1) nt / G)
 * ascending, each tile's steps descending; every word of a workgroup's partial is owned by one lane, the first (tile, t) storing and
 * the others adding; the G partials are summed in ascending order in fp64 and rounded once.  The order of every sum is a function of
 * (T, S, GAQ_GRAD_GROUPS) alone; no atomics.
 * Scratch: the handle's gradient scratch (calls on one handle must be ordered, as above) holds the partials -- sized for 512
 * workgroups whatever the call needs -- and then the tape of h_t, G x T x 64 x H x 4 bytes (537 MB at G = 512, T = 64, H = 64).  It grows,
 * and its pointers move, only when a call needs more than every call before it: a graph captured after a warm-up call with the largest
 * T and S stays valid.  Two launches. */
int gaq_policy_grad_ppo_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs_dev, const float* actions_dev, const uint8_t* done_dev,
                                const float* h0_dev, const float* logp_old_dev, const float* adv_dev, const float* ret_dev_or_null,
                                const float* v_old_dev_or_null, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                                float* grad_out_dev, float* grad_value_out_dev_or_null, float* grad_log_std_out_dev, double* stats_out_dev,
                                void* stream);

/* ---- shuffled minibatches: index-gathered gradient calls and a permutation on the device ---------------------------------------
 * The four loss gradients above with the minibatch as an argument: the input arrays are the rollout's own buffers, src_rows rows
 * (S_src columns) long, and row j of the call is source row idx[j] (sequence s is column idx[s] of every [T, S_src, ...] input, done
 * and h0 [S_src, H] included).  idx is int32 [rows] ([S]) on the handle's device, 4-byte aligned -- perm + k * mb is a minibatch;
 * duplicates are allowed, the inputs are only read.  After idx and src_rows the arguments are the parent call's from obs_dev on.
 * DEFINING PROPERTY: with every index in range, every output bit -- gradients, grad_value, grad_log_std, the parent's statistics -- is
 *   the parent call's on the gathered arrays x[idx] (x[:, idx] and h0[idx]).  `rows` (`S`) alone decides G, the tiles of each workgroup
 *   and every order of summation, as stated for the parent calls; only the addresses of the kernels' loads differ, and no gathered
 *   copy is ever written.  An attached gaq_obs_norm is honoured where the observation is staged.
 * INDICES OUT OF RANGE cannot be refused without a host synchronisation, so the kernels never form an address from an index outside
 *   [0, src_rows) ([0, S_src)): such a row (sequence) is a dead lane of its tile and contributes exactly 0 to every gradient and
 *   statistic, as the lanes past the end of a ragged last tile do.  They are counted: stats_out is the parent's statistics followed by
 *   ONE MORE double, the number of indices skipped -- 5, 7, 3 and 7 doubles for the four calls -- a per-lane sum reduced in fp64 in
 *   ascending order like the others.  The `rows` (T S) statistic stays the count given; scale is whatever the caller passes.
 * Everything the parent call refuses is refused with its code and its text under the new function's name.  Also GAQ_ERR_INVALID: a
 * null idx with rows > 0, a misaligned idx, src_rows < 1 with rows > 0, src_rows > 2^31 - 1, idx overlapping an output.  The input
 * spans are src_rows long, the idx span `rows`.  rows == 0: zeros to every output, nothing launched.  Two launches, no host
 * synchronisation.  Scratch: the handle's one, with the parent's sizes -- an idx call counts as a gradient call for the warm-up rule,
 * and a contiguous call after an idx call (or the other way round) finds the scratch where it was. */
int gaq_policy_grad_ppo_idx_dev(gaq_policy* p, int64_t rows, const int32_t* idx_dev, int64_t src_rows, const float* obs_dev,
                                const float* actions_dev, const float* logp_old_dev, const float* adv_dev, float clip_eps, float scale,
                                float* grad_out_dev, float* grad_log_std_out_dev, double* stats_out_dev, void* stream);
int gaq_policy_grad_ppo_ac_idx_dev(gaq_policy* p, int64_t rows, const int32_t* idx_dev, int64_t src_rows, const float* obs_dev,
                                   const float* actions_dev, const float* logp_old_dev, const float* adv_dev, const float* ret_dev,
                                   const float* v_old_dev_or_null, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                                   float* grad_out_dev, float* grad_value_out_dev, float* grad_log_std_out_dev, double* stats_out_dev,
                                   void* stream);
int gaq_critic_grad_mse_idx_dev(gaq_critic* c, int64_t rows, const int32_t* idx_dev, int64_t src_rows, const float* obs_dev,
                                const float* target_dev, float scale, float* grad_out_dev, double* stats_out_dev, void* stream);
int gaq_policy_grad_ppo_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx_dev, int64_t S_src, const float* obs_dev,
                                    const float* actions_dev, const uint8_t* done_dev, const float* h0_dev, const float* logp_old_dev,
                                    const float* adv_dev, const float* ret_dev_or_null, const float* v_old_dev_or_null, float clip_eps,
                                    float vclip, float vf_coef, float ent_coef, float scale, float* grad_out_dev,
                                    float* grad_value_out_dev_or_null, float* grad_log_std_out_dev, double* stats_out_dev, void* stream);
/* ---- gradients of an LSTM policy: the same passes over stored sequences for GAQ_POLICY_CELL_LSTM -------------------------------
 * The two halves the GRU has above and the index-gathered form of the second, for a policy created with gaq_policy_create_rnn and
 * GAQ_POLICY_CELL_LSTM: a cell of H in {16, 32, 48, 64} (80 is the first refused width), 0 to 2 head layers of width <= 64 (tanh or
 * relu), out_tanh 0 or 1, any in_dim that fits the kernel's LDS.  A backward step holds the observation, hin, the carried dh, the
 * carried dc and four delta planes of H rows of a 64-sequence tile in LDS at once:
 *   8.25 KiB + 272 B x (in_dim rounded up to 16 + 3 H + max(4 H, H + the head widths))      (+ 256 B for the idx form)
 * -- 135.75 KiB at 18-LSTM64-64-64 against 160 KiB; the forward call takes 8.25 KiB + 272 B x (in_dim rounded up to 16 + 2 H + the head
 * widths).  A call whose figure passes 160 KiB is refused before any launch ("in_dim too large ...").  A GRU policy (the text names
 * the GRU), a feed-forward policy (the text says a recurrent cell is required), a wider net (the text names the width) and weights
 * never set: GAQ_ERR_INVALID.  The GRU entry points above keep refusing an LSTM handle.
 * Inputs as for the GRU calls, with a second state: h0 and c0 [S, H], the registered hidden and cell states as they stood before the
 * rollout call.  With (h, c)_{-1} = (h0, c0), for t = 0 .. T-1:
 *   (hin, cin)_t = (t > 0 and done[t-1]) ? (0, 0) : (h, c)_{t-1}   (a select),
 *   (h_t, c_t) = LSTM(obs_t, hin_t, cin_t) in the rollout kernel's arithmetic: each of the gate sums i, f, g, o starts at b_ih + b_hh
 *   (one fp32 add) and takes the x products then the h products as ascending k-ordered chains; i, f, o are sigmoids, g = tanhf;
 *   c' = fmaf(f, cin, i g), h' = o tanhf(c');
 *   the head, V and logp as in gaq_policy_eval_seq_dev -- so mean, V, h and c are bit for bit what gaq_step_policy_ac_many_dev computed.
 *   An attached gaq_obs_norm is honoured where the observation is staged; it is frozen and takes no gradient.
 * Every refusal of the GRU calls is made here with its code and its text under the new function's name: T < 1, S < 0, a null required
 * pointer (c0 is required like h0), a misaligned pointer (h0, c0, h_out and c_out 16 bytes, stats_out 8, the others a float's), an
 * output that overlaps an input or another output (c_out over c0 included), clip_eps outside (0, 1), vclip negative or NaN, vclip > 0
 * with a NULL v_old, a NaN coefficient or scale; the value-head and log_std rules with GAQ_ERR_STATE.  S == 0 writes zeros to the
 * gradient outputs and the statistics and launches nothing.
 * gaq_policy_eval_lstm_seq_dev: logp_out, value_out, mean_out, h_out and c_out [S, H] are each optional (NULL).  h_out and c_out are
 * (h, c)_{T-1} with the rows of done[T-1] zeroed: what the rollout leaves in the two registered buffers.  One launch. */
int gaq_policy_eval_lstm_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs_dev, const float* actions_dev_or_null,
                                 const uint8_t* done_dev, const float* h0_dev, const float* c0_dev, float* logp_out_dev_or_null,
                                 float* value_out_dev_or_null, float* mean_out_dev_or_null, float* h_out_dev_or_null,
                                 float* c_out_dev_or_null, void* stream);
/* gaq_policy_grad_ppo_seq_dev for the LSTM: the same loss, branch rules, entropy term and six statistics.  Truncated BPTT: nothing
 * flows into h0 or c0, and both dh and dc flow from step t to t - 1 exactly where done[t-1] is clear.
 * grad_out [gaq_policy_weight_count_rnn] is in the packed LSTM layout: W_ih', b_ih, W_hh', b_hh, then the head.  b_ih and b_hh are
 * separate words that receive the same sum, bit for bit, for all four gates.
 * Determinism is the GRU call's: the same G, the same ownership of every word of a partial, the fp64 reduction in ascending order.
 * Scratch: the handle's gradient scratch, with the tape of h_t and c_t behind the partials: G x T x 64 x 2 H x 4 bytes (a sequence's h_t
 * and c_t side by side; 1.07 GB at G = 512, T = 64, H = 64), twice the GRU's.  It grows, and its pointers move, only when a call needs
 * more than every call before it: a graph captured after a warm-up call with the largest T and S stays valid.  The scratch belongs to
 * the handle, so a warm-up on a GRU handle of the same sizes says nothing about an LSTM handle's.  Two launches. */
int gaq_policy_grad_ppo_lstm_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs_dev, const float* actions_dev,
                                     const uint8_t* done_dev, const float* h0_dev, const float* c0_dev, const float* logp_old_dev,
                                     const float* adv_dev, const float* ret_dev_or_null, const float* v_old_dev_or_null, float clip_eps,
                                     float vclip, float vf_coef, float ent_coef, float scale, float* grad_out_dev,
                                     float* grad_value_out_dev_or_null, float* grad_log_std_out_dev, double* stats_out_dev, void* stream);
/* Its index-gathered form, under the contract of "shuffled minibatches" above: sequence s is column idx[s] of every [T, S_src, ...]
 * input and of h0 and c0 [S_src, H]; with every index in range each output bit is the contiguous call's on x[:, idx], h0[idx] and
 * c0[idx]; an index outside [0, S_src) is a dead lane and is counted in stats_out[6] (7 doubles). */
int gaq_policy_grad_ppo_lstm_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx_dev, int64_t S_src, const float* obs_dev,
                                         const float* actions_dev, const uint8_t* done_dev, const float* h0_dev, const float* c0_dev,
                                         const float* logp_old_dev, const float* adv_dev, const float* ret_dev_or_null,
                                         const float* v_old_dev_or_null, float clip_eps, float vclip, float vf_coef, float ent_coef,
                                         float scale, float* grad_out_dev, float* grad_value_out_dev_or_null, float* grad_log_std_out_dev,
                                         double* stats_out_dev, void* stream);

/* ---- sequences through an encoder: the learner's forward pass for gaq_policy_create_rnn_enc policies ----------------------------
 * A policy with an encoder in front of its cell (obs -> 1..2 Linear + act -> GRU | LSTM -> head) is refused by every call above, and
 * keeps being refused there.  Its passes have names of their own and take BOTH cells: the handle's cell picks the kernel, c0 and c_out
 * are an LSTM's and must be NULL for a GRU (GAQ_ERR_INVALID, a text of its own).  Additive: GAQ_ABI_VERSION stays 5.
 * The encoder is not recurrent, so it is not part of the kernel that is serial in T.  The call is two launches:
 *   1. the rollout's own encoder kernel on the T x S stored rows obs [T S, obs_dim] -> features [T S, E] (E = the encoder's last width),
 *      through the attached gaq_obs_norm where there is one: the features are the rollout's bits;
 *   2. the forward sequence kernel of the cell (gaq_policy_eval_seq_dev's / gaq_policy_eval_lstm_seq_dev's, unchanged) with the features
 *      as its observation, in_dim = E and no normaliser.
 * So mean, V, h_out and c_out are bit for bit what gaq_step_policy_ac_many_dev computed from the same observations, dones and states.
 * Family: encoder widths <= 128, H and head widths <= 64 (the text names the width); E is bounded by the sequence kernel's LDS,
 *   8.25 KiB + 272 B x (E + 2 H + the head widths) for this forward call, refused past 160 KiB with the text of the calls above.
 * T x S <= 2^31 - 1 rows.  Refused with GAQ_ERR_INVALID and nothing launched: a policy without an encoder (the text says "encoder"),
 * encoder weights never set, weights never set.  Every other argument, refusal, alignment and overlap rule is
 * gaq_policy_eval_lstm_seq_dev's under this function's name, with obs_dev [T, S, the env's obs_dim].
 * Scratch: GAQ_ENC_FEAT_BYTES(T, S, E) of features in the handle's gradient scratch, behind its fixed part where a gradient call keeps
 * its tape; it grows, and its pointers move, only when a call needs more than every call on the handle before it, so a graph captured
 * after the largest call stays valid.  Calls on one handle must be ordered, as for every gradient call.
 * The optimiser's step in place for such a policy is gaq_optim_create_policy_enc / gaq_optim_step_enc_dev ("the optimiser on the
 * device"); gaq_optim_create_policy keeps refusing it. */
#define GAQ_ENC_FEAT_BYTES(T, S, E) ((size_t)(T) * (size_t)(S) * (size_t)(E) * 4u)
int gaq_policy_eval_enc_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs_dev, const float* actions_dev_or_null,
                                const uint8_t* done_dev, const float* h0_dev, const float* c0_dev_or_null, float* logp_out_dev_or_null,
                                float* value_out_dev_or_null, float* mean_out_dev_or_null, float* h_out_dev_or_null,
                                float* c_out_dev_or_null, void* stream);
/* The truncated-BPTT gradient of gaq_policy_grad_ppo_seq_dev's loss through the cell AND the encoder: gaq_policy_grad_ppo_lstm_seq_dev's
 * arguments (c0_dev NULL for a GRU) plus grad_enc_out_dev [gaq_policy_encoder_weight_count], the encoder's block in its packed layout
 * (per layer W' [W/16][in][16], then the bias), after grad_out_dev.  grad_out, grad_value_out, grad_log_std_out and the six statistics
 * are what the cell's call gives on the features.  An attached gaq_obs_norm is honoured where the observation is staged and is frozen.
 * Split passes, not one fused kernel -- the encoder's work is a batch over the T x S stored rows, T times the parallelism of the kernel
 * that is serial in T:
 *   1. the encoder's forward over the rows -> feat [T S, E] (as in gaq_policy_eval_enc_seq_dev);
 *   2. the cell's backward sequence kernel on feat, which besides its own gradients writes dfeat_t = W_ih^T [da_r; da_z; da_n] (the LSTM:
 *      all four gate deltas) for every live (t, sequence) to dfeat [T S, E], one 16-byte store per lane; then the reduce of its partials;
 *   3. the encoder's backward over the rows: the observation staged through the normaliser, the layers recomputed, dfeat times act'(h)
 *      as the last layer's delta, dW as MFMAs over the tile's 64 rows, db as row sums, W^T delta between two layers; the workgroups'
 *      partials are then summed in ascending order in fp64 and rounded once.  No atomics, no statistics of its own.
 * Five launches.  Deterministic for a given GAQ_GRAD_GROUPS.  LDS of the sequence kernel: the backward formulas of the GRU / LSTM
 * sections with in_dim = E (127.25 KiB at enc64-GRU64-64-64, 144.25 KiB at enc64-LSTM64-64-64; LSTM64-64-64 behind E = 128 is refused
 * with "in_dim too large ..."; E = 112 is the largest it accepts, 157 KiB, 157.25 KiB in the idx form: the most any kernel of the
 * library asks for); of the encoder's backward 272 B x (obs_dim rounded up to 16 + its widths).
 * Scratch, behind the tape in the handle's gradient scratch: feat and dfeat (GAQ_ENC_FEAT_BYTES each, with S_src for S in the idx form),
 * the encoder's partials GAQ_ENC_PART_BYTES(G', count) (G' = min(ceil(T S / 64), GAQ_GRAD_GROUPS or 512)), and for the idx form
 * GAQ_ENC_ROWIDX_BYTES(T, S).  grad_scratch's rule: it grows only when a call needs more than every call before it.
 * S == 0 writes zeros to every output and launches nothing.  Refusals: those of gaq_policy_eval_enc_seq_dev and of the cell's gradient
 * call, under this function's name. */
#define GAQ_ENC_PART_BYTES(G, count) ((size_t)(G) * (((size_t)(count) + 15u) & ~(size_t)15u) * 4u)
#define GAQ_ENC_ROWIDX_BYTES(T, S) (2u * ((((size_t)(T) * (size_t)(S) * 4u) + 15u) & ~(size_t)15u) + 16u)
int gaq_policy_grad_ppo_enc_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs_dev, const float* actions_dev,
                                    const uint8_t* done_dev, const float* h0_dev, const float* c0_dev_or_null, const float* logp_old_dev,
                                    const float* adv_dev, const float* ret_dev_or_null, const float* v_old_dev_or_null, float clip_eps,
                                    float vclip, float vf_coef, float ent_coef, float scale, float* grad_out_dev, float* grad_enc_out_dev,
                                    float* grad_value_out_dev_or_null, float* grad_log_std_out_dev, double* stats_out_dev, void* stream);
/* Its index-gathered form, under the contract of "shuffled minibatches": sequence s is column idx[s] of every [T, S_src, ...] input and of
 * h0 (and c0) [S_src, H]; with every index in range each output bit is the contiguous call's on the gathered inputs.  feat and dfeat
 * live at source positions [T, S_src, E] (row = source row), so the sequence kernel's idx form reads features exactly as it reads
 * observations.  One elementwise launch first writes the row indices t S_src + idx[j]; the encoder's gathered forward (the rollout's
 * terminal-pass kernel) and its backward read their rows through them, so only rows that an index names are encoded or read.  An
 * index outside [0, S_src) forms no address (the gathered forward encodes column 0 of that step once more, to the same bits, in its
 * place), contributes exactly 0 to every output and is counted once in stats_out[6] (7 doubles).  T x S_src <= 2^31 - 1. */
int gaq_policy_grad_ppo_enc_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx_dev, int64_t S_src, const float* obs_dev,
                                        const float* actions_dev, const uint8_t* done_dev, const float* h0_dev, const float* c0_dev_or_null,
                                        const float* logp_old_dev, const float* adv_dev, const float* ret_dev_or_null,
                                        const float* v_old_dev_or_null, float clip_eps, float vclip, float vf_coef, float ent_coef,
                                        float scale, float* grad_out_dev, float* grad_enc_out_dev, float* grad_value_out_dev_or_null,
                                        float* grad_log_std_out_dev, double* stats_out_dev, void* stream);

/* idx_out [n] (int32, device) = a permutation of 0 .. n-1 that is a pure function of (n, seed, epoch): one elementwise launch on
 * `stream` (on the stream's device, as gaq_hbm_copy_dev), no sort, no atomics, no scratch, no host synchronisation.  With epoch_dev
 * given (a device word, 8-byte aligned) the kernel reads the epoch from it when it RUNS and ignores the by-value argument: advance the
 * word with any enqueued operation -- also inside a captured graph -- and every replay draws a new permutation.  The kernel writes
 * idx_out only.  Refused (GAQ_ERR_INVALID): n < 1, n > 2^31 - 1, a null or misaligned idx_out, a misaligned epoch_dev.
 * THE FORMULA IS THE CONTRACT (checkpoints and multi-rank learners reproduce a permutation from it); all arithmetic is on unsigned
 * 32-bit words unless a 64-bit product is written:
 *   b = the smallest even number >= max(2, ceil(log2 n)), h = b / 2, mask = 2^h - 1.
 *   Round keys key[0 .. 7]: key[4 j + q] = word q of Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, key
 *     increments 0x9E3779B9, 0xBB67AE85) with key (seed low, seed high) and counter (epoch low, epoch high ^ (140 << 24), j, 0), j = 0, 1.
 *   P(x), x < 2^b: (L, R) = (x >> h, x & mask); then 8 rounds, r = 0 .. 7:
 *       p = 0xD2511F53 * (R ^ key[r])               (64-bit product)
 *       q = 0xCD9E8D57 * ((p >> 32) ^ (p & 0xFFFFFFFF))   (64-bit product)
 *       f = ((q >> 32) ^ (q & 0xFFFFFFFF)) >> (32 - h)
 *       (L, R) = (R, L ^ f)
 *     and P(x) = (L << h) | R.
 *   idx_out[i] = the first of P(i), P(P(i)), ... that is below n (cycle walking).
 * P is a bijection of [0, 2^b) for every key, so the walk follows i's cycle, which returns to i < n: it always ends, after at most
 * 4 applications on average (2^b <= 4 n), and distinct i end on distinct values. */
int gaq_perm_dev(int64_t n, uint64_t seed, uint64_t epoch, const uint64_t* epoch_dev_or_null, int32_t* idx_out_dev, void* stream);

/* ---- the wide learner: the same gradients for hidden widths up to 256 -----------------------------------------------------------
 * The calls above ("gradients on the device", "shuffled minibatches") refuse a hidden width above 128; the rollout side runs
 * feed-forward nets up to 256.  These three take every net of that family -- a gaq_policy on GAQ_POLICY_ENGINE_MFMA without a cell,
 * with or without a value head, log_std on the host or in the exploration table; a gaq_critic; 1 to 3 hidden layers, tanh or relu,
 * widths multiples of 16 in [16, 256], out_tanh 0 or 1, any in_dim, an attached gaq_obs_norm honoured (frozen) where the observation
 * is staged -- under ONE limit, the same for all three, so that a net one call accepts is accepted by all:
 *     in_dim rounded up to 16 + the sum of the hidden widths <= 560.
 * A 64-row tile keeps every layer's activations in LDS, 272 B per row of that sum behind a head region of 8.25 KiB (+ 256 B with an
 * index vector): 156 672 B at 18-256-256, 161 024 B at 560 rows, under the 163 840 B a workgroup may ask for; 18-256-256-32 (165 376 B)
 * is the first shape refused.  THREE LAYERS OF 256 (18-256-256-256) ARE REFUSED: three 256-wide fp32 layers do not fit 64-row tiles,
 * and spilling activations to global scratch or working on half tiles is not built.  The refusal (GAQ_ERR_INVALID) names LDS and the
 * sum.  The VALU, bf16, recurrent and encoder engines are refused with a text that names the engine.
 * The arithmetic is the narrow calls', in their order: on any net of widths <= 128 a wide call returns the narrow call's bits (mean,
 * logp and V the rollout's, as stated there).  Checks, their order, alignment and overlap rules are the narrow calls'; rows = 0 writes
 * zeros and launches nothing.  idx_dev = NULL: the call's rows are rows 0 .. rows - 1 of the inputs and src_rows is ignored; else row j
 * is source row idx_dev[j] of inputs of src_rows rows, an index outside [0, src_rows) forms no address, contributes exactly 0 and is
 * counted, and stats_out is one double longer (its last: the indices skipped).  Scratch is the handle's (about 145 MB at 18-256-256-4
 * for the default 512 workgroups) and grows only when a call needs more than every call before it: a graph captured after a warm-up
 * call stays valid.  A caller-given output gradient (gaq_policy_backward_dev) has no wide form.
 *
 * gaq_policy_eval_wide_dev: gaq_policy_eval_ac_dev's contract without the requirement of a value head: logp_out [rows] always,
 *   mean_out [rows, 4] optional, value_out [rows] written when the policy has a value head and NULL when it has none.
 * gaq_policy_grad_ppo_wide_dev: with a value head gaq_policy_grad_ppo_ac_dev's (idx_dev: gaq_policy_grad_ppo_ac_idx_dev's) loss,
 *   outputs and statistics (stats_out [6], [7] with idx_dev).  Without one ret_dev, v_old_dev and grad_value_out_dev must be NULL, the
 *   loss is L_clip - ent_coef H, vclip and vf_coef are checked and unused, and the statistics keep their places (the value loss and
 *   the rows its clip cut: 0).
 * gaq_critic_grad_mse_wide_dev: gaq_critic_grad_mse_dev's (idx_dev: gaq_critic_grad_mse_idx_dev's) contract, stats_out [2] or [3]. */
int gaq_policy_eval_wide_dev(gaq_policy* p, int64_t rows, const float* obs_dev, const float* actions_dev, float* logp_out_dev,
                             float* value_out_dev_or_null, float* mean_out_dev_or_null, void* stream);
int gaq_policy_grad_ppo_wide_dev(gaq_policy* p, int64_t rows, const int32_t* idx_dev_or_null, int64_t src_rows, const float* obs_dev,
                                 const float* actions_dev, const float* logp_old_dev, const float* adv_dev, const float* ret_dev_or_null,
                                 const float* v_old_dev_or_null, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                                 float* grad_out_dev, float* grad_value_out_dev_or_null, float* grad_log_std_out_dev, double* stats_out_dev,
                                 void* stream);
int gaq_critic_grad_mse_wide_dev(gaq_critic* c, int64_t rows, const int32_t* idx_dev_or_null, int64_t src_rows, const float* obs_dev,
                                 const float* target_dev, float scale, float* grad_out_dev, double* stats_out_dev, void* stream);

/* ---- the wide recurrent learner: the sequence passes for a GRU of up to 128 units ------------------------------------------------
 * "gradients of a recurrent policy" above stops at H = 64 because a backward step keeps four delta planes of H rows in LDS.  These two
 * calls work on the cell's units in GROUPS OF 64: per group the gates are recomputed, the group's four planes (4 x min(H, 64) rows)
 * are written, its dW blocks and bias sums go to the partial and its part of W_hh^T [da_r; da_z; dn_h] is accumulated in registers
 * (32 per lane at H = 128).  LDS = 8.25 KiB + 272 B x (in_dim rounded up to 16 + 2 H + max(4 min(H, 64), H + the head widths))
 * (+ 256 B with an index vector): 156 416 B at 18-GRU128-64-64, 156 672 B with idx_dev, under the 163 840 B a workgroup may ask for;
 * at H = 128 the first in_dim refused is 49 (165 120 B).
 * Accepted: a GAQ_POLICY_CELL_GRU policy without an encoder, H a multiple of 16 in [16, 128], 0 to 2 head layers of width <= 64 (tanh
 * or relu), out_tanh 0 or 1, with or without a value head, log_std on the host or in the exploration table, an attached gaq_obs_norm
 * honoured (frozen) where the observation is staged.  Refused with GAQ_ERR_INVALID, each with a text of its own: an LSTM policy (the
 * text names the LSTM), a policy with an encoder ("encoder"), a feed-forward policy, H above 128 or a head layer above 64 (the text
 * names the width), an in_dim whose LDS figure passes 160 KiB (the text names LDS), weights never set.
 * The arithmetic is the narrow calls', in their order: the forward chain of every unit is gru_cell's at every H, so mean, V and h are
 * the rollout's bits; at H <= 64 there is one group and every output of both calls is the narrow call's bits.  The narrow calls keep
 * their limit and their texts.
 * gaq_policy_eval_seq_wide_dev: gaq_policy_eval_seq_dev's arguments and contract (its optional outputs, its h_out rule, its
 *   GAQ_ERR_STATE texts).  One launch.
 * gaq_policy_grad_ppo_seq_wide_dev: gaq_policy_grad_ppo_seq_idx_dev's arguments.  idx_dev = NULL: the call's sequences are the columns
 *   0 .. S - 1 of the inputs, S_src is ignored and stats_out is 6 doubles (gaq_policy_grad_ppo_seq_dev's contract); else sequence s is
 *   column idx_dev[s] of inputs of S_src columns, an index outside [0, S_src) forms no address, contributes exactly 0 and is counted,
 *   and stats_out is 7 doubles.  Loss, branch rules, entropy term, statistics, refusals and their order, determinism and the split
 *   into workgroups are the parents'.  S == 0 writes zeros and launches nothing.  Two launches, no host synchronisation.
 * Scratch: the handle's, with the tape G x T x 64 x H x 4 bytes behind the partials (1.07 GB at G = 512, T = 64, H = 128); the warm-up
 * rule for graphs is unchanged.
 * Not built: the LSTM (its carried dc would have to live in the owning lanes' registers to fit the same LDS), the encoder forms,
 * H > 128, head layers wider than 64.  Every (tile, t) still read-modify-writes the workgroup's whole partial; that traffic bounds
 * the kernel (DESIGN.md 4a "The wide recurrent learner"). */
int gaq_policy_eval_seq_wide_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs_dev, const float* actions_dev_or_null,
                                 const uint8_t* done_dev, const float* h0_dev, float* logp_out_dev_or_null, float* value_out_dev_or_null,
                                 float* mean_out_dev_or_null, float* h_out_dev_or_null, void* stream);
int gaq_policy_grad_ppo_seq_wide_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx_dev_or_null, int64_t S_src, const float* obs_dev,
                                     const float* actions_dev, const uint8_t* done_dev, const float* h0_dev, const float* logp_old_dev,
                                     const float* adv_dev, const float* ret_dev_or_null, const float* v_old_dev_or_null, float clip_eps,
                                     float vclip, float vf_coef, float ent_coef, float scale, float* grad_out_dev,
                                     float* grad_value_out_dev_or_null, float* grad_log_std_out_dev, double* stats_out_dev, void* stream);

/* ---- the optimiser on the device: Adam / AdamW that steps a handle's weights in place ------------------------------------------
 * The stage behind the gradient calls: it takes their output buffers as they are, clips them by their global norm and steps the
 * handle's own weights where the rollout and gradient kernels read them, enqueued on `stream` with no host synchronisation and no
 * allocation after creation.  Additive like the sections above: GAQ_ABI_VERSION and every existing struct stay as they are.
 * Parameter groups, fixed at creation: the packed weights (the handle's weight count, any layout: the step is elementwise); the
 * value head, W + 1 floats, if the policy has one at creation; log_std, 4 floats, if GAQ_OPTIM_STEP_LOG_STD is set and the policy
 * explores.  Accepted: every policy and critic whose live weights are the fp32 packed buffer alone -- VALU, fp32 MFMA, GRU and LSTM
 * policies and gaq_critic.  The bf16 engine is GAQ_ERR_INVALID (the text names the engine: its repacked fragments would go stale);
 * weights never set: GAQ_ERR_INVALID.  The optimiser keeps the handle's address: destroy the optimiser first.
 * The pointers it steps never move: a handle's packed weight buffer is allocated when the handle is created and its value-head
 * buffer by the first gaq_policy_set_value_head[_dev]; no later gaq_*_set_weights*, gaq_policy_set_value_head* or
 * gaq_policy_set_explore call re-allocates either (they copy into the same buffers), so a captured step stays valid across them.
 * One step, with t = steps taken + 1 and g' = coef g:
 *   m = m + (1 - beta1) (g' - m),  v = beta2 v + (1 - beta2) g'^2,
 *   theta = theta (1 - lr weight_decay) - [lr / (1 - beta1^t)] m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * -- torch.optim.AdamW's single-tensor form (Adam's at weight_decay 0); the decay is decoupled and never applies to log_std.
 * coef = min(1, max_grad_norm / (norm + 1e-6)) (torch's clip_grad_norm_; max_grad_norm 0: coef = 1), norm the L2 norm over all the
 * groups together.  beta^t, the two corrections and coef are formed in fp64 on the device and rounded once; the elements are fp32.
 * The step count, lr and the other hyper-parameters live in device memory, not in kernel arguments: a captured step advances t at
 * every replay, and gaq_optim_set_lr_dev between replays takes effect without a new capture.
 * A squared norm that is not finite skips the step: theta, m, v and t keep their bits and the skipped counter goes up by one.
 * stats_out (NULL: none), 4 doubles: the norm before clipping, the coef applied (0 for a skipped step), the step count after the
 * call, 1 if the step was skipped else 0.
 * Determinism: the squared norm is a sum of fp64 partials, one per chunk of 2048 consecutive elements of the concatenated groups,
 * each from a fixed tree and added in ascending order -- a function of the group sizes alone, no atomics; the same inputs on the same
 * state give the same bits, eagerly and in replay, on any stream.  Two launches (GAQ_OPTIM_LAUNCHES=1 at creation, a measurement
 * switch: one launch of one workgroup, with its own fixed order).
 * log_std of a DEVICE-mode policy ("log_std on the device" above; the mode at creation counts): the third group IS the table's
 * log_std[4] -- no master copy -- and the lane that steps element k publishes std[k] = (float)exp((double)x) and inv_std[k] =
 * (float)exp(-(double)x) beside it in the same launch, in both launch forms; a skipped step leaves the 12 words their bits.  The
 * policy's next launch on the stream, captured or not, uses the new exploration scale with no host synchronisation: a graph of a
 * gradient call + gaq_optim_step_dev learns log_std.  gaq_optim_sync_log_std is GAQ_OK and does nothing (no wait);
 * gaq_optim_get_log_std reads the table (it waits for the device).  Nothing is owned: a gaq_policy_set_explore with new values between
 * steps is what the next step steps, the moments kept; NULL (deterministic) makes gaq_optim_step_dev return GAQ_ERR_STATE.
 * Registering or unregistering a table after the optimiser was created: GAQ_ERR_STATE from gaq_optim_step_dev and
 * gaq_optim_sync_log_std, like a value head added or removed.  The rest of this paragraph is HOST mode.
 * log_std: the rollout and gradient kernels take log_std by value from the host copy in the handle, so the optimiser steps a device
 * master copy, initialised from the handle at creation.  Until gaq_optim_sync_log_std the handle's kernels use the OLD log_std.  That
 * call waits for `stream`, reads the 16 bytes and calls gaq_policy_set_explore: the one synchronous call of a minibatch; it cannot be
 * captured in a graph.  (GAQ_OK and nothing done when the optimiser steps no log_std.)
 * A CAPTURED launch keeps the log_std it was captured with: gaq_policy_logp_dev, the gaq_policy_grad_* calls and the rollouts put
 * log_std into their kernel arguments when they are enqueued, so a graph that holds one replays with the log_std of capture time
 * whatever gaq_optim_sync_log_std or gaq_policy_set_explore do later.  A graph of a gradient call + gaq_optim_step_dev is therefore
 * right with an optimiser that steps no log_std (flags 0: log_std stays what it was at capture); with one that does, capture it again
 * after every gaq_optim_sync_log_std -- otherwise the replayed gradients are those of the old log_std while the master copy moves on.
 * An optimiser that steps log_std owns it: if gaq_policy_set_explore has since been called with other values, or with NULL, the
 * device copy has not seen that, and gaq_optim_step_dev and gaq_optim_sync_log_std return GAQ_ERR_STATE (nothing launched, nothing
 * overwritten) until the policy's log_std is again what gaq_optim_get_log_std returns; create a new optimiser to change it.
 * gaq_optim_step_dev is refused, nothing launched, the handle stays usable: a NULL or misaligned grad (4 bytes; stats_out 8):
 * GAQ_ERR_INVALID; grad_value given while the optimiser steps no value head, or missing while it steps one: GAQ_ERR_INVALID;
 * grad_log_std missing while it steps log_std: GAQ_ERR_INVALID (it is ignored otherwise); a value head added or removed since
 * creation: GAQ_ERR_STATE.  Creation refuses (GAQ_ERR_INVALID): a struct_size mismatch, beta outside [0, 1), eps <= 0, a negative or
 * non-finite lr, weight_decay or max_grad_norm, unknown flags.
 * State (checkpoints; synchronous, they wait for the device): m and v are gaq_optim_state_count floats each, the groups concatenated
 * -- weights, head, log_std; any pointer may be NULL (left out).  The weights themselves now live in the handle:
 * gaq_policy_get_weights, gaq_policy_get_value_head (GAQ_ERR_STATE without one) and gaq_critic_get_weights copy them to the host in
 * the layout the setters take (synchronous, after everything enqueued on the device).  A handle is not thread-safe. */
typedef struct gaq_optim gaq_optim;
#define GAQ_OPTIM_STEP_LOG_STD 1u
typedef struct {
  uint32_t struct_size;   /* = sizeof(gaq_optim_desc) */
  uint32_t flags;         /* GAQ_OPTIM_STEP_LOG_STD */
  double lr, beta1, beta2, eps;
  double weight_decay;    /* decoupled (AdamW); 0: Adam */
  double max_grad_norm;   /* 0: no clipping */
} gaq_optim_desc;
int gaq_optim_create_policy(gaq_policy* p, const gaq_optim_desc* desc, gaq_optim** out);
int gaq_optim_create_critic(gaq_critic* c, const gaq_optim_desc* desc, gaq_optim** out);
int gaq_optim_destroy(gaq_optim* opt);
int64_t gaq_optim_state_count(const gaq_optim* opt);
int gaq_optim_step_dev(gaq_optim* opt, const float* grad_dev, const float* grad_value_dev_or_null, const float* grad_log_std_dev_or_null,
                       double* stats_out_dev_or_null, void* stream);
/* The optimiser of a recurrent policy WITH an encoder (gaq_policy_create_rnn_enc), which gaq_optim_create_policy refuses: everything
 * above, with the encoder's block (gaq_policy_encoder_weight_count floats, the packed layout of gaq_policy_set_encoder_weights) as a
 * FOURTH group placed after log_std.  Groups 0 .. 2 keep their indices; m and v are the four groups concatenated in that order
 * (gaq_optim_state_count, gaq_optim_get_state and gaq_optim_set_state cover all four).  The norm and the clip are joint over all
 * groups; weight decay applies to the encoder as to the weights.  The block is stepped in place where the rollout's encoder kernel
 * and the gradient passes read it, so rollout -> ... -> gaq_policy_grad_ppo_enc_seq[_idx]_dev -> gaq_optim_step_enc_dev closes on the
 * device and can be captured in a graph; device-mode log_std (gaq_policy_set_explore_dev) works as for the other policies.
 * grad_enc_dev is gaq_policy_grad_ppo_enc_seq_dev's grad_enc_out_dev.  GAQ_ERR_INVALID: a policy without an encoder (the text says
 * "encoder"), encoder weights or weights never set, gaq_optim_step_dev on such an optimiser or gaq_optim_step_enc_dev on another.
 * Additive: GAQ_ABI_VERSION stays 5. */
int gaq_optim_create_policy_enc(gaq_policy* p, const gaq_optim_desc* desc, gaq_optim** out);
int gaq_optim_step_enc_dev(gaq_optim* opt, const float* grad_dev, const float* grad_enc_dev, const float* grad_value_dev_or_null,
                           const float* grad_log_std_dev_or_null, double* stats_out_dev_or_null, void* stream);
int gaq_optim_set_lr_dev(gaq_optim* opt, double lr, void* stream);
int gaq_optim_sync_log_std(gaq_optim* opt, void* stream);
/* the master log_std as gaq_optim_sync_log_std last read it (at creation: the handle's), from the host: no device access
 * (a device-mode policy's: the table's log_std, read after everything enqueued on the device).
 * GAQ_ERR_STATE when the optimiser steps no log_std */
int gaq_optim_get_log_std(const gaq_optim* opt, float* log_std4_host);
int gaq_optim_get_state(gaq_optim* opt, uint64_t* step_or_null, uint64_t* skipped_or_null, float* m_host_or_null, float* v_host_or_null);
int gaq_optim_set_state(gaq_optim* opt, const uint64_t* step_or_null, const uint64_t* skipped_or_null, const float* m_host_or_null,
                        const float* v_host_or_null);
int gaq_policy_get_weights(gaq_policy* p, float* packed_host);
int gaq_policy_get_value_head(gaq_policy* p, float* w_then_bias_host);
int gaq_critic_get_weights(gaq_critic* c, float* packed_host);

/* ---- return normalisation: rewards over the running standard deviation of the discounted return, on the device ----------------
 * The other half of SB3's VecNormalize (norm_reward) and gymnasium's NormalizeReward: each env keeps a running discounted return, its
 * running variance scales the rewards, and the result is clamped to +-clip.  A normaliser belongs to one env; N is that env's.
 * State (device, fp64): R[N], the running discounted return of each env, zero at first; count, mean, M2 (scalars) of every return seen;
 *   the population variance is M2 / count; before any update count = 0, mean = 0 and the variance is defined as 1.
 * Update over reward [T, N] (fp32) and done [T, N] (uint8) as a rollout wrote them: for each env i, for t = 0 .. T-1 in ascending order,
 *   R_i = gamma * R_i + (double)reward[t, i] in fp64 -- the product and the sum rounded separately (no fma), gamma the fp32 argument
 *   widened to double, so a NumPy fp64 loop reproduces R bit for bit.  R_i then enters the statistics as one sample, and if done[t, i]
 *   is set R_i = 0 afterwards: VecNormalize.step_wait's order (the return that includes an episode's last reward is a sample, then the
 *   carry is cleared).  The T N samples are summed in fp64 shifted by a value common to all of them (the running mean; the batch's first
 *   reward before the first update) and merged into (count, mean, M2) with Chan's merge in a fixed order, no atomics: the same input on
 *   the same state gives the same bits.  M2 is accurate relative to n max|R - shift|^2, not to n range^2: with the shift far from the
 *   samples (returns loaded beside count = 0, or a jump of the return level since the last update) a lane loses about
 *   u (Delta / sigma)^2 relative; measured over all lanes, 1e-4 for returns of 1e5 +- 1e-2 shifted by 1e3.  The update then
 *   publishes the table.
 * Published table (device, fp32, fixed address): inv_std = (float)(1 / sqrt(var + eps)) -- the division, the root and the reciprocal in
 *   fp64, one rounding to fp32 -- and clip.  Only the last launch of an update and gaq_ret_norm_set_stats write it.
 * One element (gaq_ret_norm_apply_dev, the only place it exists): fminf(fmaxf(r * inv_std, -clip), clip) in fp32.  The mean is NOT
 *   subtracted (VecNormalize does not subtract it either); it is kept because it is part of the RunningMeanStd state users import and
 *   export.  With fresh statistics and clip = +inf it is the identity on every fp32 value, -0 included (for every eps whose
 *   1 / sqrt(1 + eps) rounds to 1.0f; SB3's 1e-8 does).
 * Statistics are fixed within a rollout: nothing inside gaq_step_policy_*_many_dev touches them, and the caller chooses whether apply runs
 *   before or after update.  This differs from SB3, which updates at every step and normalises that step's rewards with statistics that
 *   already include it; here a whole [T, N] window is normalised with one table.
 * LIFETIME: destroy it before its env.  A handle is not thread-safe: one update at a time (they share R and the partial sums), and an
 *   update, reset_returns_dev or apply on another stream than the previous one is the caller's to order.
 * Every refusal below is GAQ_ERR_INVALID, names the argument in gaq_last_error, launches nothing and leaves the handle usable.
 * update_dev, apply_dev and reset_returns_dev allocate nothing after create and never wait for the host. */
typedef struct gaq_ret_norm gaq_ret_norm;
/* gamma in [0, 1]; eps >= 0 (finite); clip > 0, +inf allowed (no clamp) */
int gaq_ret_norm_create(gaq_env* env, float gamma, float eps, float clip, gaq_ret_norm** out);
/* The update above over reward [T, N] and done [T, N] (device; reward 4-byte aligned; T >= 1): one lane per env, 5 bytes per env-step.
 * Two launches on `stream`. */
int gaq_ret_norm_update_dev(gaq_ret_norm* n, int32_t T, const float* reward_dev, const uint8_t* done_dev, void* stream);
/* out[i] = the element expression of reward[i], i < count (any count >= 0: the rewards of any shape); out may be reward (in place),
 * but may not overlap it otherwise.  Both 4-byte aligned.  One launch on `stream`. */
int gaq_ret_norm_apply_dev(gaq_ret_norm* n, int64_t count, const float* reward_dev, float* out_dev, void* stream);
/* R[i] <- 0 where mask[i] (N bytes, device) is non-zero, every R for NULL: for envs the caller resets outside a rollout.  Enqueued. */
int gaq_ret_norm_reset_returns_dev(gaq_ret_norm* n, const uint8_t* mask_dev_or_null, void* stream);
/* synchronous (they wait for the device): read / replace the statistics (count >= 0, M2 >= 0, all finite, the mean finite as an fp32 too);
 * set_stats republishes the table */
int gaq_ret_norm_get_stats(gaq_ret_norm* n, double* count, double* mean, double* m2);
int gaq_ret_norm_set_stats(gaq_ret_norm* n, double count, double mean, double m2);
/* synchronous: read / replace R (N doubles on the host; finite) -- with the statistics, the whole state a checkpoint needs */
int gaq_ret_norm_get_returns(gaq_ret_norm* n, double* host_N);
int gaq_ret_norm_set_returns(gaq_ret_norm* n, const double* host_N);
int gaq_ret_norm_destroy(gaq_ret_norm* n);

/* ---- advantage standardisation: (A - mean(A)) / (std(A) + eps) with the statistics of the batch itself, on the device -----------
 * What rl_games and SB3 compute before the PPO loss.  Nothing runs between calls: the handle owns only the partial sums, a three-word
 * fp64 state (count, mean, M2 of the last batch) and the published fp32 table (mean, inv).
 * Moments: one streaming fp64 pass shifted by the batch's first element (the observation normaliser's pass at D = 1), the workgroup
 *   split a function of count alone, Chan's merge in ascending order, no atomics: the same input gives the same bits, and a batch of
 *   equal values has M2 = 0 exactly.
 * Table: mean rounded to fp32; inv = 1 / (sqrt(M2 / (count - ddof)) + eps) -- the division, the square root and the reciprocal in fp64,
 *   one rounding each, then one to fp32.  eps is added to the standard deviation, not to the variance; ddof = 1 is torch.std's default.
 * One element: out[i] = (adv[i] - mean) * inv in fp32, two roundings.  A batch of equal values gives +0 everywhere (for eps > 0).
 * Every refusal below is GAQ_ERR_INVALID, launches nothing and leaves the handle usable.  A handle is not thread-safe. */
typedef struct gaq_adv_norm gaq_adv_norm;
/* eps >= 0 (finite); ddof 0 or 1 */
int gaq_adv_norm_create(gaq_env* env, float eps, int32_t ddof, gaq_adv_norm** out);
/* Standardise adv[0 .. count) (fp32, device, 4-byte aligned: any slice of a larger buffer) into out; out may be adv (in place), but may
 * not overlap it otherwise.  count >= 1 + ddof, and at most (2^31 - 1) * 1024.  Three launches on `stream`, no host synchronisation. */
int gaq_adv_norm_apply_dev(gaq_adv_norm* n, int64_t count, const float* adv_dev, float* out_dev, void* stream);
/* synchronous (waits for the device): count, mean and M2 of the last batch (zeros before the first) */
int gaq_adv_norm_get_stats(gaq_adv_norm* n, double* count, double* mean, double* m2);
int gaq_adv_norm_destroy(gaq_adv_norm* n);

/* GAQ_NOISE_INPUT: normals for the NEXT step, layout [sim_steps][4][N] float32 (device pointer,
 * must stay valid until that step has run).  Stands in for numpy.random.randn inside OUNoise.noise
 * (quad_utils.py:197-201) so that noisy trajectories can be compared bit-for-bit in structure. */
int gaq_set_noise_input_dev(gaq_env* env, const float* normals_dev);

/* gaq_config.sense_input: the standard draws of the NEXT step's three SensorNoise.add_noise calls (quadrotor.py:946, :970,
 * :988; a reset or gaq_observe makes one call and reads call index 2), layout [3 calls][12 slots][3][N] float32, device
 * pointer valid until that step has run.  Slots in the order the reference draws them (sensor_noise.py:116-157): 0 pos normal,
 * 1 pos uniform, 2 vel normal, 3 vel uniform, 4 gyro normal (bias model: the bias increment), 5 gyro white normal (bias model
 * only), 6 quat normal, 7 quat uniform, 8 acc static normal, 9 acc proportional normal; then the state function's own
 * draws, first column only: 10 the t2w normal, 11 the t2t normal (get_state.py:335, :375).  Normals are N(0,1), uniforms U(0,1). */
int gaq_set_sense_input_dev(gaq_env* env, const float* draws_dev);

/* see gaq_config.action_f32 */
int gaq_set_action_dtype(gaq_env* env, int32_t is_float32);

/* gaq_config.aux_outputs: per env [accelerometer 3 | omega_dot 3 | torque 3 | controller.action 4 | thrust_cmds_damp 4] of the
 * most recent step (info["obs_comp"] entries acc, omega_dot, torque, act_clipped, act_filtered; quadrotor.py:994-1006). */
#define GAQ_AUX_WORDS 17
int gaq_get_aux(gaq_env* env, float* host_out /* [N, GAQ_AUX_WORDS] */);

/* Full state exchange (teacher forcing, checkpoint/resume, tests).  Host buffer of
 * GAQ_STATE_PLANES planes of N doubles, plane-major:
 *   0-2 pos, 3-5 vel, 6-14 rot (row-major), 15-17 omega, 18-21 thrust_rot_damp,
 *   22-25 thrust_cmds_damp, 26-29 OU state, 30-33 previous action, 34-36 goal,
 *   37 tick, 38 SVD counter (sub-steps since the last re-orthonormalisation),
 *   39-41 gyro bias of the sensor-noise model (SensorNoise.gyro_bias, sensor_noise.py:98). */
#define GAQ_STATE_PLANES 42
int gaq_get_state(gaq_env* env, double* host_planes);
int gaq_set_state(gaq_env* env, const double* host_planes);

/* Observation of the current state without stepping (state_vector(self), quadrotor.py:1143). */
int gaq_observe(gaq_env* env, float* obs_out);

/* Rollout bookkeeping around step() (the loops of quadrotor.py:1278-1305, :1424-1428; `traj_count` :990).
 * - terminal observations: with auto_reset the row returned with done=1 belongs to the NEW episode; when a buffer
 *   [N,obs_dim] is registered here, the last observation of the finished episode (what the reference returns with
 *   done=True; every termination on this path is a time-limit truncation) is written to that env's row in the same
 *   launch.  Rows of envs that did not finish are left untouched.  NULL unregisters.
 * - episode tracking: per-env running return and length on the device; gaq_episode_stats returns (and optionally
 *   clears) the totals over the episodes finished so far. */
int gaq_set_terminal_obs_dev(gaq_env* env, float* term_obs_dev);
int gaq_track_episodes(gaq_env* env, int32_t enabled);
int gaq_episode_stats(gaq_env* env, int64_t* episodes, double* return_sum, double* length_sum, double* return_sqsum,
                      int32_t clear);

/* compact_done: indices (local) of the envs that reported done in the last step. */
int gaq_done_list(gaq_env* env, uint32_t* idx_out, int64_t capacity, int64_t* count_out);

/* Multi-GPU return path ("pack [obs, reward, done] into the same buffer as a 20-word row to keep it a single
 * collective"): rows_dev[i] = [obs[i, 0..D-1], reward[i], (float)done[i]], i.e. [N, obs_dim + 2] float32 row-major.  One
 * small launch on `stream`; the caller then issues ONE gather of the packed rows (gym_art_amd/sharding.py). */
int gaq_pack_rows_dev(gaq_env* env, const float* obs_dev, const float* reward_dev, const uint8_t* done_dev, float* rows_dev,
                      void* stream);

/* The same rows WITHOUT the extra launch: once a buffer [N, obs_dim + 2] is registered here, every gaq_step_dev call also leaves the
 * packed rows of its outputs in it -- for the split-state kernels whose observation is the state's heads (obs_state_alias 1 / 2 with the
 * 18-word observation: BASELINE config 4's shards) assembled in the step kernel's LDS buffer and stored with the launch's other 16-byte
 * pieces, for every other configuration by the pack launch, enqueued by gaq_step_dev itself: bit for bit what gaq_pack_rows_dev makes of
 * obs / reward / done either way.  The step's ordinary outputs are still written.  NULL unregisters.  Not honoured by the fused
 * rollouts of gaq_step_many_dev (it then steps one launch at a time). */
int gaq_set_packed_rows_dev(gaq_env* env, float* rows_dev_or_null);

/* number of envs whose reward was non-finite since the last call (clears the counter) */
int gaq_nan_count(gaq_env* env, int64_t* count_out);

/* HIP-graph capture.  The *_dev entry points only enqueue kernels, so they can be captured (e.g. inside
 * torch.cuda.graph together with the policy).  By default the step index that keys the noise / reset random streams
 * is a host counter passed by value -- a captured launch would replay the same draws.  With graph-safe mode on, the
 * index lives in device memory, so every replay is a new step.  At small batches (where a launch is latency: up to two waves per
 * SIMD) the split-state kernels advance it THEMSELVES -- every wave checks in with one non-returning atomic after reading it: ONE graph
 * node per step and nothing waits; larger batches and every other kernel are followed by a one-thread launch.
 * Alias layout: capture with the observation buffer used in place (same tensor in and out of every captured step). */
int gaq_set_graph_safe(gaq_env* env, int32_t enabled);

/* Uniform tick / SVD counters.  `done` is tick > ep_len and nothing else, so the envs of a handle that were created or fully reset
 * together carry the same counter word (tick | svd_ctr << 16) until the caller desynchronises them: gaq_set_state, a masked reset.  While
 * that holds, gaq_step_dev passes the word to its launch as an argument and the launch neither reads nor writes the 4-byte-per-env counter
 * plane; every other entry point that looks at the counters writes the word into the plane first, and from then on the plane counts.  An
 * unmasked gaq_reset / gaq_reset_dev returns the handle to the argument path where the library still knows every env's svd_ctr.  Results do
 * not depend on any of this.  Not used in graph-safe mode, nor by handles with per_env_params, nor under GAQ_UNIFORM_CTR=0 (read by
 * gaq_create, for the life of the handle).
 * Test infrastructure: valid_out = 1 while the next gaq_step_dev would take the argument path; word_out = the word the library keeps
 * (meaningful in its upper half while it knows svd_ctr); guard_intact_out = 1 while the words the library keeps behind the counter plane
 * still hold their pattern, i.e. nothing has written past the plane's ntiles * 64 words (waits for the handle's work).  Any may be NULL. */
int gaq_uniform_counters(gaq_env* env, int32_t* valid_out, uint32_t* word_out, int32_t* guard_intact_out);

/* Device time (ms, HIP events on the launch stream) of the most recent gaq_step*_dev /
 * gaq_step call's kernel(s); used by bench.py for the roofline figure. */
int gaq_last_kernel_ms(gaq_env* env, float* ms_out);
int gaq_set_timing(gaq_env* env, int32_t enabled);

/* Measurement aid (bench.py roofline.peak_measured; SURVEY 8d "also measure an on-box copy kernel"): copy `bytes` (a multiple of 16) from
 * src to dst on the current device with the access shape of the step kernels' streaming traffic -- one 16-byte load and one 16-byte store
 * per lane -- asynchronously on `stream`.  2 x bytes / time is the bandwidth the step kernels' layout can reach on THIS box. */
int gaq_hbm_copy_dev(void* dst_dev, const void* src_dev, size_t bytes, void* stream);

int gaq_synchronize(gaq_env* env);
/* the handle's private hipStream_t (used by the host-pointer entry points) */
void* gaq_stream(gaq_env* env);

/* ---- one batch over several devices, ONE process (BASELINE config 4 for a plain-C caller; SURVEY 8b `device_ids`, 8e "single process,
 * one stream per device").  The reference loop `reset(); while not done: step()` (quadrotor.py:1278-1305, :1424-1428) stays one
 * call per step: the batch of cfg->num_envs envs is cut into contiguous shards of whole 64-env tiles (and whole swarm worlds), shard k
 * lives on device_ids[k] as an ordinary gaq_env with env_id_offset = cfg->env_id_offset + first_k -- the random streams are keyed by the
 * GLOBAL env index, so results do not depend on the sharding, bit for bit -- and every call fans out over the shards' own streams:
 *   actions [N,4] on device_ids[0] --(peer copy of each remote shard's slice)--> step launch per shard --(peer copy of the shard's
 *   obs / reward / done slices)--> the caller's [N, ...] tensors on device_ids[0].
 * Shards that live on device_ids[0] itself read and write the caller's tensors in place (no copy).  A device may be listed more than
 * once (its shards then share it: how a one-GPU box tests this).  `stream` is a stream of device_ids[0]; the call is asynchronous on
 * it like gaq_step_dev: work of the other devices is ordered after what `stream` held at the call and `stream` continues after it.
 * cfg->device is ignored; every other field means what it means for gaq_create.  Per-shard settings (parameters, randomizer, state
 * exchange, graph-safe mode ...) go through the shard handles: gaq_sharded_shard(). */
typedef struct gaq_sharded gaq_sharded;
int gaq_create_sharded(const gaq_config* cfg, const int32_t* device_ids, int32_t num_devices, gaq_sharded** out);
/* the same over handles the caller made (shard k = envs[k], consecutive global ranges: env_id_offset of shard k+1 = that of shard k + its
 * num_envs; same observation width; every shard but the last a multiple of 64 envs).  The handles stay the caller's: destroy them
 * AFTER the sharded handle.  (gym_art_amd.QuadrotorEnv(device_ids=[...]) builds its shards as Python envs and steps them through this.) */
int gaq_sharded_from_handles(gaq_env* const* envs, int32_t num_shards, gaq_sharded** out);
int gaq_destroy_sharded(gaq_sharded* s);
int gaq_sharded_num_shards(const gaq_sharded* s);
gaq_env* gaq_sharded_shard(gaq_sharded* s, int32_t k);                 /* borrowed */
int gaq_sharded_range(const gaq_sharded* s, int32_t k, int64_t* first, int64_t* count, int32_t* device);
int64_t gaq_sharded_num_envs(const gaq_sharded* s);
/* the split gaq_create_sharded makes of n envs over `num_shards` shards (pure host arithmetic: no device needed): whole 64-env tiles,
 * rounded up to `align` envs (swarm agents per world, 1 otherwise), the first shards one unit larger */
int gaq_shard_range(int64_t n, int32_t num_shards, int32_t k, int32_t align, int64_t* first, int64_t* count);
/* QuadrotorEnv.reset() / step() of the whole batch; device pointers on device_ids[0], asynchronous on `stream` */
int gaq_reset_sharded_dev(gaq_sharded* s, const uint8_t* mask_dev_or_null, float* obs_dev, void* stream);
int gaq_step_sharded_dev(gaq_sharded* s, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);
/* ... and with host pointers (synchronous; staged through device_ids[0]) */
int gaq_reset_sharded(gaq_sharded* s, const uint8_t* mask_or_null, float* obs_out);
int gaq_step_sharded(gaq_sharded* s, const float* actions, float* obs, float* reward, uint8_t* done);
int gaq_synchronize_sharded(gaq_sharded* s);

#ifdef __cplusplus
}
#endif
#endif /* GAQ_H */
