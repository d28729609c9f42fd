// gaq_host.hpp -- what the host units of libgaq share: gaq.hip (the env core: the small kernels, kernel selection, the launch logic and the
// env C ABI), gaq_params.hip (the per-env parameter pipeline and its entry points), gaq_policy.hip (the device-policy engines and every
// gaq_policy_* entry point), gaq_policy_grad.hip (the learner's forward and backward passes over stored rows), gaq_optim.hip (Adam on the
// device), gaq_learn.hip (GAE and the two running normalisers) and gaq_sharded.hip (one batch over several devices).
// Internal to csrc/: none of it is part of the C ABI (include/gaq.h).  The functions declared here are defined in gaq.hip or, where it says
// so, in gaq_params.hip, and have hidden visibility: they add nothing to what the library exports.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "gaq_kernels.hpp"
#include "../../include/gaq.h"

using namespace gaqk;   // (the five units are written in terms of gaq_kernels.hpp: StepCfg, DevPtrs, kTile ...)

// (an anonymous namespace in a header, on purpose: the params_*_kernel passes of gaq_params.hip take it by value, and its linkage is part
//  of their mangled names, which the recorded profiles key on.  A plain aggregate, the same in every unit.)
namespace {
struct Randomizer {           // gaq_randomizer, by value in the launch arguments (660 B)
  int32_t sampler, every;
  double ratio[gaq::TL_COUNT];
  gaq::ParamTree base;
};
}  // namespace

// What an env's parameters bring, one byte per env (gaq_env::pflags); the handle-wide counts of each bit feed the kernel selection
enum ParamFlag : uint8_t { PF_LAG = 1, PF_DRAG = 2, PF_NONCOMPACT = 4, PF_DAMP = 8 };   // motor lag, rotor drag, not compact-constructible, vel / omega damping
inline uint8_t param_flags(double tau_up, double tau_down, double c_drag, double c_roll, bool compact_ok, double vel_damp, double damp_q) {
  return (uint8_t)((!(tau_up >= 1.0 && tau_down >= 1.0) ? PF_LAG : 0) | ((c_drag != 0.0 || c_roll != 0.0) ? PF_DRAG : 0) |
                   (!compact_ok ? PF_NONCOMPACT : 0) | ((vel_damp != 0.0 || damp_q != 0.0) ? PF_DAMP : 0));
}

// The environment switches that take part in the kernel choice (gaq.hip: kernel selection), read once per handle: GAQ_FORCE_GENERIC=1 (tests:
// generic vs specialised), GAQ_NO_AUXP=1, and the measurement overrides of the small-batch rule GAQ_PREDRAW / GAQ_NT (1, 0; -1 unset: by size)
struct Overrides { bool force_generic = false, no_auxp = false; int predraw = -1, nt = -1; bool uniform_ctr = true; };   // (GAQ_UNIFORM_CTR=0: no part in the choice)

// What the host knows of the handle's tick / SVD counters (quad_core.hpp: uniform counters; gaq.hip: counters_to_plane).
//   svd_known: every env's svd_ctr is word >> 16.  It counts sub-steps whatever the episode clocks do, so it survives masked resets.
//   valid:     every env's whole counter word is `word`, and the counter plane is stale: step launches take the word as an argument.
// valid implies svd_known.  Handles with per-env parameters (whose passes clear single envs' svd_ctr) never set either.
struct UniformCtr { bool eligible = false, valid = false, svd_known = false; uint32_t word = 0; };

struct gaq_env {
  gaq_config cfg;
  StepCfg sc;
  Model<double> um;
  DevPtrs d;
  int obs_dim = 18;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timing = false, timed = false;
  uint64_t reset_calls = 0;
  const float* noise_next = nullptr;
  uint32_t noted_step = 0xFFFFFFFFu, noted_roll = 0xFFFFFFFFu, noted_proll = 0xFFFFFFFFu;   // last masks handed to launch_record()
  int lds_raised_for = -1; bool reset_lds_raised = false;   // hipFuncAttributeMaxDynamicSharedMemorySize already raised
  hipStream_t user_stream = nullptr;   // the stream of the most recent *_dev call (NULL = HIP's legacy default stream)
  bool user_stream_used = false;
  const float* sense_next = nullptr;   // gaq_set_sense_input_dev: draws of the next step / reset
  std::vector<double> host_par;   // [ntiles][kPar][64] staging for per-env params
  bool dev_params = false;        // the parameters are managed on the device (randomizer / gaq_set_param_trees): host_par is stale
  bool rz_on = false;             // gaq_set_randomizer installed
  bool cold_stale = false;        // an F_RZ launch has promoted envs with the hot planes only: the other planes of those envs are behind
                                  // their resample count (device word per env: pfull_of) until somebody writes them whole again
  int rz_since_refill = 0;        // step launches since the last refill pass of the staged parameter planes
  bool rz_refill_now = false;     // run the refill pass before the next step launch (ticks may have been set by the caller)
  Randomizer rz;
  std::vector<uint8_t> pflags;    // per env: ParamFlag bits
  int64_t cnt_lag = 0, cnt_drag = 0, cnt_noncompact = 0, cnt_damp = 0;   // envs with each flag set
  bool any_lag = false, any_drag = false;
  Overrides ov;           // as the environment had them at gaq_create
  UniformCtr uni;
  bool ctr_spread = false;  // graph-safe mode: F_CTR launches have left check-ins in the counter's words beyond the first
  int num_cus = 256;      // compute units of the device (hipDeviceProp_t::multiProcessorCount): the small-batch size rule counts waves per SIMD
  int variant = 0;        // gaq::Feature mask of the step kernel in use
  int lds_per_wave = 0;   // bytes of LDS each wave of the step kernel uses
  bool needs_generic = false;
  bool fused_rollout = true;     // gaq_step_many_dev uses the fused T-step kernel when it can (GAQ_NO_FUSED=1 disables)
  bool alias = false;     // obs_state_alias in effect: state head lives in the observation tensor `last_obs`
  bool pack = false;      // split state (alias) whose observation is NOT the heads: packed explicitly (F_PACK); implies shadow
  bool shadow = false;    // obs_state_alias == 2: split state with LIBRARY-owned heads (own_obs); the caller's tensor gets a copy
  bool check_alias = false;       // GAQ_CHECK_ALIAS=1 (debug): checksum the aliased observation rows after every launch and
  uint64_t* alias_sum_dev = nullptr;   // verify them before the next one (the caller must not have modified them)
  uint64_t alias_sum = 0; bool alias_sum_valid = false;
  bool lomix = false;     // alias layout with the mixed residual rows (omega exact): per-env parameters or a model with motor lag
  bool fp32 = false;      // fp32_state in effect (implies alias): fp32 arithmetic, the observation rows are the whole state
  float* own_obs = nullptr;      // [n][18] library-owned observation buffer (host-pointer entry points, set_state)
  const float* last_obs = nullptr;  // where the previous step / reset wrote the observation
  const float* cur_obs = nullptr;   // the caller's device buffer the last step / reset wrote the observation to (every layout; nullptr =
                                    // none that outlives the call): the input of a closed-loop rollout's first policy evaluation
  uint64_t* step_ctr_mem = nullptr; // device word behind DevPtrs::step_ctr (allocated at create, used in graph-safe mode)
  // Staging of the host-pointer step (gaq.hip: ensure_stage, transport_of, mirror_info, export_state), allocated by the first gaq_step and kept.
  // The stage is one block [actions 16n | reward 4n | done n | pad | obs 4 D n]; its size decides, once, how a call's arrays travel:
  //   mapped    stage <= 1 MiB: stage_pin is mapped host memory and stage_map the device's address of it.  The launch reads and writes
  //             the host's block itself: no copy (but the observation's, when the launch has to write it to own_obs)
  //   pinned    the same sizes under GAQ_ZERO_COPY=0 (read by that first step), or when the runtime gave no device address:
  //             stage_pin -> stage_dev, the launch, stage_dev -> stage_pin in one or two copies
  //   pageable  larger stages: no stage_pin; the caller's actions -> stage_dev, the launch, three copies to the caller's arrays
  // The info mirror: on the two staged transports an info-dict handle (aux_outputs) also brings the exported state planes and the aux rows
  // home in the step's one synchronisation, so that the gaq_get_state + gaq_get_aux that build the info dict (quadrotor.py:993-1028) cost
  // no further round trip.  info_pin is [42][n] doubles, then the aux rows; mapped (info_map) iff the stage is, and then written by
  // export_kernel itself, else filled by two copies from export_dev and the aux rows.  info_valid: the mirror describes the state -- until
  // the next launch or upload that changes it; every such path clears the flag.  Pageable handles never set it: the getters read the device.
  char* stage_dev = nullptr; char* stage_pin = nullptr; char* stage_map = nullptr; size_t stage_bytes = 0;
  size_t off_rew = 0, off_done = 0, off_obs = 0;    // of reward / done / obs inside the stage
  char* info_pin = nullptr; char* info_map = nullptr; bool info_valid = false;
  double* export_dev = nullptr;     // device [42][n] doubles: where export_kernel writes when its reader is a copy (gaq_get_state, unmapped mirror)
};

#pragma GCC visibility push(hidden)

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(GAQ_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

// Which instantiations this PROCESS has launched (gaq_launched_variants): the test suite's kernel coverage report is built from it
// (tools/kernel_coverage.py).  A handle remembers the last mask it recorded, so the steady state costs one compare per launch.
struct LaunchRecord {
  std::mutex mu;
  std::set<uint32_t> seen[3];      // 0: step_kernel<F>, 1: rollout_kernel<F>, 2: policy_rollout_kernel<F>
  void note(int kind, uint32_t f) { std::lock_guard<std::mutex> g(mu); seen[kind].insert(f); }
};
LaunchRecord& launch_record();   // the one instance of the process

int fail(int code, const std::string& msg);   // sets the calling thread's gaq_last_error() text, returns `code`
int env_override(const char* name);            // GAQ_* environment switches: 1, 0, or -1 when unset
// gaq_policy.hip: the per-step path and the fused T-step launch of gaq_step_policy_many_dev
int launch_step(gaq_env* e, const float* actions, float* obs, float* reward, uint8_t* done, hipStream_t st);
uint32_t fused_variant(const gaq_env* e);
int fused_rollout(gaq_env* e, int32_t T, float* obs, hipStream_t st, const std::function<int()>& launch);
// gaq_sharded.hip: the host-pointer forms wait for, and look at, every shard
int sync_handle(gaq_env* e);
int check_overrun(gaq_env* e);
// gaq_params.hip: the handle's plan from its parameter flags now
void refresh_feature_flags(gaq_env* e);

// ---- defined in gaq_params.hip: what the core needs of the per-env parameter pipeline ----
void derive_model(const gaq_model& g, double dt, Model<double>& m);   // gaq_create, gaq_plan
bool inverse_jacobian(const gaq_model& g, double out[16]);
int check_model(const gaq_model& g);
int launch_refill(gaq_env* e, hipStream_t st);                     // the refill pass of the staged planes
int launch_jinv(gaq_env* e, hipStream_t st, const uint8_t* done);  // inverse jacobians from the planes: every env, or those with done[i] set
int launch_catch_up(gaq_env* e, hipStream_t st);                   // launch_step with cold_stale set, before promotions that move all planes
int rebuild_params(gaq_env* e);                                    // gaq_set_counters: planes, inverse jacobians and staged planes from the counts

struct Scratch {   // device staging for the host-pointer entry points
  void* p = nullptr;
  ~Scratch() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    return e == hipSuccess ? 0 : fail(GAQ_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
};

// index of env i's value of `plane` inside a tile-major array with `planes` planes per tile
inline size_t tidx(int64_t i, int planes, int plane) {
  return (size_t)(i / kTile) * planes * kTile + (size_t)plane * kTile + (size_t)(i % kTile);
}

#pragma GCC visibility pop
