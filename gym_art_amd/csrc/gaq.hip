// gaq.hip -- the env core of libgaq: the env C ABI of include/gaq.h, kernel selection, the launch logic and the small kernels (reset, export,
// bookkeeping) around the fused step / rollout kernels of gaq_kernels.hpp (instantiated in gaq_inst.hip).  The per-env parameter pipeline
// (gaq_set_params*, gaq_get_params, the device sampler and its passes, the inverse jacobians) is in gaq_params.hip, the device policies
// (gaq_policy_*, gaq_step_policy_many_dev) in gaq_policy.hip, the learner-side passes (gaq_gae_*, gaq_obs_norm_*, gaq_ret_norm_*) in
// gaq_learn.hip, the one-process multi-device batch (gaq_*_sharded*) in gaq_sharded.hip; gaq_host.hpp holds what the five share.
//
// One lane = one environment; one wavefront = one TILE of 64 environments.  Device state is kept
// tile-major ("array of struct of arrays"): for every tile each state component is a run of 64 values
// and the components of a tile are contiguous, so a wavefront's whole working set is a handful of
// contiguous 1-KiB pieces.  The step kernel moves those pieces with 16-byte-per-lane transfers --
// HBM -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds, no VGPR staging), LDS -> HBM by ds_read_b128 +
// buffer_store_dwordx4 -- and each lane picks its own environment's values out of the LDS image with
// conflict-free ds_read_b64.  (Measured on MI355X: a copy runs at 6.2 TB/s with 16 B/lane, 5.8 with
// 8 B/lane and 3.8 with 4 B/lane; the first version of this kernel used 8- and 4-byte plane accesses
// and ran exactly at the rate those widths allow.)  The caller-facing observation tensor [N,D] is
// transposed through the same LDS buffer and written with 16 B/lane stores.  No MFMA in the physics: the largest
// contraction is 3x3.3x3; the MFMA kernels are the policy engines of gaq_policy.hip: policy_mfma_kernel (fp32), policy_gru_kernel (fp32, a
// GRU cell in front of the MLP head) and policy_mfma_bf16_kernel (bf16).  See DESIGN.md for the byte accounting and quad_core.hpp for the
// arithmetic.
#include "gaq_host.hpp"

// every step / rollout instantiation is compiled in gaq_inst.hip (eight translation units); here they are only declared
#define GAQ_X(FEAT) extern template __global__ GAQ_STEP_SIG(FEAT)
GAQ_STEP_ALL(GAQ_X)
#undef GAQ_X
#define GAQ_X(FEAT) extern template __global__ GAQ_ROLL_SIG(FEAT)
GAQ_ROLL_ALL(GAQ_X)
#undef GAQ_X

namespace {

using namespace gaqk;

// ---- optional episode bookkeeping: running return / length per env, totals of finished episodes ----
__global__ __launch_bounds__(kBlock) void episode_kernel(int64_t n, const float* __restrict__ reward,
                                                          const uint8_t* __restrict__ done, float* __restrict__ ep_ret,
                                                          uint32_t* __restrict__ ep_len, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  float ret = 0.0f; uint32_t len = 0; bool fin = false;
  if (i < n) {
    ret = ep_ret[i] + reward[i];
    len = ep_len[i] + 1u;
    fin = done[i] != 0;
    ep_ret[i] = fin ? 0.0f : ret;
    ep_len[i] = fin ? 0u : len;
  }
  // wave-level reduction of the finished episodes, then one atomic per wave and quantity
  double c = fin ? 1.0 : 0.0, sr = fin ? (double)ret : 0.0, sl = fin ? (double)len : 0.0, sq = fin ? (double)ret * ret : 0.0;
  if (__ballot(fin)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_down(c, o); sr += __shfl_down(sr, o); sl += __shfl_down(sl, o); sq += __shfl_down(sq, o); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(acc + 0, c); atomicAdd(acc + 1, sr); atomicAdd(acc + 2, sl); atomicAdd(acc + 3, sq); }
  }
}

// ---- multi-GPU return path: [obs | reward | done] packed into one [N, D+2] fp32 row array, so that the
// stacked result travels in ONE collective.  4 B per lane, fully coalesced on the store side; 20 MB at 131 072 envs.
__global__ __launch_bounds__(kBlock) void pack_rows_kernel(int64_t n, int D, const float* __restrict__ obs,
                                                            const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                            float* __restrict__ rows) {
  const int W = D + 2;
  const int64_t total = n * W;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < total; k += (int64_t)gridDim.x * kBlock) {
    const int64_t i = k / W;
    const int c = (int)(k - i * W);
    rows[k] = c < D ? obs[i * D + c] : c == D ? reward[i] : (float)done[i];
  }
}

// order-independent 64-bit checksum of a word array: sum over i of mix(word_i, i) (GAQ_CHECK_ALIAS)
__global__ __launch_bounds__(kBlock) void checksum_kernel(const uint32_t* __restrict__ w, int64_t n, uint64_t* __restrict__ out) {
  uint64_t acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    uint64_t x = ((uint64_t)w[i] << 32) ^ (uint64_t)i * 0x9E3779B97F4A7C15ull;
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
    acc += x;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)acc);
}

// On-box HBM calibration (gaq_hbm_copy_dev; bench.py's roofline.peak_measured, SURVEY 8d "also measure an on-box copy kernel"): the access
// shape of the step kernels' streaming traffic -- one 16-byte buffer load and one 16-byte buffer store per lane, every byte once
__global__ __launch_bounds__(kBlock) void hbm_copy_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n16) {
  size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (; i < n16; i += stride) dst[i] = src[i];
}

// graph-safe mode: the step index lives in device memory so that a captured graph draws fresh noise / reset keys on every replay (a
// host-side counter would be baked in).  Single-step launches advance it themselves (gaq_kernels.hpp: step_counter_checkin); the fused
// T-step rollout is followed by this one-thread launch (inc = T << ctr_shift, onto the first of the counter's words)
__global__ void bump_kernel(uint64_t* ctr, uint64_t inc) { *ctr += inc; }
// ... and before a launch that reads the first word alone (every step kernel without F_CTR) the check-ins of earlier F_CTR launches,
// spread over the counter's other words, are folded into it
__global__ void fold_counter_kernel(uint64_t* ctr) {
  uint64_t sum = 0;
  for (int k = 0; k < kCtrSlots; ++k) { sum += ctr[k * kCtrStride]; ctr[k * kCtrStride] = 0; }
  ctr[0] = sum;
}

// the counter plane of a batch whose counters the host has kept (counters_to_plane): every word, the padding lanes' included
__global__ __launch_bounds__(kBlock) void fill_counters_kernel(uint32_t* __restrict__ ctr, int64_t words, uint32_t word) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < words) ctr[i] = word;
}

// ---- reset / observe kernel (not on the per-step path: plain 8- and 4-byte tile accesses) -----------------
struct TileDirect {
  const DevPtrs& p; int64_t tile; uint32_t lane;
  __device__ __forceinline__ double ld64(const double* arr, int planes, int plane) const {
    auto r = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(arr + tile * planes * kTile), 0, planes * kTile * 8, 0x00020000);
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, lane * 8u, plane * (kTile * 8), 0));
  }
  __device__ __forceinline__ void st64(double* arr, int planes, int plane, double v) const {
    auto r = __builtin_amdgcn_make_buffer_rsrc(arr + tile * planes * kTile, 0, planes * kTile * 8, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, lane * 8u, plane * (kTile * 8), 0);
  }
  __device__ __forceinline__ float ld32(const float* arr, int plane) const {
    auto r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(arr + tile * 4 * kTile), 0, kGrpBytes, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, lane * 4u, plane * (kTile * 4), 0));
  }
  __device__ __forceinline__ void st32(float* arr, int plane, float v) const {
    auto r = __builtin_amdgcn_make_buffer_rsrc(arr + tile * 4 * kTile, 0, kGrpBytes, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v), r, lane * 4u, plane * (kTile * 4), 0);
  }
};

// `obs`: where the observation goes (or null).  Split-state layouts whose observation IS the heads: the same rows are the
// state (obs = the head rows).  `hi_out` != null (F_PACK handles): the heads go to the library's rows `hi_out` with plain
// stores and the observation is packed like in the plain layout.
__global__ __launch_bounds__(kBlock) void reset_kernel(DevPtrs p, StepCfg cfg, Model<double> um, const uint8_t* __restrict__ mask,
                                                        int do_reset, float* obs, int alias, uint64_t key_offset, float* hi_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (p.step_ctr) cfg.step_index = step_counter_peek(p, lane);
  cfg.step_index += key_offset;                                            // reset calls are keyed apart from steps
  const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + wave;
  if (tile >= p.ntiles) return;
  const int D = cfg.obs_dim;
  char* rows = smem + wave * (kTile * D * 4);
  const int64_t i = tile * kTile + lane;
  const TileDirect t{p, tile, lane};
  if (i < p.n) {
    EnvState<double> s;
#pragma unroll
    for (int j = 0; j < 3; ++j) { s.goal[j] = (double)t.ld32(p.goal, j); s.gyro_bias[j] = t.ld32(p.gyro, j); }
    if (alias) {   // value = observation word + residual (quad_core.hpp F_ALIAS); the goal is the default one
      double v[18];   // (alias == 2, fp32 mode: the observation word is the whole value)
#pragma unroll
      for (int k = 0; k < 18; ++k) v[k] = lo_decode(alias, p.obs_in, p.lo, i, k);
#pragma unroll
      for (int j = 0; j < 3; ++j) { s.pos[j] = v[j] + s.goal[j]; s.vel[j] = v[3 + j]; s.omega[j] = v[15 + j]; }
#pragma unroll
      for (int j = 0; j < 9; ++j) s.rot[j] = v[6 + j];
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) { s.pos[j] = t.ld64(p.core, kCorePlanes, j); s.vel[j] = t.ld64(p.core, kCorePlanes, 3 + j);
                                    s.omega[j] = t.ld64(p.core, kCorePlanes, 15 + j); }
#pragma unroll
      for (int j = 0; j < 9; ++j) s.rot[j] = t.ld64(p.core, kCorePlanes, 6 + j);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { s.rot_damp[j] = t.ld64(p.lag, kLagPlanes, j); s.cmds_damp[j] = t.ld32(p.cmds, j);
                                  s.ou[j] = t.ld32(p.ou, j); s.act_prev[j] = t.ld32(p.actp, j); }
    const uint32_t cw = p.ctr[i];
    s.tick = cw & 0xFFFFu; s.svd_ctr = cw >> 16;
    float acc[3] = {0.0f, 0.0f, 9.81f};
    float hist[4] = {s.act_prev[0], s.act_prev[1], s.act_prev[2], s.act_prev[3]};
    if (do_reset && (mask == nullptr || mask[i])) {
      gaq::reset_env<double, gaq::F_GENERIC>(s, cfg, cfg.env_offset + (uint64_t)i, cfg.step_index);
#pragma unroll
      for (int j = 0; j < 3; ++j) t.st32(p.goal, j, (float)s.goal[j]);
      if (!alias) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { t.st64(p.core, kCorePlanes, j, s.pos[j]); t.st64(p.core, kCorePlanes, 3 + j, s.vel[j]);
                                      t.st64(p.core, kCorePlanes, 15 + j, s.omega[j]); }
#pragma unroll
        for (int j = 0; j < 9; ++j) t.st64(p.core, kCorePlanes, 6 + j, s.rot[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { t.st64(p.lag, kLagPlanes, j, s.rot_damp[j]); t.st32(p.cmds, j, s.cmds_damp[j]);
                                    t.st32(p.actp, j, s.act_prev[j]); }
      p.ctr[i] = (s.tick & 0xFFFFu) | (s.svd_ctr << 16);
      hist[0] = hist[1] = hist[2] = hist[3] = 0.0f;
    }
    float hi18[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) hi18[k] = 0.0f;
    if (alias) {   // extra mantissa bits of the (possibly new) state; its head goes out as the observation below
      double v[18];
#pragma unroll
      for (int j = 0; j < 3; ++j) { v[j] = s.pos[j] - s.goal[j]; v[3 + j] = s.vel[j]; v[15 + j] = s.omega[j]; }
#pragma unroll
      for (int j = 0; j < 9; ++j) v[6 + j] = s.rot[j];
#pragma unroll
      for (int k = 0; k < 18; ++k) {
        if (alias == 2) { hi18[k] = (float)v[k]; }
        else { lo_encode(alias, p.lo, i, k, v[k]); hi18[k] = split_hi(v[k]); }
      }
      if (hi_out) {
#pragma unroll
        for (int k = 0; k < 18; ++k) hi_out[i * 18 + k] = hi18[k];
      }
    }
    if (obs) {
      float* row = reinterpret_cast<float*>(rows) + lane * D;
      if (alias && !hi_out) {          // the observation words ARE the (truncated) state heads
#pragma unroll
        for (int k = 0; k < 18; ++k) row[k] = hi18[k];
      } else {
        const float* sz = p.sense_in;
        const int64_t n = p.n;
        double t2w = 0.0, t2t = 0.0;
        if (cfg.obs_flags & (gaq::OBS_APPEND_T2W | gaq::OBS_APPEND_T2T)) {   // as in env_step: sum(thrust_max) = g m t2w
          double th[4], tq0 = um.torque_max[0], im = um.inv_mass;
#pragma unroll
          for (int j = 0; j < 4; ++j) th[j] = um.thrust_max[j];
          if (p.par) {
#pragma unroll
            for (int j = 0; j < 4; ++j) th[j] = t.ld64(p.par, kPar, PP_THRUST_MAX + j);
            tq0 = t.ld64(p.par, kPar, PP_TORQUE_MAX); im = t.ld64(p.par, kPar, PP_INV_MASS);
          }
          t2w = (((th[0] + th[1]) + th[2]) + th[3]) * im / 9.81; t2t = tq0 / th[0];
        }
        gaq::pack_obs<double, gaq::F_GENERIC | gaq::F_DIAG>(s, cfg, acc, hist, [&](int k, float v, int) { row[k] = v; },
                                            cfg.env_offset + (uint64_t)i, cfg.step_index, 1, WaveSwarm{lane, cfg.swarm.agents},
                                            [&](int c, int slot, int j) { return sz ? sz[((int64_t)(c * 12 + slot) * 3 + j) * n + i] : 0.0f; }, t2w, t2t);
        // state_vector() advanced the bias random walk (sensor_noise.py:166): kept for the envs this call is about -- all of them for
        // gaq_observe and an unmasked reset, the masked ones for a masked reset.  The others get an observation too (the call returns
        // the whole batch), but as a peek: a masked reset leaves every bit of an unmasked env alone
        // (tests/test_gpu_api_matrix.py found the bias of the unmasked envs one add_noise call ahead of an undisturbed twin's).
        if (cfg.gyro_bias && (!do_reset || mask == nullptr || mask[i])) {
#pragma unroll
          for (int j = 0; j < 3; ++j) t.st32(p.gyro, j, s.gyro_bias[j]);
        }
      }
    }
  }
  if (obs) {
    wave_lds_fence();
    flush_obs(obs, p.n, D, tile, rows, lane);
  }
}

// ---- gaq_get_state, device half: tile-major arrays (or the split alias rows) -> GAQ_STATE_PLANES x N doubles ----
// plane-major so that the host needs ONE copy; not on the per-step path (plain 8-/4-byte accesses).
__global__ __launch_bounds__(kBlock) void export_kernel(DevPtrs p, int alias, double* __restrict__ out, float* __restrict__ aux_out = nullptr) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  if (aux_out) {   // (gaq_step without copies: the info dict's aux rows ride along)
    for (int k = 0; k < gaq::AUX_WORDS; ++k) aux_out[i * gaq::AUX_WORDS + k] = p.aux[i * gaq::AUX_WORDS + k];
  }
  const int64_t n = p.n;
  const int64_t tile = i / kTile;
  const int lane = (int)(i % kTile);
  auto grp = [&](const float* a, int plane) { return (double)a[tile * (4 * kTile) + plane * kTile + lane]; };
  for (int k = 0; k < 3; ++k) out[(34 + k) * n + i] = grp(p.goal, k);
  if (alias) {
    for (int k = 0; k < 18; ++k)
      out[(int64_t)k * n + i] = lo_decode(alias, p.obs_in, p.lo, i, k) + (k < 3 ? grp(p.goal, k) : 0.0);
  } else {
    for (int k = 0; k < kCorePlanes; ++k) out[(int64_t)k * n + i] = p.core[tile * (kCorePlanes * kTile) + k * kTile + lane];
  }
  for (int j = 0; j < 4; ++j) {
    out[(18 + j) * n + i] = p.lag[tile * (kLagPlanes * kTile) + j * kTile + lane];
    out[(22 + j) * n + i] = grp(p.cmds, j);
    out[(26 + j) * n + i] = grp(p.ou, j);
    out[(30 + j) * n + i] = grp(p.actp, j);
  }
  const uint32_t c = p.ctr[i];
  out[37 * n + i] = (double)(c & 0xFFFFu);
  out[38 * n + i] = (double)(c >> 16);
  for (int k = 0; k < 3; ++k) out[(39 + k) * n + i] = grp(p.gyro, k);
}

// ---- host side ---------------------------------------------------------------------------------------
thread_local std::string g_err;

int svd_period_of(double dt) {   // replay of `since_last_svd += dt; if since_last_svd > 0.5` (quadrotor.py:381-386)
  double t = 0.0; int k = 0;
  while (!(t > 0.5)) { t += dt; ++k; if (k > 1000000) break; }
  return k;
}

}  // namespace

// ---- declared in gaq_host.hpp: what gaq_params.hip, gaq_policy.hip and gaq_sharded.hip call.  These, and what stands outside the anonymous
// namespace further down (refresh_feature_flags; launch_step ... fused_rollout; sync_handle, check_overrun)
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int env_override(const char* name) { const char* v = getenv(name); return v ? (v[0] == '1' ? 1 : 0) : -1; }
LaunchRecord& launch_record() { static LaunchRecord r; return r; }

namespace {

// the overrides that take part in the kernel choice, read from the environment: gaq_create once (the handle keeps them), gaq_plan per call
Overrides read_overrides() {
  return {env_override("GAQ_FORCE_GENERIC") == 1, env_override("GAQ_NO_AUXP") == 1, env_override("GAQ_PREDRAW"), env_override("GAQ_NT"),
          env_override("GAQ_UNIFORM_CTR") != 0};
}
constexpr uint32_t kCtrGuard = 0xA5C3A5C3u;    // what the kCtrGuardWords words behind DevPtrs::ctr hold for the life of the handle: the plane's
constexpr int kCtrGuardWords = kTile;          // writers (the step kernels' buffer resource, the fill, gaq_set_state) end at ntiles * kTile words
constexpr int kSweepDefault = 1;     // StepCfg::sweep of a handle created without GAQ_SWEEP (profiles/r28_sweep_ab.txt: no size at which it costs)

// ---- kernel selection: PURE host logic (no HIP call, no handle, no environment variable) shared by gaq_create, the parameter entry points
// and gaq_plan, so that the whole (configuration -> feature mask -> instantiation) map can be enumerated on a GPU-less host
// (tests/test_plan_cpu.py, tests/plan_sweep.py): a reachable mask without an instantiation is a test failure there, not a runtime
// GAQ_ERR_STATE.  Every fact is worked out once:
//   config_traits (gaq_config, StepCfg, Overrides) -> Traits, the named predicates the choice rests on
//   decide_layout / feature_mask / lds_bytes        what follows from them: state layout, instantiation, LDS per wave
//   plan_kernel                                     the one sequence of these: the layout from the parameter flags as at create, the
//                                                   selection from the flags now (gaq_create, every parameter upload, gaq_plan)
struct Layout { bool alias, pack, shadow, fp32; };       // how the 18 integrator words are stored (gaq_config.obs_state_alias)
struct Selection { uint32_t variant; bool generic; int lds_per_wave; };
struct ParamFlags { bool lag, drag; };                   // what the parameters bring: motor lag, rotor drag
struct Plan { Layout layout; Selection sel; };

bool step_instantiated(uint32_t f) {
  switch (f) {
#define GAQ_X(FEAT) case (FEAT):
    GAQ_STEP_ALL(GAQ_X)
#undef GAQ_X
      return true;
    default: return false;
  }
}
bool roll_instantiated(uint32_t f) {
  switch (f) {
#define GAQ_X(FEAT) case (FEAT):
    GAQ_ROLL_ALL(GAQ_X)
#undef GAQ_X
      return true;
    default: return false;
  }
}

const void* step_kernel_ptr(uint32_t f) {
  switch (f) {
#define GAQ_X(FEAT) case (FEAT): return (const void*)&step_kernel<(FEAT)>;
    GAQ_STEP_ALL(GAQ_X)
#undef GAQ_X
    default: return nullptr;
  }
}
// whether the instantiation takes the counters of a uniform batch from its arguments (gaq_kernels.hpp: kUniCtr)
bool takes_uniform_ctr(uint32_t f) {
  switch (f) {
#define GAQ_X(FEAT) case (FEAT): return kUniCtr<(FEAT)>;
    GAQ_STEP_ALL(GAQ_X)
#undef GAQ_X
    default: return false;
  }
}
// the instantiation gaq_step_many_dev's fused path launches for a step variant (0xFFFFFFFF: no fused rollout for this variant)
uint32_t rollout_variant_of(uint32_t variant, const Layout& L, bool generic) {
  const uint32_t base = variant & ~(gaq::F_PREDRAW | gaq::F_NT | gaq::F_ROWS | gaq::F_CTR);
  if (!L.alias || L.pack || generic || (variant & gaq::F_MELL)) return 0xFFFFFFFFu;
  if ((base >= 16u && base <= 23u) || (variant >= 48u && variant <= 55u)) return base;
  return 0xFFFFFFFFu;
}

// Twins of the alias kernels (quad_core.hpp F_ROWS / F_CTR): what a step launch runs when the packed rows are registered / in graph-safe
// mode.  Rows win when both are on (the counter is then advanced by bump_kernel as for every kernel without a F_CTR twin).
uint32_t rows_twin_of(uint32_t variant) { return step_instantiated(variant | gaq::F_ROWS) ? (variant | gaq::F_ROWS) : 0xFFFFFFFFu; }
uint32_t ctr_twin_of(uint32_t variant) { return step_instantiated(variant | gaq::F_CTR) ? (variant | gaq::F_CTR) : 0xFFFFFFFFu; }

int observation_dim(const gaq_config* cfg) {
  int D = (cfg->obs_flags & GAQ_OBS_QUAT) ? 13 : 18;
  if (cfg->obs_flags & GAQ_OBS_APPEND_T2W) D += 1;
  if (cfg->obs_flags & GAQ_OBS_APPEND_T2T) D += 1;
  if (cfg->obs_flags & GAQ_OBS_APPEND_H) D += 1;
  if (cfg->obs_flags & GAQ_OBS_APPEND_ACC) D += 3;
  if (cfg->obs_flags & GAQ_OBS_APPEND_ACT) D += 4;
  if (cfg->swarm.agents > 1) D += 6 * (cfg->swarm.agents - 1);
  return D;
}

// gaq_config -> what is fixed for the life of the handle, validated.  Everything that depends on the PARAMETERS (motor lag, rotor
// drag, compact / zero-damping planes) is filled in by refresh_feature_flags / flags_from_counts.
int fill_step_cfg(const gaq_config* cfg, StepCfg& sc, int& obs_dim) {
  if (cfg->struct_size != sizeof(gaq_config) || cfg->abi_version != GAQ_ABI_VERSION)
    return fail(GAQ_ERR_INVALID, "gaq_config size/version mismatch (header vs library)");
  if (cfg->num_envs <= 0) return fail(GAQ_ERR_INVALID, "num_envs must be positive");
  if (cfg->num_envs > (int64_t)1 << 27) return fail(GAQ_ERR_INVALID, "num_envs above 2^27 per handle is not supported");
  if (!(cfg->sim_freq > 0) || cfg->sim_steps <= 0) return fail(GAQ_ERR_INVALID, "sim_freq and sim_steps must be positive");
  if (cfg->sim_steps > 64)   // the OU noise streams of the sub-steps are ids 0 .. sim_steps-1; 64+ belong to resets and sensors
    return fail(GAQ_ERR_INVALID, "sim_steps above 64 is not supported (random-stream ids of the sub-steps)");
  if (cfg->ep_len < 0 || cfg->ep_len >= 0xFFFF) return fail(GAQ_ERR_INVALID, "ep_len must be in [0, 65534]");
  if (cfg->control < 0 || cfg->control > 2) return fail(GAQ_ERR_INVALID, "unknown control mode");
  if (cfg->noise < 0 || cfg->noise > 2) return fail(GAQ_ERR_INVALID, "unknown noise mode");
  if (cfg->reward_mode < 0 || cfg->reward_mode > 1) return fail(GAQ_ERR_INVALID, "unknown reward mode");
  if (cfg->obs_flags & ~127) return fail(GAQ_ERR_INVALID, "unknown obs flags");
  if ((cfg->obs_flags & GAQ_OBS_QUAT) && cfg->swarm.agents > 1) return fail(GAQ_ERR_INVALID, "the quaternion observation is not available for swarms");
  if (cfg->swarm.agents > 1) {
    const int a = cfg->swarm.agents;
    // the observation rows of a wave's 64 agents (18 + 6 (agents - 1) words each) are staged in LDS, four waves per workgroup:
    // 16 agents need 110 KB of the CU's 160 KB, 32 would need 209 KB
    if (a > 16 || (a & (a - 1)) != 0) return fail(GAQ_ERR_INVALID, "swarm.agents must be a power of two <= 16");
    if (cfg->num_envs % a != 0 || cfg->env_id_offset % a != 0)
      return fail(GAQ_ERR_INVALID, "num_envs and env_id_offset must be multiples of swarm.agents (whole worlds per handle)");
    if (!(cfg->swarm.prox_dist > 0.0f) || !(cfg->swarm.collision_dist >= 0.0f) || !(cfg->swarm.goal_radius >= 0.0f))
      return fail(GAQ_ERR_INVALID, "swarm distances must be positive");
  }
  const double dt = 1.0 / cfg->sim_freq;
  const int period = svd_period_of(dt);
  if (period >= 0xFFFF) return fail(GAQ_ERR_INVALID, "sim_freq too high for the 16-bit SVD counter");
  if (cfg->sim_freq < 50.0) return fail(GAQ_ERR_INVALID, "sim_freq below 50 Hz is outside the rotation series' range");
  const int D = observation_dim(cfg);
  obs_dim = D;
  std::memset(&sc, 0, sizeof(sc));
  sc.dt = dt; sc.gravity = cfg->gravity;
  sc.room_lo[0] = -cfg->room_size; sc.room_lo[1] = -cfg->room_size; sc.room_lo[2] = 0.0;
  sc.room_hi[0] = cfg->room_size; sc.room_hi[1] = cfg->room_size; sc.room_hi[2] = cfg->room_size;
  sc.goal_default[0] = 0.0; sc.goal_default[1] = 0.0; sc.goal_default[2] = 2.0;   // quadrotor.py:1081
  sc.init_box = 2.0;                                                               // :728
  sc.sim_steps = cfg->sim_steps; sc.ep_len = cfg->ep_len; sc.svd_period = period;
  sc.control = cfg->control; sc.noise = cfg->noise; sc.reward_mode = cfg->reward_mode;
  sc.obs_flags = cfg->obs_flags; sc.obs_dim = D;
  static_assert(sizeof(gaq::RewCoeff) == sizeof(gaq_rew_coeff), "reward coefficient layout");
  std::memcpy(&sc.rew, &cfg->rew, sizeof(sc.rew));
  static_assert(sizeof(gaq::SwarmCfg) == sizeof(gaq_swarm), "swarm layout");
  std::memcpy(&sc.swarm, &cfg->swarm, sizeof(sc.swarm));
  if (sc.swarm.agents <= 1) std::memset(&sc.swarm, 0, sizeof(sc.swarm));
  static_assert(sizeof(gaq::SenseNoise) == sizeof(gaq_sense_noise), "sensor noise layout");
  static_assert(gaq::AUX_WORDS == GAQ_AUX_WORDS, "aux row layout");
  std::memcpy(&sc.sense, &cfg->sense, sizeof(sc.sense));
  if (cfg->sense.enabled && cfg->sense.gyro_norm_std != 0.0f) {
    // add_noise_to_omega (sensor_noise.py:160-168) with dt = env.dt = 1/sim_freq (quadrotor.py:790)
    const double tau = cfg->sense.gyro_bias_correlation_time;
    if (!(tau > 0.0)) return fail(GAQ_ERR_INVALID, "gyro_bias_correlation_time must be positive");
    const double sg = (double)cfg->sense.gyro_noise_density / std::sqrt(dt);
    const double sb = std::sqrt(-(sg * sg) * (tau / 2) * (std::exp(-2 * dt / tau) - 1));
    const double pi = std::exp(-dt / tau);
    sc.gyro_bias = 1;
    sc.gyro_pi = (float)pi; sc.gyro_sigma = (float)sb;
    sc.gyro_pi_step = (float)(pi * pi * pi); sc.gyro_sigma_step = (float)(sb * std::sqrt(1.0 + pi * pi + pi * pi * pi * pi));
  }
  sc.need_act_prev = ((cfg->obs_flags & GAQ_OBS_APPEND_ACT) || cfg->rew.action_change != 0.0f) ? 1 : 0;
  sc.resample_goal = cfg->resample_goal ? 1 : 0;
  sc.excite = cfg->excite ? 1 : 0;
  sc.aux = cfg->aux_outputs ? 1 : 0;
  sc.action_f32 = cfg->action_f32 ? 1 : 0;
  sc.sense_input = (cfg->sense_input && (cfg->sense.enabled || (cfg->obs_flags & (GAQ_OBS_APPEND_T2W | GAQ_OBS_APPEND_T2T)))) ? 1 : 0;
  sc.t2w_std = (float)cfg->t2w_std; sc.t2w_min = 1.5f; sc.t2w_max = 10.0f;       // quadrotor.py:706-712
  sc.t2t_std = (float)cfg->t2t_std; sc.t2t_min = 0.005f; sc.t2t_max = 1.0f;
  sc.per_env_goal = (sc.resample_goal || sc.excite || sc.swarm.agents > 1) ? 1 : 0;
  sc.auto_reset = cfg->auto_reset ? 1 : 0;
  sc.init_random_state = cfg->init_random_state ? 1 : 0;
  sc.use_acos = (cfg->rew.rot != 0.0f || cfg->rew.attitude != 0.0f) ? 1 : 0;
  sc.seed = cfg->seed; sc.step_index = 0; sc.env_offset = (uint64_t)cfg->env_id_offset;
  return GAQ_OK;
}

// The predicates of a configuration, each under one name.  `auxp`: the aux row / quaternion / t2w / t2t observation ride on the split state
// (quad_core.hpp F_AUXP) -- only what those kernels hold: RawControl (uniform or per-env models) or Mellinger on a uniform model, fp64
// arithmetic, a split layout asked for, no swarm, and a reason to be there at all.  `envx`: so do the per-env planes that are state beside
// the 18 values: goals (resample_goal, excite; F_ENVX) and, for a uniform RawControl model, the gyro bias of SensorNoise's random walk
// (F_BIAS; per-env batches and Mellinger keep the generic kernel for the walk).
struct Traits {
  bool obs_diag;            // quaternion / t2w / t2t observation
  bool bias_walk;           // SensorNoise's gyro-bias random walk is on
  bool obs_packable;        // only the flags the packed observations of the split state hold (F_PACK): body frame, appended height / acc / action
  bool obs_packable_auxp;   // ... widened by the observations F_AUXP adds, where it is available
  bool heads_are_obs;       // the observation is exactly the 18 heads (world frame, no noise, nothing appended, no aux row beside it)
  bool split_asked, shadow_asked, fp32_asked;   // the layout request: obs_state_alias != 0, == 2, fp32_state
  bool auxp, envx;
  bool mell_generic, swarm_generic;             // Mellinger / the swarm layer outside what the specialised kernels hold
  bool generic;             // needs the generic instantiation (which honours every runtime flag and keeps fp64 state planes)
  bool heavy;               // ... with one of the register-hungry rarities on (the full tier, not F_LITE)
  bool diag;                // ... with the diagnostics tier (F_DIAG)
};

Traits config_traits(const gaq_config& c, const StepCfg& sc, const Overrides& ov) {
  constexpr int kPackFlags = GAQ_OBS_BODY_FRAME | GAQ_OBS_APPEND_H | GAQ_OBS_APPEND_ACC | GAQ_OBS_APPEND_ACT;
  constexpr int kDiagFlags = GAQ_OBS_QUAT | GAQ_OBS_APPEND_T2W | GAQ_OBS_APPEND_T2T;
  const bool mell = c.control == GAQ_CTRL_MELLINGER, swarm = sc.swarm.agents > 1, moving_goal = sc.resample_goal || sc.excite;
  const bool plain_obs = c.obs_flags == 0 && !c.sense.enabled && !sc.need_act_prev;
  Traits t;
  t.obs_diag = (c.obs_flags & kDiagFlags) != 0;
  t.bias_walk = sc.sense.enabled && sc.gyro_bias;
  t.obs_packable = (c.obs_flags & ~kPackFlags) == 0;
  t.split_asked = c.obs_state_alias != 0; t.shadow_asked = c.obs_state_alias == 2; t.fp32_asked = c.fp32_state != 0;
  const bool envx_wanted = (moving_goal || t.bias_walk) && !((c.per_env_params || mell) && t.bias_walk);
  t.auxp = (sc.aux || t.obs_diag || envx_wanted) && !(mell && c.per_env_params) && t.split_asked && !t.fp32_asked && !swarm && !ov.no_auxp;
  t.envx = t.auxp && envx_wanted;
  t.obs_packable_auxp = (c.obs_flags & ~(kPackFlags | (t.auxp ? kDiagFlags : 0))) == 0;
  // (the aux row is packed beside the observation: never the heads-are-the-observation kernels)
  t.heads_are_obs = sc.obs_dim == 18 && plain_obs && !(t.auxp && sc.aux) && !t.envx;
  // Mellinger runs in the specialised kernels (F_MELL), uniform or per-env models (one inverse jacobian per env, read where it is used): the
  // 18-word observation in any layout, the packed observations on the split state; the quaternion / t2w / t2t variants where F_AUXP holds
  // them; fp32 state and fp64 planes with a packed observation keep the generic kernel
  t.mell_generic = mell && (t.fp32_asked || !(plain_obs || (t.obs_packable && t.split_asked) || t.auxp));
  // the swarm layer runs on the split state (F_SWARM) for a uniform model under RawControl with one of the packable observations, when
  // a split layout was asked for (obs_state_alias != 0: the class default); anything else about it keeps the light generic kernel
  t.swarm_generic = swarm && (c.per_env_params || mell || !t.split_asked || t.fp32_asked || c.sense.enabled || !t.obs_packable);
  t.generic = ov.force_generic || sc.drag || t.mell_generic || c.noise == GAQ_NOISE_INPUT || (moving_goal && !t.envx) || (sc.aux && !t.auxp) ||
              sc.sense_input || (t.obs_diag && !t.auxp) || (t.bias_walk && !t.envx) || t.swarm_generic;
  // the lighter generic instantiation: everything generic except the register-hungry rarities
  t.heavy = ov.force_generic || sc.drag || mell || c.noise == GAQ_NOISE_INPUT || sc.sense_input || t.bias_walk ||
            ((sc.aux || t.obs_diag) && c.per_env_params);
  // the diagnostics tier of the full generic kernel (aux outputs, injected sensor draws, quaternion / t2w / t2t observations); the aux row
  // and those observation variants ALONE on a uniform model (info=True, obs_repr="xyz_vxyz_quat_omega" ... on a RawControl batch) ride
  // on the light kernel: F_LITE | F_DIAG (per-env models: the light kernel's 247 VGPRs leave no room for them)
  t.diag = sc.aux || t.obs_diag || (t.heavy && sc.sense_input);
  return t;
}

// split state: when the observation is exactly the 18 heads they can be one and the same rows; otherwise (body frame, appended height /
// accelerometer / action, sensor noise, what F_AUXP adds) the state is still stored split, library-owned, and the observation is packed
// beside it (F_PACK) -- unless the generic kernel is needed: then fp64 planes, whatever was asked
Layout decide_layout(const Traits& t) {
  Layout L;
  L.alias = (t.split_asked || t.fp32_asked) && (t.heads_are_obs || (!t.fp32_asked && t.obs_packable_auxp)) && !t.generic;
  L.pack = L.alias && !t.heads_are_obs;
  L.fp32 = t.fp32_asked;
  L.shadow = L.alias && (t.shadow_asked || L.pack) && !t.fp32_asked;
  return L;
}

// The instantiation: the specialised ones cover RawControl / Mellinger, the observations of decide_layout, the default reward terms and
// the yaw-only reset; anything else runs a generic tier.  `L` is the handle's layout, fixed at create; `t` the traits of its parameters now.
// `num_cus`: compute units of the device (hipDeviceProp_t::multiProcessorCount; 256 on a whole MI355X, fewer on a partitioned one).
uint32_t feature_mask(const gaq_config& c, const StepCfg& sc, const Traits& t, const Layout& L, int rz_every, int num_cus, const Overrides& ov) {
  uint32_t f = c.per_env_params ? gaq::F_PER_ENV : 0u;
  if (t.generic) {
    f |= gaq::F_GENERIC | (t.heavy ? 0u : gaq::F_LITE) | (t.diag ? gaq::F_DIAG : 0u);   // (F_LITE | F_DIAG: the aux row and nothing else of that tier)
  } else {
    if (sc.motor_lag) f |= gaq::F_LAG;
    if (c.noise == GAQ_NOISE_PHILOX) f |= gaq::F_NOISE;
    if (c.control == GAQ_CTRL_MELLINGER) f |= gaq::F_MELL;
    if (sc.swarm.agents > 1) f |= gaq::F_SWARM;
    if (L.alias) f |= gaq::F_ALIAS | (L.fp32 ? gaq::F_FP32 : 0u);
    if (L.pack) f |= gaq::F_PACK | (t.auxp ? gaq::F_AUXP : 0u) | (t.envx ? gaq::F_ENVX : 0u) | (t.envx && t.bias_walk ? gaq::F_BIAS : 0u);
  }
  // per-episode re-randomisation on the device: the instantiation that promotes finished envs to their staged planes (one per
  // feature set, no batch-size-specific variants: big and small handles -- shards -- run the very same code)
  if (c.per_env_params && rz_every > 0) f |= gaq::F_RZ;
  // small batches: noise drawn under the load latency / non-temporal streaming, by waves per SIMD (4 SIMDs per CU)
  if (f == 20u || f == 22u || f == 23u) {
    const int64_t tiles = (c.num_envs + kTile - 1) / kTile;
    const int64_t simds = (int64_t)(num_cus > 0 ? num_cus : 256) * 4;
    // defaults by batch size, from the 2 x 2 measurement profiles/r02_v4_small_batch_policy_2x2.txt:
    // non-temporal streaming up to two waves per SIMD (-3 % at 65 536 envs, -9 ... -15 % at 131 072 on 256 CUs; +6 % at 2^20);
    // noise drawn under the load latency from two waves per SIMD up (-1.4 ... -4 %; at ONE wave per SIMD it costs 6-7 %)
    // (Overrides::predraw / nt, the GAQ_PREDRAW / GAQ_NT measurement overrides: -1 = the size rule decides)
    const bool nt = ov.nt >= 0 ? ov.nt != 0 : tiles <= 2 * simds, predraw = ov.predraw >= 0 ? ov.predraw != 0 : tiles > simds;
    if (predraw && sc.sim_steps <= 2) f |= gaq::F_PREDRAW;
    if (nt) f |= gaq::F_NT;
  }
  return f;
}

// Bytes of LDS a wave of step_kernel<f> uses: the tile image as the kernel itself lays it out (gaq_kernels.hpp tile_image<F>); the
// observation rows reuse that buffer, and the info dict's aux rows sit behind them in the kernels that stage them (kAuxRowsInLds).
// (the F_ROWS twins stage their 20-word packed rows in the same buffer: 5120 B, below the alias image's 8192+)
int lds_bytes(uint32_t f, const StepCfg& sc) {
  int img;
  switch (f) {
#define GAQ_X(FEAT) case (FEAT): img = tile_image<(FEAT)>(sc).total; break;
    GAQ_STEP_ALL(GAQ_X)
#undef GAQ_X
    default: img = tile_image<gaq::F_GENERIC>(sc).total;   // no such kernel (gaq_create refuses the handle): the largest image of these flags
  }
  const int obs_rows = kTile * sc.obs_dim * 4;
  int lpw = std::max(img, obs_rows);
  if ((f & gaq::F_AUXP) || ((f & gaq::F_GENERIC) && (f & gaq::F_DIAG))) lpw = std::max(lpw, ((obs_rows + 15) & ~15) + kTile * gaq::AUX_WORDS * 4);
  return (lpw + 15) & ~15;
}

// The one sequence behind gaq_create, every parameter upload and gaq_plan: the layout is fixed at create, i.e. decided from the parameter
// flags the handle starts with (start_flags below); the selection follows the flags of the parameters it holds now.
Plan plan_kernel(const gaq_config& c, StepCfg sc, ParamFlags at_create, ParamFlags now, int rz_every, int num_cus, const Overrides& ov) {
  Plan p;
  sc.motor_lag = at_create.lag; sc.drag = at_create.drag;
  p.layout = decide_layout(config_traits(c, sc, ov));
  sc.motor_lag = now.lag; sc.drag = now.drag;
  const Traits t = config_traits(c, sc, ov);
  p.sel.generic = t.generic;
  p.sel.variant = feature_mask(c, sc, t, p.layout, rz_every, num_cus, ov);
  p.sel.lds_per_wave = lds_bytes(p.sel.variant, sc);
  return p;
}
// motor lag / rotor drag a handle starts with: its model's (`um`: derive_model of it); per-env handles: lag and no drag until parameters arrive
ParamFlags start_flags(const gaq_config& c, const Model<double>& um) {
  if (c.per_env_params) return {true, false};
  const uint8_t f = param_flags(um.tau_up, um.tau_down, c.model.c_drag, c.model.c_roll, true, 0.0, 0.0);
  return {(f & PF_LAG) != 0, (f & PF_DRAG) != 0};
}

// Graph-safe step counter of a handle of `ntiles` tiles: a self-counting step launch has `waves` waves (whole workgroups: the waves past
// the last tile check in too), every one adds 1 except the launch's first, which adds inc0 = 2^shift - (waves - 1): 2^shift per launch,
// and fewer than 2^shift have landed whenever a wave of the launch reads (its own is missing): gaq_kernels.hpp step_counter_checkin.
// Pure host arithmetic (gaq_plan reports it; tests/test_plan_cpu.py models the check-ins against it for every launch size).
void counter_plan(int64_t ntiles, uint64_t& waves, uint32_t& shift, uint32_t& inc0) {
  const int wpb = kBlock / kTile;
  waves = (uint64_t)((ntiles + wpb - 1) / wpb) * wpb;
  shift = 0;
  while (((uint64_t)1 << shift) < waves) ++shift;
  inc0 = (uint32_t)(((uint64_t)1 << shift) - (waves - 1));
}

}  // namespace

// the handle's plan from its parameter flags now; gaq_create and every parameter upload (gaq_params.hip).  (The layout comes out the same
// each time: the flags as at create and the overrides are the handle's own.)
void refresh_feature_flags(gaq_env* e) {
  e->sc.motor_lag = e->any_lag ? 1 : 0;
  e->sc.drag = e->any_drag ? 1 : 0;
  const Plan p = plan_kernel(e->cfg, e->sc, start_flags(e->cfg, e->um), {e->any_lag, e->any_drag}, e->d.rz_every, e->num_cus, e->ov);
  e->alias = p.layout.alias; e->pack = p.layout.pack; e->shadow = p.layout.shadow; e->fp32 = p.layout.fp32;
  e->variant = (int)p.sel.variant;
  e->needs_generic = p.sel.generic;
  e->lds_per_wave = p.sel.lds_per_wave;
}

namespace {

Layout layout_of(const gaq_env* e) { return {e->alias, e->pack, e->shadow, e->fp32}; }

// state-encoding mode of the reset / export kernels: 0 fp64 planes, 1 split with 16-bit residuals, 2 fp32 rows, 3 split
// with the mixed residual rows (pos / vel / R 16 bits, omega exact)
int alias_mode(const gaq_env* e) { return e->fp32 ? 2 : !e->alias ? 0 : e->lomix ? 3 : 1; }

// GAQ_CHECK_ALIAS=1 (debug): in alias mode 1 the observation tensor returned by step k is step k+1's input.  A caller that
// edits it in place (running-mean normalisation, clamp_, buffer reuse) corrupts the physics silently -- unless the rows are
// checksummed after every launch and verified before the next one.  Costs a reduction kernel and a stream sync per step.
int record_alias_rows(gaq_env* e, hipStream_t st) {
  if (!e->check_alias || e->shadow) return GAQ_OK;
  HIP_TRY(hipMemsetAsync(e->alias_sum_dev, 0, sizeof(uint64_t), st));
  const int64_t words = e->d.n * 18;
  hipLaunchKernelGGL(checksum_kernel, dim3(1024), dim3(kBlock), 0, st, reinterpret_cast<const uint32_t*>(e->last_obs), words, e->alias_sum_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&e->alias_sum, e->alias_sum_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  e->alias_sum_valid = true;
  return GAQ_OK;
}
int verify_alias_rows(gaq_env* e, hipStream_t st) {
  if (!e->check_alias || e->shadow || !e->alias_sum_valid) return GAQ_OK;
  uint64_t now = 0;
  HIP_TRY(hipMemsetAsync(e->alias_sum_dev, 0, sizeof(uint64_t), st));
  const int64_t words = e->d.n * 18;
  hipLaunchKernelGGL(checksum_kernel, dim3(1024), dim3(kBlock), 0, st, reinterpret_cast<const uint32_t*>(e->last_obs), words, e->alias_sum_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&now, e->alias_sum_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (now != e->alias_sum)
    return fail(GAQ_ERR_STATE, "obs_state_alias: the observation tensor returned by the previous step / reset was modified before "
                               "this call -- it is the integrator state's fp32 head (include/gaq.h gaq_config.obs_state_alias); "
                               "copy it before editing, or create the handle with obs_state_alias = 2 (library-owned heads)");
  return GAQ_OK;
}

// the instantiation the next step launch runs: the handle's kernel, or its F_ROWS / F_CTR twin (packed rows registered / graph-safe mode)
uint32_t launch_variant_of(const gaq_env* e) {
  const uint32_t v = (uint32_t)e->variant;
  if (e->d.rows_out && rows_twin_of(v) != 0xFFFFFFFFu) return rows_twin_of(v);
  if (e->d.step_ctr && ctr_twin_of(v) != 0xFFFFFFFFu) return ctr_twin_of(v);
  return v;
}

bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) == hipSuccess) return cs == hipStreamCaptureStatusActive;
  (void)hipGetLastError();
  return false;
}

// Uniform counters, the host's side (quad_core.hpp; UniformCtr in gaq_host.hpp).  counters_to_plane stands at the top of every path, other
// than the single-step launch, that reads or writes DevPtrs::ctr: it writes the word the host kept into the plane (one small fill on the
// stream of the launch that follows) and ends the argument path.  A launch that is being captured runs later and any number of times:
// the fill then goes to the handle's own stream instead of into the graph, and the host stops counting sub-steps.
int counters_to_plane(gaq_env* e, hipStream_t st) {
  UniformCtr& u = e->uni;
  if (!u.svd_known) return GAQ_OK;                  // (valid implies svd_known: nothing is known, the plane is what counts)
  const bool capturing = stream_capturing(st);
  if (u.valid) {
    u.valid = false;
    e->sc.sweep &= 1;
    if (capturing && st == e->stream) return fail(GAQ_ERR_STATE, "the handle's own stream is being captured");
    const int64_t words = e->d.ntiles * kTile;
    hipLaunchKernelGGL(fill_counters_kernel, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, capturing ? e->stream : st,
                       e->d.ctr, words, u.word);
    HIP_TRY(hipGetLastError());
  }
  if (capturing) u.svd_known = false;
  return GAQ_OK;
}
// T step launches' worth of the counters' evolution, after a launch that ran them
void advance_uniform_ctr(gaq_env* e, int64_t T) {
  UniformCtr& u = e->uni;
  if (!u.svd_known) return;
  for (int64_t t = 0; t < T; ++t) u.word = gaq::uniform_ctr_advance(u.word, e->sc.sim_steps, e->sc.svd_period, e->sc.ep_len, e->sc.auto_reset);
}

}  // namespace

int launch_step(gaq_env* e, const float* actions, float* obs, float* reward, uint8_t* done, hipStream_t st) {
  e->info_valid = false;
  if ((reinterpret_cast<uintptr_t>(actions) & 15) != 0) return fail(GAQ_ERR_INVALID, "actions must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(obs) & 15) != 0) return fail(GAQ_ERR_INVALID, "obs must be 16-byte aligned");
  if (e->sc.noise == gaq::NOISE_INPUT) {
    if (!e->noise_next) return fail(GAQ_ERR_STATE, "GAQ_NOISE_INPUT: call gaq_set_noise_input_dev before each step");
    e->d.noise_in = e->noise_next;
    e->noise_next = nullptr;
  }
  if (e->sc.sense_input) {
    if (!e->sense_next) return fail(GAQ_ERR_STATE, "sense_input: call gaq_set_sense_input_dev before each step");
    e->d.sense_in = e->sense_next;
    e->sense_next = nullptr;
  }
  const int tiles_per_block = kBlock / kTile;
  const dim3 grid((unsigned)((e->d.ntiles + tiles_per_block - 1) / tiles_per_block)), block(kBlock);
  const size_t lds = (size_t)e->lds_per_wave * tiles_per_block;
  const int lpw = e->lds_per_wave;
  const float* caller_obs = obs;              // (the shadow layouts step on the library's own rows below)
  if (e->alias) {
    if (e->needs_generic) return fail(GAQ_ERR_STATE, "obs_state_alias: parameters now need the generic kernel (rotor drag); "
                                                     "create the handle without obs_state_alias");
    e->d.obs_in = e->last_obs;
    if (int rc = verify_alias_rows(e, st)) return rc;
    e->d.obs_copy = nullptr;
    if (e->shadow) {              // heads stay in the library's own rows (updated in place); the caller's tensor gets a copy
      if (obs != e->own_obs) e->d.obs_copy = obs;
      obs = e->own_obs;
    }
  }
  if (lds > 65536 && e->lds_raised_for != e->variant) {
    // large swarm observation rows: more dynamic LDS than the 64 KB a launch may use by default (the CU has 160 KB)
    const void* fn = step_kernel_ptr((uint32_t)e->variant);
    if (!fn || lds > 160 * 1024) return fail(GAQ_ERR_INVALID, "observation rows too large for the CU's LDS");
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    e->lds_raised_for = e->variant;
  }
  const uint32_t launch_variant = launch_variant_of(e);
  if (e->d.rz_every > 0 && (launch_variant & gaq::F_RZ) != 0) {
    // (the condition of the step kernel's epilogue: gaq_kernels.hpp `hot_only`)
    const bool hot_only = e->sc.compact_params != 0 && e->sc.zero_damp != 0 && (launch_variant & gaq::F_FP32) == 0;
    if (hot_only) e->cold_stale = true;
    else if (e->cold_stale) {
      // this launch's promotions move all 45 planes and say nothing about the env's earlier ones: bring the envs that hot-only promotions
      // left behind up to date first (rare: the parameter flags changed under a live randomizer)
      if (int rc = launch_catch_up(e, st)) return rc;
    }
  }
  if (e->d.rz_every > 0 && e->rz_refill_now) { if (int rc = launch_refill(e, st)) return rc; }
  if (e->uni.svd_known) {
    // the counters as an argument of this launch (gaq_kernels.hpp: kUniCtr), unless it is captured or its kernel keeps them per env
    if (!takes_uniform_ctr(launch_variant) || e->d.step_ctr || stream_capturing(st)) { if (int rc = counters_to_plane(e, st)) return rc; }
    e->sc.sweep = (e->sc.sweep & 1) | (e->uni.valid ? (int32_t)gaq::uniform_ctr_pack(e->uni.word) : 0);
  }
  const bool self_counting = (launch_variant & gaq::F_CTR) != 0;
  if (e->d.step_ctr && !self_counting) {   // this kernel reads the counter's first word alone: fold the others into it
    // Eagerly the host knows whether F_CTR launches have left check-ins in the other words (ctr_spread).  A launch that is being CAPTURED
    // runs later, any number of times, after who knows which other launches (an F_CTR graph, eager small-batch steps): its graph always
    // carries the fold node, so that a replay never reads a stale first word.
    bool capturing = false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess) capturing = cs == hipStreamCaptureStatusActive; else (void)hipGetLastError();
    if (e->ctr_spread || capturing) {
      hipLaunchKernelGGL(fold_counter_kernel, dim3(1), dim3(1), 0, st, e->d.step_ctr);
      HIP_TRY(hipGetLastError());
      if (!capturing) e->ctr_spread = false;
    }
  }
  if (launch_variant != e->noted_step) { launch_record().note(0, launch_variant); e->noted_step = launch_variant; }
#define GAQ_LAUNCH(FEAT) \
  hipLaunchKernelGGL(step_kernel<(FEAT)>, grid, block, lds, st, e->d, e->sc, e->um, actions, obs, reward, done, lpw)
  switch (launch_variant) {
#define GAQ_X(FEAT) case (int)(FEAT): GAQ_LAUNCH(FEAT); break;
    GAQ_STEP_ALL(GAQ_X)
#undef GAQ_X
    default: return fail(GAQ_ERR_STATE, "internal: no kernel instantiation for this feature mask");
  }
#undef GAQ_LAUNCH
  HIP_TRY(hipGetLastError());
  if (e->d.ep_ret) {
    const dim3 g2((unsigned)((e->d.n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(episode_kernel, g2, block, 0, st, e->d.n, reward, done, e->d.ep_ret, e->d.ep_len, e->d.ep_acc);
    HIP_TRY(hipGetLastError());
  }
  if (e->d.rz_every > 0 && e->d.jinv) { if (int rc = launch_jinv(e, st, done)) return rc; }     // (the promoted envs' inverse jacobians)
  if (e->d.rz_every > 0) {
    // dynamics_randomize_every on the device: the step kernel promoted the finished, due envs to their staged planes; the
    // refill pass (the next draw of every promoted env -> par_next) is due before any of them can finish again, i.e. within
    // ep_len + 1 steps.  Under graph capture (device-resident step index) the host cannot count replays: every step.
    e->rz_since_refill += 1;
    const int period = e->sc.ep_len + 1 < 64 ? e->sc.ep_len + 1 : 64;
    if (e->d.step_ctr || e->rz_since_refill >= period) {
      if (int rc = launch_refill(e, st)) return rc;
    }
  }
  if (e->d.rows_out && (launch_variant & gaq::F_ROWS) == 0) {   // packed rows of the multi-GPU return path: no fused twin for this kernel
    const int64_t total = e->d.n * (e->obs_dim + 2);
    int64_t blocks = (total + kBlock - 1) / kBlock;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, e->d.n, e->obs_dim, caller_obs, (const float*)reward,
                       (const uint8_t*)done, e->d.rows_out);
    HIP_TRY(hipGetLastError());
  }
  if (e->d.step_ctr) {            // graph-safe mode: an F_CTR kernel advanced the device-resident counter itself
    if (self_counting) e->ctr_spread = true;
    else { hipLaunchKernelGGL(bump_kernel, dim3(1), dim3(1), 0, st, e->d.step_ctr, (uint64_t)1 << e->d.ctr_shift); HIP_TRY(hipGetLastError()); }
  }
  e->sc.step_index += 1;
  advance_uniform_ctr(e, 1);
  e->cur_obs = caller_obs;
  if (e->alias) { e->last_obs = obs; if (int rc = record_alias_rows(e, st)) return rc; }
  return GAQ_OK;
}

// the variant of the fused T-step kernels (rollout_kernel<F> / policy_rollout_kernel<F>) the handle launches, or 0xFFFFFFFF when it takes
// the per-step path: no fused form of its layout, GAQ_NO_FUSED, episode bookkeeping, done lists, info rows or periodic re-randomisation
uint32_t fused_variant(const gaq_env* e) {
  const uint32_t v = rollout_variant_of((uint32_t)e->variant, layout_of(e), e->needs_generic);
  const bool ok = v != 0xFFFFFFFFu && e->fused_rollout && !e->d.ep_ret && !e->d.done_list && !e->d.rows_out && !(e->rz_on && e->rz.every > 0);
  return ok ? v : 0xFFFFFFFFu;
}
// one fused T-step launch, `launch()`, between the bookkeeping around it: the alias-row check and the kernel's input heads before; the
// graph-safe step counter, the step index, the observation heads and the alias-row checksum after
int fused_rollout(gaq_env* e, int32_t T, float* obs, hipStream_t st, const std::function<int()>& launch) {
  const int64_t n = e->d.n;
  if (int rc = counters_to_plane(e, st)) return rc;
  e->d.obs_in = e->last_obs;
  if (int rc = verify_alias_rows(e, st)) return rc;
  e->d.obs_copy = nullptr;
  e->d.hi_final = e->shadow ? e->own_obs : nullptr;     // shadow mode: the final heads return to the library's own rows
  if (int rc = launch()) return rc;
  HIP_TRY(hipGetLastError());
  if (e->d.step_ctr) { hipLaunchKernelGGL(bump_kernel, dim3(1), dim3(1), 0, st, e->d.step_ctr, (uint64_t)T << e->d.ctr_shift); HIP_TRY(hipGetLastError()); }
  e->sc.step_index += (uint64_t)T;
  advance_uniform_ctr(e, T);
  e->last_obs = e->shadow ? e->own_obs : obs + (size_t)(T - 1) * n * 18;
  e->cur_obs = obs + (size_t)(T - 1) * n * 18;
  e->d.hi_final = nullptr;
  return record_alias_rows(e, st);
}

namespace {

int launch_reset(gaq_env* e, const uint8_t* mask, int do_reset, float* obs, hipStream_t st) {
  e->info_valid = false;      // (an observing pass advances the gyro-bias walk: state, too)
  if (obs && (reinterpret_cast<uintptr_t>(obs) & 15) != 0) return fail(GAQ_ERR_INVALID, "obs must be 16-byte aligned");
  if (int rc = counters_to_plane(e, st)) return rc;
  StepCfg sc = e->sc;
  uint64_t key_offset = 0;
  if (do_reset) { e->reset_calls += 1; key_offset = e->reset_calls << 44; }
  if (sc.sense_input && obs) {
    if (!e->sense_next) return fail(GAQ_ERR_STATE, "sense_input: call gaq_set_sense_input_dev before an observing reset / gaq_observe");
    e->d.sense_in = e->sense_next;
    e->sense_next = nullptr;
  }
  if (e->alias) {
    // the observation written here becomes the state head: without a caller buffer use the library's own
    if (!obs && !e->pack) obs = e->own_obs;
    e->d.obs_in = e->last_obs;
    if (int rc = verify_alias_rows(e, st)) return rc;
  }
  float* caller_obs = obs;
  float* hi_out = nullptr;
  if (e->alias && e->pack) hi_out = e->own_obs;                 // heads to the library's rows, the packed observation to the caller
  else if (e->alias && e->shadow) obs = e->own_obs;
  const int tiles_per_block = kBlock / kTile;
  const dim3 grid((unsigned)((e->d.ntiles + tiles_per_block - 1) / tiles_per_block)), block(kBlock);
  const size_t lds = (size_t)kTile * e->obs_dim * 4 * tiles_per_block;
  if (lds > 65536 && !e->reset_lds_raised) {
    if (lds > 160 * 1024) return fail(GAQ_ERR_INVALID, "observation rows too large for the CU's LDS");
    HIP_TRY(hipFuncSetAttribute((const void*)&reset_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    e->reset_lds_raised = true;
  }
  hipLaunchKernelGGL(reset_kernel, grid, block, lds, st, e->d, sc, e->um, mask, do_reset, obs, alias_mode(e), key_offset, hi_out);
  HIP_TRY(hipGetLastError());
  // an unmasked full reset zeroes every tick and leaves svd_ctr alone: where the host still knows that one, the batch is uniform again
  if (do_reset && !mask && e->uni.svd_known && !e->d.step_ctr) { e->uni.valid = true; e->uni.word &= 0xFFFF0000u; }
  if (caller_obs) e->cur_obs = caller_obs;
  if (e->alias) {
    e->last_obs = e->pack ? e->own_obs : obs;
    if (e->shadow && !e->pack && caller_obs != obs)
      HIP_TRY(hipMemcpyAsync(caller_obs, obs, sizeof(float) * (size_t)e->d.n * 18, hipMemcpyDeviceToDevice, st));
    if (int rc = record_alias_rows(e, st)) return rc;
  }
  return GAQ_OK;
}

// graph-safe mode: the device-resident step counter (kCtrSlots words, sum = step_index << ctr_shift; gaq_kernels.hpp)
int read_step_counter(gaq_env* e, uint64_t* step) {
  std::vector<uint64_t> w((size_t)kCtrSlots * kCtrStride);
  HIP_TRY(hipMemcpy(w.data(), e->step_ctr_mem, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  uint64_t sum = 0;
  for (int k = 0; k < kCtrSlots; ++k) sum += w[k * kCtrStride];
  *step = sum >> e->d.ctr_shift;
  return GAQ_OK;
}
int write_step_counter(gaq_env* e, uint64_t step) {
  std::vector<uint64_t> w((size_t)kCtrSlots * kCtrStride, 0);
  w[0] = step << e->d.ctr_shift;
  HIP_TRY(hipMemcpy(e->step_ctr_mem, w.data(), w.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  e->ctr_spread = false;
  return GAQ_OK;
}

// ---- the host-pointer step's staging: the stage, the three transports, the info mirror (gaq_env in gaq_host.hpp has the picture) ----------

size_t planes_bytes(const gaq_env* e) { return sizeof(double) * GAQ_STATE_PLANES * (size_t)e->d.n; }
size_t aux_bytes(const gaq_env* e) { return sizeof(float) * gaq::AUX_WORDS * (size_t)e->d.n; }
// the two parts of the info mirror, [42][n] doubles and the aux rows behind them, in the host's view of it (info_pin) or the device's (info_map)
double* mirror_planes(char* base) { return reinterpret_cast<double*>(base); }
float* mirror_aux(const gaq_env* e, char* base) { return reinterpret_cast<float*>(base + planes_bytes(e)); }

// the device's address of a mapped host block, or nullptr when the runtime has none to give (the caller then copies)
char* device_view(char* pinned) {
  void* dp = nullptr;
  if (hipHostGetDevicePointer(&dp, pinned, 0) == hipSuccess && dp) return static_cast<char*>(dp);
  (void)hipGetLastError();
  return nullptr;
}

// ABI state planes (include/gaq.h) <- tile-major device arrays, and with aux_dst the aux rows beside them: the one launch of export_kernel.
// planes_dst == nullptr: into export_dev, the handle's device scratch, for a copy to the host to read.
int export_state(gaq_env* e, double* planes_dst, float* aux_dst, hipStream_t st) {
  if (!planes_dst) {
    if (!e->export_dev) HIP_TRY(hipMalloc((void**)&e->export_dev, planes_bytes(e)));
    planes_dst = e->export_dev;
  }
  if (int rc = counters_to_plane(e, st)) return rc;
  if (e->alias) e->d.obs_in = e->last_obs;
  const dim3 grid((unsigned)((e->d.n + kBlock - 1) / kBlock)), block(kBlock);
  hipLaunchKernelGGL(export_kernel, grid, block, 0, st, e->d, alias_mode(e), planes_dst, aux_dst);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

// the info dict's inputs ride along with a staged step: state planes and aux rows into the info mirror, written there by one small kernel
// when the device reaches it, else exported on the device and brought over by two copies (queued on e->stream; gaq_step's synchronisation
// completes them)
int mirror_info(gaq_env* e) {
  if (!e->info_pin) {
    const bool mapped = e->stage_map != nullptr;
    HIP_TRY(hipHostMalloc((void**)&e->info_pin, planes_bytes(e) + aux_bytes(e), mapped ? hipHostMallocMapped : hipHostMallocDefault));
    if (mapped) e->info_map = device_view(e->info_pin);
  }
  if (e->info_map) return export_state(e, mirror_planes(e->info_map), mirror_aux(e, e->info_map), e->stream);
  if (int rc = export_state(e, nullptr, nullptr, e->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(mirror_planes(e->info_pin), e->export_dev, planes_bytes(e), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(mirror_aux(e, e->info_pin), e->d.aux, aux_bytes(e), hipMemcpyDeviceToHost, e->stream));
  return GAQ_OK;
}

// first gaq_step of a handle: the persistent device block [actions 16n | reward 4n | done n | pad | obs 4 D n] and, for small batches, its
// pinned host mirror -- which settles the handle's transport for good
int ensure_stage(gaq_env* e) {
  if (e->stage_dev) return GAQ_OK;
  const size_t n = (size_t)e->d.n;
  e->off_rew = (16 * n + 15) & ~(size_t)15;
  e->off_done = e->off_rew + 4 * n;
  e->off_obs = (e->off_done + n + 15) & ~(size_t)15;
  e->stage_bytes = e->off_obs + 4 * (size_t)e->obs_dim * n;
  HIP_TRY(hipMalloc((void**)&e->stage_dev, e->stage_bytes));
  // below ~1 MiB the call is latency-bound: one pinned H2D + one pinned D2H beat four pageable copies (2.5x at
  // N = 1); above it the extra host memcpy costs more than the pageable DMA path loses
  if (e->stage_bytes > ((size_t)1 << 20)) return GAQ_OK;
  // ... and the kernels reach that mirror themselves (mapped, host-coherent memory): the actions are read and observation / reward / done
  // written over the bus by the step launch, no copy-engine operation at all -- a single-env step() is then one launch + one
  // synchronisation instead of a copy in, a launch and a copy out (GAQ_ZERO_COPY=0: the copies, for the A/B)
  const bool zc = env_override("GAQ_ZERO_COPY") != 0;
  HIP_TRY(hipHostMalloc((void**)&e->stage_pin, e->stage_bytes, zc ? hipHostMallocMapped : hipHostMallocDefault));
  if (zc) e->stage_map = device_view(e->stage_pin);
  return GAQ_OK;
}

// How one gaq_step's arrays travel.  mapped: {stage_map, stage_pin, no copy in}; pinned: {stage_dev, stage_pin, copy in}; pageable:
// {stage_dev, nullptr, copy in}.  What comes out follows: a launch that wrote device memory (copy_in) has reward / done / obs copied out of
// `io`, one that wrote own_obs has the observation copied from there, and both land in `home` when there is one, else in the caller's arrays.
struct Transport {
  char* io;        // the stage as the launch sees it: it reads the actions from here and writes reward / done / obs here
  char* home;      // the stage as the host sees it (actions staged before, results read after the synchronisation), or nullptr
  bool copy_in;    // the launch reads device memory: the actions are copied there first
  bool own_obs;    // the launch writes the observation to the library's own_obs, not into `io`
};
Transport transport_of(const gaq_env* e) {
  const bool mapped = e->stage_map != nullptr;
  // A split state without a packed observation keeps its heads in a device buffer that outlives the call, and the host-pointer calls have
  // only own_obs to offer.  The alias layout proper has to be given it as the observation: what the launch writes IS the state.  The shadow
  // layout steps on own_obs whatever it is given and copies the rows to the caller's tensor (obs_copy): into the mapped stage that copy is the
  // transfer home, for free; on the copying transports it would be a device-side copy for nothing, as the D2H can read own_obs itself.
  const bool own_obs = e->alias && !e->pack && !(mapped && e->shadow);
  return {mapped ? e->stage_map : e->stage_dev, e->stage_pin, !mapped, own_obs};
}

}  // namespace

// Wait for this HANDLE's work only: its private stream and the stream the caller last handed to a *_dev entry point
// (a device-wide synchronise would stall every other handle and every other library on the GPU).
int sync_handle(gaq_env* e) {
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->user_stream_used) HIP_TRY(hipStreamSynchronize(e->user_stream));
  return GAQ_OK;
}

// Per-episode re-randomisation keeps every env's NEXT draw staged (par_next) and refills it off the critical path; an env promoted twice
// between two refill passes flew on a stale draw.  The refill schedule makes that impossible (launch_step), the device counts it anyway,
// and every synchronous entry point that hands results to the caller looks at the count: wrong parameters must not pass silently.
int check_overrun(gaq_env* e) {
  if (!e->d.rz_overrun) return GAQ_OK;
  uint32_t o = 0;
  HIP_TRY(hipMemcpy(&o, e->d.rz_overrun, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (o) return fail(GAQ_ERR_STATE, "internal: an env was re-randomised before its staged parameter planes were refilled");
  return GAQ_OK;
}

extern "C" {

int gaq_abi_version(void) { return GAQ_ABI_VERSION; }
const char* gaq_last_error(void) { return g_err.c_str(); }

int gaq_num_devices(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gaq_create(const gaq_config* cfg, gaq_env** out) {
  if (!cfg || !out) return fail(GAQ_ERR_INVALID, "null argument");
  StepCfg sc0;
  int D = 18;
  if (int rc = fill_step_cfg(cfg, sc0, D)) return rc;
  if (!cfg->per_env_params && check_model(cfg->model) != GAQ_OK) return GAQ_ERR_INVALID;
  int ndev = gaq_num_devices();
  if (ndev <= 0) return fail(GAQ_ERR_DEVICE, "no HIP device visible: libgaq has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(GAQ_ERR_INVALID, "device ordinal out of range");
  HIP_TRY(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));

  gaq_env* e = new (std::nothrow) gaq_env();
  if (!e) return fail(GAQ_ERR_DEVICE, "out of host memory");
  e->cfg = *cfg;
  e->obs_dim = D;
  e->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;   // the small-batch size rule counts waves per SIMD
  StepCfg& sc = e->sc;
  sc = sc0;
  const double dt = sc.dt;

  if (!cfg->per_env_params) {
    derive_model(cfg->model, dt, e->um);
    e->um.jinv = nullptr;
    if (cfg->control == GAQ_CTRL_MELLINGER && !inverse_jacobian(cfg->model, sc.jinv)) {
      delete e;
      return fail(GAQ_ERR_INVALID, "singular quadrotor jacobian");
    }
  } else {
    std::memset(&e->um, 0, sizeof(e->um));
  }
  { const ParamFlags f = start_flags(*cfg, e->um); e->any_lag = f.lag; e->any_drag = f.drag; }   // (per-env: decided when parameters arrive)
  { const char* nf = getenv("GAQ_NO_FUSED"); if (nf && nf[0] == '1') e->fused_rollout = false; }
  e->ov = read_overrides();     // for the life of the handle: a later change of the variables does not reach it
  e->lomix = cfg->per_env_params != 0 || e->any_lag;    // fixed for the life of the handle (the residual rows' format)
  { const char* ca = getenv("GAQ_CHECK_ALIAS"); e->check_alias = ca && ca[0] == '1'; }
  // The order step_kernel walks the batch in (gaq_kernels.hpp: sweep order): ascending on even steps and descending on odd ones, at every
  // size -- where the step's lines fit the Infinity Cache the order makes no difference, where they do not it is what lets a step find
  // the previous step's last lines there (profiles/r28_sweep_ab.txt).  GAQ_SWEEP=0 / 1 overrides it for the life of the handle; results do
  // not depend on it, and it takes no part in the kernel selection.
  { const int sw = env_override("GAQ_SWEEP"); sc.sweep = sw < 0 ? kSweepDefault : sw; }
  {   // timing-only ablations (tools/latency_breakdown.py, tools/rz_ablate.sh): wrong physics by construction, so they exist
      // only in a measurement build (-DGAQ_DIAG_BUILD) -- the product library refuses the variable instead of ignoring it
    const char* ab = getenv("GAQ_ABLATE");
    sc.ablate = ab ? atoi(ab) : 0;
    if (sc.ablate != 0 && !kDiagBuild) {
      delete e;
      return fail(GAQ_ERR_INVALID, "GAQ_ABLATE is set but this libgaq is not a measurement build (make EXTRA=-DGAQ_DIAG_BUILD OUT=...): "
                                   "the ablations skip parts of the step and give wrong physics; unset the variable");
    }
    if (sc.ablate != 0) fprintf(stderr, "libgaq: GAQ_ABLATE=%d in a measurement build -- results are WRONG by construction, only timings mean anything\n", sc.ablate);
  }
  // uniform tick / SVD counters (quad_core.hpp): a new handle's are all zero.  Not with per-env parameters, whose passes and promotions
  // clear single envs' svd_ctr; not where the counter does not fit the argument's 14 bits; never in a measurement build's ablations
  e->uni.eligible = e->ov.uniform_ctr && !cfg->per_env_params && sc.ablate == 0 && sc.svd_period >= 1 &&
                    (uint32_t)sc.svd_period <= gaq::kUniCtrSvdMax;
  e->uni.valid = e->uni.svd_known = e->uni.eligible;
  refresh_feature_flags(e);
  if (e->fp32 && !e->alias) {   // an explicit request for reduced precision is never dropped silently
    delete e;
    return fail(GAQ_ERR_INVALID, "fp32_state needs the specialised kernels (18-word world-frame obs, RawControl, default reward terms)");
  }
  if (!step_instantiated((uint32_t)e->variant)) {   // (tests/test_plan_cpu.py enumerates the reachable masks: this cannot happen)
    delete e;
    return fail(GAQ_ERR_STATE, "internal: no kernel instantiation for this feature mask");
  }

  DevPtrs& d = e->d;
  std::memset(&d, 0, sizeof(d));
  d.n = cfg->num_envs;
  d.ntiles = (cfg->num_envs + kTile - 1) / kTile;
  {   // graph-safe step counter: one step launch adds 2^ctr_shift in all (gaq_kernels.hpp: step_counter_checkin)
    uint64_t waves;
    counter_plan(d.ntiles, waves, d.ctr_shift, d.ctr_inc0);
  }
  const size_t nt = (size_t)d.ntiles;
  hipError_t he = hipSuccess;
  auto alloc0 = [&](void** p, size_t bytes) {
    if (he != hipSuccess) return;
    he = hipMalloc(p, bytes);
    if (he == hipSuccess) he = hipMemset(*p, 0, bytes);
  };
  if (e->alias) {
    if (!e->fp32) alloc0((void**)&d.lo, nt * (e->lomix ? (size_t)kMixRowsBytes : (size_t)kLoRowsBytes));
    alloc0((void**)&e->own_obs, nt * kRowsBytes);
  } else {
    alloc0((void**)&d.core, nt * kCoreBytes);
  }
  alloc0((void**)&d.lag, nt * kLagBytes);
  alloc0((void**)&d.ou, nt * kGrpBytes);
  alloc0((void**)&d.cmds, nt * kGrpBytes);
  alloc0((void**)&d.actp, nt * kGrpBytes);
  alloc0((void**)&d.goal, nt * kGrpBytes);
  alloc0((void**)&d.gyro, nt * kGrpBytes);
  alloc0((void**)&e->step_ctr_mem, sizeof(uint64_t) * kCtrSlots * kCtrStride);
  alloc0((void**)&e->alias_sum_dev, sizeof(uint64_t));
  alloc0((void**)&d.ctr, (nt * kTile + kCtrGuardWords) * sizeof(uint32_t));      // (+ the guard words behind the plane: gaq_uniform_counters)
  if (he == hipSuccess) he = hipMemsetD32((hipDeviceptr_t)(d.ctr + nt * kTile), (int)kCtrGuard, kCtrGuardWords);
  alloc0((void**)&d.done_count, sizeof(uint32_t) * 2);
  alloc0((void**)&d.nan_count, sizeof(uint32_t));
  if (cfg->compact_done) alloc0((void**)&d.done_list, nt * kTile * sizeof(uint32_t));
  if (cfg->aux_outputs) alloc0((void**)&d.aux, nt * kTile * gaq::AUX_WORDS * sizeof(float));
  if (cfg->per_env_params) {
    double* par = nullptr;
    double* jinv_dev = nullptr;
    alloc0((void**)&par, nt * kParBytes);
    if (cfg->control == GAQ_CTRL_MELLINGER) alloc0((void**)&jinv_dev, nt * kTile * 16 * sizeof(double));
    d.par = par;
    d.jinv = jinv_dev;
    alloc0((void**)&d.traj, 4 * nt * kTile * sizeof(uint32_t));          // traj | rcount | rz_flag | pfull (small kernels only: pfull_of)
    d.rcount = d.traj ? d.traj + nt * kTile : nullptr;
    d.rz_flag = d.traj ? d.traj + 2 * nt * kTile : nullptr;
    // padding envs (and envs whose parameters have not arrived yet) get a harmless unit model so their lanes stay
    // finite: every plane 1 except drag / damping (0) and the construction hints (t2t 1, motor_xy 1, com 0 -> +-1)
    e->host_par.assign(nt * kPar * kTile, 1.0);
    for (size_t t = 0; t < nt; ++t)
      for (int pl : {(int)PP_VEL_DAMP, (int)PP_DAMP_Q, (int)PP_C_DRAG, (int)PP_C_ROLL, (int)PP_COMX, (int)PP_COMY, (int)PP_OU_SIGMA})
        std::fill_n(e->host_par.begin() + (t * kPar + pl) * kTile, kTile, 0.0);
    e->pflags.assign((size_t)cfg->num_envs, 0);
  }
  if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
  if (he == hipSuccess) he = hipEventCreate(&e->ev0);
  if (he == hipSuccess) he = hipEventCreate(&e->ev1);
  if (he != hipSuccess) {
    std::string msg = std::string("device allocation failed: ") + hipGetErrorString(he);
    gaq_destroy(e);
    return fail(GAQ_ERR_DEVICE, msg);
  }
  // identity rotation and the default goal so that an un-reset env is a valid rigid body
  auto init_state = [&]() -> int {
    std::vector<float> goal(nt * 4 * kTile, 0.0f);
    for (int64_t i = 0; i < d.ntiles * kTile; ++i) {
      goal[tidx(i, 4, 2)] = 2.0f;
      if (sc.swarm.agents > 1) {   // formation goals (the first reset recomputes them on the device)
        const float ang = 6.2831853071795864769f * (float)(((uint64_t)cfg->env_id_offset + (uint64_t)i) % (uint64_t)sc.swarm.agents) /
                          (float)sc.swarm.agents;
        goal[tidx(i, 4, 0)] = sc.swarm.goal_radius * cosf(ang);
        goal[tidx(i, 4, 1)] = sc.swarm.goal_radius * sinf(ang);
      }
    }
    HIP_TRY(hipMemcpy(d.goal, goal.data(), goal.size() * sizeof(float), hipMemcpyHostToDevice));
    if (e->alias) {
      std::vector<float> rows(nt * kTile * 18, 0.0f);
      for (int64_t i = 0; i < d.ntiles * kTile; ++i) {
        rows[i * 18 + 0] = -goal[tidx(i, 4, 0)]; rows[i * 18 + 1] = -goal[tidx(i, 4, 1)];   // pos - goal with pos = 0 (formation goals: swarm)
        rows[i * 18 + 2] = -2.0f;
        for (int j : {6, 10, 14}) rows[i * 18 + j] = 1.0f;
      }
      HIP_TRY(hipMemcpy(e->own_obs, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
      e->last_obs = e->own_obs;
    } else {
      std::vector<double> core(nt * kCorePlanes * kTile, 0.0);
      for (int64_t i = 0; i < d.ntiles * kTile; ++i)
        for (int j : {6, 10, 14}) core[tidx(i, kCorePlanes, j)] = 1.0;
      HIP_TRY(hipMemcpy(d.core, core.data(), core.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (cfg->per_env_params)
      HIP_TRY(hipMemcpy(const_cast<double*>(d.par), e->host_par.data(), e->host_par.size() * sizeof(double), hipMemcpyHostToDevice));
    return GAQ_OK;
  };
  if (int rc = init_state()) { gaq_destroy(e); return rc; }
  *out = e;
  return GAQ_OK;
}

int gaq_destroy(gaq_env* e) {
  if (!e) return GAQ_OK;
  (void)hipSetDevice(e->cfg.device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  (void)hipDeviceSynchronize();
  (void)hipFree(e->d.core); (void)hipFree(e->d.lo); (void)hipFree(e->own_obs); (void)hipFree(e->d.lag); (void)hipFree(e->d.ou); (void)hipFree(e->d.cmds);
  (void)hipFree(e->d.actp); (void)hipFree(e->d.goal); (void)hipFree(e->d.gyro); (void)hipFree(e->step_ctr_mem); if (e->info_pin) (void)hipHostFree(e->info_pin); (void)hipFree(e->alias_sum_dev); (void)hipFree(e->d.ctr);
  (void)hipFree(e->d.done_count); (void)hipFree(e->d.nan_count); (void)hipFree(e->d.done_list);
  (void)hipFree(e->d.ep_ret); (void)hipFree(e->d.ep_len); (void)hipFree(e->d.ep_acc); (void)hipFree(e->d.aux);
  (void)hipFree(const_cast<double*>(e->d.par)); (void)hipFree(const_cast<double*>(e->d.jinv));
  (void)hipFree(e->d.traj); (void)hipFree(e->d.rz_overrun);
  (void)hipFree(e->stage_dev); (void)hipFree(e->export_dev);
  if (e->stage_pin) (void)hipHostFree(e->stage_pin);
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return GAQ_OK;
}

int gaq_is_diag_build(void) { return kDiagBuild ? 1 : 0; }

// The kernel selection of gaq_create (+ what parameters would bring) without a device: input validation, the defaults for lag and drag, plan_kernel.
int gaq_plan(const gaq_config* cfg, int32_t motor_lag, int32_t rotor_drag, int32_t randomize_every, int32_t num_cus, gaq_plan_info* out) {
  if (!cfg || !out) return fail(GAQ_ERR_INVALID, "null argument");
  StepCfg sc;
  int D = 18;
  if (int rc = fill_step_cfg(cfg, sc, D)) return rc;
  Model<double> um{};
  if (!cfg->per_env_params) {
    if (check_model(cfg->model) != GAQ_OK) return GAQ_ERR_INVALID;
    derive_model(cfg->model, sc.dt, um);
  }
  // defaults: what gaq_create starts with.  A uniform model's flags are for life; per-env handles get theirs with the parameters
  const ParamFlags start = start_flags(*cfg, um);
  const ParamFlags now{motor_lag < 0 ? start.lag : motor_lag > 0, rotor_drag < 0 ? start.drag : rotor_drag > 0};
  const int rz = (cfg->per_env_params && randomize_every > 0) ? randomize_every : 0;
  const Plan p = plan_kernel(*cfg, sc, cfg->per_env_params ? start : now, now, rz, num_cus, read_overrides());
  const Layout& L = p.layout;
  const Selection& sel = p.sel;
  out->obs_dim = D;
  out->state_layout = !L.alias ? 0 : L.shadow ? 2 : 1;
  out->fp32 = (L.fp32 && L.alias) ? 1 : 0;
  out->step_variant = (int32_t)sel.variant;
  out->step_instantiated = step_instantiated(sel.variant) ? 1 : 0;
  // (rotor drag arriving on a split-state handle is refused at the launch: obs_state_alias needs the specialised kernels)
  out->launchable = (out->step_instantiated && !(L.alias && sel.generic) && !(L.fp32 && !L.alias)) ? 1 : 0;
  const uint32_t rv = (rz > 0) ? 0xFFFFFFFFu : rollout_variant_of(sel.variant, L, sel.generic);
  out->rollout_variant = rv == 0xFFFFFFFFu ? -1 : (int32_t)rv;
  out->rollout_instantiated = rv == 0xFFFFFFFFu ? 0 : (roll_instantiated(rv) ? 1 : 0);
  out->lds_per_wave = sel.lds_per_wave;
  const uint32_t rt = rows_twin_of(sel.variant), ct = ctr_twin_of(sel.variant);
  out->rows_variant = rt == 0xFFFFFFFFu ? -1 : (int32_t)rt;
  out->ctr_variant = ct == 0xFFFFFFFFu ? -1 : (int32_t)ct;
  {
    uint64_t waves; uint32_t sh, inc0;
    counter_plan((cfg->num_envs + kTile - 1) / kTile, waves, sh, inc0);
    out->ctr_waves = (int32_t)waves; out->ctr_shift = (int32_t)sh; out->ctr_inc0 = (int32_t)inc0;
  }
  return GAQ_OK;
}

int gaq_kernel_variant(const gaq_env* e) { return e ? e->variant : GAQ_ERR_INVALID; }
int gaq_launch_variant(const gaq_env* e) { return e ? (int)launch_variant_of(e) : GAQ_ERR_INVALID; }
int gaq_launched_variants(int kind, uint32_t* out, int capacity) {
  if (kind < 0 || kind > 2 || capacity < 0 || (capacity > 0 && !out)) return GAQ_ERR_INVALID;
  LaunchRecord& r = launch_record();
  std::lock_guard<std::mutex> g(r.mu);
  int k = 0;
  for (uint32_t f : r.seen[kind]) { if (k < capacity) out[k] = f; ++k; }
  return k;
}
int gaq_obs_dim(const gaq_env* e) { return e ? e->obs_dim : GAQ_ERR_INVALID; }
int gaq_obs_is_state(const gaq_env* e) { return (e && e->alias && !e->shadow) ? 1 : 0; }
int gaq_state_layout(const gaq_env* e) { return !e ? GAQ_ERR_INVALID : !e->alias ? 0 : e->shadow ? 2 : 1; }
int64_t gaq_num_envs(const gaq_env* e) { return e ? e->d.n : GAQ_ERR_INVALID; }

int gaq_reset_dev(gaq_env* e, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(e->cfg.device));
  e->user_stream = (hipStream_t)stream; e->user_stream_used = true;
  return launch_reset(e, mask_dev, 1, obs_dev, (hipStream_t)stream);
}

int gaq_reset(gaq_env* e, const uint8_t* mask, float* obs_out) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;   // earlier *_dev calls may still be running on the caller's stream
  const int64_t n = e->d.n;
  Scratch dm, dobs;
  if (mask) { if (dm.alloc(n)) return GAQ_ERR_DEVICE; HIP_TRY(hipMemcpyAsync(dm.p, mask, n, hipMemcpyHostToDevice, e->stream)); }
  float* dev_obs = nullptr;
  if (e->alias && !e->pack) dev_obs = e->own_obs;     // the device copy must outlive the call: it is state
  else if (obs_out) { if (dobs.alloc(sizeof(float) * n * e->obs_dim)) return GAQ_ERR_DEVICE; dev_obs = (float*)dobs.p; }
  int rc = launch_reset(e, mask ? (const uint8_t*)dm.p : nullptr, 1, dev_obs, e->stream);
  if (rc) return rc;
  if (dev_obs == dobs.p) e->cur_obs = nullptr;     // (the staging buffer is freed on return)
  if (obs_out) HIP_TRY(hipMemcpyAsync(obs_out, dev_obs, sizeof(float) * n * e->obs_dim, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GAQ_OK;
}

int gaq_observe(gaq_env* e, float* obs_out) {
  if (!e || !obs_out) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  const int64_t n = e->d.n;
  if (e->alias && !e->pack) {   // the current observation is the state head itself
    HIP_TRY(hipMemcpy(obs_out, e->last_obs, sizeof(float) * n * 18, hipMemcpyDeviceToHost));
    return GAQ_OK;
  }
  Scratch dobs;
  if (dobs.alloc(sizeof(float) * n * e->obs_dim)) return GAQ_ERR_DEVICE;
  const float* keep_obs = e->cur_obs;
  int rc = launch_reset(e, nullptr, 0, (float*)dobs.p, e->stream);
  e->cur_obs = keep_obs;                           // (the staging buffer is freed on return)
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(obs_out, dobs.p, sizeof(float) * n * e->obs_dim, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GAQ_OK;
}

int gaq_step_dev(gaq_env* e, const float* actions, float* obs, float* reward, uint8_t* done, void* stream) {
  if (!e || !actions || !obs || !reward || !done) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  e->user_stream = (hipStream_t)stream; e->user_stream_used = true;
  hipStream_t st = (hipStream_t)stream;
  if (e->timing) HIP_TRY(hipEventRecord(e->ev0, st));
  int rc = launch_step(e, actions, obs, reward, done, st);
  if (rc) return rc;
  if (e->timing) { HIP_TRY(hipEventRecord(e->ev1, st)); e->timed = true; }
  return GAQ_OK;
}

int gaq_step_many_dev(gaq_env* e, int32_t T, const float* actions, float* obs, float* reward, uint8_t* done, void* stream) {
  if (!e || !actions || !obs || !reward || !done) return fail(GAQ_ERR_INVALID, "null argument");
  if (T <= 0) return fail(GAQ_ERR_INVALID, "T must be positive");
  e->info_valid = false;
  if (e->sc.noise == gaq::NOISE_INPUT) return fail(GAQ_ERR_INVALID, "step_many does not support GAQ_NOISE_INPUT");
  const int64_t n = e->d.n;
  if (T > 1 && (((size_t)n * e->obs_dim * 4) & 15)) return fail(GAQ_ERR_INVALID, "step_many needs N*obs_dim*4 to be a multiple of 16");
  HIP_TRY(hipSetDevice(e->cfg.device));
  e->user_stream = (hipStream_t)stream; e->user_stream_used = true;
  hipStream_t st = (hipStream_t)stream;
  if (e->timing) HIP_TRY(hipEventRecord(e->ev0, st));
  const uint32_t roll_variant = T > 1 ? fused_variant(e) : 0xFFFFFFFFu;
  if (roll_variant != 0xFFFFFFFFu) {
    if ((reinterpret_cast<uintptr_t>(actions) & 15) || (reinterpret_cast<uintptr_t>(obs) & 15))
      return fail(GAQ_ERR_INVALID, "actions and obs must be 16-byte aligned");
    const int tiles_per_block = kBlock / kTile;
    const dim3 grid((unsigned)((e->d.ntiles + tiles_per_block - 1) / tiles_per_block)), block(kBlock);
    const size_t lds = (size_t)e->lds_per_wave * tiles_per_block;
    const int lpw = e->lds_per_wave;
    int rc = fused_rollout(e, T, obs, st, [&]() -> int {
      if (roll_variant != e->noted_roll) { launch_record().note(1, roll_variant); e->noted_roll = roll_variant; }
      switch (roll_variant) {
#define GAQ_X(FEAT) case (FEAT): \
        hipLaunchKernelGGL(rollout_kernel<(FEAT)>, grid, block, lds, st, e->d, e->sc, e->um, (int)T, actions, obs, reward, done, lpw); break;
        GAQ_ROLL_ALL(GAQ_X)
#undef GAQ_X
        default: return fail(GAQ_ERR_STATE, "internal: no rollout instantiation for this feature mask");
      }
      return GAQ_OK;
    });
    if (rc) return rc;
  } else {
    for (int32_t t = 0; t < T; ++t) {
      int rc = launch_step(e, actions + (size_t)t * n * 4, obs + (size_t)t * n * e->obs_dim, reward + (size_t)t * n,
                           done + (size_t)t * n, st);
      if (rc) return rc;
    }
  }
  if (e->timing) { HIP_TRY(hipEventRecord(e->ev1, st)); e->timed = true; }
  return GAQ_OK;
}

int gaq_step(gaq_env* e, const float* actions, float* obs, float* reward, uint8_t* done) {
  if (!e || !actions || !obs || !reward || !done) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  if (int rc_ = ensure_stage(e)) return rc_;
  const Transport t = transport_of(e);
  const size_t n = (size_t)e->d.n, obs_bytes = 4 * (size_t)e->obs_dim * n;
  float* obs_arg = t.own_obs ? e->own_obs : reinterpret_cast<float*>(t.io + e->off_obs);
  if (t.home) std::memcpy(t.home, actions, 16 * n);
  if (t.copy_in) HIP_TRY(hipMemcpyAsync(t.io, t.home ? (const void*)t.home : (const void*)actions, 16 * n, hipMemcpyHostToDevice, e->stream));
  int rc = gaq_step_dev(e, reinterpret_cast<const float*>(t.io), obs_arg, reinterpret_cast<float*>(t.io + e->off_rew),
                        reinterpret_cast<uint8_t*>(t.io + e->off_done), e->stream);
  if (rc) return rc;
  if (t.home) {
    // reward | done, and the observation behind them in the same copy where the launch wrote it there
    if (t.copy_in) HIP_TRY(hipMemcpyAsync(t.home + e->off_rew, t.io + e->off_rew, (t.own_obs ? e->off_obs : e->stage_bytes) - e->off_rew, hipMemcpyDeviceToHost, e->stream));
    if (t.own_obs) HIP_TRY(hipMemcpyAsync(t.home + e->off_obs, e->own_obs, obs_bytes, hipMemcpyDeviceToHost, e->stream));
    if (e->d.aux) { if (int rc_ = mirror_info(e)) return rc_; }
  } else {   // (no info mirror either: gaq_get_state / gaq_get_aux read the device)
    HIP_TRY(hipMemcpyAsync(obs, obs_arg, obs_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(reward, t.io + e->off_rew, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(done, t.io + e->off_done, n, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (t.home) {
    e->info_valid = e->d.aux != nullptr;
    std::memcpy(reward, t.home + e->off_rew, 4 * n);
    std::memcpy(done, t.home + e->off_done, n);
    std::memcpy(obs, t.home + e->off_obs, obs_bytes);
  }
  if (int rc_ = check_overrun(e)) return rc_;
  // the reference raises on a non-finite reward inside step() (quadrotor.py:633-636): same here, on the host copy
  for (size_t i = 0; i < n; ++i) {
    if (!std::isfinite(reward[i])) {
      HIP_TRY(hipMemset(e->d.nan_count, 0, sizeof(uint32_t)));
      return fail(GAQ_ERR_NAN, "QuadEnv: reward is Nan");
    }
  }
  return GAQ_OK;
}

int gaq_set_noise_input_dev(gaq_env* e, const float* normals_dev) {
  if (!e || !normals_dev) return fail(GAQ_ERR_INVALID, "null argument");
  if (e->sc.noise != gaq::NOISE_INPUT) return fail(GAQ_ERR_STATE, "handle was not created with GAQ_NOISE_INPUT");
  e->noise_next = normals_dev;
  return GAQ_OK;
}

int gaq_set_sense_input_dev(gaq_env* e, const float* draws_dev) {
  if (!e || !draws_dev) return fail(GAQ_ERR_INVALID, "null argument");
  if (!e->sc.sense_input) return fail(GAQ_ERR_STATE, "handle was not created with sense_input (and sensor noise or a t2w / t2t observation)");
  e->sense_next = draws_dev;
  return GAQ_OK;
}

int gaq_set_action_dtype(gaq_env* e, int32_t is_float32) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  e->sc.action_f32 = is_float32 ? 1 : 0;       // a launch constant: takes effect with the next step
  return GAQ_OK;
}

int gaq_get_aux(gaq_env* e, float* host_out) {
  if (!e || !host_out) return fail(GAQ_ERR_INVALID, "null argument");
  if (!e->d.aux) return fail(GAQ_ERR_STATE, "handle was created with aux_outputs = 0");
  if (e->info_valid) { std::memcpy(host_out, mirror_aux(e, e->info_pin), aux_bytes(e)); return GAQ_OK; }
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  HIP_TRY(hipMemcpy(host_out, e->d.aux, aux_bytes(e), hipMemcpyDeviceToHost));
  return GAQ_OK;
}

int gaq_get_state(gaq_env* e, double* hp) {
  if (!e || !hp) return fail(GAQ_ERR_INVALID, "null argument");
  if (e->info_valid) { std::memcpy(hp, mirror_planes(e->info_pin), planes_bytes(e)); return GAQ_OK; }
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  if (int rc_ = export_state(e, nullptr, nullptr, e->stream)) return rc_;
  HIP_TRY(hipMemcpyAsync(hp, e->export_dev, planes_bytes(e), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GAQ_OK;
}

int gaq_set_state(gaq_env* e, const double* hp) {
  if (!e || !hp) return fail(GAQ_ERR_INVALID, "null argument");
  e->info_valid = false;
  e->cur_obs = nullptr;                            // the last observation written no longer describes the state
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (int rc_ = sync_handle(e)) return rc_;
  const int64_t n = e->d.n;
  const size_t nt = (size_t)e->d.ntiles;
  std::vector<double> core(nt * kCorePlanes * kTile, 0.0), lag(nt * kLagPlanes * kTile, 0.0);
  std::vector<float> ou(nt * 4 * kTile, 0.f), cmds(nt * 4 * kTile, 0.f), actp(nt * 4 * kTile, 0.f), goal(nt * 4 * kTile, 0.f),
      gyro(nt * 4 * kTile, 0.f);
  std::vector<uint32_t> c(nt * kTile, 0u);
  for (int64_t i = n; i < (int64_t)(nt * kTile); ++i) { for (int j : {6, 10, 14}) core[tidx(i, kCorePlanes, j)] = 1.0; }
  for (int64_t i = 0; i < n; ++i) {
    for (int pl = 0; pl < kCorePlanes; ++pl) core[tidx(i, kCorePlanes, pl)] = hp[(size_t)pl * n + i];
    for (int j = 0; j < 4; ++j) {
      lag[tidx(i, kLagPlanes, j)] = hp[(size_t)(18 + j) * n + i];
      cmds[tidx(i, 4, j)] = (float)hp[(size_t)(22 + j) * n + i];
      ou[tidx(i, 4, j)] = (float)hp[(size_t)(26 + j) * n + i];
      actp[tidx(i, 4, j)] = (float)hp[(size_t)(30 + j) * n + i];
    }
    for (int j = 0; j < 3; ++j) goal[tidx(i, 4, j)] = (float)hp[(size_t)(34 + j) * n + i];
    for (int j = 0; j < 3; ++j) gyro[tidx(i, 4, j)] = (float)hp[(size_t)(39 + j) * n + i];
    const double t = hp[(size_t)37 * n + i], s = hp[(size_t)38 * n + i];
    if (!(t >= 0 && t <= 65535 && s >= 0 && s <= 65535)) return fail(GAQ_ERR_INVALID, "tick / SVD counter out of range");
    c[i] = ((uint32_t)t & 0xFFFFu) | ((uint32_t)s << 16);
  }
  if (e->alias) {
    std::vector<float> hi(nt * kTile * 18, 0.0f);
    const int mode = alias_mode(e);
    std::vector<unsigned char> lo(nt * (size_t)(e->lomix ? kMixRowsBytes : kLoRowsBytes), 0);
    for (int64_t i = 0; i < n; ++i)
      for (int k = 0; k < 18; ++k) {
        const double v = core[tidx(i, kCorePlanes, k)] - (k < 3 ? (double)goal[tidx(i, 4, k)] : 0.0);
        hi[i * 18 + k] = e->fp32 ? (float)v : split_hi(v);
        lo_encode(mode, lo.data(), i, k, v);
      }
    HIP_TRY(hipMemcpy(e->own_obs, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
    if (!e->fp32) HIP_TRY(hipMemcpy(e->d.lo, lo.data(), lo.size(), hipMemcpyHostToDevice));
    e->last_obs = e->own_obs;
  } else {
    HIP_TRY(hipMemcpy(e->d.core, core.data(), core.size() * 8, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(e->d.lag, lag.data(), lag.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d.ou, ou.data(), ou.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d.cmds, cmds.data(), cmds.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d.actp, actp.data(), actp.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d.goal, goal.data(), goal.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d.gyro, gyro.data(), gyro.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d.ctr, c.data(), c.size() * 4, hipMemcpyHostToDevice));
  e->uni.valid = e->uni.svd_known = false;      // (the whole plane was just written: nothing to fill)
  e->sc.sweep &= 1;
  e->rz_refill_now = true;      // the caller may have moved episode clocks: refill the staged parameter planes before the next step
  return GAQ_OK;
}

int gaq_done_list(gaq_env* e, uint32_t* idx_out, int64_t capacity, int64_t* count_out) {
  if (!e || !count_out) return fail(GAQ_ERR_INVALID, "null argument");
  if (!e->d.done_list) return fail(GAQ_ERR_STATE, "handle was created with compact_done = 0");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (int rc_ = sync_handle(e)) return rc_;
  uint64_t step = e->sc.step_index;
  if (e->d.step_ctr) { if (int rc_ = read_step_counter(e, &step)) return rc_; }   // replays advance only this one
  if (step == 0) { *count_out = 0; return GAQ_OK; }
  uint32_t cnt = 0;
  HIP_TRY(hipMemcpy(&cnt, e->d.done_count + ((step - 1) & 1), sizeof(uint32_t), hipMemcpyDeviceToHost));
  *count_out = cnt;
  if (idx_out && cnt) {
    const int64_t m = cnt < capacity ? cnt : capacity;
    HIP_TRY(hipMemcpy(idx_out, e->d.done_list, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
  }
  return GAQ_OK;
}

int gaq_pack_rows_dev(gaq_env* e, const float* obs, const float* reward, const uint8_t* done, float* rows, void* stream) {
  if (!e || !obs || !reward || !done || !rows) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  e->user_stream = (hipStream_t)stream; e->user_stream_used = true;
  const int64_t total = e->d.n * (e->obs_dim + 2);
  int64_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > 16384) blocks = 16384;                                      // grid-stride above 4 M words
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, e->d.n, e->obs_dim, obs, reward,
                     done, rows);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

int gaq_set_packed_rows_dev(gaq_env* e, float* rows_dev) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  if (rows_dev && (reinterpret_cast<uintptr_t>(rows_dev) & 15) != 0) return fail(GAQ_ERR_INVALID, "rows must be 16-byte aligned");
  e->d.rows_out = rows_dev;
  return GAQ_OK;
}

int gaq_nan_count(gaq_env* e, int64_t* count_out) {
  if (!e || !count_out) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (int rc_ = sync_handle(e)) return rc_;
  uint32_t c = 0;
  HIP_TRY(hipMemcpy(&c, e->d.nan_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(e->d.nan_count, 0, sizeof(uint32_t)));
  *count_out = c;
  return check_overrun(e);
}

int gaq_set_terminal_obs_dev(gaq_env* e, float* term_obs_dev) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  e->d.term_obs = term_obs_dev;
  return GAQ_OK;
}

int gaq_track_episodes(gaq_env* e, int32_t enabled) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  if (enabled && !e->d.ep_ret) {
    const size_t np = (size_t)e->d.ntiles * kTile;
    HIP_TRY(hipMalloc((void**)&e->d.ep_ret, np * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&e->d.ep_len, np * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&e->d.ep_acc, 4 * sizeof(double)));
    HIP_TRY(hipMemset(e->d.ep_ret, 0, np * sizeof(float)));
    HIP_TRY(hipMemset(e->d.ep_len, 0, np * sizeof(uint32_t)));
    HIP_TRY(hipMemset(e->d.ep_acc, 0, 4 * sizeof(double)));
  } else if (!enabled && e->d.ep_ret) {
    (void)hipFree(e->d.ep_ret); (void)hipFree(e->d.ep_len); (void)hipFree(e->d.ep_acc);
    e->d.ep_ret = nullptr; e->d.ep_len = nullptr; e->d.ep_acc = nullptr;
  }
  return GAQ_OK;
}

int gaq_episode_stats(gaq_env* e, int64_t* episodes, double* return_sum, double* length_sum, double* return_sqsum, int32_t clear) {
  if (!e || !episodes || !return_sum || !length_sum || !return_sqsum) return fail(GAQ_ERR_INVALID, "null argument");
  if (!e->d.ep_acc) return fail(GAQ_ERR_STATE, "episode tracking is off (gaq_track_episodes)");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  double a[4];
  HIP_TRY(hipMemcpy(a, e->d.ep_acc, sizeof(a), hipMemcpyDeviceToHost));
  if (clear) HIP_TRY(hipMemset(e->d.ep_acc, 0, sizeof(a)));
  *episodes = (int64_t)(a[0] + 0.5); *return_sum = a[1]; *length_sum = a[2]; *return_sqsum = a[3];
  return GAQ_OK;
}

int gaq_get_counters(gaq_env* e, gaq_counters* out, uint32_t* episodes_out, uint32_t* resamples_out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  if (int rc_ = check_overrun(e)) return rc_;
  out->step_index = e->sc.step_index;
  if (e->d.step_ctr) { if (int rc_ = read_step_counter(e, &out->step_index)) return rc_; }   // graph replays advance only this one
  out->reset_calls = e->reset_calls;
  if ((episodes_out || resamples_out) && !e->d.traj) return fail(GAQ_ERR_STATE, "handle was created with per_env_params = 0: no per-env counts");
  const size_t bytes = sizeof(uint32_t) * (size_t)e->d.n;
  if (episodes_out) HIP_TRY(hipMemcpy(episodes_out, e->d.traj, bytes, hipMemcpyDeviceToHost));
  if (resamples_out) HIP_TRY(hipMemcpy(resamples_out, e->d.rcount, bytes, hipMemcpyDeviceToHost));
  return GAQ_OK;
}

int gaq_set_counters(gaq_env* e, const gaq_counters* in, const uint32_t* episodes, const uint32_t* resamples) {
  if (!e || !in) return fail(GAQ_ERR_INVALID, "null argument");
  if ((episodes || resamples) && !e->d.traj) return fail(GAQ_ERR_STATE, "handle was created with per_env_params = 0: no per-env counts");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  e->info_valid = false;
  e->sc.step_index = in->step_index;
  e->reset_calls = in->reset_calls;
  if (e->d.step_ctr) { if (int rc_ = write_step_counter(e, in->step_index)) return rc_; }
  HIP_TRY(hipMemset(e->d.done_count, 0, sizeof(uint32_t) * 2));
  const size_t bytes = sizeof(uint32_t) * (size_t)e->d.n;
  if (episodes) HIP_TRY(hipMemcpy(e->d.traj, episodes, bytes, hipMemcpyHostToDevice));
  if (resamples) {
    HIP_TRY(hipMemcpy(e->d.rcount, resamples, bytes, hipMemcpyHostToDevice));
    if (e->rz_on) { if (int rc = rebuild_params(e)) return rc; }   // the parameters are a function of (seed, global env index, resample count)
  }
  e->rz_refill_now = true;
  return GAQ_OK;
}

int gaq_set_graph_safe(gaq_env* e, int32_t enabled) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc_ = sync_handle(e)) return rc_;
  if (enabled && !e->d.step_ctr) {
    // replays advance the counters behind the host's back: per env, in the plane, from here on
    if (int rc_ = counters_to_plane(e, e->stream)) return rc_;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->uni.svd_known = false;
    if (int rc_ = write_step_counter(e, e->sc.step_index)) return rc_;
    e->d.step_ctr = e->step_ctr_mem;
  } else if (!enabled && e->d.step_ctr) {
    uint64_t v = 0;
    if (int rc_ = read_step_counter(e, &v)) return rc_;
    e->sc.step_index = v;
    e->d.step_ctr = nullptr;
  }
  return GAQ_OK;
}

int gaq_uniform_counters(gaq_env* e, int32_t* valid_out, uint32_t* word_out, int32_t* guard_intact_out) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  if (valid_out) *valid_out = e->uni.valid ? 1 : 0;
  if (word_out) *word_out = e->uni.word;
  if (guard_intact_out) {
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int rc_ = sync_handle(e)) return rc_;
    uint32_t g[kCtrGuardWords];
    HIP_TRY(hipMemcpy(g, e->d.ctr + e->d.ntiles * kTile, sizeof(g), hipMemcpyDeviceToHost));
    *guard_intact_out = 1;
    for (uint32_t w : g) if (w != kCtrGuard) *guard_intact_out = 0;
  }
  return GAQ_OK;
}

int gaq_set_timing(gaq_env* e, int32_t enabled) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  e->timing = enabled != 0; e->timed = false;
  return GAQ_OK;
}

int gaq_last_kernel_ms(gaq_env* e, float* ms_out) {
  if (!e || !ms_out) return fail(GAQ_ERR_INVALID, "null argument");
  if (!e->timed) return fail(GAQ_ERR_STATE, "no timed launch recorded (gaq_set_timing)");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipEventSynchronize(e->ev1));
  HIP_TRY(hipEventElapsedTime(ms_out, e->ev0, e->ev1));
  return GAQ_OK;
}

void* gaq_stream(gaq_env* e) { return e ? (void*)e->stream : nullptr; }

int gaq_synchronize(gaq_env* e) {
  if (!e) return fail(GAQ_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GAQ_OK;
}

int gaq_hbm_copy_dev(void* dst, const void* src, size_t bytes, void* stream) {
  if (!dst || !src) return fail(GAQ_ERR_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src) | bytes) & 15) return fail(GAQ_ERR_INVALID, "gaq_hbm_copy_dev: 16-byte alignment");
  const size_t n16 = bytes / 16;
  if (n16 == 0) return GAQ_OK;
  size_t blocks = (n16 + kBlock - 1) / kBlock;
  if (blocks > ((size_t)1 << 20)) blocks = (size_t)1 << 20;          // (grid-stride beyond 4 GiB)
  hipLaunchKernelGGL(hbm_copy_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, reinterpret_cast<const u32x4*>(src),
                     reinterpret_cast<u32x4*>(dst), n16);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

}  // extern "C"
