// gaq_policy.hip -- the device policies of libgaq (include/gaq.h gaq_policy): each engine's kernel, its LDS size and its entry in the engine
// table, every gaq_policy_* entry point and the closed-loop rollouts gaq_step_policy_many_dev / gaq_step_policy_ac_many_dev /
// gaq_step_policy_ac_term_many_dev.  Of the env core (gaq.hip) it uses the handle (gaq_host.hpp), launch_step for the per-step path and
// fused_variant / fused_rollout for the fused one; of the observation normaliser (gaq_learn.hip) what gaq_norm.hpp holds.
#include "gaq_host.hpp"
#include "gaq_norm.hpp"
#include "gaq_grad.hpp"

// the closed-loop rollout instantiations are compiled in gaq_inst.hip; here they are only declared
#define GAQ_X(FEAT) extern template __global__ GAQ_PROLL_SIG(FEAT)
GAQ_PROLL_ALL(GAQ_X)
#undef GAQ_X

namespace {

// obs [N, D] -> actions [N, 4]: the fallback path's policy launch (one wave per workgroup; LDS = the tile's rows + the scratch)
__global__ __launch_bounds__(kPolBlock) void policy_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, const float* __restrict__ obs, int D,
                                                           float* __restrict__ act_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lane = threadIdx.x & 63u;
  if (p.step_ctr) cfg.step_index = step_counter_peek(p, lane);            // graph-safe mode: the index of the step about to run
  const int64_t tile = (int64_t)blockIdx.x;
  if (tile >= p.ntiles) return;
  const int64_t i = tile * kTile + lane;
  const bool live = i < p.n;
  float* row = reinterpret_cast<float*>(smem) + lane * D;
  for (int k = 0; k < D; ++k) row[k] = live ? obs[i * D + k] : 0.0f;
  wave_lds_fence();
  float* scratch = reinterpret_cast<float*>(smem + ((kTile * D * 4 + 15) & ~15));
  float a[4];
  policy_eval(pol, row, scratch, lane, cfg.seed, cfg.env_offset + (uint64_t)i, cfg.step_index, a);
  if (live) *reinterpret_cast<float4*>(act_out + i * 4) = make_float4(a[0], a[1], a[2], a[3]);
}

// ---- the MFMA policy engine (GAQ_POLICY_ENGINE_MFMA): obs [N, D] -> actions [N, 4] on v_mfma_f32_16x16x4_f32 ---------------------------
// One workgroup = one tile of 64 envs, 4 waves.  The tile's activations live in ONE LDS buffer H[unit][64] (the observation rows first,
// each hidden layer's output over them in place); within a row env e sits at column pol_col(e), so that the 4 envs l, l+16, l+32, l+48 are
// side by side and one ds_read_b128 gives a lane its B operands for the tile's 4 env blocks (conflict-free: rows are 256 B).
// Per hidden layer wave w owns the output chunks c = w, w+4, w+8, w+12 (16 units each; up to 4 for a 256-wide layer): D[unit][env] =
// bias + sum_k A[unit][k] B[k][env] with A = the packed W'[c][k][16] (64 contiguous floats per k-step: one coalesced dword per lane,
// straight from L1/L2) and B = H.  The accumulators start at the bias and the k-steps ascend, and each MFMA is a k-ordered fmaf chain
// (cdna_hip_programming.md "FP32-input MFMA"): bit for bit policy_eval's VALU chain.  The first layer's K = in_dim is padded to a multiple
// of 4 with A = +0 (the weights past k = in_dim - 1 are never read) and B = -0: +0 x -0 = -0 adds nothing to any accumulator, -0 included.
// The accumulators stay in registers (4 chunks x 4 env blocks x 4 = 64 VGPRs at width 256) until every wave has read the layer's input
// (barrier), then go through pol_act into H.  The 4 outputs run on the VALU, wave o summing output o over the last layer's units in
// ascending order (wave-uniform weights: scalar loads), as policy_eval does; wave 0 finishes them with policy_out_tail.
// The kernel, the GRU engine's and the actor-critic and terminal-value forms of both are compositions of one set of stages ("the stages
// the six fp32-MFMA kernels are composed of", below).
// LDS = 1 KiB (the 4 x 64 output sums) + 256 B x max(in_dim rounded up to 4, widest layer): 65 KiB at width 256, two tiles per CU.
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kPolMfmaWaves = 4;
constexpr int kPolMfmaBlock = kPolMfmaWaves * kTile;
constexpr int kPolMfmaMaxWidth = 256;
constexpr int kPolMfmaOutBytes = 4 * kTile * 4;
__device__ __forceinline__ int pol_col(int e) { return (e & 15) * 4 + (e >> 4); }

// this wave's NC chunks of one hidden layer (`in` inputs: the rows 0 .. in-1 of H, zero-padded to a multiple of 4) into acc[chunk][env block]
template <int NC, int Kernel>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ wl, int in, int width, int wave, const float* H, uint32_t lane,
                                           f32x4 (&acc)[4][4]) {
  const int h = (int)(lane >> 4);
  const float* bl = wl + width * in;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const float* b = bl + (wave + 4 * j) * 16 + 4 * h;
    const f32x4 b4 = {b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[j][eb] = b4;
  }
  const float* hrow = H + h * kTile + (lane & 15) * 4;
  auto kstep = [&](const f32x4& x, const float (&a)[NC]) {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[j][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], x[eb], acc[j][eb], 0, 0, 0);
    }
  };
  auto xload = [&](int k0) { return *reinterpret_cast<const f32x4*>(hrow + k0 * kTile); };
  auto wload = [&](int k0, float (&a)[NC]) {
#pragma unroll
    for (int j = 0; j < NC; ++j) a[j] = wl[((wave + 4 * j) * in + k0) * 16 + lane];
  };
  const int kfull = in & ~3;
  if (kfull > 0) {
    // two operand sets in turn: the loads of one k-step are issued before the MFMAs of the previous one (the sched barriers keep the
    // scheduler from sinking them back under the MFMAs); a clamped index re-loads an in-bounds step where there is no next one
    float a0[NC], a1[NC];
    wload(0, a0);
    f32x4 x0 = xload(0), x1;
    int k0 = 0;
#pragma unroll 1
    for (; k0 + 8 <= kfull; k0 += 8) {
      wload(k0 + 4, a1);
      x1 = xload(k0 + 4);
      __builtin_amdgcn_sched_barrier(0);
      kstep(x0, a0);
      __builtin_amdgcn_sched_barrier(0);
      const int kn = k0 + 8 < kfull ? k0 + 8 : k0 + 4;
      wload(kn, a0);
      x0 = xload(kn);
      __builtin_amdgcn_sched_barrier(0);
      kstep(x1, a1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (k0 < kfull) kstep(x0, a0);                                // an odd number of full k-steps (first layer only)
  }
  if (kfull < in) {                                               // the first layer's last, partial k-step
    float a[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) a[j] = kfull + h < in ? wl[((wave + 4 * j) * in + kfull) * 16 + lane] : 0.0f;
    kstep(xload(kfull), a);
  }
}

template <int NC, int Kernel>
__device__ __forceinline__ void mfma_store(const f32x4 (&acc)[4][4], int act, int wave, float* H, uint32_t lane) {
  const int h = (int)(lane >> 4);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x4 v = {pol_act(act, acc[j][0][r]), pol_act(act, acc[j][1][r]), pol_act(act, acc[j][2][r]), pol_act(act, acc[j][3][r])};
      *reinterpret_cast<f32x4*>(H + ((wave + 4 * j) * 16 + 4 * h + r) * kTile + (lane & 15) * 4) = v;
    }
  }
}

// ---- actor-critic outputs (gaq_step_policy_ac_many_dev): what policy_mfma_ac_kernel / policy_gru_ac_kernel write beside the action -------
// A struct of its own, so that PolicyDev and with it the arguments of every existing policy launch stay as they were.
// V = w_v . y + b_v over the rows y the 4-output layer reads: wave w sums its quarter of the units in ascending order (one fmaf chain from 0;
// the widths are multiples of 16), wave 0 adds the four partial sums as (s0 + s1) + (s2 + s3) and then the bias: deterministic, and a
// different order from the 4 output sums', which promise VALU bit-compatibility where V promises none.  The partial sums take 1 KiB of LDS
// between the output sums and the activation rows.  value_only: the bootstrap launch after the last step writes V alone -- no action, no
// draw and, for a GRU, no h'.
struct PolicyAcDev {
  const float* wv;                // the value head: last width weights, then the bias (nullptr: no V asked for)
  float* value_out;               // [N]
  float* logp_out;                // [N], or nullptr
  float log_std[4];               // the caller's, as given to gaq_policy_set_explore (PolicyDev keeps exp() of them); 0 in device mode
  int32_t value_only;
};
constexpr int kPolAcBytes = kPolMfmaWaves * kTile * 4;
constexpr float kTwoLn2Pi = 3.67575413281869f;

// ---- exploration from device memory (gaq_policy_set_explore_dev) ---------------------------------------------------------------------------
// A policy in device mode has PolicyDev::explore = kPolExploreDev, and the 8 bytes of std4[0 .. 1] hold the address of the caller's table
// of 12 floats, log_std[4] | std[4] | inv_std[4]: PolicyDev and with it the arguments of every policy launch keep their layout, and no
// launch of such a policy carries a value of log_std.  Only the kernels of this file, gaq_policy_grad.hip and gaq_policy_grad_seq.hip know
// the mode (the VALU and bf16 engines refuse it); they read the words where they use them, as wave-uniform loads, like the weights an
// optimiser stepped in an earlier launch.
constexpr int kPolExploreDev = 2;
constexpr int kExploreStd = 4, kExploreInvStd = 8, kExploreWords = 12;   // float offsets in the table
__device__ __forceinline__ kconst_float* pol_explore_tab(const PolicyDev& P) {
  uint64_t a;
  __builtin_memcpy(&a, P.std4, sizeof(a));
  return (kconst_float*)a;
}
// the std of this launch's draw: the table's, or the host's in the arguments
__device__ __forceinline__ void pol_explore_std(const PolicyDev& P, float (&sd)[4]) {
  if (P.explore == kPolExploreDev) {
    kconst_float* tab = pol_explore_tab(P);
#pragma unroll
    for (int o = 0; o < 4; ++o) sd[o] = tab[kExploreStd + o];
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o) sd[o] = P.std4[o];
  }
}
// policy_out_tail (gaq_kernels.hpp) for the kernels of this file: the same tanh, the same draw, the same fmaf, std from either place
__device__ __forceinline__ void policy_out_tail_dev(const PolicyDev& P, uint64_t seed, uint64_t env, uint64_t step, float out[4]) {
  if (P.out_tanh) {
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = tanhf(out[o]);
  }
  if (P.explore) {
    float z[4], sd[4];
    const gaq::Philox r(seed, env, step, gaq::RNG_POLICY);
    gaq::normals4(r, z);
    pol_explore_std(P, sd);
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = __builtin_fmaf(sd[o], z[o], out[o]);
  }
}

// policy_out_tail that also returns log N(a; mean, std) of the action it draws: sum_k (-z_k^2 / 2 - log_std_k) - 2 ln 2 pi, k ascending.
// The same draw (same Philox key) and the same fmaf as policy_out_tail: the actions are its bits.  No Jacobian term: the noise is added
// after the output tanh.
__device__ __forceinline__ float policy_out_tail_ac(const PolicyDev& P, const PolicyAcDev& ac, uint64_t seed, uint64_t env, uint64_t step,
                                                    float out[4]) {
  if (P.out_tanh) {
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = tanhf(out[o]);
  }
  float lp = 0.0f;
  if (P.explore) {
    float z[4], sd[4], ls[4];
    const gaq::Philox r(seed, env, step, gaq::RNG_POLICY);
    gaq::normals4(r, z);
    pol_explore_std(P, sd);
    if (P.explore == kPolExploreDev) {
      kconst_float* tab = pol_explore_tab(P);
#pragma unroll
      for (int o = 0; o < 4; ++o) ls[o] = tab[o];
    } else {
#pragma unroll
      for (int o = 0; o < 4; ++o) ls[o] = ac.log_std[o];
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = __builtin_fmaf(sd[o], z[o], out[o]);
#pragma unroll
    for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
    lp -= kTwoLn2Pi;
  }
  return lp;
}

// this wave's quarter of V for env `lane` (y: the env's column of the last layer's rows) -> vsum[wave][lane]
// (Kernel, here and in the other value stages: the separate-critic kernels pass their tags, so that the instantiation the six kernels
// above share -- 0 -- has the callers it had and those kernels stay instruction for instruction what they were)
template <int Kernel = 0>
__device__ __forceinline__ void policy_value_part(const PolicyAcDev& ac, const float* ycol, int in, int wave, uint32_t lane, float* vsum) {
  kconst_float* wv = as_const(ac.wv);
  const int q = in / kPolMfmaWaves;
  float v = 0.0f;
#pragma unroll 8
  for (int u = wave * q; u < (wave + 1) * q; ++u) v = __builtin_fmaf(wv[u], ycol[u * kTile], v);
  vsum[wave * kTile + lane] = v;
}
// wave 0, after the barrier: the four parts and the bias
template <int Kernel = 0>
__device__ __forceinline__ float policy_value_sum(const PolicyAcDev& ac, int in, uint32_t lane, const float* vsum) {
  return ((vsum[lane] + vsum[kTile + lane]) + (vsum[2 * kTile + lane] + vsum[3 * kTile + lane])) + as_const(ac.wv)[in];
}

// ---- the stages the six fp32-MFMA kernels are composed of --------------------------------------------------------------------------------
// policy_mfma_kernel and policy_gru_kernel, their actor-critic forms and their gathered terminal-value forms (below) are each a list of
// these stages plus the lines that make the form; the barriers between the stages stand in the kernels.  Every stage is written once and
// inlined into each kernel, so the six share their arithmetic by construction: each fmaf chain, the bias-first accumulators, the ascending
// k-steps and the -0 padding are one piece of text.
// Kernel: each kernel passes its own number (0 .. 5) to mfma_hidden and gru_cell, which hand it to mfma_layer / mfma_store / cell_kloop, so
// that each kernel inlines instantiations of its own.  It steers code generation only: without it policy_mfma_kernel and its two forms
// compile to 164 VGPRs instead of the recorded 166 and policy_gru_kernel to 166 instead of 164; with it
// every line of profiles/r12_kernel_resources.txt is the one recorded for the written-out kernels (r09 .. r11).
// (The separate-critic kernels pass 6, 7, 8 and the LSTM engine's three kernels 9, 10, 11, for the same reason.)
// Each of these kernels is a template over a trailing parameter pack with two instantiations: the empty pack, which is the kernel as
// described, and <PolObsNorm>, which stages the observations through a normaliser's table.  pol_tag (below) gives the second one the
// first's number + 16, so that the two inline instantiations of their own as well.

// the workgroup's tile: rows first .. first + nlive - 1 of the batch, or those slots of the gathered list
struct PolTile {
  uint32_t lane;
  int wave;
  int64_t first;
  int nlive;
};
// which row of the batch lane / slot e of the tile is: the tile's own rows, or the listed envs (read for e < nlive only)
struct PolRowBatch {
  int64_t first;
  __device__ __forceinline__ int64_t operator()(int e) const { return first + e; }
};
struct PolRowList {
  const uint32_t* list;
  int64_t first;
  __device__ __forceinline__ int64_t operator()(int e) const { return (int64_t)list[first + e]; }
};

// tile blockIdx.x of `rows` rows
__device__ __forceinline__ void pol_tile_span(PolTile& t, int64_t rows) {
  t.lane = threadIdx.x & 63u;
  t.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  t.first = (int64_t)blockIdx.x * kTile;
  t.nlive = (int)((rows - t.first) < kTile ? (rows - t.first) : kTile);
}
// the batch form (false: a workgroup past the last tile); graph-safe mode: cfg.step_index <- the index of the step about to run
__device__ __forceinline__ bool pol_tile_batch(PolTile& t, const DevPtrs& p, StepCfg& cfg) {
  pol_tile_span(t, p.n);
  if (t.wave == 0 && p.step_ctr) cfg.step_index = step_counter_peek(p, t.lane);
  return (int64_t)blockIdx.x < p.ntiles;
}
// the gathered form: the list's slots (false: all but the first few workgroups)
__device__ __forceinline__ bool pol_tile_list(PolTile& t, const uint32_t* count) {
  const int64_t rows = (int64_t)*count;
  pol_tile_span(t, rows);
  return t.first < rows;
}

// the Kernel number of an instantiation: the kernel's own for the empty pack, + 16 for <PolObsNorm> (the one place the 16 comes from)
template <int Base, class... Norm>
constexpr int pol_tag = Base + 16 * (int)sizeof...(Norm);
// the number the value stages (policy_value_part, policy_value_store, policy_ac_tail) take in the kernels 2 .. 5: their plain
// instantiations share the stages' instantiation 0, as the four kernels always did (with numbers of their own policy_gru_ac_kernel<>
// and policy_gru_term_kernel<> differ from the recorded kernels in 19 and 13 lines)
template <int Base, class... Norm>
constexpr int pol_value_tag = sizeof...(Norm) ? pol_tag<Base, Norm...> : 0;
// one staged input of policy_mfma_bf16_kernel, which stages in a loop of its own: as it is, or through the table
__device__ __forceinline__ float pol_stage_elem(float x, int) { return x; }
__device__ __forceinline__ float pol_stage_elem(float x, int k, const PolObsNorm& nm) { return nm(x, k); }

// the tile's observations -> X rows 0 .. kin-1, env e at column pol_col(e) (dead envs / slots past the count 0, padded inputs -0)
template <class Row>
__device__ __forceinline__ void pol_stage_obs(float* X, const float* obs, int D, const PolTile& t, Row row) {
  const int kin = (D + 3) & ~3;
  for (int f = (int)threadIdx.x; f < kTile * kin; f += kPolMfmaBlock) {
    const int e = f / kin, k = f - e * kin;
    X[k * kTile + pol_col(e)] = k >= D ? -0.0f : e < t.nlive ? obs[row(e) * D + k] : 0.0f;
  }
}
// the same through a normaliser's table (the <PolObsNorm> instantiations): live inputs only -- dead lanes stay 0 and padded inputs -0
template <class Row>
__device__ __forceinline__ void pol_stage_obs(float* X, const float* obs, int D, const PolTile& t, Row row, const PolObsNorm& nm) {
  const int kin = (D + 3) & ~3;
  for (int f = (int)threadIdx.x; f < kTile * kin; f += kPolMfmaBlock) {
    const int e = f / kin, k = f - e * kin;
    X[k * kTile + pol_col(e)] = k >= D ? -0.0f : e < t.nlive ? nm(obs[row(e) * D + k], k) : 0.0f;
  }
}

// the hidden layers l0 .. n_hidden-1 over the rows of H in place (`in` inputs to layer l0); returns the last layer's width.  Wave-uniform
// nc: every wave meets both barriers of every layer.
template <int Kernel>
__device__ __forceinline__ int mfma_hidden(const PolicyDev& pol, int l0, int in, float* H, const PolTile& t) {
#pragma unroll 1
  for (int l = l0; l < pol.n_hidden; ++l) {
    const int width = pol.width[l];
    const float* wl = pol.w + pol.off[l];
    const int nc = (width / 16 - t.wave + 3) / 4;                 // chunks wave, wave + 4, ... below width / 16
    f32x4 acc[4][4];
    switch (nc) {
      case 1: mfma_layer<1, Kernel>(wl, in, width, t.wave, H, t.lane, acc); break;
      case 2: mfma_layer<2, Kernel>(wl, in, width, t.wave, H, t.lane, acc); break;
      case 3: mfma_layer<3, Kernel>(wl, in, width, t.wave, H, t.lane, acc); break;
      case 4: mfma_layer<4, Kernel>(wl, in, width, t.wave, H, t.lane, acc); break;
      default: break;
    }
    __syncthreads();                                              // every wave has read the layer's input
    switch (nc) {
      case 1: mfma_store<1, Kernel>(acc, pol.hidden_act, t.wave, H, t.lane); break;
      case 2: mfma_store<2, Kernel>(acc, pol.hidden_act, t.wave, H, t.lane); break;
      case 3: mfma_store<3, Kernel>(acc, pol.hidden_act, t.wave, H, t.lane); break;
      case 4: mfma_store<4, Kernel>(acc, pol.hidden_act, t.wave, H, t.lane); break;
      default: break;
    }
    __syncthreads();
    in = width;
  }
  return in;
}

// output `wave` of env `lane` (y: the env's column of the last layer's rows): the bias, then the units in ascending order -> outs[wave][lane]
__device__ __forceinline__ void policy_out_part(const PolicyDev& pol, const float* ycol, int in, const PolTile& t, float* outs) {
  kconst_float* wo = as_const(pol.w + pol.off[pol.n_hidden]);
  float s = wo[in * 4 + t.wave];
#pragma unroll 8
  for (int u = 0; u < in; ++u) s = __builtin_fmaf(wo[u * 4 + t.wave], ycol[u * kTile], s);
  outs[t.wave * kTile + t.lane] = s;
}
// the value tail, wave 0's half after the barrier that follows policy_value_part: V of env / slot `lane` -> value_out[its row]
template <int Kernel = 0, class Row>
__device__ __forceinline__ void policy_value_store(const PolicyAcDev& ac, int in, const PolTile& t, const float* vsum, Row row) {
  const float v = policy_value_sum<Kernel>(ac, in, t.lane, vsum);
  if ((int)t.lane < t.nlive) ac.value_out[row((int)t.lane)] = v;
}
// wave 0, after the barrier: the env's 4 sums -> its action
__device__ __forceinline__ void policy_act_tail(const PolicyDev& pol, const StepCfg& cfg, const PolTile& t, const float* outs, float* act_out) {
  float a[4] = {outs[t.lane], outs[kTile + t.lane], outs[2 * kTile + t.lane], outs[3 * kTile + t.lane]};
  const int64_t i = t.first + t.lane;
  policy_out_tail_dev(pol, cfg.seed, cfg.env_offset + (uint64_t)i, cfg.step_index, a);
  if ((int)t.lane < t.nlive) *reinterpret_cast<float4*>(act_out + i * 4) = make_float4(a[0], a[1], a[2], a[3]);
}
// the same for the actor-critic forms: V, then (unless this is the bootstrap launch) the action and its log-probability
template <int Kernel = 0>
__device__ __forceinline__ void policy_ac_tail(const PolicyDev& pol, const PolicyAcDev& ac, const StepCfg& cfg, int in, const PolTile& t,
                                               const float* outs, const float* vsum, float* act_out) {
  if (ac.wv) policy_value_store<Kernel>(ac, in, t, vsum, PolRowBatch{t.first});
  if (ac.value_only) return;                                      // the bootstrap launch: V alone
  float a[4] = {outs[t.lane], outs[kTile + t.lane], outs[2 * kTile + t.lane], outs[3 * kTile + t.lane]};
  const int64_t i = t.first + t.lane;
  const float lp = policy_out_tail_ac(pol, ac, cfg.seed, cfg.env_offset + (uint64_t)i, cfg.step_index, a);
  if ((int)t.lane < t.nlive && ac.logp_out) ac.logp_out[i] = lp;
  if ((int)t.lane < t.nlive) *reinterpret_cast<float4*>(act_out + i * 4) = make_float4(a[0], a[1], a[2], a[3]);
}

// (2 waves per SIMD: 158 VGPRs, no spill; the compiler's own choice was 100 VGPRs + 177 AGPRs = one wave per SIMD)
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_mfma_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, const float* __restrict__ obs, int D, float* __restrict__ act_out,
                        Norm... nm) {
  constexpr int Tag = pol_tag<0, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* outs = reinterpret_cast<float*>(smem);                   // [4][64] output sums
  float* H = reinterpret_cast<float*>(smem + kPolMfmaOutBytes);   // [rows][64] activations
  PolTile t;
  if (!pol_tile_batch(t, p, cfg)) return;
  pol_stage_obs(H, obs, D, t, PolRowBatch{t.first}, nm...);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 0, pol.in_dim, H, t);
  policy_out_part(pol, H + pol_col((int)t.lane), in, t, outs);
  __syncthreads();
  if (t.wave == 0) policy_act_tail(pol, cfg, t, outs, act_out);
}

// policy_mfma_kernel's actor-critic form: the same stages, then V's parts beside the 4 output sums
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_mfma_ac_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, PolicyAcDev ac, const float* __restrict__ obs, int D,
                           float* __restrict__ act_out, Norm... nm) {
  constexpr int Tag = pol_tag<2, Norm...>, VTag = pol_value_tag<2, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* outs = reinterpret_cast<float*>(smem);                   // [4][64] output sums
  float* vsum = reinterpret_cast<float*>(smem + kPolMfmaOutBytes);   // [4][64] parts of V
  float* H = reinterpret_cast<float*>(smem + kPolMfmaOutBytes + kPolAcBytes);   // [rows][64] activations
  PolTile t;
  if (!pol_tile_batch(t, p, cfg)) return;
  pol_stage_obs(H, obs, D, t, PolRowBatch{t.first}, nm...);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 0, pol.in_dim, H, t);
  const float* y = H + pol_col((int)t.lane);
  if (ac.wv) policy_value_part<VTag>(ac, y, in, t.wave, t.lane, vsum);
  if (!ac.value_only) policy_out_part(pol, y, in, t, outs);
  __syncthreads();
  if (t.wave == 0) policy_ac_tail<VTag>(pol, ac, cfg, in, t, outs, vsum, act_out);
}

// ---- the GRU policy engine (gaq_policy_desc_rnn, GAQ_POLICY_CELL_GRU): [obs | h] -> h' -> head -> actions on v_mfma_f32_16x16x4_f32 ------
// One workgroup = one tile of 64 envs, 4 waves, the MFMA engine's operand layout (pol_col columns, one coalesced weight dword per lane).
// LDS: the 4 x 64 output sums, X = the observation rows (kin = in_dim rounded up to 4, padded with -0) then the H rows of h (rows of envs
// that reported done in the previous step, and dead lanes, are 0), then S = max(H, head widths) rows that receive h' and then the head's
// activations in place.  The gate units of 16-unit chunk c are the rows c, c + H/16, c + 2H/16 of W_ih' / W_hh' (gate order r, z, n).
// Wave w takes the chunks c = w, w + 4, ... one at a time with four accumulator sets: r and z start at b_i + b_h and take the x products
// then the h products (each an ascending fmaf chain), n keeps n_x = b_in + W_in x and n_h = b_hn + W_hn h apart (torch applies r to n_h).
// Then n = tanh(n_x + r n_h), h' = n + z (h - n) go to S and to the caller's row (each tile owns its rows: in place is safe) before the
// next chunk, so only one chunk's 64 accumulator registers are live at a time.  The head layers and the output are policy_mfma_kernel's.
// LDS = 1 KiB + 256 B x (kin + H + max(H, head widths)): 134 KiB at H = 256 with 18 inputs (one tile per CU), 70 KiB at H = 128.
struct PolicyGruDev {
  float* h;                       // the caller's [N, H] state: read, then overwritten with h'
  const uint8_t* done_prev;       // done [N] of the previous step of this call (those rows start from h = 0), or nullptr
  int32_t hid;                    // H
  int32_t off_hh;                 // float offset of W_hh' in pol.w (W_ih' is at pol.off[0]; pol.off[1..] are the head's layers)
};

// the chunks c, c + cs, ... c + (NG-1) cs -- one per gate -- of one product of a recurrent cell (`in` inputs: the rows 0 .. in-1 of X,
// zero-padded to a multiple of 4) accumulated into acc[0 .. NG-2] and, the last gate, acc[JL]: mfma_layer's k-loop without its bias.
// (GRU: <3, 2> for the x product and <3, 3> for the h product, which keep n_x and n_h apart; LSTM: <4, 3> for both.)
template <int NG, int JL, int Kernel>
__device__ __forceinline__ void cell_kloop(const float* __restrict__ wl, int in, int c, int cs, const float* X, uint32_t lane,
                                          f32x4 (&acc)[4][4]) {
  const int h = (int)(lane >> 4);
  const float* xrow = X + h * kTile + (lane & 15) * 4;
  auto kstep = [&](const f32x4& x, const float (&a)[NG]) {
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int s = j == NG - 1 ? JL : j;
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[s][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], x[eb], acc[s][eb], 0, 0, 0);
    }
  };
  auto xload = [&](int k0) { return *reinterpret_cast<const f32x4*>(xrow + k0 * kTile); };
  auto wload = [&](int k0, float (&a)[NG]) {
#pragma unroll
    for (int j = 0; j < NG; ++j) a[j] = wl[((c + j * cs) * in + k0) * 16 + lane];
  };
  const int kfull = in & ~3;
  if (kfull > 0) {
    float a0[NG], a1[NG];
    wload(0, a0);
    f32x4 x0 = xload(0), x1;
    int k0 = 0;
#pragma unroll 1
    for (; k0 + 8 <= kfull; k0 += 8) {
      wload(k0 + 4, a1);
      x1 = xload(k0 + 4);
      __builtin_amdgcn_sched_barrier(0);
      kstep(x0, a0);
      __builtin_amdgcn_sched_barrier(0);
      const int kn = k0 + 8 < kfull ? k0 + 8 : k0 + 4;
      wload(kn, a0);
      x0 = xload(kn);
      __builtin_amdgcn_sched_barrier(0);
      kstep(x1, a1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (k0 < kfull) kstep(x0, a0);
  }
  if (kfull < in) {                                               // the x product's last, partial k-step
    float a[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) a[j] = kfull + h < in ? wl[((c + j * cs) * in + kfull) * 16 + lane] : 0.0f;
    kstep(xload(kfull), a);
  }
}

__device__ __forceinline__ float gru_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// the LDS regions of a GRU kernel after the sums' `head` bytes: X = [kin + H][64] (the observation, then h at Xh), S = [max(H, head
// widths)][64] (h', then the head's activations)
struct GruLds {
  float *X, *Xh, *S;
};
__device__ __forceinline__ GruLds gru_lds(char* smem, int head, int D, int hid) {
  GruLds m;
  m.X = reinterpret_cast<float*>(smem + head);
  m.Xh = m.X + ((D + 3) & ~3) * kTile;
  m.S = m.Xh + hid * kTile;
  return m;
}

// this lane's row of h (hrow; keep = false: a dead lane or a row that starts over, read as 0) -> Xh: lane = env / slot (conflict-free
// LDS rows), 4 units per 16-byte load.  Which row and whether it is kept is what differs between the forms, and stands in the kernels
// (taking a row functor and the mask here instead cost the two step kernels 2 VGPRs: 166 against the recorded 164).
__device__ __forceinline__ void gru_stage_h(float* Xh, const float* hrow, bool keep, int hid, const PolTile& t) {
  const int e = (int)t.lane;
  for (int q = t.wave; q < hid / 4; q += kPolMfmaWaves) {
    const f32x4 v = keep ? *reinterpret_cast<const f32x4*>(hrow + 4 * q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r) Xh[(4 * q + r) * kTile + pol_col(e)] = v[r];
  }
}

// the cell over X = [obs | h]: h' -> S and, with write_back, to the rows first .. of the caller's state (the batch forms only)
template <int Kernel>
__device__ __forceinline__ void gru_cell(const PolicyDev& pol, const PolicyGruDev& g, const GruLds& m, const PolTile& t, bool write_back) {
  const int hid = g.hid, hc = hid / 16;
  const float* wih = pol.w + pol.off[0];
  const float* bih = wih + 3 * hid * pol.in_dim;
  const float* whh = pol.w + g.off_hh;
  const float* bhh = whh + 3 * hid * hid;
  const uint32_t lane = t.lane;
  const int h4 = (int)(lane >> 4);
#pragma unroll 1
  for (int c = t.wave; c < hc; c += kPolMfmaWaves) {
    const int u0 = c * 16 + 4 * h4;                               // this lane's 4 units of the chunk
    f32x4 acc[4][4];                                              // r, z, n_x, n_h
    {
      f32x4 b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        b[0][r] = bih[u0 + r] + bhh[u0 + r];
        b[1][r] = bih[hid + u0 + r] + bhh[hid + u0 + r];
        b[2][r] = bih[2 * hid + u0 + r];
        b[3][r] = bhh[2 * hid + u0 + r];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) acc[s][eb] = b[s];
    }
    cell_kloop<3, 2, Kernel>(wih, pol.in_dim, c, hc, m.X, lane, acc);
    cell_kloop<3, 3, Kernel>(whh, hid, c, hc, m.Xh, lane, acc);
    f32x4 hn[4];                                                  // h' per env block
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float hold = m.Xh[(u0 + r) * kTile + (lane & 15) * 4 + eb];
        const float rg = gru_sigmoid(acc[0][eb][r]), zg = gru_sigmoid(acc[1][eb][r]);
        const float n = tanhf(__builtin_fmaf(rg, acc[3][eb][r], acc[2][eb][r]));
        hn[eb][r] = __builtin_fmaf(zg, hold - n, n);
      }
      const int e = eb * 16 + (int)(lane & 15);
      if (write_back && e < t.nlive) *reinterpret_cast<f32x4*>(g.h + (t.first + e) * hid + u0) = hn[eb];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x4 v = {hn[0][r], hn[1][r], hn[2][r], hn[3][r]};
      *reinterpret_cast<f32x4*>(m.S + (u0 + r) * kTile + (lane & 15) * 4) = v;
    }
  }
}

// h <- GRU(obs, h) with the rows that finished in the previous step (g.done_prev) started from 0, the head over S, the action
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_gru_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, PolicyGruDev g, const float* __restrict__ obs, int D,
                       float* __restrict__ act_out, Norm... nm) {
  constexpr int Tag = pol_tag<1, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* outs = reinterpret_cast<float*>(smem);                   // [4][64] output sums
  const GruLds m = gru_lds(smem, kPolMfmaOutBytes, D, g.hid);
  PolTile t;
  if (!pol_tile_batch(t, p, cfg)) return;
  const PolRowBatch row{t.first};
  pol_stage_obs(m.X, obs, D, t, row, nm...);
  const bool keep = (int)t.lane < t.nlive && !(g.done_prev && g.done_prev[t.first + t.lane]);
  gru_stage_h(m.Xh, g.h + (t.first + t.lane) * g.hid, keep, g.hid, t);
  __syncthreads();
  gru_cell<Tag>(pol, g, m, t, true);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 1, g.hid, m.S, t);           // the head: the hidden layers 1 .. n_hidden-1 over S in place
  policy_out_part(pol, m.S + pol_col((int)t.lane), in, t, outs);
  __syncthreads();
  if (t.wave == 0) policy_act_tail(pol, cfg, t, outs, act_out);
}

// policy_gru_kernel's actor-critic form: V from the rows the output layer reads; the bootstrap launch (value_only) computes h' into S as
// ever but leaves the caller's state alone
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_gru_ac_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, PolicyGruDev g, PolicyAcDev ac, const float* __restrict__ obs, int D,
                          float* __restrict__ act_out, Norm... nm) {
  constexpr int Tag = pol_tag<3, Norm...>, VTag = pol_value_tag<3, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* outs = reinterpret_cast<float*>(smem);                   // [4][64] output sums
  float* vsum = reinterpret_cast<float*>(smem + kPolMfmaOutBytes);   // [4][64] parts of V
  const GruLds m = gru_lds(smem, kPolMfmaOutBytes + kPolAcBytes, D, g.hid);
  PolTile t;
  if (!pol_tile_batch(t, p, cfg)) return;
  const PolRowBatch row{t.first};
  pol_stage_obs(m.X, obs, D, t, row, nm...);
  const bool keep = (int)t.lane < t.nlive && !(g.done_prev && g.done_prev[t.first + t.lane]);
  gru_stage_h(m.Xh, g.h + (t.first + t.lane) * g.hid, keep, g.hid, t);
  __syncthreads();
  gru_cell<Tag>(pol, g, m, t, !ac.value_only);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 1, g.hid, m.S, t);
  const float* y = m.S + pol_col((int)t.lane);
  if (ac.wv) policy_value_part<VTag>(ac, y, in, t.wave, t.lane, vsum);
  if (!ac.value_only) policy_out_part(pol, y, in, t, outs);
  __syncthreads();
  if (t.wave == 0) policy_ac_tail<VTag>(pol, ac, cfg, in, t, outs, vsum, act_out);
}

// rows of a [N, H] hidden state (H a multiple of 4, 16-byte aligned) whose mask byte is non-zero (every row for nullptr) <- 0
__global__ __launch_bounds__(kBlock) void hidden_zero_kernel(float* __restrict__ h, const uint8_t* __restrict__ mask, int64_t n, int hid) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t per = hid / 4;
  if (q >= n * per) return;
  if (mask && !mask[q / per]) return;
  reinterpret_cast<float4*>(h)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- time-limit bootstrapping (gaq_step_policy_ac_term_many_dev): V of the terminal observations, on compacted rows ---------------------
// Dones are sparse (about N / L envs per step with staggered episodes of L steps), so the terminal pass does not run over the batch: after
// step t's launch term_gather_kernel compacts the indices of the envs with done[t] into `list`, and a value-only form of the actor-critic
// kernel of the policy's engine runs on those rows alone -- lane e of workgroup b is env list[64 b + e], its observation the env's row of
// the terminal-observation buffer (the row step t's launch has just written) and, for a GRU, its h the env's row of the registered state
// as policy launch t left it, unmasked.  Which slot an env gets depends on the order in which the waves' atomics arrive, and changes
// nothing: V of an env is a function of its own column of the tile alone (each MFMA column, each fmaf chain of policy_value_part and the
// sum of policy_value_sum are per env), so the bits are those the env would get in any slot of any tile -- the bits value_out[t + 1]
// would have held had the episode gone on.
struct PolicyTermDev {
  const uint32_t* list;           // the envs that reported done in this step, in the order the atomics handed out the slots
  const uint32_t* count;          // how many
  const float* term_obs;          // [N, D] terminal observations (only the listed rows are read)
};

// done [N] of one step -> list / *count (one ballot, one popcount and one vector atomic add per wave that holds a done), row <- +0
// (every element of the row is written here; the value pass then overwrites the listed ones), *count_next <- 0 for the next step's gather
// (its last reader, the value pass of the step before, has finished: the launches are in stream order)
__global__ __launch_bounds__(kBlock) void term_gather_kernel(const uint8_t* __restrict__ done, int64_t n, uint32_t* __restrict__ list,
                                                             uint32_t* __restrict__ count, uint32_t* __restrict__ count_next,
                                                             float* __restrict__ row) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) *count_next = 0u;
  const bool d = i < n && done[i] != 0;
  if (i < n) row[i] = 0.0f;
  const uint64_t m = __ballot(d);                                 // (every lane of the wave is here: none has returned)
  if (m == 0) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
  if (d) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)i;
}

// policy_mfma_ac_kernel's value-only launch on gathered rows.  The LDS layout is that kernel's (the output sums' 1 KiB unused), so the
// launch's LDS size is too.  Writes ac.value_out[env] of the listed envs and nothing else.
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_mfma_term_kernel(PolicyDev pol, PolicyAcDev ac, PolicyTermDev tm, int D, Norm... nm) {
  constexpr int Tag = pol_tag<4, Norm...>, VTag = pol_value_tag<4, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* vsum = reinterpret_cast<float*>(smem + kPolMfmaOutBytes);   // [4][64] parts of V
  float* H = reinterpret_cast<float*>(smem + kPolMfmaOutBytes + kPolAcBytes);   // [rows][64] activations
  PolTile t;
  if (!pol_tile_list(t, tm.count)) return;
  const PolRowList row{tm.list, t.first};
  pol_stage_obs(H, tm.term_obs, D, t, row, nm...);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 0, pol.in_dim, H, t);
  policy_value_part<VTag>(ac, H + pol_col((int)t.lane), in, t.wave, t.lane, vsum);
  __syncthreads();
  if (t.wave == 0) policy_value_store<VTag>(ac, in, t, vsum, row);
}

// policy_gru_ac_kernel's value-only launch on gathered rows: h is the listed env's row of the registered state as it is -- no done mask --
// and is only read; h' lives in S alone.
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_gru_term_kernel(PolicyDev pol, PolicyGruDev g, PolicyAcDev ac, PolicyTermDev tm, int D, Norm... nm) {
  constexpr int Tag = pol_tag<5, Norm...>, VTag = pol_value_tag<5, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* vsum = reinterpret_cast<float*>(smem + kPolMfmaOutBytes);   // [4][64] parts of V
  const GruLds m = gru_lds(smem, kPolMfmaOutBytes + kPolAcBytes, D, g.hid);
  PolTile t;
  if (!pol_tile_list(t, tm.count)) return;
  const PolRowList row{tm.list, t.first};
  pol_stage_obs(m.X, tm.term_obs, D, t, row, nm...);
  const bool keep = (int)t.lane < t.nlive;
  gru_stage_h(m.Xh, g.h + (keep ? row((int)t.lane) : (int64_t)0) * g.hid, keep, g.hid, t);
  __syncthreads();
  gru_cell<Tag>(pol, g, m, t, false);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 1, g.hid, m.S, t);
  policy_value_part<VTag>(ac, m.S + pol_col((int)t.lane), in, t.wave, t.lane, vsum);
  __syncthreads();
  if (t.wave == 0) policy_value_store<VTag>(ac, in, t, vsum, row);
}

// ---- the LSTM policy engine (gaq_policy_desc_rnn, GAQ_POLICY_CELL_LSTM): [obs | h], c -> h', c' -> head -> actions ------------------------
// The GRU engine's tile, operand layout and LDS regions (GruLds: X = the observation rows then the H rows of h, S = max(H, head widths)
// rows), with a second caller-owned [N, H] state c.  The gate units of 16-unit chunk k are the rows k, k + H/16, k + 2H/16, k + 3H/16 of
// W_ih' / W_hh' (gate order i, f, g, o).  Wave w takes the chunks k = w, w + 4, ... one at a time with four accumulator sets, one per
// gate: each starts at b_i + b_h and takes the x products then the h products (each an ascending fmaf chain) -- every gate takes both
// products, so there is no set kept apart as the GRU's n_h is.  Then i, f, o = gru_sigmoid, g = tanhf, c' = fmaf(f, c, i g),
// h' = o tanhf(c').
// c takes no LDS region of its own (a third block of H rows would pass the CU's 160 KiB at H = 256): it is staged into S by the stage
// that puts h into Xh (so the done mask and the dead lanes zero it exactly as they zero h), and in the cell the lane that owns 4 units x
// 4 envs of a chunk reads their c from S before it stores their h' to the same 16 words; no other lane touches those words before the
// barrier that follows the cell.  h' and c' go back to the caller's rows in place (each tile owns its rows).  The head is the GRU's.
// LDS = the GRU engine's: 1 KiB (+ 1 KiB of value parts) + 256 B x (kin + H + max(H, head widths)).
struct PolicyLstmDev {
  float* h;                       // the caller's [N, H] hidden state: read, then overwritten with h'
  float* c;                       // the caller's [N, H] cell state: read, then overwritten with c'
  const uint8_t* done_prev;       // done [N] of the previous step of this call (those rows start from h = c = 0), or nullptr
  int32_t hid;                    // H (W_ih' is at pol.off[0], b_ih, W_hh' and b_hh follow it; pol.off[1..] are the head's layers)
};

// the cell over X = [obs | h] and the c staged in S: h' -> S and, with write_back, h' and c' to the rows first .. of the caller's two
// states (the batch forms only)
template <int Kernel>
__device__ __forceinline__ void lstm_cell(const PolicyDev& pol, const PolicyLstmDev& g, const GruLds& m, const PolTile& t, bool write_back) {
  const int hid = g.hid, hc = hid / 16;
  const float* wih = pol.w + pol.off[0];
  const float* bih = wih + 4 * hid * pol.in_dim;
  const float* whh = bih + 4 * hid;
  const float* bhh = whh + 4 * hid * hid;
  const uint32_t lane = t.lane;
  const int h4 = (int)(lane >> 4);
#pragma unroll 1
  for (int c = t.wave; c < hc; c += kPolMfmaWaves) {
    const int u0 = c * 16 + 4 * h4;                               // this lane's 4 units of the chunk
    f32x4 acc[4][4];                                              // i, f, g, o
    {
      f32x4 b[4];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) b[s][r] = bih[s * hid + u0 + r] + bhh[s * hid + u0 + r];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) acc[s][eb] = b[s];
    }
    cell_kloop<4, 3, Kernel>(wih, pol.in_dim, c, hc, m.X, lane, acc);
    cell_kloop<4, 3, Kernel>(whh, hid, c, hc, m.Xh, lane, acc);
    f32x4 hn[4];                                                  // h' per env block
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) {
      f32x4 cn;                                                   // c' of the env block
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float cold = m.S[(u0 + r) * kTile + (lane & 15) * 4 + eb];
        const float ig = gru_sigmoid(acc[0][eb][r]), fg = gru_sigmoid(acc[1][eb][r]);
        const float gg = tanhf(acc[2][eb][r]), og = gru_sigmoid(acc[3][eb][r]);
        cn[r] = __builtin_fmaf(fg, cold, ig * gg);
        hn[eb][r] = og * tanhf(cn[r]);
      }
      const int e = eb * 16 + (int)(lane & 15);
      if (write_back && e < t.nlive) {
        *reinterpret_cast<f32x4*>(g.h + (t.first + e) * hid + u0) = hn[eb];
        *reinterpret_cast<f32x4*>(g.c + (t.first + e) * hid + u0) = cn;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                 // over the words this lane has just read c from
      const f32x4 v = {hn[0][r], hn[1][r], hn[2][r], hn[3][r]};
      *reinterpret_cast<f32x4*>(m.S + (u0 + r) * kTile + (lane & 15) * 4) = v;
    }
  }
}

// (h, c) <- LSTM(obs, h, c) with the rows that finished in the previous step (g.done_prev) started from 0, the head over S, the action
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_lstm_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, PolicyLstmDev g, const float* __restrict__ obs, int D,
                        float* __restrict__ act_out, Norm... nm) {
  constexpr int Tag = pol_tag<9, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* outs = reinterpret_cast<float*>(smem);                   // [4][64] output sums
  const GruLds m = gru_lds(smem, kPolMfmaOutBytes, D, g.hid);
  PolTile t;
  if (!pol_tile_batch(t, p, cfg)) return;
  const PolRowBatch row{t.first};
  pol_stage_obs(m.X, obs, D, t, row, nm...);
  const bool keep = (int)t.lane < t.nlive && !(g.done_prev && g.done_prev[t.first + t.lane]);
  gru_stage_h(m.Xh, g.h + (t.first + t.lane) * g.hid, keep, g.hid, t);
  gru_stage_h(m.S, g.c + (t.first + t.lane) * g.hid, keep, g.hid, t);
  __syncthreads();
  lstm_cell<Tag>(pol, g, m, t, true);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 1, g.hid, m.S, t);           // the head: the hidden layers 1 .. n_hidden-1 over S in place
  policy_out_part(pol, m.S + pol_col((int)t.lane), in, t, outs);
  __syncthreads();
  if (t.wave == 0) policy_act_tail(pol, cfg, t, outs, act_out);
}

// policy_lstm_kernel's actor-critic form: V from the rows the output layer reads; the bootstrap launch (value_only) computes h' into S
// as ever but leaves both of the caller's states alone
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_lstm_ac_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, PolicyLstmDev g, PolicyAcDev ac, const float* __restrict__ obs, int D,
                           float* __restrict__ act_out, Norm... nm) {
  constexpr int Tag = pol_tag<10, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* outs = reinterpret_cast<float*>(smem);                   // [4][64] output sums
  float* vsum = reinterpret_cast<float*>(smem + kPolMfmaOutBytes);   // [4][64] parts of V
  const GruLds m = gru_lds(smem, kPolMfmaOutBytes + kPolAcBytes, D, g.hid);
  PolTile t;
  if (!pol_tile_batch(t, p, cfg)) return;
  const PolRowBatch row{t.first};
  pol_stage_obs(m.X, obs, D, t, row, nm...);
  const bool keep = (int)t.lane < t.nlive && !(g.done_prev && g.done_prev[t.first + t.lane]);
  gru_stage_h(m.Xh, g.h + (t.first + t.lane) * g.hid, keep, g.hid, t);
  gru_stage_h(m.S, g.c + (t.first + t.lane) * g.hid, keep, g.hid, t);
  __syncthreads();
  lstm_cell<Tag>(pol, g, m, t, !ac.value_only);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 1, g.hid, m.S, t);
  const float* y = m.S + pol_col((int)t.lane);
  if (ac.wv) policy_value_part<Tag>(ac, y, in, t.wave, t.lane, vsum);
  if (!ac.value_only) policy_out_part(pol, y, in, t, outs);
  __syncthreads();
  if (t.wave == 0) policy_ac_tail<Tag>(pol, ac, cfg, in, t, outs, vsum, act_out);
}

// policy_lstm_ac_kernel's value-only launch on gathered rows: h and c are the listed env's rows of the registered states as they are
// -- no done mask -- and are only read; h' lives in S alone and c' nowhere.
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_lstm_term_kernel(PolicyDev pol, PolicyLstmDev g, PolicyAcDev ac, PolicyTermDev tm, int D, Norm... nm) {
  constexpr int Tag = pol_tag<11, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* vsum = reinterpret_cast<float*>(smem + kPolMfmaOutBytes);   // [4][64] parts of V
  const GruLds m = gru_lds(smem, kPolMfmaOutBytes + kPolAcBytes, D, g.hid);
  PolTile t;
  if (!pol_tile_list(t, tm.count)) return;
  const PolRowList row{tm.list, t.first};
  pol_stage_obs(m.X, tm.term_obs, D, t, row, nm...);
  const bool keep = (int)t.lane < t.nlive;
  const int64_t mine = (keep ? row((int)t.lane) : (int64_t)0) * g.hid;
  gru_stage_h(m.Xh, g.h + mine, keep, g.hid, t);
  gru_stage_h(m.S, g.c + mine, keep, g.hid, t);
  __syncthreads();
  lstm_cell<Tag>(pol, g, m, t, false);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 1, g.hid, m.S, t);
  policy_value_part<Tag>(ac, m.S + pol_col((int)t.lane), in, t.wave, t.lane, vsum);
  __syncthreads();
  if (t.wave == 0) policy_value_store<Tag>(ac, in, t, vsum, row);
}

// ---- a separate critic (gaq_critic, gaq_step_policy_critic_many_dev): V from a trunk of its own ---------------------------------------
// The critic is obs -> [Linear -> act] x n_hidden -> Linear -> 1: a second trunk in PolicyDev's terms (mfma_hidden reads w, n_hidden,
// hidden_act, width and off of it and nothing else) whose 1-output layer is laid out as a value head, so V is policy_value_part /
// policy_value_sum on the critic's last hidden layer: the three kernels below are compositions of the stages above, with tags of their
// own (6, 7, 8), and V of a row is the bits policy_mfma_ac_kernel gives for a policy with the same hidden layers and that value head.
// A struct of its own, as PolicyAcDev was: PolicyDev, PolicyAcDev and the arguments of every existing launch stay as they were.
struct PolicyCriticDev {
  PolicyDev trunk;                // the critic's hidden layers; off[n_hidden] = its 1-output layer (last width weights, then the bias)
};
// the value-head view of a critic whose V goes to value_out
__device__ __forceinline__ PolicyAcDev critic_ac(const PolicyCriticDev& cr, float* value_out) {
  return PolicyAcDev{cr.trunk.w + cr.trunk.off[cr.trunk.n_hidden], value_out, nullptr, {0.0f, 0.0f, 0.0f, 0.0f}, 1};
}

// the batch form: V of obs [rows, D] -> value_out [rows] (gaq_critic_eval_dev; in a rollout the bootstrap row and, for a GRU actor, every
// step's row: the critic is feed-forward and sees the observation only).  No draw, no step counter, no h'.
// LDS = 1 KiB (the parts of V) + 256 B x max(in_dim rounded up to 4, widest layer).
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void critic_mfma_kernel(PolicyCriticDev cr, int64_t rows, const float* __restrict__ obs, int D, float* __restrict__ value_out, Norm... nm) {
  constexpr int Tag = pol_tag<6, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* vsum = reinterpret_cast<float*>(smem);                   // [4][64] parts of V
  float* H = reinterpret_cast<float*>(smem + kPolAcBytes);        // [rows][64] activations
  PolTile t;
  pol_tile_span(t, rows);
  if (t.first >= rows) return;
  const PolRowBatch row{t.first};
  const PolicyAcDev ac = critic_ac(cr, value_out);
  pol_stage_obs(H, obs, D, t, row, nm...);
  __syncthreads();
  const int in = mfma_hidden<Tag>(cr.trunk, 0, cr.trunk.in_dim, H, t);
  policy_value_part<Tag>(ac, H + pol_col((int)t.lane), in, t.wave, t.lane, vsum);
  __syncthreads();
  if (t.wave == 0) policy_value_store<Tag>(ac, in, t, vsum, row);
}

// the gathered form: V of the terminal observations of the listed envs -> value_out[env] (policy_*_term_kernel's place in a rollout
// whenever a critic is given, for MLP and GRU actors alike).  The LDS layout is critic_mfma_kernel's.
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void critic_mfma_term_kernel(PolicyCriticDev cr, PolicyTermDev tm, int D, float* __restrict__ value_out, Norm... nm) {
  constexpr int Tag = pol_tag<7, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* vsum = reinterpret_cast<float*>(smem);                   // [4][64] parts of V
  float* H = reinterpret_cast<float*>(smem + kPolAcBytes);        // [rows][64] activations
  PolTile t;
  if (!pol_tile_list(t, tm.count)) return;
  const PolRowList row{tm.list, t.first};
  const PolicyAcDev ac = critic_ac(cr, value_out);
  pol_stage_obs(H, tm.term_obs, D, t, row, nm...);
  __syncthreads();
  const int in = mfma_hidden<Tag>(cr.trunk, 0, cr.trunk.in_dim, H, t);
  policy_value_part<Tag>(ac, H + pol_col((int)t.lane), in, t.wave, t.lane, vsum);
  __syncthreads();
  if (t.wave == 0) policy_value_store<Tag>(ac, in, t, vsum, row);
}

// the fused form for an MLP actor: policy_mfma_ac_kernel's launch with V from the critic's trunk.  The actor's trunk runs first and its 4
// output sums go to `outs`; mfma_hidden works in place, so the observations are staged a second time into the same rows (72 B per env,
// from L2) for the critic's trunk, whose parts of V go to `vsum`; outs is outside the activation rows and survives.  ac.wv is the
// critic's 1-output layer (the host sets it) and the tail is policy_ac_tail with the critic's last width.
// LDS = the sums' 2 KiB + 256 B x max(in_dim rounded up to 4, every actor width, every critic width): 66 KiB at width 256.
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_mfma_critic_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, PolicyAcDev ac, PolicyCriticDev cr, const float* __restrict__ obs,
                               int D, float* __restrict__ act_out, Norm... nm) {
  constexpr int Tag = pol_tag<8, Norm...>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* outs = reinterpret_cast<float*>(smem);                   // [4][64] output sums
  float* vsum = reinterpret_cast<float*>(smem + kPolMfmaOutBytes);   // [4][64] parts of V
  float* H = reinterpret_cast<float*>(smem + kPolMfmaOutBytes + kPolAcBytes);   // [rows][64] activations
  PolTile t;
  if (!pol_tile_batch(t, p, cfg)) return;
  const PolRowBatch row{t.first};
  pol_stage_obs(H, obs, D, t, row, nm...);
  __syncthreads();
  const int in = mfma_hidden<Tag>(pol, 0, pol.in_dim, H, t);
  policy_out_part(pol, H + pol_col((int)t.lane), in, t, outs);
  __syncthreads();                                                // every wave has read the actor's last layer
  pol_stage_obs(H, obs, D, t, row, nm...);
  __syncthreads();
  const int cin = mfma_hidden<Tag>(cr.trunk, 0, cr.trunk.in_dim, H, t);
  policy_value_part<Tag>(ac, H + pol_col((int)t.lane), cin, t.wave, t.lane, vsum);
  __syncthreads();
  if (t.wave == 0) policy_ac_tail<Tag>(pol, ac, cfg, cin, t, outs, vsum, act_out);
}

// ---- the bf16 MFMA policy engine (GAQ_POLICY_ENGINE_MFMA_BF16): obs [N, D] -> actions [N, 4] on v_mfma_f32_16x16x32_bf16 ---------------
// Numerical contract (gaq.h): weights and every layer input rounded to bf16 (RNE, v_cvt_pk_bf16_f32), fp32 accumulation from the fp32 bias.
// One workgroup = one tile of 64 envs, kBfWaves = 4 waves.  The activations live in ONE LDS buffer X[env][stride] of bf16 (the observation
// first, each hidden layer's output over it in place): a lane's B operand of k-step s, X[env][32s + 8h .. 32s + 8h + 7] (h = lane >> 4), is
// one ds_read_b128, and the row stride (a multiple of 32 elements + 8) is an odd number of 16-byte units, so the 16 envs of a read land on 16
// different 16-byte bank groups.  A = the weights, repacked at set-weights time (policy_bf16_pack_kernel) into one 16-byte fragment per lane
// per (16-unit chunk, k-step): 1 KiB contiguous per fragment, one coalesced global_load_dwordx4.  Per hidden layer wave w owns the chunks
// c = w, w + kBfWaves, ... and every env block of the workgroup, so each weight fragment it loads feeds 4 MFMAs.  D[unit][env]
// holds 4 consecutive units of one env per lane: pol_act in fp32, rounded, one 8-byte LDS write.  K is padded to a multiple of 32 with
// weights +0 (written by the repack, never read from the caller's layout) against inputs -0: each padded product is -0 and adds nothing.
// The 4-output layer is one more MFMA chunk whose rows 4..15 are zero; lanes 0..15 then hold an env's 4 sums and finish them with
// policy_out_tail.  LDS = 64 x stride x 2 B: 33 KiB at width 256.  (Wider workgroups, 4 or 8 waves over 2 or 4 tiles, were slower:
// DESIGN.md section 4a.)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
constexpr int kBfWaves = 4;
constexpr int kBfEnvs = kTile;
constexpr int kBfBlock = kBfWaves * 64;
constexpr int kBfBlocks = kBfEnvs / 16;                           // env blocks of 16 (the MFMA's N)

struct PolicyBf16Dev {
  const bf16x8* w;                        // the repacked weights: per layer [chunk][k-step][64 lanes] fragments
  int32_t off[kPolMaxHidden + 1];         // fragment offset of each layer (the output layer last)
  int32_t stride;                         // LDS row of one env, bf16 elements
};
__device__ __forceinline__ int bf_kpad(int k) { return (k + 31) & ~31; }

// this wave's NC chunks of one hidden layer (`in` inputs, ks = kpad(in) / 32 k-steps) over the workgroup's env blocks into acc
// then, once every wave has read the layer's input (the barrier), through pol_act into X as bf16
template <int NC>
__device__ __forceinline__ void bf_layer(const bf16x8* __restrict__ wl, const float* __restrict__ bias, int ks, int act, int wave, __bf16* X,
                                         int stride, uint32_t lane) {
  const int h = (int)(lane >> 4);
  f32x4 acc[NC][kBfBlocks];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const float* b = bias + (wave + kBfWaves * j) * 16 + 4 * h;
    const f32x4 b4 = {b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int eb = 0; eb < kBfBlocks; ++eb) acc[j][eb] = b4;
  }
  const __bf16* xrow = X + (int)(lane & 15) * stride + 8 * h;
  bf16x8 a[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) a[j] = wl[(wave + kBfWaves * j) * ks * 64 + lane];
#pragma unroll 1
  for (int s = 0; s < ks; ++s) {
    const int sn = s + 1 < ks ? s + 1 : s;                        // the next k-step's fragments load under this one's MFMAs
    bf16x8 an[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) an[j] = wl[((wave + kBfWaves * j) * ks + sn) * 64 + lane];
#pragma unroll
    for (int eb = 0; eb < kBfBlocks; ++eb) {
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(xrow + eb * 16 * stride + 32 * s);
#pragma unroll
      for (int j = 0; j < NC; ++j) acc[j][eb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], x, acc[j][eb], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) a[j] = an[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NC; ++j) {
#pragma unroll
    for (int eb = 0; eb < kBfBlocks; ++eb) {
      const f32x4 v = acc[j][eb];
      const bf16x4 o = {(__bf16)pol_act(act, v[0]), (__bf16)pol_act(act, v[1]), (__bf16)pol_act(act, v[2]), (__bf16)pol_act(act, v[3])};
      *reinterpret_cast<bf16x4*>(X + (eb * 16 + (int)(lane & 15)) * stride + (wave + kBfWaves * j) * 16 + 4 * h) = o;
    }
  }
}

template <class... Norm>
__global__ __launch_bounds__(kBfBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_mfma_bf16_kernel(DevPtrs p, StepCfg cfg, PolicyDev pol, PolicyBf16Dev pb, const float* __restrict__ obs, int D,
                             float* __restrict__ act_out, Norm... nm) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* X = reinterpret_cast<__bf16*>(smem);                    // [kBfEnvs][stride]
  const int stride = pb.stride;
  const uint32_t lane = threadIdx.x & 63u;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (p.step_ctr) cfg.step_index = step_counter_peek(p, lane);    // graph-safe mode: the index of the step about to run
  const int64_t first = (int64_t)blockIdx.x * kBfEnvs;
  if (first >= p.n) return;
  const int nlive = (int)((p.n - first) < kBfEnvs ? (p.n - first) : kBfEnvs);
  // the observations -> X[e][0 .. kin-1] in bf16 (dead envs 0, padded inputs -0)
  const int kin = bf_kpad(D);
  for (int f = (int)threadIdx.x; f < kBfEnvs * kin; f += kBfBlock) {
    const int e = f / kin, k = f - e * kin;
    X[e * stride + k] = (__bf16)(k >= D ? -0.0f : e < nlive ? pol_stage_elem(obs[(first + e) * D + k], k, nm...) : 0.0f);
  }
  __syncthreads();
  int in = pol.in_dim;
#pragma unroll 1
  for (int l = 0; l < pol.n_hidden; ++l) {
    const int width = pol.width[l], ks = bf_kpad(in) / 32;
    const bf16x8* wl = pb.w + pb.off[l];
    const float* bias = pol.w + pol.off[l] + width * in;
    const int nc = (width / 16 - wave + kBfWaves - 1) / kBfWaves;  // chunks wave, wave + kBfWaves, ... below width / 16
    switch (nc) {                                                 // (nc is wave-uniform: every wave meets one barrier here)
      case 1: bf_layer<1>(wl, bias, ks, pol.hidden_act, wave, X, stride, lane); break;
      case 2: bf_layer<2>(wl, bias, ks, pol.hidden_act, wave, X, stride, lane); break;
      case 3: bf_layer<3>(wl, bias, ks, pol.hidden_act, wave, X, stride, lane); break;
      case 4: bf_layer<4>(wl, bias, ks, pol.hidden_act, wave, X, stride, lane); break;
      default: __syncthreads(); break;
    }
    if (width & 16) {                                             // the next layer's K pads to a multiple of 32: inputs -0
      for (int f = (int)threadIdx.x; f < kBfEnvs * 16; f += kBfBlock) X[(f >> 4) * stride + width + (f & 15)] = (__bf16)-0.0f;
    }
    __syncthreads();
    in = width;
  }
  // the output layer: one chunk (rows 0..3 = the 4 outputs, rows 4..15 zero weights) per env block; wave w takes blocks w, w + kBfWaves, ...
  const int ks = bf_kpad(in) / 32, h = (int)(lane >> 4);
  const bf16x8* wo = pb.w + pb.off[pol.n_hidden];
  const float* bo = pol.w + pol.off[pol.n_hidden] + in * 4;
  const __bf16* xrow = X + (int)(lane & 15) * stride + 8 * h;
#pragma unroll 1
  for (int eb = wave; eb < kBfBlocks; eb += kBfWaves) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (h == 0) acc = f32x4{bo[0], bo[1], bo[2], bo[3]};
    for (int s = 0; s < ks; ++s)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wo[s * 64 + lane], *reinterpret_cast<const bf16x8*>(xrow + eb * 16 * stride + 32 * s),
                                                    acc, 0, 0, 0);
    const int e = eb * 16 + (int)lane;
    if (h == 0) {
      float a[4] = {acc[0], acc[1], acc[2], acc[3]};
      const int64_t i = first + e;
      policy_out_tail(pol, cfg.seed, cfg.env_offset + (uint64_t)i, cfg.step_index, a);
      if (e < nlive) *reinterpret_cast<float4*>(act_out + i * 4) = make_float4(a[0], a[1], a[2], a[3]);
    }
  }
}

// the caller's fp32 packed layout (pol.w) -> the bf16 fragments of policy_mfma_bf16_kernel, one 16-byte fragment per thread; `total`
// fragments in all.  Weights past a layer's real K and the output chunk's rows 4..15 are +0.
__global__ void policy_bf16_pack_kernel(PolicyDev pol, PolicyBf16Dev pb, bf16x8* __restrict__ out, int total) {
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= total) return;
  int l = 0;
  while (l < pol.n_hidden && f >= pb.off[l + 1]) ++l;
  const int r = f - pb.off[l], lane = r & 63, q = r >> 6;
  const int in = l == 0 ? pol.in_dim : pol.width[l - 1];
  const int ks = bf_kpad(in) / 32;
  const int c = q / ks, s = q - c * ks, row = lane & 15, k0 = 32 * s + 8 * (lane >> 4);
  const float* w = pol.w + pol.off[l];
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    float x = 0.0f;
    if (k < in) {
      if (l < pol.n_hidden) x = w[((int64_t)c * in + k) * 16 + row];
      else if (row < 4) x = w[k * 4 + row];
    }
    v[j] = (__bf16)x;
  }
  out[f] = v;
}

#include "gaq_policy_encoder.inc"   // policy_encode_kernel, policy_encode_term_kernel: an encoder in front of a recurrent cell

}  // namespace

extern "C" {

// ---- device MLP policy (include/gaq.h gaq_policy) ---------------------------------------------------------------------------
struct gaq_policy {
  PolicyNet net;                  // what it shares with a critic (gaq_grad.hpp): n_out = 4
  gaq_policy_desc desc{};
  int engine = GAQ_POLICY_ENGINE_VALU;
  size_t lds_base = 0;            // dynamic LDS of the per-step policy launch before the scratch (PolicyEngine::lds_base)
  PolicyBf16Dev bd{};             // bf16 engine: the repacked weights (bd.w = wb_dev) and their layout
  bf16x8* wb_dev = nullptr;
  int64_t nwb = 0;                // fragments in wb_dev
  float* act_tmp = nullptr; int64_t act_tmp_n = 0;   // fallback without actions_out: one step's actions
  int cell = GAQ_POLICY_CELL_NONE;                  // GAQ_POLICY_CELL_GRU / _LSTM: hidden layer 0 is that cell (policy_gru_kernel / policy_lstm_kernel)
  int32_t off_hh = 0;                               // GRU, LSTM: float offset of W_hh' in the packed weights
  int64_t n = 0;                                    // the env's N (rows of the hidden state)
  float* hid_dev = nullptr;                         // GRU, LSTM: the caller's [N, H] state h (gaq_policy_set_hidden_dev)
  float* cell_dev = nullptr;                        // LSTM: the caller's [N, H] state c (gaq_policy_set_cell_dev)
  float* wv_dev = nullptr;                          // the value head: last width weights + bias (gaq_policy_set_value_head), its own buffer
  bool value_set = false;
  float log_std[4] = {0.0f, 0.0f, 0.0f, 0.0f};      // the caller's log_std (pd.std4 = exp of it): the log-probabilities subtract it
  // device mode (gaq_policy_set_explore_dev): the caller's table, and the 12 words as the host last wrote them -- log_std | std |
  // inv_std, the source of every copy into the table.  While a table is registered and the policy explores, pd.explore is
  // kPolExploreDev and pd.std4's first 8 bytes are the table's address (policy_explore_apply).
  float* explore_tab = nullptr;
  float explore_host[kExploreWords] = {};
  // gaq_step_policy_ac_term_many_dev, allocated on first use and kept like act_tmp:
  uint32_t* term_list = nullptr;                    // [ntiles * 64] the envs that finished in one step, then 2 counters (used in turn)
  float* term_obs_tmp = nullptr;                    // [N, obs_dim] terminal observations when the caller has registered no buffer
  // an encoder in front of the cell (gaq_policy_create_rnn_enc; enc.n_hidden = 0: none, and nothing below is used):
  PolicyDev enc{};                                  // its layers (enc.w = enc_w_dev, enc.in_dim = the env's obs_dim); desc.in_dim is then E
  int64_t enc_nw = 0;                               // floats of its block: per layer W' [W/16][in][16], then the bias
  float* enc_w_dev = nullptr;
  bool enc_set = false;
  float* feat_dev = nullptr;                        // [N, E] features, allocated at create: a captured graph keeps valid pointers
};

// ---- separate critic (include/gaq.h gaq_critic) ---------------------------------------------------------------------------------
struct gaq_critic {
  PolicyNet net;                  // what it shares with a policy: n_out = 1
  gaq_critic_desc desc{};
  bool fused = true;              // an MLP actor's V comes from policy_mfma_critic_kernel (GAQ_NO_FUSED_CRITIC=1 at create: two launches)
};

namespace {
constexpr size_t kLdsMax = 160 * 1024;

extern "C++" {                    // (templates below)
// ---- what a policy and a critic share: the record's layout, checks, weights, normaliser (Net: anything with in_dim, n_hidden, width) ----
// The activation rows of a tile on the MFMA engine: max(in_dim rounded up to 4, widest layer), of 64 floats each
template <class Net> int net_act_rows(const Net& d) {
  int rows = (d.in_dim + 3) & ~3;
  for (int l = 0; l < d.n_hidden; ++l) rows = std::max(rows, (int)d.width[l]);
  return rows;
}
// The packed layout (gym_art_amd/policy.py unpack_weights describes the same one): per hidden layer W'[width/16][in][16] then bias[width],
// then the output layer [in][n_out], bias[n_out].  layer0: the floats of hidden layer 0 where it is no such layer (a recurrent cell's),
// -1: it is.  Returns the total; off (nullptr: not wanted) receives the float offset of every layer, the output layer's at off[n_hidden].
template <class Net> int64_t net_layout(const Net& d, int64_t layer0, int n_out, int32_t* off = nullptr) {
  int64_t n = 0, in = d.in_dim;
  for (int l = 0; l < d.n_hidden; ++l) {
    if (off) off[l] = (int32_t)n;
    n += l == 0 && layer0 >= 0 ? layer0 : (int64_t)d.width[l] * in + d.width[l];
    in = d.width[l];
  }
  if (off) off[d.n_hidden] = (int32_t)n;
  return n + n_out * in + n_out;
}
// the words in which a policy's and a critic's refusals differ
struct NetWords {
  const char* who;                // "policy" / "critic"
  bool name_layer;                // the width text names the layer ("width[l] must be a multiple") or all ("hidden widths must be multiples")
  const char* act;                // how the text calls hidden_act
  std::string note;               // behind the width text (the engine)
};
template <class Desc> int net_check_fields(const Desc& d, int out_tanh, const NetWords& w, int max_width) {
  const std::string who = std::string(w.who) + ": ";
  if (d.n_hidden < 1 || d.n_hidden > kPolMaxHidden) return fail(GAQ_ERR_INVALID, who + "n_hidden must be 1, 2 or 3");
  for (int l = 0; l < d.n_hidden; ++l)
    if (d.width[l] < 16 || d.width[l] > max_width || d.width[l] % 16 != 0)
      return fail(GAQ_ERR_INVALID, who + (w.name_layer ? "width[" + std::to_string(l) + "] must be a multiple" : "hidden widths must be multiples") +
                                       " of 16 in [16, " + std::to_string(max_width) + "]" + w.note);
  if (d.hidden_act != GAQ_POLICY_TANH && d.hidden_act != GAQ_POLICY_RELU) return fail(GAQ_ERR_INVALID, who + "unknown " + w.act);
  if (out_tanh != 0 && out_tanh != 1) return fail(GAQ_ERR_INVALID, who + "out_tanh must be 0 or 1");
  if (d.in_dim <= 0) return fail(GAQ_ERR_INVALID, who + "in_dim must be positive");
  return GAQ_OK;
}
// the record of a checked description on e's device, and its weights' buffer (on failure the caller destroys the handle)
template <class Desc> int net_create(PolicyNet& net, const gaq_env* e, const Desc& d, int out_tanh, int64_t layer0, int n_out) {
  net.device = e->cfg.device; net.env = e; net.n_out = n_out;
  PolicyDev& pd = net.pd;
  pd.in_dim = d.in_dim; pd.n_hidden = d.n_hidden; pd.hidden_act = d.hidden_act; pd.out_tanh = out_tanh;
  for (int l = 0; l < kPolMaxHidden; ++l) pd.width[l] = l < d.n_hidden ? d.width[l] : 0;
  net.nw = net_layout(d, layer0, n_out, pd.off);
  net.rows = net_act_rows(d);
  hipError_t he = hipMalloc(&net.w_dev, sizeof(float) * (size_t)net.nw);
  if (he != hipSuccess) return fail(GAQ_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(he));
  pd.w = net.w_dev;
  return GAQ_OK;
}
}  // extern "C++"
// copy the caller's weights into w_dev (synchronous)
int net_set_weights(PolicyNet* net, const float* w, hipMemcpyKind kind) {
  if (!net || !w) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(net->device));
  HIP_TRY(hipMemcpy(net->w_dev, w, sizeof(float) * (size_t)net->nw, kind));
  net->weights_set = true;
  return GAQ_OK;
}
// attach a normaliser of the same env (nullptr: detach)
int net_set_obs_norm(PolicyNet& net, const char* who, const gaq_obs_norm* n) {
  if (n && n->env != net.env) return fail(GAQ_ERR_INVALID, std::string(who) + ": the normaliser was created for another env handle");
  net.norm = n;
  return GAQ_OK;
}
// the record's device buffers, on its device (which stays current for the handle's own)
void net_free(PolicyNet& net) {
  (void)hipSetDevice(net.device);
  if (net.w_dev) (void)hipFree(net.w_dev);
  if (net.grad_scratch) (void)hipFree(net.grad_scratch);
}

// policy_kernel's LDS: the tile's observation rows
size_t policy_valu_lds(const gaq_policy_desc& d) { return (size_t)kTile * d.in_dim * 4; }
// policy_mfma_kernel's LDS: the output sums, then the activation rows
size_t policy_mfma_lds(const gaq_policy_desc& d) { return (size_t)kPolMfmaOutBytes + (size_t)net_act_rows(d) * kTile * 4; }
// policy_mfma_bf16_kernel's LDS row of one env (bf16 elements): the widest layer input padded to a multiple of 32, + 8
int policy_bf16_stride(const gaq_policy_desc& d) {
  int k = (d.in_dim + 31) & ~31;
  for (int l = 0; l < d.n_hidden; ++l) k = std::max(k, (d.width[l] + 31) & ~31);
  return k + 8;
}
size_t policy_bf16_lds(const gaq_policy_desc& d) { return (size_t)kBfEnvs * (size_t)policy_bf16_stride(d) * 2; }

// policy_gru_kernel's LDS, and policy_lstm_kernel's (c is staged in the rows that then receive h'): the output sums, the observation
// and h rows, then max(H, head widths) rows for h' and the head
size_t policy_gru_lds(const gaq_policy_desc& d) {
  int rows = d.width[0];
  for (int l = 1; l < d.n_hidden; ++l) rows = std::max(rows, (int)d.width[l]);
  return (size_t)kPolMfmaOutBytes + (size_t)(((d.in_dim + 3) & ~3) + d.width[0] + rows) * kTile * 4;
}

extern "C++" {                    // (templates below)
// one policy launch of a rollout, whichever kernel it is: everything any of them takes
struct PolicyLaunchArgs {
  dim3 grid, block; size_t lds; hipStream_t st;
  const gaq_env* e; const gaq_policy* p;
  PolicyCriticDev critic;         // the critic's kernels only: the trunk of its record
  PolicyEncDev enc;               // the encoder's kernels only: its layers and the feature rows
  int64_t rows;                  // the critic's and the encoder's batch forms only
  StepCfg sc;
  const uint8_t* done_prev;       // recurrent: done [N] of the previous step (those rows start from 0), or nullptr
  PolicyAcDev ac;                 // the actor-critic and the gathered forms
  PolicyTermDev tm;               // the gathered forms
  PolObsNorm nm;                  // the normaliser of the net(s) this launch evaluates (tab = nullptr: none, the plain instantiation)
  const float* in; int D; float* a;
};

// the two instantiations of a kernel template -- plain, normalising -- from one naming of it
#define GAQ_TWINS(NAME) &NAME##_kernel<>, &NAME##_kernel<PolObsNorm>
// the one launch of every form: the normalising instantiation with the table appended when the launch carries one, else the plain one
template <auto Kernel, auto Norm, class... A> void policy_launch(const PolicyLaunchArgs& x, const A&... a) {
  if (x.nm.tab) hipLaunchKernelGGL(Norm, x.grid, x.block, x.lds, x.st, a..., x.nm);
  else hipLaunchKernelGGL(Kernel, x.grid, x.block, x.lds, x.st, a...);
}
// a kernel's two instantiations (policy_lds / critic_lds set the LDS attribute of the one launched) and their launch
struct PolicyForm {
  const void* kernel;
  const void* kernel_norm;        // nullptr: the kernel takes no normaliser
  void (*launch)(const PolicyLaunchArgs&);
  const void* pick(const PolObsNorm& nm) const { return nm.tab ? kernel_norm : kernel; }
};
template <auto Kernel, auto Norm> PolicyForm policy_form(void (*launch)(const PolicyLaunchArgs&)) {
  return PolicyForm{(const void*)Kernel, (const void*)Norm, launch};
}
// FORM: the form of kernel template NAME, launched by a function NAME_launch with the arguments `...` of PolicyLaunchArgs x.  (A named
// function, as PolicyCell's are: its symbol is its own wherever in the file the form stands.)
#define GAQ_FORM(FORM, NAME, ...)                                                                             \
  void NAME##_launch(const PolicyLaunchArgs& x) { policy_launch<GAQ_TWINS(NAME)>(x, __VA_ARGS__); } \
  const PolicyForm FORM = policy_form<GAQ_TWINS(NAME)>(NAME##_launch)

// The feed-forward forms beside PolicyCell's: the three engines' plain launches, the fp32 MFMA engine's actor-critic and gathered forms,
// the MLP actor and the critic in one launch, the critic's gathered form (V -> ac.value_out) and its batch form (critic_launch).
// (They stand before PolicyCell's on purpose.  The kernel templates are instantiated in the order the host code first names them, and
// the four plain kernels that share instantiation 0 of the value stages -- pol_value_tag -- compile to the recorded instructions with
// the MLP's two named before the GRU's two, as the kernels were once defined; named after them, all four come out different.
// tools/kernel_asm_same.py against the parent commit shows either.)
void policy_valu_launch(const PolicyLaunchArgs& x) {
  hipLaunchKernelGGL(policy_kernel, x.grid, x.block, x.lds, x.st, x.e->d, x.sc, x.p->net.pd, x.in, x.D, x.a);
}
const PolicyForm kValuStepForm{(const void*)&policy_kernel, nullptr, policy_valu_launch};
GAQ_FORM(kMfmaStepForm, policy_mfma, x.e->d, x.sc, x.p->net.pd, x.in, x.D, x.a);
GAQ_FORM(kBf16StepForm, policy_mfma_bf16, x.e->d, x.sc, x.p->net.pd, x.p->bd, x.in, x.D, x.a);
GAQ_FORM(kMfmaAcForm, policy_mfma_ac, x.e->d, x.sc, x.p->net.pd, x.ac, x.in, x.D, x.a);
GAQ_FORM(kMfmaTermForm, policy_mfma_term, x.p->net.pd, x.ac, x.tm, x.D);
// (one table for both trunks: rollout_plan fuses only when actor and critic carry the same normaliser, or none)
GAQ_FORM(kFusedCriticForm, policy_mfma_critic, x.e->d, x.sc, x.p->net.pd, x.ac, x.critic, x.in, x.D, x.a);
GAQ_FORM(kCriticTermForm, critic_mfma_term, x.critic, x.tm, x.D, x.ac.value_out);
GAQ_FORM(kCriticForm, critic_mfma, x.critic, x.rows, x.in, x.D, x.ac.value_out);

// what differs between the policy engines (GAQ_POLICY_ENGINE_*)
struct PolicyEngine {
  int max_width;                                  // hidden widths: multiples of 16 in [16, max_width]
  const char* name;                               // named by the error texts (nullptr: the VALU engine's texts name none)
  size_t (*lds_base)(const gaq_policy_desc&);     // dynamic LDS of the per-step policy launch before the scratch
  size_t lds_max;                                 // create-time limit of lds_base (the VALU engine's is checked per launch)
  bool scratch;                                   // the hidden activations go to a scratch after the base
  int block;                                      // the per-step policy launch (one workgroup per 64-env tile)
  PolicyForm step;                                // (kernel_norm = nullptr: the engine takes no normaliser)
};
// nullptr for an unknown engine
const PolicyEngine* policy_engine(int engine) {
  static const PolicyEngine valu{kPolMaxWidth, nullptr, policy_valu_lds, SIZE_MAX, true, kPolBlock, kValuStepForm};
  static const PolicyEngine mfma{kPolMfmaMaxWidth, "MFMA engine", policy_mfma_lds, kLdsMax, false, kPolMfmaBlock, kMfmaStepForm};
  static const PolicyEngine bf16{kPolMfmaMaxWidth, "bf16 engine", policy_bf16_lds, kLdsMax, false, kBfBlock, kBf16StepForm};
  switch (engine) {
    case GAQ_POLICY_ENGINE_VALU: return &valu;
    case GAQ_POLICY_ENGINE_MFMA: return &mfma;
    case GAQ_POLICY_ENGINE_MFMA_BF16: return &bf16;
    default: return nullptr;
  }
}

// the state argument of a recurrent launch
template <class Dev> Dev policy_cell_dev(const PolicyLaunchArgs& x);
template <> PolicyGruDev policy_cell_dev(const PolicyLaunchArgs& x) {
  return PolicyGruDev{x.p->hid_dev, x.done_prev, (int32_t)x.p->desc.width[0], x.p->off_hh};
}
template <> PolicyLstmDev policy_cell_dev(const PolicyLaunchArgs& x) {
  return PolicyLstmDev{x.p->hid_dev, x.p->cell_dev, x.done_prev, (int32_t)x.p->desc.width[0]};
}
// the three forms of a cell's kernels: state <- cell(obs, state) with the rows that finished in the previous step zeroed first; the
// same with V and the log-prob beside the action; V alone on gathered rows
template <class Dev, auto Kernel, auto Norm> void policy_cell_step(const PolicyLaunchArgs& x) {
  policy_launch<Kernel, Norm>(x, x.e->d, x.sc, x.p->net.pd, policy_cell_dev<Dev>(x), x.in, x.D, x.a);
}
template <class Dev, auto Kernel, auto Norm> void policy_cell_ac(const PolicyLaunchArgs& x) {
  policy_launch<Kernel, Norm>(x, x.e->d, x.sc, x.p->net.pd, policy_cell_dev<Dev>(x), x.ac, x.in, x.D, x.a);
}
template <class Dev, auto Kernel, auto Norm> void policy_cell_term(const PolicyLaunchArgs& x) {
  policy_launch<Kernel, Norm>(x, x.p->net.pd, policy_cell_dev<Dev>(x), x.ac, x.tm, x.D);
}

// what differs between the recurrent cells (GAQ_POLICY_CELL_*); both run on the MFMA engine
struct PolicyCell {
  int gates;                      // rows of W_ih' / W_hh' and of each bias per unit: GRU 3 (r, z, n), LSTM 4 (i, f, g, o)
  const char* name;               // as the error texts name it
  bool has_c;                     // a second caller-owned state c (gaq_policy_set_cell_dev)
  PolicyForm step, ac, term;
};
// nullptr for no cell (a feed-forward policy) or an unknown one
const PolicyCell* policy_cell(int cell) {
  using G = PolicyGruDev;
  using L = PolicyLstmDev;
#define GAQ_CELL_FORM(DEV, NAME, LAUNCH) policy_form<GAQ_TWINS(NAME)>(LAUNCH<DEV, GAQ_TWINS(NAME)>)
  static const PolicyCell gru{3, "GRU engine", false, GAQ_CELL_FORM(G, policy_gru, policy_cell_step),
                              GAQ_CELL_FORM(G, policy_gru_ac, policy_cell_ac), GAQ_CELL_FORM(G, policy_gru_term, policy_cell_term)};
  static const PolicyCell lstm{4, "LSTM engine", true, GAQ_CELL_FORM(L, policy_lstm, policy_cell_step),
                               GAQ_CELL_FORM(L, policy_lstm_ac, policy_cell_ac), GAQ_CELL_FORM(L, policy_lstm_term, policy_cell_term)};
#undef GAQ_CELL_FORM
#undef GAQ_FORM
#undef GAQ_TWINS
  switch (cell) {
    case GAQ_POLICY_CELL_GRU: return &gru;
    case GAQ_POLICY_CELL_LSTM: return &lstm;
    default: return nullptr;
  }
}

// The encoder's two forms (gaq_policy_encoder.inc): the batch launch in front of an actor launch, the gathered one in front of the
// cell's terminal-value launch.  (Named after every other form, so that no other kernel's place in the order of instantiation moves.)
void policy_encode_launch(const PolicyLaunchArgs& x) {
  policy_launch<&policy_encode_kernel<>, &policy_encode_kernel<PolObsNorm>>(x, x.enc, x.rows, x.in, x.D);
}
void policy_encode_term_launch(const PolicyLaunchArgs& x) {
  policy_launch<&policy_encode_term_kernel<>, &policy_encode_term_kernel<PolObsNorm>>(x, x.enc, x.tm, x.D);
}
const PolicyForm kEncodeForm = policy_form<&policy_encode_kernel<>, &policy_encode_kernel<PolObsNorm>>(policy_encode_launch);
const PolicyForm kEncodeTermForm =
    policy_form<&policy_encode_term_kernel<>, &policy_encode_term_kernel<PolObsNorm>>(policy_encode_term_launch);

// the plain description of either extended one (gaq_policy_desc_ex, gaq_policy_desc_rnn: the same fields first)
template <class Ext>
gaq_policy_desc policy_plain_desc(const Ext& x) {
  gaq_policy_desc d{};
  d.struct_size = sizeof(gaq_policy_desc);
  d.in_dim = x.in_dim; d.n_hidden = x.n_hidden; d.hidden_act = x.hidden_act; d.out_tanh = x.out_tanh;
  for (int l = 0; l < 3; ++l) d.width[l] = x.width[l];
  return d;
}
}  // extern "C++"

int policy_check_fields(const gaq_policy_desc* d, const PolicyEngine& eng) {
  return net_check_fields(*d, d->out_tanh, {"policy", false, "hidden activation", eng.name ? std::string(" (") + eng.name + ")" : std::string()},
                          eng.max_width);
}
int policy_check_desc(const gaq_policy_desc* d) {
  if (!d || d->struct_size != sizeof(gaq_policy_desc)) return fail(GAQ_ERR_INVALID, "gaq_policy_desc size mismatch (header vs library)");
  return policy_check_fields(d, *policy_engine(GAQ_POLICY_ENGINE_VALU));
}
// gaq_policy_desc_ex -> the plain description + its engine
int policy_check_desc_ex(const gaq_policy_desc_ex* x, gaq_policy_desc& d, int& engine) {
  if (!x || x->struct_size != sizeof(gaq_policy_desc_ex)) return fail(GAQ_ERR_INVALID, "gaq_policy_desc_ex size mismatch (header vs library)");
  const PolicyEngine* eng = policy_engine(x->engine);
  if (!eng) return fail(GAQ_ERR_INVALID, "policy: unknown engine");
  d = policy_plain_desc(*x);
  engine = x->engine;
  return policy_check_fields(&d, *eng);
}
// gaq_policy_desc_rnn -> the plain description (hidden layer 0 = the cell, width[0] = H)
int policy_check_desc_rnn(const gaq_policy_desc_rnn* x, gaq_policy_desc& d) {
  if (!x || x->struct_size != sizeof(gaq_policy_desc_rnn)) return fail(GAQ_ERR_INVALID, "gaq_policy_desc_rnn size mismatch (header vs library)");
  if (!policy_cell(x->cell))
    return fail(GAQ_ERR_INVALID, "policy: unknown recurrent cell (GAQ_POLICY_CELL_GRU and GAQ_POLICY_CELL_LSTM are the cells)");
  if (x->engine != GAQ_POLICY_ENGINE_MFMA) return fail(GAQ_ERR_INVALID, "policy: a recurrent policy runs on the MFMA engine only");
  d = policy_plain_desc(*x);
  return policy_check_fields(&d, *policy_engine(GAQ_POLICY_ENGINE_MFMA));
}
// the activation rows of an encoder's tile: the observation (rounded up to 4) and a first layer of two; the last layer's output goes
// from the accumulators to the feature rows
int encoder_rows(int in_dim, int layers, const int32_t* width) {
  int rows = (in_dim + 3) & ~3;
  for (int l = 0; l + 1 < layers; ++l) rows = std::max(rows, (int)width[l]);
  return rows;
}
// gaq_policy_desc_rnn_enc -> the plain description of the cell and the head (in_dim = E), the cell, and the encoder's layers
int policy_check_desc_rnn_enc(const gaq_policy_desc_rnn_enc* x, gaq_policy_desc& d, int& cell, PolicyDev& enc) {
  if (!x || x->struct_size != sizeof(gaq_policy_desc_rnn_enc))
    return fail(GAQ_ERR_INVALID, "gaq_policy_desc_rnn_enc size mismatch (header vs library): a recurrent policy with an encoder");
  gaq_policy_desc_rnn r{};
  r.struct_size = sizeof(r);
  r.in_dim = x->in_dim; r.n_hidden = x->n_hidden; r.hidden_act = x->hidden_act; r.out_tanh = x->out_tanh;
  for (int l = 0; l < 3; ++l) r.width[l] = x->width[l];
  r.engine = x->engine; r.cell = x->cell;
  if (x->enc_layers < 1 || x->enc_layers > 2) return fail(GAQ_ERR_INVALID, "policy: encoder: enc_layers must be 1 or 2");
  for (int l = 0; l < x->enc_layers; ++l)
    if (x->enc_width[l] < 16 || x->enc_width[l] > kPolMfmaMaxWidth || x->enc_width[l] % 16 != 0)
      return fail(GAQ_ERR_INVALID, "policy: encoder: enc_width[" + std::to_string(l) + "] must be a multiple of 16 in [16, " +
                                       std::to_string(kPolMfmaMaxWidth) + "]");
  if (x->enc_in_dim <= 0) return fail(GAQ_ERR_INVALID, "policy: encoder: enc_in_dim must be positive");
  if (x->in_dim != x->enc_width[x->enc_layers - 1])
    return fail(GAQ_ERR_INVALID, "policy: encoder: the cell's in_dim (" + std::to_string(x->in_dim) + ") must be the encoder's last width (" +
                                     std::to_string(x->enc_width[x->enc_layers - 1]) + ")");
  if ((size_t)encoder_rows(x->enc_in_dim, x->enc_layers, x->enc_width) * kTile * 4 > kLdsMax)
    return fail(GAQ_ERR_INVALID, "policy: encoder: enc_in_dim too large for the encoder's LDS");
  if (int rc = policy_check_desc_rnn(&r, d)) return rc;             // the cell and the head: gaq_policy_desc_rnn's checks and texts
  cell = x->cell;
  enc = PolicyDev{};
  enc.in_dim = x->enc_in_dim; enc.n_hidden = x->enc_layers; enc.hidden_act = x->hidden_act;
  int64_t n = 0, in = x->enc_in_dim;
  for (int l = 0; l < x->enc_layers; ++l) {
    enc.width[l] = x->enc_width[l];
    enc.off[l] = (int32_t)n;
    n += (int64_t)x->enc_width[l] * in + x->enc_width[l];
    in = x->enc_width[l];
  }
  enc.off[x->enc_layers] = (int32_t)n;                            // (the block's floats: the encoder has no output layer)
  return GAQ_OK;
}
// LDS of one policy launch's workgroup: `base` bytes of rows / image, then the hidden-activation scratch
int policy_lds(const void* fn, size_t base, const PolicyDev& pd, size_t& lds) {
  lds = ((base + 15) & ~(size_t)15) + (size_t)pd.scratch_bytes;
  if (lds > kLdsMax) return fail(GAQ_ERR_INVALID, "policy: state image + hidden activations exceed the CU's LDS");
  if (lds > 65536) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return GAQ_OK;
}

// the floats of hidden layer 0 as net_layout takes them.  A recurrent cell of H = width[0] units and G gates (PolicyCell::gates):
// W_ih' [GH/16][in_dim][16], b_ih [GH], W_hh' [GH/16][H][16], b_hh [GH]; -1 for no cell: a layer like the others
int64_t policy_layer0_count(const gaq_policy_desc& d, int cell) {
  if (cell == GAQ_POLICY_CELL_NONE) return -1;
  const int64_t g = policy_cell(cell)->gates;
  return g * (int64_t)d.width[0] * (d.in_dim + d.width[0]) + 2 * g * (int64_t)d.width[0];
}

// enc: the layers of an encoder in front of the cell (nullptr: none), which then takes the observation in d->in_dim's place
int policy_create(gaq_env* e, const gaq_policy_desc* d, int engine, int cell, gaq_policy** out, const PolicyDev* enc = nullptr) {
  if (e->cfg.control == GAQ_CTRL_MELLINGER) return fail(GAQ_ERR_INVALID, "policy: the env runs the Mellinger controller (RawControl only)");
  if (enc && enc->in_dim != e->obs_dim) return fail(GAQ_ERR_INVALID, "policy: encoder: enc_in_dim != the env's obs_dim");
  if (!enc && d->in_dim != e->obs_dim) return fail(GAQ_ERR_INVALID, "policy: in_dim != the env's obs_dim");
  HIP_TRY(hipSetDevice(e->cfg.device));
  gaq_policy* p = new (std::nothrow) gaq_policy;
  if (!p) return fail(GAQ_ERR_INVALID, "out of host memory");
  const PolicyEngine& eng = *policy_engine(engine);
  p->desc = *d; p->engine = engine;
  const bool rnn = cell != GAQ_POLICY_CELL_NONE;
  p->cell = cell; p->n = e->d.n;
  p->lds_base = rnn ? policy_gru_lds(*d) : eng.lds_base(*d);
  if (int rc = net_create(p->net, e, *d, d->out_tanh, policy_layer0_count(*d, cell), 4)) { (void)gaq_policy_destroy(p); return rc; }
  // the cell: W_ih', b_ih, then W_hh', b_hh
  if (rnn) p->off_hh = (int32_t)(policy_cell(cell)->gates * ((int64_t)d->width[0] * d->in_dim + (int64_t)d->width[0]));
  int64_t scratch = 0;
  for (int l = 0; l < d->n_hidden - 1; ++l) scratch += (int64_t)d->width[l] * kTile * 4;     // the last hidden layer is never stored
  p->net.pd.scratch_bytes = eng.scratch ? (int32_t)scratch : 0;
  p->net.pd.explore = 0;
  if (engine == GAQ_POLICY_ENGINE_MFMA_BF16) {
    int64_t fo = 0, k = d->in_dim;
    for (int l = 0; l < d->n_hidden; ++l) { p->bd.off[l] = (int32_t)fo; fo += (int64_t)(d->width[l] / 16) * ((k + 31) / 32) * 64; k = d->width[l]; }
    p->bd.off[d->n_hidden] = (int32_t)fo;
    p->nwb = fo + ((k + 31) / 32) * 64;                           // the output layer: one chunk
    p->bd.stride = policy_bf16_stride(*d);
    hipError_t hb = hipMalloc(&p->wb_dev, sizeof(bf16x8) * (size_t)p->nwb);
    if (hb != hipSuccess) { (void)gaq_policy_destroy(p); return fail(GAQ_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(hb)); }
    p->bd.w = p->wb_dev;
  }
  if (enc) {                      // its weights' block and the feature rows, both for the handle's life
    p->enc = *enc;
    p->enc_nw = enc->off[enc->n_hidden];
    hipError_t he = hipMalloc(&p->enc_w_dev, sizeof(float) * (size_t)p->enc_nw);
    if (he == hipSuccess) he = hipMalloc(&p->feat_dev, sizeof(float) * (size_t)p->n * (size_t)d->in_dim);
    if (he != hipSuccess) { (void)gaq_policy_destroy(p); return fail(GAQ_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(he)); }
    p->enc.w = p->enc_w_dev;
  }
  *out = p;
  return GAQ_OK;
}

// net_set_weights; the bf16 engine then rounds them to its fragments (policy_bf16_pack_kernel), and the weights count as set after that
int policy_set_weights(gaq_policy* p, const float* w, hipMemcpyKind kind) {
  const bool was_set = p && p->net.weights_set;
  if (int rc = net_set_weights(p ? &p->net : nullptr, w, kind)) return rc;
  if (p->engine == GAQ_POLICY_ENGINE_MFMA_BF16) {
    p->net.weights_set = was_set;
    const int total = (int)p->nwb;
    hipLaunchKernelGGL(policy_bf16_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, p->net.pd, p->bd, p->wb_dev, total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    p->net.weights_set = true;
  }
  return GAQ_OK;
}
}  // namespace

int64_t gaq_policy_weight_count(const gaq_policy_desc* d) {
  if (int rc = policy_check_desc(d)) return rc;
  return net_layout(*d, -1, 4);
}

int64_t gaq_policy_weight_count_ex(const gaq_policy_desc_ex* x) {
  gaq_policy_desc d{};
  int engine = 0;
  if (int rc = policy_check_desc_ex(x, d, engine)) return rc;
  return net_layout(d, -1, 4);
}

int gaq_policy_create(gaq_env* e, const gaq_policy_desc* d, gaq_policy** out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = policy_check_desc(d)) return rc;
  return policy_create(e, d, GAQ_POLICY_ENGINE_VALU, GAQ_POLICY_CELL_NONE, out);
}

int gaq_policy_create_ex(gaq_env* e, const gaq_policy_desc_ex* x, gaq_policy** out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  gaq_policy_desc d{};
  int engine = 0;
  if (int rc = policy_check_desc_ex(x, d, engine)) return rc;
  const PolicyEngine& eng = *policy_engine(engine);
  if (eng.lds_base(d) > eng.lds_max) return fail(GAQ_ERR_INVALID, std::string("policy: in_dim too large for the ") + eng.name + "'s LDS");
  return policy_create(e, &d, engine, GAQ_POLICY_CELL_NONE, out);
}

int64_t gaq_policy_weight_count_rnn(const gaq_policy_desc_rnn* x) {
  gaq_policy_desc d{};
  if (int rc = policy_check_desc_rnn(x, d)) return rc;
  return net_layout(d, policy_layer0_count(d, x->cell), 4);
}

int gaq_policy_create_rnn(gaq_env* e, const gaq_policy_desc_rnn* x, gaq_policy** out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  gaq_policy_desc d{};
  if (int rc = policy_check_desc_rnn(x, d)) return rc;
  if (policy_gru_lds(d) > kLdsMax)
    return fail(GAQ_ERR_INVALID, std::string("policy: in_dim too large for the ") + policy_cell(x->cell)->name + "'s LDS");
  return policy_create(e, &d, GAQ_POLICY_ENGINE_MFMA, x->cell, out);
}

// ---- an encoder in front of the cell (include/gaq.h gaq_policy_desc_rnn_enc) ----------------------------------------------------
int64_t gaq_policy_encoder_weight_count(const gaq_policy_desc_rnn_enc* x) {
  gaq_policy_desc d{};
  int cell = 0;
  PolicyDev enc{};
  if (int rc = policy_check_desc_rnn_enc(x, d, cell, enc)) return rc;
  return enc.off[enc.n_hidden];
}

int gaq_policy_create_rnn_enc(gaq_env* e, const gaq_policy_desc_rnn_enc* x, gaq_policy** out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  gaq_policy_desc d{};
  int cell = 0;
  PolicyDev enc{};
  if (int rc = policy_check_desc_rnn_enc(x, d, cell, enc)) return rc;
  if (policy_gru_lds(d) + kPolAcBytes > kLdsMax)
    return fail(GAQ_ERR_INVALID, std::string("policy: encoder: its last width is too large an input for the ") + policy_cell(cell)->name +
                                     "'s LDS at this H");
  return policy_create(e, &d, GAQ_POLICY_ENGINE_MFMA, cell, out, &enc);
}

int gaq_policy_encoder_width(const gaq_policy* p) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  return p->enc.n_hidden ? (int)p->enc.width[p->enc.n_hidden - 1] : 0;
}

namespace {
int policy_set_encoder_weights(gaq_policy* p, const float* w, hipMemcpyKind kind) {
  if (!p || !w) return fail(GAQ_ERR_INVALID, "null argument");
  if (!p->enc.n_hidden) return fail(GAQ_ERR_INVALID, "policy: it has no encoder (gaq_policy_create_rnn_enc builds one)");
  HIP_TRY(hipSetDevice(p->net.device));
  HIP_TRY(hipMemcpy(p->enc_w_dev, w, sizeof(float) * (size_t)p->enc_nw, kind));
  p->enc_set = true;
  return GAQ_OK;
}
}  // namespace

int gaq_policy_set_encoder_weights(gaq_policy* p, const float* w) { return policy_set_encoder_weights(p, w, hipMemcpyHostToDevice); }

int gaq_policy_set_encoder_weights_dev(gaq_policy* p, const float* w) { return policy_set_encoder_weights(p, w, hipMemcpyDeviceToDevice); }

int gaq_policy_engine(const gaq_policy* p) { return p ? p->engine : fail(GAQ_ERR_INVALID, "null argument"); }

int gaq_policy_cell(const gaq_policy* p) { return p ? p->cell : fail(GAQ_ERR_INVALID, "null argument"); }

int gaq_policy_set_hidden_dev(gaq_policy* p, float* hidden_dev) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->cell == GAQ_POLICY_CELL_NONE) return fail(GAQ_ERR_INVALID, "policy: a feed-forward policy has no hidden state");
  if (reinterpret_cast<uintptr_t>(hidden_dev) & 15) return fail(GAQ_ERR_INVALID, "policy: the hidden-state buffer must be 16-byte aligned");
  p->hid_dev = hidden_dev;
  return GAQ_OK;
}

int gaq_policy_set_cell_dev(gaq_policy* p, float* cell_dev) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->cell != GAQ_POLICY_CELL_LSTM) return fail(GAQ_ERR_INVALID, "policy: only an LSTM policy has a cell state");
  if (reinterpret_cast<uintptr_t>(cell_dev) & 15) return fail(GAQ_ERR_INVALID, "policy: the cell-state buffer must be 16-byte aligned");
  p->cell_dev = cell_dev;
  return GAQ_OK;
}

namespace {
// rows of the registered hidden state (an LSTM's h and c: one launch each) whose mask byte is non-zero (all for nullptr) <- 0,
// enqueued on `st`
int policy_zero_hidden(gaq_policy* p, const uint8_t* mask, hipStream_t st) {
  const int64_t words = p->n * (p->desc.width[0] / 4);
  for (float* state : {p->hid_dev, policy_cell(p->cell)->has_c ? p->cell_dev : nullptr}) {
    if (!state) continue;
    hipLaunchKernelGGL(hidden_zero_kernel, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, state, mask, p->n,
                       (int)p->desc.width[0]);
    HIP_TRY(hipGetLastError());
  }
  return GAQ_OK;
}
// GAQ_ERR_STATE unless every state buffer of a recurrent policy is registered
int policy_states_registered(const gaq_policy* p) {
  if (!p->hid_dev) return fail(GAQ_ERR_STATE, "policy: no hidden-state buffer registered (gaq_policy_set_hidden_dev)");
  if (policy_cell(p->cell)->has_c && !p->cell_dev)
    return fail(GAQ_ERR_STATE, "policy: no cell-state buffer registered (gaq_policy_set_cell_dev)");
  return GAQ_OK;
}
}  // namespace

int gaq_policy_reset_hidden_dev(gaq_policy* p, const uint8_t* mask, void* stream) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->cell == GAQ_POLICY_CELL_NONE) return fail(GAQ_ERR_INVALID, "policy: a feed-forward policy has no hidden state");
  if (int rc = policy_states_registered(p)) return rc;
  HIP_TRY(hipSetDevice(p->net.device));
  return policy_zero_hidden(p, mask, (hipStream_t)stream);
}

int gaq_policy_set_weights_dev(gaq_policy* p, const float* w) { return policy_set_weights(p, w, hipMemcpyDeviceToDevice); }

int gaq_policy_set_weights(gaq_policy* p, const float* w) { return policy_set_weights(p, w, hipMemcpyHostToDevice); }

namespace {
// the engine of a policy as the error texts name it
const char* policy_engine_name(const gaq_policy* p) {
  if (const PolicyCell* cell = policy_cell(p->cell)) return cell->name;
  const char* name = policy_engine(p->engine)->name;
  return name ? name : "VALU engine";
}
// true for the engines with an actor-critic form: fp32 MFMA, GRU and LSTM
bool policy_has_ac(const gaq_policy* p) { return p->engine == GAQ_POLICY_ENGINE_MFMA; }

int policy_set_value_head(gaq_policy* p, const float* wb, hipMemcpyKind kind) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (!policy_has_ac(p))
    return fail(GAQ_ERR_INVALID, std::string("policy: no value head on the ") + policy_engine_name(p) + " (fp32 MFMA and GRU policies only)");
  if (!wb) { p->value_set = false; return GAQ_OK; }
  const size_t bytes = sizeof(float) * ((size_t)p->desc.width[p->desc.n_hidden - 1] + 1);
  HIP_TRY(hipSetDevice(p->net.device));
  if (!p->wv_dev) HIP_TRY(hipMalloc(&p->wv_dev, bytes));
  HIP_TRY(hipMemcpy(p->wv_dev, wb, bytes, kind));
  p->value_set = true;
  return GAQ_OK;
}
}  // namespace

int gaq_policy_set_value_head(gaq_policy* p, const float* wb) { return policy_set_value_head(p, wb, hipMemcpyHostToDevice); }

int gaq_policy_set_value_head_dev(gaq_policy* p, const float* wb) { return policy_set_value_head(p, wb, hipMemcpyDeviceToDevice); }

int gaq_policy_value_width(const gaq_policy* p) {
  return p ? (int)p->desc.width[p->desc.n_hidden - 1] : fail(GAQ_ERR_INVALID, "null argument");
}

namespace {
// what the launches of an exploring policy take: the host's std4, or (a table is registered) the table's address in its place
void policy_explore_apply(gaq_policy* p) {
  PolicyDev& pd = p->net.pd;
  if (p->explore_tab) {
    const uint64_t a = reinterpret_cast<uintptr_t>(p->explore_tab);
    std::memset(pd.std4, 0, sizeof(pd.std4));
    std::memcpy(pd.std4, &a, sizeof(a));
    pd.explore = kPolExploreDev;
  } else {
    std::memcpy(pd.std4, p->explore_host + kExploreStd, sizeof(pd.std4));
    pd.explore = 1;
  }
}
}  // namespace

int gaq_policy_set_explore(gaq_policy* p, const float* log_std) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (!log_std) { p->net.pd.explore = 0; return GAQ_OK; }
  float words[kExploreWords];
  for (int k = 0; k < 4; ++k) {
    if (!std::isfinite(log_std[k])) return fail(GAQ_ERR_INVALID, "policy: log_std must be finite");
    words[k] = log_std[k];
    words[kExploreStd + k] = (float)std::exp((double)log_std[k]);
    words[kExploreInvStd + k] = (float)std::exp(-(double)log_std[k]);
  }
  if (p->explore_tab) {           // device mode: the 12 words into the table, after everything enqueued that reads or steps it
    HIP_TRY(hipSetDevice(p->net.device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(p->explore_tab, words, sizeof(words), hipMemcpyHostToDevice));
  }
  std::memcpy(p->explore_host, words, sizeof(words));
  for (int k = 0; k < 4; ++k) p->log_std[k] = log_std[k];
  policy_explore_apply(p);
  return GAQ_OK;
}

int gaq_policy_set_explore_dev(gaq_policy* p, float* table12, void* stream) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (!policy_has_ac(p))
    return fail(GAQ_ERR_INVALID, std::string("policy: no exploration table on the ") + policy_engine_name(p) +
                                     " (fp32 MFMA, GRU and LSTM policies only)");
  if (!table12) {                 // back to host mode, with the values the table holds
    if (!p->explore_tab) return GAQ_OK;
    float ls[4];
    HIP_TRY(hipSetDevice(p->net.device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ls, p->explore_tab, sizeof(ls), hipMemcpyDeviceToHost));
    const bool explores = p->net.pd.explore != 0;
    p->explore_tab = nullptr;
    if (int rc = gaq_policy_set_explore(p, ls)) return rc;
    if (!explores) p->net.pd.explore = 0;
    return GAQ_OK;
  }
  if (!p->net.pd.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no exploration to keep on the device");
  if (reinterpret_cast<uintptr_t>(table12) & 15) return fail(GAQ_ERR_INVALID, "policy: the exploration table must be 16-byte aligned");
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, table12) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != p->net.device) {
    (void)hipGetLastError();
    return fail(GAQ_ERR_INVALID, "policy: the exploration table must be device memory on the policy's device");
  }
  // the host-computed words, so that every kernel sees the bits it saw in host mode
  HIP_TRY(hipSetDevice(p->net.device));
  HIP_TRY(hipMemcpyAsync(table12, p->explore_host, sizeof(p->explore_host), hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  p->explore_tab = table12;
  policy_explore_apply(p);
  return GAQ_OK;
}

int gaq_policy_explore_mode(const gaq_policy* p) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  return !p->net.pd.explore ? GAQ_EXPLORE_NONE : p->explore_tab ? GAQ_EXPLORE_DEVICE : GAQ_EXPLORE_HOST;
}

int gaq_policy_get_log_std(const gaq_policy* p, float* out4) {
  if (!p || !out4) return fail(GAQ_ERR_INVALID, "null argument");
  if (!p->net.pd.explore) return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore)");
  if (!p->explore_tab) { std::memcpy(out4, p->log_std, sizeof(p->log_std)); return GAQ_OK; }
  HIP_TRY(hipSetDevice(p->net.device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out4, p->explore_tab, sizeof(float) * 4, hipMemcpyDeviceToHost));
  return GAQ_OK;
}

int gaq_policy_destroy(gaq_policy* p) {
  if (!p) return GAQ_OK;
  net_free(p->net);
  if (p->wb_dev) (void)hipFree(p->wb_dev);
  if (p->act_tmp) (void)hipFree(p->act_tmp);
  if (p->wv_dev) (void)hipFree(p->wv_dev);
  if (p->term_list) (void)hipFree(p->term_list);
  if (p->term_obs_tmp) (void)hipFree(p->term_obs_tmp);
  if (p->enc_w_dev) (void)hipFree(p->enc_w_dev);
  if (p->feat_dev) (void)hipFree(p->feat_dev);
  delete p;
  return GAQ_OK;
}

// ---- separate critic (include/gaq.h gaq_critic) ---------------------------------------------------------------------------------
namespace {
int critic_check_desc(const gaq_critic_desc* d) {
  if (!d || d->struct_size != sizeof(gaq_critic_desc)) return fail(GAQ_ERR_INVALID, "gaq_critic_desc: struct_size mismatch (header vs library)");
  return net_check_fields(*d, 0, {"critic", true, "hidden_act", std::string()}, kPolMfmaMaxWidth);
}
// LDS of the two critic kernels: the parts of V, then the activation rows
int critic_lds(const gaq_critic* c, const void* fn, size_t& lds) {
  lds = (size_t)kPolAcBytes + (size_t)c->net.rows * kTile * 4;
  if (lds > 65536) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return GAQ_OK;
}
// one critic_mfma_kernel launch: V of obs [rows, D] -> value_out [rows]
int critic_launch(const gaq_critic* c, int64_t rows, const float* obs, float* value_out, hipStream_t st) {
  PolicyLaunchArgs x{};
  x.grid = dim3((unsigned)((rows + kTile - 1) / kTile)); x.block = dim3(kPolMfmaBlock); x.st = st;
  x.critic = PolicyCriticDev{c->net.pd}; x.rows = rows; x.nm = policy_norm_dev(c->net.norm); x.in = obs; x.D = (int)c->desc.in_dim;
  x.ac.value_out = value_out;
  if (int rc = critic_lds(c, kCriticForm.pick(x.nm), x.lds)) return rc;
  kCriticForm.launch(x);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}
}  // namespace

int64_t gaq_critic_weight_count(const gaq_critic_desc* d) {
  if (int rc = critic_check_desc(d)) return rc;
  return net_layout(*d, -1, 1);
}

int gaq_critic_create(gaq_env* e, const gaq_critic_desc* d, gaq_critic** out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = critic_check_desc(d)) return rc;
  if (d->in_dim != e->obs_dim) return fail(GAQ_ERR_INVALID, "critic: in_dim != the env's obs_dim");
  if ((size_t)kPolMfmaOutBytes + kPolAcBytes + (size_t)net_act_rows(*d) * kTile * 4 > kLdsMax)
    return fail(GAQ_ERR_INVALID, "critic: in_dim too large for the MFMA engine's LDS");
  HIP_TRY(hipSetDevice(e->cfg.device));
  gaq_critic* c = new (std::nothrow) gaq_critic;
  if (!c) return fail(GAQ_ERR_INVALID, "out of host memory");
  c->desc = *d;
  c->fused = env_override("GAQ_NO_FUSED_CRITIC") != 1;
  if (int rc = net_create(c->net, e, *d, 0, -1, 1)) { (void)gaq_critic_destroy(c); return rc; }
  *out = c;
  return GAQ_OK;
}

int gaq_critic_set_weights_dev(gaq_critic* c, const float* w) { return net_set_weights(c ? &c->net : nullptr, w, hipMemcpyDeviceToDevice); }

int gaq_critic_set_weights(gaq_critic* c, const float* w) { return net_set_weights(c ? &c->net : nullptr, w, hipMemcpyHostToDevice); }

int gaq_critic_eval_dev(gaq_critic* c, int64_t rows, const float* obs, float* value_out, void* stream) {
  if (!c) return fail(GAQ_ERR_INVALID, "null argument");
  if (rows < 0) return fail(GAQ_ERR_INVALID, "critic: rows must not be negative");
  if (rows == 0) return GAQ_OK;
  if (!obs || !value_out) return fail(GAQ_ERR_INVALID, "null argument");
  if (rows > ((int64_t)1 << 31) * kTile - kTile) return fail(GAQ_ERR_INVALID, "critic: too many rows for one launch");
  if (!c->net.weights_set) return fail(GAQ_ERR_INVALID, "critic: weights not set");
  if ((reinterpret_cast<uintptr_t>(obs) & 3) || (reinterpret_cast<uintptr_t>(value_out) & 3))
    return fail(GAQ_ERR_INVALID, "critic: obs and value_out must be 4-byte aligned");
  HIP_TRY(hipSetDevice(c->net.device));
  return critic_launch(c, rows, obs, value_out, (hipStream_t)stream);
}

int gaq_critic_destroy(gaq_critic* c) {
  if (!c) return GAQ_OK;
  net_free(c->net);
  delete c;
  return GAQ_OK;
}

int gaq_policy_set_obs_norm(gaq_policy* p, gaq_obs_norm* n) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (n && !policy_engine(p->engine)->step.kernel_norm)
    return fail(GAQ_ERR_INVALID, std::string("policy: no observation normaliser on the ") + policy_engine_name(p) +
                                     " (MFMA, bf16, GRU and LSTM policies only)");
  return net_set_obs_norm(p->net, "policy", n);
}

int gaq_critic_set_obs_norm(gaq_critic* c, gaq_obs_norm* n) {
  return c ? net_set_obs_norm(c->net, "critic", n) : fail(GAQ_ERR_INVALID, "null argument");
}

namespace {
// what the four rollout entry points take besides the handles and the stream
constexpr float kNoLogStd[4] = {0.0f, 0.0f, 0.0f, 0.0f};
struct RolloutArgs {
  int32_t T;
  float *obs, *reward; uint8_t* done;
  float *act_out, *value, *logp, *term_value;   // optional
};
// the observation the first policy launch reads: the state head the library tracks where the observation IS that, else the last one written
const float* rollout_obs_in(const gaq_env* e) { return e->alias && !e->pack ? e->last_obs : e->cur_obs; }

// every refusal of a rollout call
int rollout_check(const gaq_env* e, const gaq_policy* p, const gaq_critic* c, const RolloutArgs& a) {
  const auto [T, obs, reward, done, act_out, value, logp, term_value] = a;
  if (!e || !p || !obs || !reward || !done) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->net.env != e) return fail(GAQ_ERR_INVALID, "policy: created for another env handle");
  if (c && c->net.env != e) return fail(GAQ_ERR_INVALID, "critic: created for another env handle");
  if (T <= 0) return fail(GAQ_ERR_INVALID, "T must be positive");
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  if (p->enc.n_hidden && !p->enc_set) return fail(GAQ_ERR_INVALID, "policy: encoder weights not set (gaq_policy_set_encoder_weights)");
  if (e->cfg.control == GAQ_CTRL_MELLINGER) return fail(GAQ_ERR_INVALID, "policy: the env runs the Mellinger controller (RawControl only)");
  // (with an encoder the observation goes to the encoder, and desc.in_dim is the encoder's last width)
  if ((p->enc.n_hidden ? p->enc.in_dim : p->desc.in_dim) != e->obs_dim) return fail(GAQ_ERR_INVALID, "policy: in_dim != the env's obs_dim");
  if (e->sc.noise == gaq::NOISE_INPUT) return fail(GAQ_ERR_INVALID, "policy rollouts do not support GAQ_NOISE_INPUT");
  const PolicyCell* cell = policy_cell(p->cell);     // recurrent (nullptr: feed-forward): the cell picks the kernels
  if (cell) if (int rc = policy_states_registered(p)) return rc;
  const int64_t n = e->d.n;
  if ((reinterpret_cast<uintptr_t>(obs) & 15) || (reinterpret_cast<uintptr_t>(act_out) & 15))
    return fail(GAQ_ERR_INVALID, "obs and actions_out must be 16-byte aligned");
  if (T > 1 && (((size_t)n * e->obs_dim * 4) & 15)) return fail(GAQ_ERR_INVALID, "step_many needs N*obs_dim*4 to be a multiple of 16");
  const bool ac_form = value || logp;
  if (ac_form || term_value || c) {
    if (!policy_has_ac(p))
      return fail(GAQ_ERR_INVALID, std::string("policy: values and log-probabilities are not computed by the ") + policy_engine_name(p) +
                                       " (fp32 MFMA and GRU policies only)");
    if (c && p->value_set)
      return fail(GAQ_ERR_STATE, "policy: it has a value head and a critic was given: remove one of them (gaq_policy_set_value_head(p, "
                                 "NULL), or critic = NULL); the library does not pick");
    if (c && !c->net.weights_set) return fail(GAQ_ERR_INVALID, "critic: weights not set");
    if (value && !c && !p->value_set) return fail(GAQ_ERR_STATE, "policy: values asked for without a value head (gaq_policy_set_value_head)");
    if (logp && !p->net.pd.explore) return fail(GAQ_ERR_STATE, "policy: log-probabilities asked for on a deterministic policy (gaq_policy_set_explore)");
    if ((reinterpret_cast<uintptr_t>(value) & 15) || (reinterpret_cast<uintptr_t>(logp) & 15))
      return fail(GAQ_ERR_INVALID, "value_out and logp_out must be 16-byte aligned");
  }
  if (term_value) {
    if (!c && !p->value_set) return fail(GAQ_ERR_STATE, "policy: terminal values asked for without a value head (gaq_policy_set_value_head)");
    if (!e->cfg.auto_reset)
      return fail(GAQ_ERR_STATE, "policy: term_value_out on a handle created with auto_reset = 0: no observation is replaced by a new episode's "
                                 "there, value_out[t + 1] already is the value of the terminal observation");
    if (reinterpret_cast<uintptr_t>(term_value) & 15) return fail(GAQ_ERR_INVALID, "term_value_out must be 16-byte aligned");
  }
  if (!rollout_obs_in(e)) return fail(GAQ_ERR_STATE, "policy: no current observation on the device (gaq_reset_dev / gaq_step_dev first)");
  return GAQ_OK;
}

// The launches of a per-step rollout call, chosen once: a function of the two handles and of which outputs were asked for, nothing else
// (no allocation, and no HIP call but the LDS attribute policy_lds / critic_lds set on the kernels it picked).
struct RolloutPlan {
  // the actor launch -- the T launches and the bootstrap launch: the MLP actor with the critic, the cell's form (a recurrent policy), the
  // MLP's actor-critic form (V and the log-prob beside the action) or the engine's plain launch
  PolicyForm actor;
  // the terminal pass: V of gathered rows from the critic, the cell's gathered form or the MLP's
  PolicyForm term;
  // with a critic V is not the actor launch's business: an MLP actor's launch is the fused policy_mfma_critic_kernel (V from the
  // critic's trunk, beside the action); a recurrent actor's, or with GAQ_NO_FUSED_CRITIC=1, is the launch the call without values
  // makes, followed by critic_mfma_kernel on the same observation
  // (the fused launch stages the observation once per trunk through ONE table: an actor and a critic with different normalisers, or
  // only one of them with one, take the two launches)
  bool crit_fused, crit_batch, actor_ac;
  // the normalisers: the actor's for its launches, and for the terminal pass that of the net V comes from
  PolObsNorm actor_nm, term_nm;
  size_t actor_lds, term_lds;     // (term_lds: 0 unless terminal values were asked for)
  // an encoder in front of the cell: its launch stages the observation, so it carries the policy's normaliser (enc_nm) and the cell's
  // launches -- the actor's, and the terminal pass unless a critic makes it -- read the feature rows as they are (actor_nm, term_nm: none)
  PolObsNorm enc_nm;
  size_t enc_lds;
};
// the LDS attribute of the encoder's two kernels (the instantiations enc_nm picks), where its rows pass the default limit
int encoder_lds(const gaq_policy* p, const PolObsNorm& nm, bool term, size_t& lds) {
  lds = (size_t)encoder_rows(p->enc.in_dim, p->enc.n_hidden, p->enc.width) * kTile * 4;
  if (lds <= 65536) return GAQ_OK;
  HIP_TRY(hipFuncSetAttribute(kEncodeForm.pick(nm), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (term) HIP_TRY(hipFuncSetAttribute(kEncodeTermForm.pick(nm), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return GAQ_OK;
}
int rollout_plan(const gaq_policy* p, const gaq_critic* c, bool value, bool logp, bool term_value, RolloutPlan& pl) {
  const PolicyCell* cell = policy_cell(p->cell);     // recurrent (nullptr: feed-forward): the cell picks the kernels
  pl.term = c ? kCriticTermForm : cell ? cell->term : kMfmaTermForm;
  pl.actor_nm = policy_norm_dev(p->net.norm);
  pl.term_nm = policy_norm_dev(c ? c->net.norm : p->net.norm);
  pl.enc_nm = PolObsNorm{nullptr, 0};
  pl.enc_lds = 0;
  if (p->enc.n_hidden) {
    pl.enc_nm = pl.actor_nm;
    pl.actor_nm = PolObsNorm{nullptr, 0};
    if (!c) pl.term_nm = PolObsNorm{nullptr, 0};
    if (int rc = encoder_lds(p, pl.enc_nm, term_value && !c, pl.enc_lds)) return rc;
  }
  pl.term_lds = 0;
  if (term_value) {
    if (c) { if (int rc = critic_lds(c, pl.term.pick(pl.term_nm), pl.term_lds)) return rc; }
    else if (int rc = policy_lds(pl.term.pick(pl.term_nm), p->lds_base + kPolAcBytes, p->net.pd, pl.term_lds)) return rc;
  }
  pl.crit_fused = c && value && !cell && c->fused && c->net.norm == p->net.norm;
  pl.crit_batch = c && value && !pl.crit_fused;
  pl.actor_ac = c ? logp : value || logp;
  pl.actor = pl.crit_fused ? kFusedCriticForm
             : cell        ? (pl.actor_ac ? cell->ac : cell->step)
             : pl.actor_ac ? kMfmaAcForm
                           : policy_engine(p->engine)->step;
  // (the fused launch's activation rows: the wider of the actor's and the critic's)
  const size_t lds_base = !pl.crit_fused ? p->lds_base + (pl.actor_ac ? kPolAcBytes : 0)
      : (size_t)kPolMfmaOutBytes + kPolAcBytes + (size_t)std::max(p->net.rows, c->net.rows) * kTile * 4;
  return policy_lds(pl.actor.pick(pl.actor_nm), lds_base, p->net.pd, pl.actor_lds);
}

// the launches of a checked call on `st`: the fused closed-loop launch where the layout has one, else the plan's, T times
int rollout_run(gaq_env* e, gaq_policy* p, gaq_critic* c, const RolloutArgs& a, hipStream_t st) {
  const auto [T, obs, reward, done, act_out, value, logp, term_value] = a;
  const int64_t n = e->d.n;
  const bool heads = e->alias && !e->pack;           // (rollout_obs_in)
  const float* in = rollout_obs_in(e);
  // an MFMA or bf16 policy always takes the per-step path below
  const uint32_t roll_variant = p->engine == GAQ_POLICY_ENGINE_VALU ? fused_variant(e) : 0xFFFFFFFFu;
  if (roll_variant != 0xFFFFFFFFu) {
    return fused_rollout(e, T, obs, st, [&]() -> int {
      decltype(&policy_rollout_kernel<16u>) kernel = nullptr;
      switch (roll_variant) {
#define GAQ_X(FEAT) case (FEAT): kernel = &policy_rollout_kernel<(FEAT)>; break;
        GAQ_PROLL_ALL(GAQ_X)
#undef GAQ_X
        default: return fail(GAQ_ERR_STATE, "internal: no closed-loop rollout instantiation for this feature mask");
      }
      size_t lds = 0;
      if (int rc = policy_lds((const void*)kernel, (size_t)e->lds_per_wave, p->net.pd, lds)) return rc;
      if (roll_variant != e->noted_proll) { launch_record().note(2, roll_variant); e->noted_proll = roll_variant; }
      hipLaunchKernelGGL(kernel, dim3((unsigned)e->d.ntiles), dim3(kPolBlock), lds, st, e->d, e->sc, e->um, (int)a.T, p->net.pd, a.act_out,
                         a.obs, a.reward, a.done, e->lds_per_wave);
      return GAQ_OK;
    });
  }
  // one policy launch on the current observation, then the ordinary step launch, T times
  if (!act_out && p->act_tmp_n < n) {
    if (p->act_tmp) { HIP_TRY(hipStreamSynchronize(st)); (void)hipFree(p->act_tmp); p->act_tmp = nullptr; p->act_tmp_n = 0; }
    HIP_TRY(hipMalloc(&p->act_tmp, sizeof(float) * 4 * (size_t)n));
    p->act_tmp_n = n;
  }
  // terminal values: the list and its two counters, and a terminal-observation buffer of the library's own where the caller has none
  // (registered for this call's step launches only: the guard puts the caller's registration back on every way out)
  const int64_t term_cap = e->d.ntiles * kTile;
  struct TermObsGuard { gaq_env* e; float* user; ~TermObsGuard() { e->d.term_obs = user; } } term_guard{e, e->d.term_obs};
  uint32_t* term_cnt = nullptr;
  if (term_value) {
    if (!p->term_list) HIP_TRY(hipMalloc(&p->term_list, sizeof(uint32_t) * ((size_t)term_cap + 2)));
    if (!e->d.term_obs) {
      if (!p->term_obs_tmp) HIP_TRY(hipMalloc(&p->term_obs_tmp, sizeof(float) * (size_t)n * (size_t)e->obs_dim));
      e->d.term_obs = p->term_obs_tmp;
    }
    term_cnt = p->term_list + term_cap;
  }
  RolloutPlan pl;
  if (int rc = rollout_plan(p, c, value != nullptr, logp != nullptr, term_value != nullptr, pl)) return rc;
  if (term_value) HIP_TRY(hipMemsetAsync(term_cnt, 0, 2 * sizeof(uint32_t), st));
  const bool ac_form = value || logp;
  PolicyLaunchArgs x{};
  x.grid = dim3((unsigned)e->d.ntiles); x.block = dim3(policy_engine(p->engine)->block); x.st = st; x.lds = pl.actor_lds;
  x.e = e; x.p = p; x.D = e->obs_dim; x.nm = pl.actor_nm;
  if (c) x.critic = PolicyCriticDev{c->net.pd};
  // An encoder in front of the cell: every actor launch is preceded by the encoder's launch on the observation, and reads the feature
  // rows [N, E] in the observation's place (x.D = E = desc.in_dim; pl.actor_nm is none).  The critic and the step keep the observation.
  const bool enc = p->enc.n_hidden != 0;
  if (enc) { x.D = (int)p->desc.in_dim; x.enc = PolicyEncDev{p->enc, p->feat_dev}; x.rows = n; }
  auto actor_in = [&](const float* o) -> const float* {
    if (!enc) return o;
    PolicyLaunchArgs y = x;
    y.lds = pl.enc_lds; y.nm = pl.enc_nm; y.in = o; y.D = e->obs_dim;
    kEncodeForm.launch(y);
    return p->feat_dev;
  };
  // (a device-mode policy's launches carry the table's address in p->net.pd and no value of log_std)
  const float* ls = p->explore_tab ? kNoLogStd : p->log_std;
  PolicyAcDev ac{c ? (pl.crit_fused ? c->net.w_dev + c->net.pd.off[c->net.pd.n_hidden] : nullptr) : value ? p->wv_dev : nullptr, nullptr,
                 nullptr, {ls[0], ls[1], ls[2], ls[3]}, 0};
  for (int32_t t = 0; t < T; ++t) {
    if (ac_form) {
      ac.value_out = value ? value + (size_t)t * n : nullptr;
      ac.logp_out = logp ? logp + (size_t)t * n : nullptr;
    }
    // a recurrent launch reads its state with the rows that finished in step t - 1 zeroed first
    x.sc = e->sc; x.done_prev = t ? done + (size_t)(t - 1) * n : nullptr; x.ac = ac; x.in = actor_in(in);
    x.a = act_out ? act_out + (size_t)t * n * 4 : p->act_tmp;
    pl.actor.launch(x);
    HIP_TRY(hipGetLastError());
    // (before the step launch: in the alias layout it overwrites the observation)
    if (pl.crit_batch) if (int rc = critic_launch(c, n, in, value + (size_t)t * n, st)) return rc;
    float* o = obs + (size_t)t * n * e->obs_dim;
    if (int rc = launch_step(e, x.a, o, reward + (size_t)t * n, done + (size_t)t * n, st)) return rc;
    in = heads ? e->last_obs : o;
    if (term_value) {
      // V of the rows step t has just written to the terminal-observation buffer, before policy launch t + 1 (or the bootstrap launch,
      // or the masked zero below) reads done[t] and a GRU's finished rows of h start over: the states as they are, no done mask
      float* row = term_value + (size_t)t * n;
      hipLaunchKernelGGL(term_gather_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, done + (size_t)t * n, n,
                         p->term_list, term_cnt + (t & 1), term_cnt + ((t + 1) & 1), row);
      HIP_TRY(hipGetLastError());
      PolicyLaunchArgs y = x;
      y.lds = pl.term_lds; y.done_prev = nullptr; y.nm = pl.term_nm;
      y.ac = PolicyAcDev{p->wv_dev, row, nullptr, {0.0f, 0.0f, 0.0f, 0.0f}, 1};
      y.tm = PolicyTermDev{p->term_list, term_cnt + (t & 1), e->d.term_obs};
      if (enc && c) y.D = e->obs_dim;                // (the critic's gathered form reads the terminal observations themselves)
      if (enc && !c) {
        // the encoder's gathered launch: the terminal observations of the listed envs -> those envs' feature rows (launch t's
        // features have been consumed, launch t + 1 rewrites every row), which the cell's gathered form then reads by env
        PolicyLaunchArgs z = y;
        z.lds = pl.enc_lds; z.nm = pl.enc_nm; z.D = e->obs_dim;
        kEncodeTermForm.launch(z);
        HIP_TRY(hipGetLastError());
        y.tm.term_obs = p->feat_dev;
      }
      pl.term.launch(y);
      HIP_TRY(hipGetLastError());
    }
  }
  if (value && c) {
    // the bootstrap row from the critic: V of the observation the call ends on
    if (int rc = critic_launch(c, n, in, value + (size_t)T * n, st)) return rc;
  } else if (value) {
    // the bootstrap row: V of the observation the call ends on, as the next call's first launch will see it (a GRU's h with the rows of
    // done[T-1] read as 0), from the actor launch with value_only: it writes nothing else and leaves the step counter alone
    ac.value_only = 1; ac.value_out = value + (size_t)T * n; ac.logp_out = nullptr;
    x.sc = e->sc; x.done_prev = done + (size_t)(T - 1) * n; x.ac = ac; x.in = actor_in(in); x.a = nullptr;
    pl.actor.launch(x);
    HIP_TRY(hipGetLastError());
  }
  // the rows that finished in the last step start the next call from h = 0 (an LSTM's from h = c = 0)
  if (p->cell != GAQ_POLICY_CELL_NONE) return policy_zero_hidden(p, done + (size_t)(T - 1) * n, st);
  return GAQ_OK;
}

// gaq_step_policy_many_dev (value = logp = nullptr: the launches it always made), gaq_step_policy_ac_many_dev, with term_value
// gaq_step_policy_ac_term_many_dev (term_value = nullptr: the launches of the other two, nothing else) and, with a critic,
// gaq_step_policy_critic_many_dev (c = nullptr: the launches of the other three, nothing else)
int policy_rollout(gaq_env* e, gaq_policy* p, gaq_critic* c, int32_t T, float* obs, float* reward, uint8_t* done, float* act_out,
                   float* value, float* logp, float* term_value, void* stream) {
  const RolloutArgs a{T, obs, reward, done, act_out, value, logp, term_value};
  if (int rc = rollout_check(e, p, c, a)) return rc;
  e->info_valid = false;
  HIP_TRY(hipSetDevice(e->cfg.device));
  e->user_stream = (hipStream_t)stream; e->user_stream_used = true;
  hipStream_t st = (hipStream_t)stream;
  if (e->timing) HIP_TRY(hipEventRecord(e->ev0, st));
  if (int rc = rollout_run(e, p, c, a, st)) return rc;
  if (e->timing) { HIP_TRY(hipEventRecord(e->ev1, st)); e->timed = true; }
  return GAQ_OK;
}
}  // namespace

int gaq_step_policy_many_dev(gaq_env* e, gaq_policy* p, int32_t T, float* obs, float* reward, uint8_t* done, float* act_out, void* stream) {
  return policy_rollout(e, p, nullptr, T, obs, reward, done, act_out, nullptr, nullptr, nullptr, stream);
}

int gaq_step_policy_ac_many_dev(gaq_env* e, gaq_policy* p, int32_t T, float* obs, float* reward, uint8_t* done, float* act_out, float* value,
                                float* logp, void* stream) {
  return policy_rollout(e, p, nullptr, T, obs, reward, done, act_out, value, logp, nullptr, stream);
}

int gaq_step_policy_ac_term_many_dev(gaq_env* e, gaq_policy* p, int32_t T, float* obs, float* reward, uint8_t* done, float* act_out,
                                     float* value, float* logp, float* term_value, void* stream) {
  return policy_rollout(e, p, nullptr, T, obs, reward, done, act_out, value, logp, term_value, stream);
}

int gaq_step_policy_critic_many_dev(gaq_env* e, gaq_policy* p, gaq_critic* c, int32_t T, float* obs, float* reward, uint8_t* done,
                                    float* act_out, float* value, float* logp, float* term_value, void* stream) {
  return policy_rollout(e, p, c, T, obs, reward, done, act_out, value, logp, term_value, stream);
}

}  // extern "C"

// ---- gaq_policy_grad.hip's view of the two handles (gaq_grad.hpp) ----------------------------------------------------------------
namespace {
int grad_check_widths(const char* what, const PolicyDev& pd) {
  for (int l = 0; l < pd.n_hidden; ++l)
    if (pd.width[l] > kGradMaxWidth)
      return fail(GAQ_ERR_INVALID, std::string(what) + ": the gradient passes take hidden widths up to " + std::to_string(kGradMaxWidth) +
                                       ", width[" + std::to_string(l) + "] is " + std::to_string(pd.width[l]));
  return GAQ_OK;
}
}  // namespace

int policy_grad_view(gaq_policy* p, GradNet& v) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->engine != GAQ_POLICY_ENGINE_MFMA || p->cell != GAQ_POLICY_CELL_NONE)
    return fail(GAQ_ERR_INVALID, std::string("policy: no gradient passes on the ") + policy_engine_name(p) +
                                     " (feed-forward fp32 MFMA policies only)");
  if (int rc = grad_check_widths("policy", p->net.pd)) return rc;
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  v = GradNet{&p->net, p->log_std, p->net.pd.explore != 0, p->value_set ? p->wv_dev : nullptr, 0, p->explore_tab};
  return GAQ_OK;
}

// the wide forms' one limit (gaq.h "the wide learner"): every layer's activations of a 64-row tile stay in LDS
namespace {
int grad_check_wide_rows(const char* what, const PolicyDev& pd) {
  int rows = (pd.in_dim + 15) & ~15;
  for (int l = 0; l < pd.n_hidden; ++l) rows += pd.width[l];
  if (rows > kGradWideRows)
    return fail(GAQ_ERR_INVALID, std::string(what) + ": the wide gradient passes keep a tile's activations in LDS: in_dim rounded up to 16 plus the "
                                     "hidden layers' sizes sum to " + std::to_string(rows) + " rows, and " + std::to_string(kGradWideRows) +
                                     " fit (three layers of 256 do not)");
  return GAQ_OK;
}
}  // namespace

int policy_grad_wide_view(gaq_policy* p, GradNet& v) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->engine != GAQ_POLICY_ENGINE_MFMA || p->cell != GAQ_POLICY_CELL_NONE)
    return fail(GAQ_ERR_INVALID, std::string("policy: no wide gradient passes on the ") + policy_engine_name(p) +
                                     " (feed-forward fp32 MFMA policies only)");
  if (int rc = grad_check_wide_rows("policy", p->net.pd)) return rc;
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  v = GradNet{&p->net, p->log_std, p->net.pd.explore != 0, p->value_set ? p->wv_dev : nullptr, 0, p->explore_tab};
  return GAQ_OK;
}

int critic_grad_wide_view(gaq_critic* c, GradNet& v) {
  if (!c) return fail(GAQ_ERR_INVALID, "null argument");
  if (int rc = grad_check_wide_rows("critic", c->net.pd)) return rc;
  if (!c->net.weights_set) return fail(GAQ_ERR_INVALID, "critic: weights not set");
  v = GradNet{&c->net, nullptr, false};
  return GAQ_OK;
}

int policy_grad_seq_view(gaq_policy* p, int cell, GradNet& v) {
  const bool lstm = cell == GAQ_POLICY_CELL_LSTM;
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->cell == GAQ_POLICY_CELL_NONE)
    return fail(GAQ_ERR_INVALID, std::string("policy: the sequence passes need a recurrent cell, this is a feed-forward policy on the ") +
                                     policy_engine_name(p) + " (gaq_policy_logp_dev and its kin take stored rows)");
  if (p->cell != cell)
    return fail(GAQ_ERR_INVALID, lstm ? "policy: the LSTM sequence passes take an LSTM policy, this one is on the GRU engine "
                                        "(gaq_policy_eval_seq_dev and gaq_policy_grad_ppo_seq_dev take it)"
                                      : "policy: no sequence passes on the LSTM engine yet (GRU policies only)");
  if (p->enc.n_hidden)
    return fail(GAQ_ERR_INVALID, "policy: no sequence passes on a policy with an encoder yet (gaq_policy_eval_seq_dev, gaq_policy_grad_ppo_seq_dev, "
                                 "their index-gathered and LSTM forms: the learner of this architecture is not built; train through torch "
                                 "and gaq_policy_set_weights_dev + gaq_policy_set_encoder_weights_dev)");
  for (int l = 0; l < p->net.pd.n_hidden; ++l)
    if (p->net.pd.width[l] > kGradSeqMaxWidth)
      return fail(GAQ_ERR_INVALID, std::string("policy: the sequence passes take ") + (lstm ? "an LSTM" : "a GRU") + " and head layers of width up to " +
                                       std::to_string(kGradSeqMaxWidth) + ", width[" + std::to_string(l) + "] is " +
                                       std::to_string(p->net.pd.width[l]));
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  v = GradNet{&p->net, p->log_std, p->net.pd.explore != 0, p->value_set ? p->wv_dev : nullptr, p->off_hh, p->explore_tab};
  return GAQ_OK;
}

int policy_grad_seq_wide_view(gaq_policy* p, GradNet& v) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->cell == GAQ_POLICY_CELL_NONE)
    return fail(GAQ_ERR_INVALID, std::string("policy: the wide sequence passes need a GRU cell, this is a feed-forward policy on the ") +
                                     policy_engine_name(p) + " (gaq_policy_eval_wide_dev and gaq_policy_grad_ppo_wide_dev take stored rows)");
  if (p->cell != GAQ_POLICY_CELL_GRU)
    return fail(GAQ_ERR_INVALID, "policy: no wide sequence passes on the LSTM engine yet (GRU policies only; gaq_policy_grad_ppo_lstm_seq_dev "
                                 "takes an LSTM of up to 64 units)");
  if (p->enc.n_hidden)
    return fail(GAQ_ERR_INVALID, "policy: no wide sequence passes on a policy with an encoder yet (gaq_policy_eval_enc_seq_dev and "
                                 "gaq_policy_grad_ppo_enc_seq_dev take a cell of up to 64 units behind an encoder)");
  for (int l = 0; l < p->net.pd.n_hidden; ++l) {
    const int lim = l ? kGradSeqMaxWidth : kGradSeqWideMaxWidth;
    if (p->net.pd.width[l] > lim)
      return fail(GAQ_ERR_INVALID, "policy: the wide sequence passes take a GRU of up to " + std::to_string(kGradSeqWideMaxWidth) +
                                       " units and head layers of width up to " + std::to_string(kGradSeqMaxWidth) + ", width[" +
                                       std::to_string(l) + "] is " + std::to_string(p->net.pd.width[l]));
  }
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  v = GradNet{&p->net, p->log_std, p->net.pd.explore != 0, p->value_set ? p->wv_dev : nullptr, p->off_hh, p->explore_tab};
  return GAQ_OK;
}

int policy_grad_enc_seq_view(gaq_policy* p, bool cell_args, GradNet& v, GradEnc& e) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (!p->enc.n_hidden)
    return fail(GAQ_ERR_INVALID, std::string("policy: the encoder sequence passes take a policy with an encoder in front of its cell "
                                             "(gaq_policy_create_rnn_enc), this one on the ") + policy_engine_name(p) + " has none");
  const bool lstm = p->cell == GAQ_POLICY_CELL_LSTM;
  if (!lstm && cell_args)
    return fail(GAQ_ERR_INVALID, "policy: c0 and c_out are an LSTM's cell state: they must be NULL for a policy on the GRU engine");
  if (int rc = grad_check_widths("policy: encoder", p->enc)) return rc;
  for (int l = 0; l < p->net.pd.n_hidden; ++l)
    if (p->net.pd.width[l] > kGradSeqMaxWidth)
      return fail(GAQ_ERR_INVALID, std::string("policy: the encoder sequence passes take ") + (lstm ? "an LSTM" : "a GRU") +
                                       " and head layers of width up to " + std::to_string(kGradSeqMaxWidth) + ", width[" + std::to_string(l) +
                                       "] is " + std::to_string(p->net.pd.width[l]));
  if (!p->enc_set) return fail(GAQ_ERR_INVALID, "policy: encoder weights not set (gaq_policy_set_encoder_weights)");
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  v = GradNet{&p->net, p->log_std, p->net.pd.explore != 0, p->value_set ? p->wv_dev : nullptr, p->off_hh, p->explore_tab};
  e = GradEnc{p, lstm, p->enc.in_dim, p->enc.width[p->enc.n_hidden - 1], p->enc, p->enc_nw};
  return GAQ_OK;
}

int policy_encode_rows(const GradEnc& e, int64_t rows, const float* obs, float* feat, hipStream_t st) {
  const gaq_policy* p = e.p;
  PolicyLaunchArgs x{};
  x.grid = dim3((unsigned)((rows + kTile - 1) / kTile)); x.block = dim3(kPolMfmaBlock); x.st = st;
  x.p = p; x.enc = PolicyEncDev{p->enc, feat}; x.rows = rows; x.nm = policy_norm_dev(p->net.norm); x.in = obs; x.D = e.in_dim;
  if (int rc = encoder_lds(p, x.nm, false, x.lds)) return rc;
  kEncodeForm.launch(x);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

int policy_encode_list(const GradEnc& e, int64_t slots, const uint32_t* list, const uint32_t* count, const float* obs, float* feat, hipStream_t st) {
  const gaq_policy* p = e.p;
  PolicyLaunchArgs x{};
  x.grid = dim3((unsigned)((slots + kTile - 1) / kTile)); x.block = dim3(kPolMfmaBlock); x.st = st;
  x.p = p; x.enc = PolicyEncDev{p->enc, feat}; x.tm = PolicyTermDev{list, count, obs}; x.nm = policy_norm_dev(p->net.norm); x.D = e.in_dim;
  if (int rc = encoder_lds(p, x.nm, true, x.lds)) return rc;
  kEncodeTermForm.launch(x);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

int critic_grad_view(gaq_critic* c, GradNet& v) {
  if (!c) return fail(GAQ_ERR_INVALID, "null argument");
  if (int rc = grad_check_widths("critic", c->net.pd)) return rc;
  if (!c->net.weights_set) return fail(GAQ_ERR_INVALID, "critic: weights not set");
  v = GradNet{&c->net, nullptr, false};
  return GAQ_OK;
}

// ---- gaq_optim.hip's view of the two handles (gaq_grad.hpp), and the weights back to the host --------------------------------------
int policy_optim_view(gaq_policy* p, OptimView& v) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (p->engine == GAQ_POLICY_ENGINE_MFMA_BF16)
    return fail(GAQ_ERR_INVALID, std::string("optim: no step in place on the ") + policy_engine_name(p) +
                                     " (its kernels read bf16 fragments repacked from the weights, which would go stale)");
  if (p->enc.n_hidden)
    return fail(GAQ_ERR_INVALID, "optim: no step in place on a policy with an encoder yet (gaq_optim_create_policy would step the cell and "
                                 "the head and leave the encoder's block behind; no gradient pass fills it)");
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  v = OptimView{&p->net, p->value_set ? p->wv_dev : nullptr, p->value_set ? (int)p->desc.width[p->desc.n_hidden - 1] + 1 : 0,
                p->net.pd.explore != 0, p->log_std, p->explore_tab};
  return GAQ_OK;
}

int policy_optim_enc_view(gaq_policy* p, OptimView& v) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  if (!p->enc.n_hidden)
    return fail(GAQ_ERR_INVALID, "optim: gaq_optim_create_policy_enc steps a policy with an encoder in front of its cell, this one has none "
                                 "(gaq_optim_create_policy takes it)");
  if (!p->enc_set) return fail(GAQ_ERR_INVALID, "policy: encoder weights not set (gaq_policy_set_encoder_weights)");
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  v = OptimView{&p->net, p->value_set ? p->wv_dev : nullptr, p->value_set ? (int)p->desc.width[p->desc.n_hidden - 1] + 1 : 0,
                p->net.pd.explore != 0, p->log_std, p->explore_tab, p->enc_w_dev, p->enc_nw};
  return GAQ_OK;
}

int critic_optim_view(gaq_critic* c, OptimView& v) {
  if (!c) return fail(GAQ_ERR_INVALID, "null argument");
  if (!c->net.weights_set) return fail(GAQ_ERR_INVALID, "critic: weights not set");
  v = OptimView{&c->net};
  return GAQ_OK;
}

namespace {
// a device buffer of a handle to the host, after everything enqueued on the device (an optimiser's step on any stream) has finished
int net_read_back(int device, const float* src, size_t floats, float* host) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, src, sizeof(float) * floats, hipMemcpyDeviceToHost));
  return GAQ_OK;
}
}  // namespace

extern "C" {

int gaq_policy_get_weights(gaq_policy* p, float* host) {
  if (!p || !host) return fail(GAQ_ERR_INVALID, "null argument");
  if (!p->net.weights_set) return fail(GAQ_ERR_INVALID, "policy: weights not set");
  return net_read_back(p->net.device, p->net.w_dev, (size_t)p->net.nw, host);
}

int gaq_policy_get_encoder_weights(gaq_policy* p, float* host) {
  if (!p || !host) return fail(GAQ_ERR_INVALID, "null argument");
  if (!p->enc.n_hidden) return fail(GAQ_ERR_INVALID, "policy: it has no encoder (gaq_policy_create_rnn_enc builds one)");
  if (!p->enc_set) return fail(GAQ_ERR_INVALID, "policy: encoder weights not set");
  return net_read_back(p->net.device, p->enc_w_dev, (size_t)p->enc_nw, host);
}

int gaq_policy_get_value_head(gaq_policy* p, float* host) {
  if (!p || !host) return fail(GAQ_ERR_INVALID, "null argument");
  if (!p->value_set) return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head)");
  return net_read_back(p->net.device, p->wv_dev, (size_t)p->desc.width[p->desc.n_hidden - 1] + 1, host);
}

int gaq_critic_get_weights(gaq_critic* c, float* host) {
  if (!c || !host) return fail(GAQ_ERR_INVALID, "null argument");
  if (!c->net.weights_set) return fail(GAQ_ERR_INVALID, "critic: weights not set");
  return net_read_back(c->net.device, c->net.w_dev, (size_t)c->net.nw, host);
}

}  // extern "C"
