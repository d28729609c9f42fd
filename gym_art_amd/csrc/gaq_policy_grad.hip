// gaq_policy_grad.hip -- the learner's passes over stored rows for the feed-forward fp32 MFMA family (include/gaq.h "gradients on the
// device"): gaq_policy_logp_dev, gaq_policy_backward_dev, gaq_policy_grad_ppo_dev, gaq_critic_backward_dev, gaq_critic_grad_mse_dev, and
// the shared-trunk actor-critic forms gaq_policy_eval_ac_dev and gaq_policy_grad_ppo_ac_dev (a value head on the policy's trunk), and
// the index-gathered forms of the three loss gradients (gaq_policy_grad_ppo_idx_dev, gaq_policy_grad_ppo_ac_idx_dev,
// gaq_critic_grad_mse_idx_dev: three more Modes of the kernel, in which only the addresses of the loads differ), and the wide forms
// for hidden widths up to 256 (gaq_policy_eval_wide_dev, gaq_policy_grad_ppo_wide_dev, gaq_critic_grad_mse_wide_dev: grad_wide_kernel,
// a sibling of grad_kernel further down).
// Of gaq_policy.hip it uses the net record of a handle that gaq_grad.hpp declares; of the observation normaliser what gaq_norm.hpp holds.
//
// One kernel template, grad_kernel<Mode>, 4 waves per workgroup, works per 64-row tile:
//   forward   the observation is staged as policy_mfma_kernel stages it (env e at column grad_col(e) = pol_col(e), padded inputs -0, dead
//             lanes 0, live inputs through the normaliser's table), then every hidden layer runs on v_mfma_f32_16x16x4_f32 with that
//             kernel's arithmetic -- accumulators start at the bias, the k-steps ascend, each MFMA a k-ordered fmaf chain, wave w owns the
//             16-unit chunks w, w + 4 -- but writes its activations to rows of its OWN, so that every layer's h stays in LDS.  The head
//             is policy_out_part's chain (bias, then the units ascending), wave o summing output o.  mean is therefore the bits
//             policy_mfma_kernel computes.  (The stages are restated here rather than shared: the rollout kernels keep their recorded
//             resource lines, and the rows here have a stride of their own.)
//   rows      wave 0, lane = row: logp, the surrogate or the squared error, the head's delta -> dlt[o][column] (dead lanes: exactly 0).
//   backward  head: thread u owns unit u of the last layer: dWo[u][:] = sum_e dlt[:][e] h[u][e] in ascending column order, then the row
//             is overwritten with delta = (Wo[u][:] . dlt[:][e]) act'(h).  Hidden layer l, from the last down: dW_l = delta_l h_{l-1}^T
//             as MFMAs whose K dimension is the tile's 64 rows (A = delta_l, B = h_{l-1}, both read "transposed": lane (n, kk) takes
//             columns 16 j + 4 kk + i of row n), db_l = the row sums of delta_l, then delta_{l-1} = (W_l^T delta_l) act'(h_{l-1}) as MFMAs
//             whose A operand is the packed W_l read 16 bytes per lane (4 consecutive units of one input: coalesced) over h_{l-1}.
// LDS rows have a stride of 68 floats, not 64: the forward reads (one row, 64 consecutive floats per 16 lanes) stay conflict-free and the
// transposed reads (16 rows, 4 floats each) land on 16 x 4 different banks.  LDS = 6 KiB + 272 B x (in_dim rounded up to 16 + the sum of
// the widths): 116 KiB at 18-128-128-128, one workgroup per CU (three at 18-64-64).
// Determinism: G workgroups, workgroup g takes the tiles [g nt / G, (g + 1) nt / G) in ascending order -- a function of `rows` alone.
// A tile's weight gradients are formed in registers (at most 4 blocks of 16 x 16 per wave at a time) and added to the workgroup's
// partial in the handle's scratch, each word by the one lane that owns it, the first tile storing instead of adding; the partials stay
// in L2.  grad_reduce_kernel then sums the G partials of every parameter in ascending order in fp64 and rounds once.  No atomics.
// (It is the one reduce of this unit's forms and of gaq_policy_grad_seq.hip's: the host's routing table places the statistics.)
// The actor-critic forms (GRAD_EVAL_AC, GRAD_PPO_AC) add the value head V = wv . y + bv to the same pass: every wave sums its quarter of
// V beside its output (policy_value_part's chain: from 0, the units ascending), wave 0 adds the parts as policy_value_sum does
// (((p0 + p1) + (p2 + p3)) + bias: the bits policy_mfma_ac_kernel writes), the row stage forms a fifth delta, the head backward a fifth
// sum per unit, and the head's W + 1 gradient words follow the packed weights in the workgroup's partial.  Their head region is larger
// (5 rows of dlt, 4 of V's parts, 10 statistics): 8.25 KiB instead of 6, 118.75 KiB at 18-128-128-128.
#include "gaq_host.hpp"
#include "gaq_norm.hpp"
#include "gaq_grad.hpp"
#include "gaq_grad_dev.hpp"

namespace {

// dlt, outs, (V's parts,) the statistics' lanes
constexpr int grad_head_bytes(bool ac) { return ac ? (5 + 4 + 4) * kTile * 4 + kGradStatsAc * kTile * 8 : 2 * 4 * kTile * 4 + kGradStats * kTile * 8; }

enum GradMode { GRAD_LOGP = 0, GRAD_BACKWARD = 1, GRAD_PPO = 2, GRAD_MSE = 3, GRAD_EVAL_AC = 4, GRAD_PPO_AC = 5,
                // the index-gathered twins (gaq.h "shuffled minibatches"): row j of the call is source row idx[j]
                GRAD_PPO_IDX = 6, GRAD_MSE_IDX = 7, GRAD_PPO_AC_IDX = 8 };
constexpr bool grad_is_idx(int mode) { return mode >= GRAD_PPO_IDX; }
constexpr int grad_base(int mode) { return mode == GRAD_PPO_IDX ? GRAD_PPO : mode == GRAD_MSE_IDX ? GRAD_MSE : mode == GRAD_PPO_AC_IDX ? GRAD_PPO_AC : mode; }
constexpr bool grad_is_ac(int mode) { return grad_base(mode) == GRAD_EVAL_AC || grad_base(mode) == GRAD_PPO_AC; }
constexpr bool grad_is_forward(int mode) { return mode == GRAD_LOGP || mode == GRAD_EVAL_AC; }

struct GradArgs {
  PolicyDev net;
  int32_t n_out;
  PolObsNorm nm;                  // tab = nullptr: no normaliser
  int64_t rows, ntiles;
  const float* obs;               // [rows, D]
  const float* a;                 // actions [rows, 4] (logp, ppo), dout [rows, n_out] (backward), target [rows] (mse)
  const float* logp_old;          // [rows] (ppo)
  const float* adv;               // [rows] (ppo)
  float clip, scale;
  float log_std[4], inv_std[4];   // the caller's log_std and exp(-log_std)
  float* logp_out;                // [rows] (logp)
  float* mean_out;                // [rows, 4] or nullptr (logp)
  float* part;                    // [G][pstride] the workgroups' partial gradients
  double* spart;                  // [G][kGradStats] (the actor-critic form: [G][kGradStatsAc])
  int64_t pstride;
  // the actor-critic forms (after what the other forms read, whose offsets stay)
  const float* wv;                // the value head: the last width's weights, then the bias
  const float* ret;               // [rows] (ppo_ac)
  const float* v_old;             // [rows] (ppo_ac with vclip > 0)
  float vclip, vf_coef;
  float* value_out;               // [rows] (eval_ac)
  // the idx forms (at the end: every offset above stays); obs, a, logp_old, adv, ret, v_old are then [src_rows, ...]
  const int32_t* idx;             // [rows] source rows
  int64_t src_rows;
  // device mode (after everything else: every offset above stays): the policy's table log_std[4] | std[4] | inv_std[4], read by the
  // row stage in place of log_std and inv_std above, which are then 0
  const float* explore_tab;
};

// this wave's NC chunks of one hidden layer: rows 0 .. in-1 of A (zero-padded to a multiple of 4) -> act(bias + W a) in the rows of O
template <int NC>
__device__ __forceinline__ void grad_fwd_layer(const float* __restrict__ wl, int in, int width, int act, int wave, const float* A, float* O,
                                               uint32_t lane) {
  const int h = (int)(lane >> 4);
  const float* bl = wl + width * in;
  f32x4 acc[NC][4];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const float* b = bl + (wave + 4 * j) * 16 + 4 * h;
    const f32x4 b4 = {b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[j][eb] = b4;
  }
  const float* arow = A + h * kGradStride + (lane & 15) * 4;
  const int kfull = in & ~3;
  for (int k0 = 0; k0 < kfull; k0 += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + k0 * kGradStride);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float a = wl[((wave + 4 * j) * in + k0) * 16 + lane];
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[j][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[j][eb], 0, 0, 0);
    }
  }
  if (kfull < in) {                                               // the first layer's last, partial k-step: no weight past in - 1 is read
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + kfull * kGradStride);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float a = kfull + h < in ? wl[((wave + 4 * j) * in + kfull) * 16 + lane] : 0.0f;
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[j][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[j][eb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x4 v = {pol_act(act, acc[j][0][r]), pol_act(act, acc[j][1][r]), pol_act(act, acc[j][2][r]), pol_act(act, acc[j][3][r])};
      *reinterpret_cast<f32x4*>(O + ((wave + 4 * j) * 16 + 4 * h + r) * kGradStride + (lane & 15) * 4) = v;
    }
  }
}

// `g` must stay the kernel's first and only argument: the row stage reads its own members of it at offset 0 of the kernel-argument
// segment (below), which a parameter put in front of `g` would silently move.
template <int M>
__global__ __launch_bounds__(kGradBlock) void grad_kernel(GradArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int Mode = grad_base(M);                              // an idx form is its parent's code with other load addresses
  constexpr bool Idx = grad_is_idx(M);
  constexpr bool Ac = grad_is_ac(Mode), Fwd = grad_is_forward(Mode);
  constexpr bool Ppo = Mode == GRAD_PPO || Mode == GRAD_PPO_AC, Logp = Mode == GRAD_LOGP || Mode == GRAD_EVAL_AC;
  constexpr int ND = Ac ? 5 : 4, NS = Ac ? kGradStatsAc : kGradStats;    // rows of dlt (the fifth: V's delta), statistics
  float* dlt = reinterpret_cast<float*>(smem);                    // [ND][64] the head's delta, row e at column grad_col(e)
  float* outs = dlt + ND * kTile;                                 // [4][64] the head's sums, row e at e
  [[maybe_unused]] float* vsum = outs + 4 * kTile;                // Ac: [4][64] the waves' parts of V, row e at e
  double* red = reinterpret_cast<double*>(smem + (ND + 4 + (Ac ? 4 : 0)) * kTile * 4);   // [NS][64]
  [[maybe_unused]] int* sidx = reinterpret_cast<int*>(smem + grad_head_bytes(Ac));   // Idx: [64] the tile's source rows (or < 0)
  float* X = reinterpret_cast<float*>(smem + grad_head_bytes(Ac) + (Idx ? kGradIdxBytes : 0));   // [kx][68] the observation; the layers' rows follow
  const PolicyDev& net = g.net;
  const int D = net.in_dim, kin = (D + 3) & ~3, kx = (D + 15) & ~15, nh = net.n_hidden, act = net.hidden_act, no = g.n_out;
  const uint32_t lane = threadIdx.x & 63u;
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w0 = net.width[0], w1 = net.width[1];
  auto Hl = [&](int l) { return X + (kx + (l > 0 ? w0 : 0) + (l > 1 ? w1 : 0)) * kGradStride; };   // layer l's rows
  const int G = (int)gridDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * g.ntiles / G, t1 = ((int64_t)blockIdx.x + 1) * g.ntiles / G;
  float* part = g.part + (int64_t)blockIdx.x * g.pstride;
  // the statistics: lane e of wave 0 keeps the sums of the rows it has seen in red[.][e] (nobody else touches them before the end)
  if (wave == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) red[s * kTile + lane] = 0.0;
  }

#pragma unroll 1
  for (int64_t tile = t0; tile < t1; ++tile) {
    const bool first = tile == t0;
    const int64_t row0 = tile * kTile;
    const int nlive = (int)((g.rows - row0) < kTile ? (g.rows - row0) : kTile);
    if constexpr (Idx) {
      // the tile's indices, read once: an index outside [0, src_rows) makes its lane a dead one (no address is ever formed from it)
      // and is counted by the row stage.  (The last readers of sidx, the previous tile's row stage, stand behind several barriers.)
      if (tid < kTile) {
        const auto& r = *(const __attribute__((address_space(4))) GradArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        int s = kGradIdxDead;
        if (tid < nlive) {
          const int64_t v = r.idx[row0 + tid];
          s = v >= 0 && v < r.src_rows ? (int)v : kGradIdxSkipped;
        }
        sidx[tid] = s;
      }
      __syncthreads();
    }
    // the tile's observations: dead rows 0, padded inputs -0, the rows up to a multiple of 16 (only dW's B operand reads them) 0
    for (int f = tid; f < kTile * kx; f += kGradBlock) {
      const int e = f / kx, k = f - e * kx;
      float v = k >= kin ? 0.0f : -0.0f;
      if (k < D) {
        v = 0.0f;
        int64_t src = row0 + e;
        bool on = e < nlive;
        if constexpr (Idx) {
          src = sidx[e];
          on = src >= 0;
        }
        if (on) {
          v = g.obs[src * D + k];
          if (g.nm.tab) v = g.nm(v, k);
        }
      }
      X[k * kGradStride + grad_col(e)] = v;
    }
    __syncthreads();
    // forward: layer l reads its input's rows and writes rows of its own
    {
      const float* A = X;
      int in = D;
#pragma unroll 1
      for (int l = 0; l < nh; ++l) {
        const int width = net.width[l];
        const float* wl = net.w + net.off[l];
        const int nc = (width / 16 - wave + 3) / 4;
        if (nc == 1) grad_fwd_layer<1>(wl, in, width, act, wave, A, Hl(l), lane);
        else if (nc == 2) grad_fwd_layer<2>(wl, in, width, act, wave, A, Hl(l), lane);
        __syncthreads();
        A = Hl(l);
        in = width;
      }
    }
    const int lw = net.width[nh - 1];                             // the last hidden layer: what the head reads
    float* Y = Hl(nh - 1);
    const float* wo = net.w + net.off[nh];                        // [lw][no], then bias[no]
    if (wave < no) {
      const float* ycol = Y + grad_col((int)lane);
      float s = wo[lw * no + wave];
#pragma unroll 8
      for (int u = 0; u < lw; ++u) s = __builtin_fmaf(wo[u * no + wave], ycol[u * kGradStride], s);
      outs[wave * kTile + lane] = s;
    }
    if constexpr (Ac) {                                           // this wave's quarter of V: policy_value_part's chain
      const float* ycol = Y + grad_col((int)lane);
      const int q = lw / kGradWaves;
      float v = 0.0f;
#pragma unroll 8
      for (int u = wave * q; u < (wave + 1) * q; ++u) v = __builtin_fmaf(g.wv[u], ycol[u * kGradStride], v);
      vsum[wave * kTile + lane] = v;
    }
    __syncthreads();
    if (wave == 0) {                                              // lane = row
      // (the row stage's arguments are read from the kernel-argument segment here, where they are used: as members of `g` they are
      //  fetched at the kernel's start and held in scalar registers through the MFMA phases, which spills)
      const auto& r = *(const __attribute__((address_space(4))) GradArgs*)__builtin_amdgcn_kernarg_segment_ptr();
      const int e = (int)lane;
      bool live = e < nlive;
      int64_t i = row0 + e;
      if constexpr (Idx) {                                        // the source row; a skipped index is counted in the spare statistic
        i = sidx[e];
        live = i >= 0;
        if (i == kGradIdxSkipped) red[(NS - 1) * kTile + e] += 1.0;
      }
      float d[ND];                                                // the head's delta (already times scale)
#pragma unroll
      for (int o = 0; o < ND; ++o) d[o] = 0.0f;
      if constexpr (Mode == GRAD_MSE) {
        const float v = outs[e];
        if (live) {
          const float df = v - r.a[i];
          d[0] = r.scale * df;
          red[e] += 0.5 * (double)df * (double)df;
        }
      } else {
        float m[4], dm[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          m[o] = o < no ? outs[o * kTile + e] : 0.0f;
          if (net.out_tanh) m[o] = tanhf(m[o]);
          dm[o] = net.out_tanh ? __builtin_fmaf(-m[o], m[o], 1.0f) : 1.0f;
        }
        if constexpr (Mode == GRAD_BACKWARD) {
          if (live) {
#pragma unroll
            for (int o = 0; o < 4; ++o)
              if (o < no) d[o] = r.scale * r.a[i * no + o] * dm[o];
          }
        } else if (live) {
          float z[4], lp = 0.0f, ls[4], is[4];
          grad_explore(r, ls, is);
#pragma unroll
          for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * is[o];
#pragma unroll
          for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
          lp -= kGradTwoLn2Pi;
          [[maybe_unused]] float V = 0.0f;
          if constexpr (Ac) V = ((vsum[e] + vsum[kTile + e]) + (vsum[2 * kTile + e] + vsum[3 * kTile + e])) + r.wv[lw];   // policy_value_sum
          if constexpr (Logp) {
            r.logp_out[i] = lp;
            if constexpr (Ac) r.value_out[i] = V;
            if (r.mean_out) {
#pragma unroll
              for (int o = 0; o < 4; ++o) r.mean_out[i * 4 + o] = m[o];
            }
          } else {                                                // GRAD_PPO, GRAD_PPO_AC
            const float x = lp - r.logp_old[i], rt = expf(x), adv = r.adv[i];
            const float s1 = rt * adv, s2 = fminf(fmaxf(rt, 1.0f - r.clip), 1.0f + r.clip) * adv;
            const float dl = s1 <= s2 ? -adv * rt : 0.0f;          // dL / dlogp
            red[e] += (double)-fminf(s1, s2);
            red[kTile + e] += s2 < s1 ? 1.0 : 0.0;
            red[2 * kTile + e] += (double)rt - 1.0 - (double)x;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              d[o] = r.scale * dl * z[o] * is[o] * dm[o];
              red[(3 + o) * kTile + e] += (double)(r.scale * dl) * ((double)z[o] * (double)z[o] - 1.0);
            }
            if constexpr (Ac) {                                   // L_V = 1/2 max(e1^2, e2^2); dL_V / dV = e1 unless the clipped error is larger
              const float ret = r.ret[i], e1 = V - ret;
              float lv = e1 * e1, dv = e1;
              if (r.vclip > 0.0f) {
                // (where the clamp does not bind the two errors are one number, a tie: e2 is taken as e1 itself, not recomputed with
                //  other roundings)
                const float vo = r.v_old[i], dvo = V - vo, cl = fminf(fmaxf(dvo, -r.vclip), r.vclip);
                const float e2 = cl == dvo ? e1 : vo + cl - ret, l2 = e2 * e2;
                if (!(lv >= l2)) {
                  lv = l2;
                  dv = 0.0f;
                  red[8 * kTile + e] += 1.0;
                }
              }
              d[4] = r.scale * r.vf_coef * dv;
              red[7 * kTile + e] += 0.5 * (double)lv;
            }
          }
        }
      }
      if constexpr (!Fwd) {
#pragma unroll
        for (int o = 0; o < ND; ++o) dlt[o * kTile + grad_col(e)] = d[o];
      }
    }
    if constexpr (!Fwd) {
      __syncthreads();
      // the head: thread u owns unit u of the last hidden layer -- dWo[u][:] (Ac: and dwv[u]), then its row becomes delta; ND more
      // threads sum dbo (and dbv).  The value head's words follow the packed weights in the partial.
      [[maybe_unused]] float* pv = part + net.off[nh] + (lw + 1) * no;
      if (tid < lw) {
        float* yrow = Y + tid * kGradStride;
        float w4[ND], gw[ND];
#pragma unroll
        for (int o = 0; o < 4; ++o) w4[o] = o < no ? wo[tid * no + o] : 0.0f;
        if constexpr (Ac) w4[4] = g.wv[tid];
#pragma unroll
        for (int o = 0; o < ND; ++o) gw[o] = 0.0f;
#pragma unroll 4
        for (int q = 0; q < kTile / 4; ++q) {
          const f32x4 hv = *reinterpret_cast<const f32x4*>(yrow + 4 * q);
          f32x4 dv[ND], nv;
#pragma unroll
          for (int o = 0; o < ND; ++o) dv[o] = *reinterpret_cast<const f32x4*>(dlt + o * kTile + 4 * q);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float s = 0.0f;
#pragma unroll
            for (int o = 0; o < ND; ++o) {
              gw[o] = __builtin_fmaf(dv[o][c], hv[c], gw[o]);
              s = __builtin_fmaf(w4[o], dv[o][c], s);
            }
            nv[c] = s * grad_actd(act, hv[c]);
          }
          *reinterpret_cast<f32x4*>(yrow + 4 * q) = nv;
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
          if (o < no) grad_put(part + net.off[nh] + tid * no + o, gw[o], first);
        if constexpr (Ac) grad_put(pv + tid, gw[4], first);
      } else if (tid >= kGradBlock - ND && (tid - (kGradBlock - ND) < no || Ac)) {
        const int o = tid - (kGradBlock - ND);
        float s = 0.0f;
        for (int c = 0; c < kTile; ++c) s += dlt[o * kTile + c];
        grad_put(o < 4 ? part + net.off[nh] + lw * no + o : pv + lw, s, first);
      }
      __syncthreads();
      // the hidden layers, from the last down: dW_l and db_l from delta_l (in Hl(l)) and the layer's input, then delta_{l-1} over the input
#pragma unroll 1
      for (int l = nh - 1; l >= 0; --l) {
        const int width = net.width[l], in = l ? net.width[l - 1] : D;
        float* A = l ? Hl(l - 1) : X;
        const float* dl = Hl(l);
        const float* wl = net.w + net.off[l];
        float* pw = part + net.off[l];
        // (grad_dw's loop and grad_row_sum, restated: called as functions they move this kernel's instructions)
        const int nkc = (in + 15) / 16;
#pragma unroll 1
        for (int uc = wave; uc < width / 16; uc += kGradWaves) {
#pragma unroll 1
          for (int kc0 = 0; kc0 < nkc; kc0 += 4) {
            switch (nkc - kc0 < 4 ? nkc - kc0 : 4) {
              case 1: grad_dw_blocks<1>(dl, uc * 16, A, in, uc, kc0, lane, pw, first); break;
              case 2: grad_dw_blocks<2>(dl, uc * 16, A, in, uc, kc0, lane, pw, first); break;
              case 3: grad_dw_blocks<3>(dl, uc * 16, A, in, uc, kc0, lane, pw, first); break;
              default: grad_dw_blocks<4>(dl, uc * 16, A, in, uc, kc0, lane, pw, first); break;
            }
          }
        }
        if (tid < width) {                                        // db_l[u]: the row's 64 columns in ascending order
          const float* drow = dl + tid * kGradStride;
          float s = 0.0f;
#pragma unroll 4
          for (int q = 0; q < kTile / 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(drow + 4 * q);
            s = ((s + v[0]) + v[1]) + v[2] + v[3];
          }
          grad_put(pw + width * in + tid, s, first);
        }
        __syncthreads();                                          // dW_l has consumed the layer's input
        if (l > 0) {
          // (KEEP IN STEP: grad_wt_delta below is this loop for grad_wide_kernel, and that kernel's row and head stages restate this
          //  kernel's; a change of arithmetic here is made there too -- tests/test_gpu_policy_grad_wide.py::test_narrow_parity holds
          //  the two kernels to equal bits)
          const int n = (int)(lane & 15), kk = (int)(lane >> 4);
#pragma unroll 1
          for (int kc = wave; kc < in / 16; kc += kGradWaves) {
            f32x4 acc[4];
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) acc[eb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            for (int uch = 0; uch < width / 16; ++uch) {
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + ((int64_t)uch * in + kc * 16 + n) * 16 + 4 * kk);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(dl + (uch * 16 + 4 * kk + i) * kGradStride + n * 4);
#pragma unroll
                for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              f32x4* pos = reinterpret_cast<f32x4*>(A + (kc * 16 + 4 * kk + r) * kGradStride + n * 4);
              const f32x4 hv = *pos;
              const f32x4 nv = {acc[0][r] * grad_actd(act, hv[0]), acc[1][r] * grad_actd(act, hv[1]), acc[2][r] * grad_actd(act, hv[2]),
                                acc[3][r] * grad_actd(act, hv[3])};
              *pos = nv;
            }
          }
          __syncthreads();
        }
      }
    } else {
      __syncthreads();                                            // the rows are read before the next tile is staged
    }
  }

  if constexpr (Ppo || Mode == GRAD_MSE) {
    if (tid < NS) {                                               // the 64 lanes in ascending order
      double s = 0.0;
      for (int e = 0; e < kTile; ++e) s += red[tid * kTile + e];
      g.spart[(int64_t)blockIdx.x * NS + tid] = s;
    }
  }
}

// ---- the wide forms (gaq.h "the wide learner": hidden widths up to 256) ------------------------------------------------------------
// grad_wide_kernel<M>, M one of GRAD_EVAL_AC, GRAD_PPO_AC, GRAD_PPO_AC_IDX, GRAD_MSE, GRAD_MSE_IDX: a sibling of grad_kernel built from
// its pieces, and not more Modes of it, for grad_feat_kernel's reason (the nine instantiations keep their instructions while that
// kernel's text stays what it is).  Tile for tile it is grad_kernel's arithmetic in grad_kernel's order -- on a net of widths <= 128 it
// returns the narrow call's bits -- and differs in three places:
//   forward   a wave owns up to 4 chunks of a layer (w, w + 4, w + 8, w + 12): grad_fwd_layer<3> and <4>, 64 accumulator registers;
//   head      the sums of dbo (and dbv) are not the unit stage's `else`: at a last width of 256 every thread owns a unit, so the last ND
//             threads sum them after their unit.  dlt is only read by both, so no barrier stands between;
//   value     the policy forms run the actor-critic layout (5 rows of dlt, V's parts, 10 statistics) with or without a value head:
//             without one (g.wv == nullptr, wave-uniform) V's parts are not summed, the fifth delta and the fifth weight are 0 (a sum
//             that starts at +0 never becomes -0), and the head's W + 1 words are neither written nor reduced.
// LDS = the head region (8.25 KiB, a critic's 6) (+ 256 B) + 272 B x (in_dim rounded up to 16 + the sum of the widths), at most 560 rows:
// 161 024 B.  Above 64 KiB grad_launch asks for it.  One workgroup per CU at 256-256.
// the one limit of the wide forms is the LDS a workgroup may ask for: the largest form (value head, index vector) at kGradWideRows rows
static_assert(grad_head_bytes(true) + kGradIdxBytes + (size_t)kGradWideRows * kGradStride * 4 <= kGradLdsMax, "kGradWideRows rows do not fit LDS");
static_assert(grad_head_bytes(true) + kGradIdxBytes + (size_t)(kGradWideRows + 16) * kGradStride * 4 > kGradLdsMax, "kGradWideRows is not the most LDS holds");
__device__ __forceinline__ void grad_wt_delta(const float* __restrict__ wl, const float* dl, float* A, int in, int width, int act, int wave,
                                              uint32_t lane) {
  // delta_{l-1} = (W_l^T delta_l) act'(h_{l-1}) over the layer's input rows A: grad_kernel's loop
  const int n = (int)(lane & 15), kk = (int)(lane >> 4);
#pragma unroll 1
  for (int kc = wave; kc < in / 16; kc += kGradWaves) {
    f32x4 acc[4];
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[eb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int uch = 0; uch < width / 16; ++uch) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + ((int64_t)uch * in + kc * 16 + n) * 16 + 4 * kk);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(dl + (uch * 16 + 4 * kk + i) * kGradStride + n * 4);
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      f32x4* pos = reinterpret_cast<f32x4*>(A + (kc * 16 + 4 * kk + r) * kGradStride + n * 4);
      const f32x4 hv = *pos;
      const f32x4 nv = {acc[0][r] * grad_actd(act, hv[0]), acc[1][r] * grad_actd(act, hv[1]), acc[2][r] * grad_actd(act, hv[2]),
                        acc[3][r] * grad_actd(act, hv[3])};
      *pos = nv;
    }
  }
}

// `g` must stay the kernel's first and only argument (as in grad_kernel: the row stage reads it from the kernel-argument segment)
template <int M>
__global__ __launch_bounds__(kGradBlock) void grad_wide_kernel(GradArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int Mode = grad_base(M);
  constexpr bool Idx = grad_is_idx(M);
  constexpr bool Ac = grad_is_ac(Mode), Fwd = grad_is_forward(Mode);
  static_assert(Mode == GRAD_EVAL_AC || Mode == GRAD_PPO_AC || Mode == GRAD_MSE, "the wide forms");
  constexpr int ND = Ac ? 5 : 4, NS = Ac ? kGradStatsAc : kGradStats;
  float* dlt = reinterpret_cast<float*>(smem);                    // [ND][64] the head's delta, row e at column grad_col(e)
  float* outs = dlt + ND * kTile;                                 // [4][64] the head's sums, row e at e
  [[maybe_unused]] float* vsum = outs + 4 * kTile;                // Ac: [4][64] the waves' parts of V, row e at e
  double* red = reinterpret_cast<double*>(smem + (ND + 4 + (Ac ? 4 : 0)) * kTile * 4);   // [NS][64]
  [[maybe_unused]] int* sidx = reinterpret_cast<int*>(smem + grad_head_bytes(Ac));   // Idx: [64] the tile's source rows (or < 0)
  float* X = reinterpret_cast<float*>(smem + grad_head_bytes(Ac) + (Idx ? kGradIdxBytes : 0));   // [kx][68] the observation; the layers' rows follow
  const PolicyDev& net = g.net;
  const int D = net.in_dim, kin = (D + 3) & ~3, kx = (D + 15) & ~15, nh = net.n_hidden, act = net.hidden_act, no = g.n_out;
  const uint32_t lane = threadIdx.x & 63u;
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w0 = net.width[0], w1 = net.width[1];
  auto Hl = [&](int l) { return X + (kx + (l > 0 ? w0 : 0) + (l > 1 ? w1 : 0)) * kGradStride; };   // layer l's rows
  const int G = (int)gridDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * g.ntiles / G, t1 = ((int64_t)blockIdx.x + 1) * g.ntiles / G;
  float* part = g.part + (int64_t)blockIdx.x * g.pstride;
  [[maybe_unused]] const bool head = g.wv != nullptr;             // Ac: the policy has a value head
  if (wave == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) red[s * kTile + lane] = 0.0;
  }

#pragma unroll 1
  for (int64_t tile = t0; tile < t1; ++tile) {
    const bool first = tile == t0;
    const int64_t row0 = tile * kTile;
    const int nlive = (int)((g.rows - row0) < kTile ? (g.rows - row0) : kTile);
    if constexpr (Idx) {
      // the tile's indices, read once: an index outside [0, src_rows) makes its lane a dead one (no address is ever formed from it)
      if (tid < kTile) {
        const auto& r = *(const __attribute__((address_space(4))) GradArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        int s = kGradIdxDead;
        if (tid < nlive) {
          const int64_t v = r.idx[row0 + tid];
          s = v >= 0 && v < r.src_rows ? (int)v : kGradIdxSkipped;
        }
        sidx[tid] = s;
      }
      __syncthreads();
    }
    // the tile's observations: dead rows 0, padded inputs -0, the rows up to a multiple of 16 (only dW's B operand reads them) 0
    for (int f = tid; f < kTile * kx; f += kGradBlock) {
      const int e = f / kx, k = f - e * kx;
      float v = k >= kin ? 0.0f : -0.0f;
      if (k < D) {
        v = 0.0f;
        int64_t src = row0 + e;
        bool on = e < nlive;
        if constexpr (Idx) {
          src = sidx[e];
          on = src >= 0;
        }
        if (on) {
          v = g.obs[src * D + k];
          if (g.nm.tab) v = g.nm(v, k);
        }
      }
      X[k * kGradStride + grad_col(e)] = v;
    }
    __syncthreads();
    {
      const float* A = X;
      int in = D;
#pragma unroll 1
      for (int l = 0; l < nh; ++l) {
        const int width = net.width[l];
        const float* wl = net.w + net.off[l];
        const int nc = (width / 16 - wave + 3) / 4;
        if (nc == 1) grad_fwd_layer<1>(wl, in, width, act, wave, A, Hl(l), lane);
        else if (nc == 2) grad_fwd_layer<2>(wl, in, width, act, wave, A, Hl(l), lane);
        else if (nc == 3) grad_fwd_layer<3>(wl, in, width, act, wave, A, Hl(l), lane);
        else if (nc == 4) grad_fwd_layer<4>(wl, in, width, act, wave, A, Hl(l), lane);
        __syncthreads();
        A = Hl(l);
        in = width;
      }
    }
    const int lw = net.width[nh - 1];                             // the last hidden layer: what the head reads
    float* Y = Hl(nh - 1);
    const float* wo = net.w + net.off[nh];                        // [lw][no], then bias[no]
    if (wave < no) {
      const float* ycol = Y + grad_col((int)lane);
      float s = wo[lw * no + wave];
#pragma unroll 8
      for (int u = 0; u < lw; ++u) s = __builtin_fmaf(wo[u * no + wave], ycol[u * kGradStride], s);
      outs[wave * kTile + lane] = s;
    }
    if constexpr (Ac) {                                           // this wave's quarter of V: policy_value_part's chain
      if (head) {
        const float* ycol = Y + grad_col((int)lane);
        const int q = lw / kGradWaves;
        float v = 0.0f;
#pragma unroll 8
        for (int u = wave * q; u < (wave + 1) * q; ++u) v = __builtin_fmaf(g.wv[u], ycol[u * kGradStride], v);
        vsum[wave * kTile + lane] = v;
      }
    }
    __syncthreads();
    if (wave == 0) {                                              // lane = row
      const auto& r = *(const __attribute__((address_space(4))) GradArgs*)__builtin_amdgcn_kernarg_segment_ptr();
      const int e = (int)lane;
      bool live = e < nlive;
      int64_t i = row0 + e;
      if constexpr (Idx) {                                        // the source row; a skipped index is counted in the spare statistic
        i = sidx[e];
        live = i >= 0;
        if (i == kGradIdxSkipped) red[(NS - 1) * kTile + e] += 1.0;
      }
      float d[ND];                                                // the head's delta (already times scale)
#pragma unroll
      for (int o = 0; o < ND; ++o) d[o] = 0.0f;
      if constexpr (Mode == GRAD_MSE) {
        const float v = outs[e];
        if (live) {
          const float df = v - r.a[i];
          d[0] = r.scale * df;
          red[e] += 0.5 * (double)df * (double)df;
        }
      } else {
        float m[4], dm[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          m[o] = o < no ? outs[o * kTile + e] : 0.0f;
          if (net.out_tanh) m[o] = tanhf(m[o]);
          dm[o] = net.out_tanh ? __builtin_fmaf(-m[o], m[o], 1.0f) : 1.0f;
        }
        if (live) {
          float z[4], lp = 0.0f, ls[4], is[4];
          grad_explore(r, ls, is);
#pragma unroll
          for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * is[o];
#pragma unroll
          for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
          lp -= kGradTwoLn2Pi;
          float V = 0.0f;
          if (head) V = ((vsum[e] + vsum[kTile + e]) + (vsum[2 * kTile + e] + vsum[3 * kTile + e])) + r.wv[lw];   // policy_value_sum
          if constexpr (Fwd) {
            r.logp_out[i] = lp;
            if (head) r.value_out[i] = V;
            if (r.mean_out) {
#pragma unroll
              for (int o = 0; o < 4; ++o) r.mean_out[i * 4 + o] = m[o];
            }
          } else {                                                // GRAD_PPO_AC
            const float x = lp - r.logp_old[i], rt = expf(x), adv = r.adv[i];
            const float s1 = rt * adv, s2 = fminf(fmaxf(rt, 1.0f - r.clip), 1.0f + r.clip) * adv;
            const float dl = s1 <= s2 ? -adv * rt : 0.0f;          // dL / dlogp
            red[e] += (double)-fminf(s1, s2);
            red[kTile + e] += s2 < s1 ? 1.0 : 0.0;
            red[2 * kTile + e] += (double)rt - 1.0 - (double)x;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              d[o] = r.scale * dl * z[o] * is[o] * dm[o];
              red[(3 + o) * kTile + e] += (double)(r.scale * dl) * ((double)z[o] * (double)z[o] - 1.0);
            }
            if (head) {                                           // L_V = 1/2 max(e1^2, e2^2); dL_V / dV = e1 unless the clipped error is larger
              const float ret = r.ret[i], e1 = V - ret;
              float lv = e1 * e1, dv = e1;
              if (r.vclip > 0.0f) {
                // (where the clamp does not bind the two errors are one number, a tie: e2 is taken as e1 itself)
                const float vo = r.v_old[i], dvo = V - vo, cl = fminf(fmaxf(dvo, -r.vclip), r.vclip);
                const float e2 = cl == dvo ? e1 : vo + cl - ret, l2 = e2 * e2;
                if (!(lv >= l2)) {
                  lv = l2;
                  dv = 0.0f;
                  red[8 * kTile + e] += 1.0;
                }
              }
              d[4] = r.scale * r.vf_coef * dv;
              red[7 * kTile + e] += 0.5 * (double)lv;
            }
          }
        }
      }
      if constexpr (!Fwd) {
#pragma unroll
        for (int o = 0; o < ND; ++o) dlt[o * kTile + grad_col(e)] = d[o];
      }
    }
    if constexpr (!Fwd) {
      __syncthreads();
      // the head: thread u owns unit u of the last hidden layer -- dWo[u][:] (and dwv[u]), then its row becomes delta; the last ND
      // threads then sum dbo (and dbv).  The value head's words follow the packed weights in the partial.
      [[maybe_unused]] float* pv = part + net.off[nh] + (lw + 1) * no;
      if (tid < lw) {
        float* yrow = Y + tid * kGradStride;
        float w4[ND], gw[ND];
#pragma unroll
        for (int o = 0; o < 4; ++o) w4[o] = o < no ? wo[tid * no + o] : 0.0f;
        if constexpr (Ac) w4[4] = head ? g.wv[tid] : 0.0f;
#pragma unroll
        for (int o = 0; o < ND; ++o) gw[o] = 0.0f;
#pragma unroll 4
        for (int q = 0; q < kTile / 4; ++q) {
          const f32x4 hv = *reinterpret_cast<const f32x4*>(yrow + 4 * q);
          f32x4 dv[ND], nv;
#pragma unroll
          for (int o = 0; o < ND; ++o) dv[o] = *reinterpret_cast<const f32x4*>(dlt + o * kTile + 4 * q);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float s = 0.0f;
#pragma unroll
            for (int o = 0; o < ND; ++o) {
              gw[o] = __builtin_fmaf(dv[o][c], hv[c], gw[o]);
              s = __builtin_fmaf(w4[o], dv[o][c], s);
            }
            nv[c] = s * grad_actd(act, hv[c]);
          }
          *reinterpret_cast<f32x4*>(yrow + 4 * q) = nv;
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
          if (o < no) grad_put(part + net.off[nh] + tid * no + o, gw[o], first);
        if constexpr (Ac)
          if (head) grad_put(pv + tid, gw[4], first);
      }
      if (tid >= kGradBlock - ND) {
        const int o = tid - (kGradBlock - ND);
        if (o < no || (Ac && o == 4 && head)) {
          float s = 0.0f;
          for (int c = 0; c < kTile; ++c) s += dlt[o * kTile + c];
          grad_put(o < 4 ? part + net.off[nh] + lw * no + o : pv + lw, s, first);
        }
      }
      __syncthreads();
      // the hidden layers, from the last down: dW_l and db_l from delta_l (in Hl(l)) and the layer's input, then delta_{l-1} over the input
#pragma unroll 1
      for (int l = nh - 1; l >= 0; --l) {
        const int width = net.width[l], in = l ? net.width[l - 1] : D;
        float* A = l ? Hl(l - 1) : X;
        const float* dl = Hl(l);
        float* pw = part + net.off[l];
#pragma unroll 1
        for (int uc = wave; uc < width / 16; uc += kGradWaves) grad_dw(dl + uc * 16 * kGradStride, A, in, uc, lane, pw, first);
        if (tid < width) grad_put(pw + width * in + tid, grad_row_sum(dl + tid * kGradStride), first);
        __syncthreads();                                          // dW_l has consumed the layer's input
        if (l > 0) {
          grad_wt_delta(net.w + net.off[l], dl, A, in, width, act, wave, lane);
          __syncthreads();
        }
      }
    } else {
      __syncthreads();                                            // the rows are read before the next tile is staged
    }
  }

  if constexpr (!Fwd) {
    if (tid < NS) {                                               // the 64 lanes in ascending order
      double s = 0.0;
      for (int e = 0; e < kTile; ++e) s += red[tid * kTile + e];
      g.spart[(int64_t)blockIdx.x * NS + tid] = s;
    }
  }
}

// The one reduce of both gradient units (GradReduce, gaq_grad.hpp): every word of the partials and every statistic is summed over the
// G workgroups in ascending order in fp64 and rounded once; the host's routing table says where a statistic lands.  The narrow forms
// pass ent = 0.0, which leaves their log_std words the bits of (float)s: s starts at +0.0, a sum that starts at +0.0 is never -0.0
// under round-to-nearest, and s + 0.0 is s for every other value.
__global__ __launch_bounds__(256) void grad_reduce_kernel(GradReduce r) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < r.nw + r.nv) {
    double s = 0.0;
    for (int gi = 0; gi < r.G; ++gi) s += (double)r.part[(int64_t)gi * r.pstride + j];
    if (j < r.nw) r.grad_out[j] = (float)s;
    else r.value_out[j - r.nw] = (float)s;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < r.ns && (r.stats_out || r.log_std_out)) {
    const int k = (int)threadIdx.x;
    double s = 0.0;
    for (int gi = 0; gi < r.G; ++gi) s += r.spart[(int64_t)gi * r.ns + k];
    if (r.stats_out && r.slot[k] >= 0) r.stats_out[r.slot[k]] = s;
    if (r.stats_out && k == 0) r.stats_out[r.rows_slot] = (double)r.rows;
    if (r.log_std_out && k >= 3 && k < 7) r.log_std_out[k - 3] = (float)(s + r.ent);
  }
}

size_t grad_lds(const PolicyDev& net, bool ac) {
  int rows = (net.in_dim + 15) & ~15;
  for (int l = 0; l < net.n_hidden; ++l) rows += net.width[l];
  return (size_t)grad_head_bytes(ac) + (size_t)rows * kGradStride * 4;
}

struct GradCall {
  const char* who;
  int mode;
  int64_t rows;
  const int32_t* idx;             // the idx forms: [rows] (the inputs are then [src_rows, ...])
  int64_t src_rows;
  const float *obs, *a, *logp_old, *adv;
  float clip, scale;
  float *logp_out, *mean_out, *grad_out, *log_std_out;
  double* stats_out;
  int n_stat;
  // the actor-critic forms
  const float *ret, *v_old;
  float vclip, vf_coef, ent_coef;
  float *value_out, *grad_value_out;
  bool wide;                      // the wide forms (gaq.h "the wide learner"): grad_wide_kernel, the value head optional
};

// the launches of a checked call
int grad_run(const GradNet& v, const GradCall& c, hipStream_t st) {
  PolicyNet& net = *v.net;
  const bool ac = grad_is_ac(c.mode);                             // the kernel's layout: 5 rows of dlt, V's parts, 10 statistics
  const bool head = ac && (!c.wide || v.wv);                      // a wide form runs that layout without a value head too
  const bool idx = grad_is_idx(c.mode);
  const size_t lds = grad_lds(net.pd, ac) + (idx ? kGradIdxBytes : 0);
  if (lds > kGradLdsMax) return fail(GAQ_ERR_INVALID, std::string(c.who) + ": in_dim too large for the gradient kernel's LDS");
  HIP_TRY(hipSetDevice(net.device));
  const bool backward = !grad_is_forward(c.mode);
  const int64_t nv = net.pd.width[net.pd.n_hidden - 1] + 1;      // the value head's words
  if (c.rows == 0) {                                              // zeros to every output, no tile work
    if (c.grad_out) HIP_TRY(hipMemsetAsync(c.grad_out, 0, sizeof(float) * (size_t)net.nw, st));
    if (c.grad_value_out) HIP_TRY(hipMemsetAsync(c.grad_value_out, 0, sizeof(float) * (size_t)nv, st));
    if (c.log_std_out) HIP_TRY(hipMemsetAsync(c.log_std_out, 0, sizeof(float) * 4, st));
    if (c.stats_out) HIP_TRY(hipMemsetAsync(c.stats_out, 0, sizeof(double) * (size_t)(c.n_stat + (idx ? 2 : 1)), st));
    return GAQ_OK;
  }
  const int64_t ntiles = (c.rows + kTile - 1) / kTile;
  if (ntiles > ((int64_t)1 << 31) - 1) return fail(GAQ_ERR_INVALID, std::string(c.who) + ": too many rows for one launch");
  const int G = backward ? grad_groups(ntiles) : (int)std::min<int64_t>(ntiles, (int64_t)1 << 20);
  GradArgs g{};
  g.net = net.pd; g.n_out = net.n_out; g.nm = policy_norm_dev(net.norm);
  g.rows = c.rows; g.ntiles = ntiles; g.obs = c.obs; g.a = c.a; g.logp_old = c.logp_old; g.adv = c.adv; g.clip = c.clip; g.scale = c.scale;
  grad_fill_std(v, g.log_std, g.inv_std);
  g.logp_out = c.logp_out; g.mean_out = c.mean_out;
  g.wv = v.wv; g.ret = c.ret; g.v_old = c.v_old; g.vclip = c.vclip; g.vf_coef = c.vf_coef; g.value_out = c.value_out;
  g.idx = c.idx; g.src_rows = c.src_rows; g.explore_tab = v.tab;
  g.pstride = (net.nw + (head ? nv : 0) + 15) & ~(int64_t)15;
  if (backward) {
    float* tape = nullptr;                                        // (none: the sequence unit's)
    if (int rc = grad_scratch(net, G, 0, g.spart, g.part, tape)) return rc;
  }
  int rc = GAQ_OK;
  if (c.wide) switch (c.mode) {
    case GRAD_EVAL_AC: rc = grad_launch(grad_wide_kernel<GRAD_EVAL_AC>, g, G, lds, st); break;
    case GRAD_PPO_AC: rc = grad_launch(grad_wide_kernel<GRAD_PPO_AC>, g, G, lds, st); break;
    case GRAD_PPO_AC_IDX: rc = grad_launch(grad_wide_kernel<GRAD_PPO_AC_IDX>, g, G, lds, st); break;
    case GRAD_MSE_IDX: rc = grad_launch(grad_wide_kernel<GRAD_MSE_IDX>, g, G, lds, st); break;
    default: rc = grad_launch(grad_wide_kernel<GRAD_MSE>, g, G, lds, st); break;
  }
  else switch (c.mode) {
    case GRAD_LOGP: rc = grad_launch(grad_kernel<GRAD_LOGP>, g, G, lds, st); break;
    case GRAD_BACKWARD: rc = grad_launch(grad_kernel<GRAD_BACKWARD>, g, G, lds, st); break;
    case GRAD_PPO: rc = grad_launch(grad_kernel<GRAD_PPO>, g, G, lds, st); break;
    case GRAD_EVAL_AC: rc = grad_launch(grad_kernel<GRAD_EVAL_AC>, g, G, lds, st); break;
    case GRAD_PPO_AC: rc = grad_launch(grad_kernel<GRAD_PPO_AC>, g, G, lds, st); break;
    case GRAD_PPO_IDX: rc = grad_launch(grad_kernel<GRAD_PPO_IDX>, g, G, lds, st); break;
    case GRAD_MSE_IDX: rc = grad_launch(grad_kernel<GRAD_MSE_IDX>, g, G, lds, st); break;
    case GRAD_PPO_AC_IDX: rc = grad_launch(grad_kernel<GRAD_PPO_AC_IDX>, g, G, lds, st); break;
    default: rc = grad_launch(grad_kernel<GRAD_MSE>, g, G, lds, st); break;
  }
  if (rc || !backward) return rc;
  GradReduce r{};
  r.part = g.part; r.spart = g.spart; r.G = G; r.pstride = g.pstride; r.nw = net.nw; r.nv = head ? nv : 0; r.rows = c.rows;
  r.ent = ac ? -(double)c.ent_coef * (double)c.scale * (double)c.rows : 0.0;
  r.grad_out = c.grad_out; r.value_out = c.grad_value_out; r.stats_out = c.stats_out; r.log_std_out = c.log_std_out;
  grad_route(r, ac, c.n_stat, idx);
  return grad_reduce(r, st);
}

// What the five entry points do with a handle's view: the checks of rows and scale, the null pointers, the mode's own arguments, the
// alignment, the overlaps -- in that order -- then grad_run.  `in` and `out` state every pointer of the call once.
int grad_checked_run(const GradNet& v, const GradCall& c, const std::vector<Span>& in, const std::vector<Span>& out, void* stream) {
  const std::string who = std::string(c.who) + ": ";
  if (c.rows < 0) return fail(GAQ_ERR_INVALID, who + "rows must not be negative");
  if (c.scale != c.scale) return fail(GAQ_ERR_INVALID, who + "scale is NaN");
  if (grad_is_idx(c.mode)) {
    if (c.rows > 0 && c.src_rows < 1) return fail(GAQ_ERR_INVALID, who + "src_rows must be at least 1");
    if (c.src_rows > ((int64_t)1 << 31) - 1) return fail(GAQ_ERR_INVALID, who + "src_rows must not exceed 2^31 - 1");
  }
  bool wide = false, misaligned = false;
  if (int rc = check_span_nulls(in, out, c.rows > 0, wide, misaligned)) return rc;
  const bool ppo = grad_base(c.mode) == GRAD_PPO || grad_base(c.mode) == GRAD_PPO_AC;
  if (c.wide && grad_is_ac(c.mode)) {                             // a wide form's value head is optional, and its arguments go with it
    if (!v.wv && (c.ret || c.v_old || c.value_out || c.grad_value_out))
      return fail(GAQ_ERR_INVALID, who + "the policy has no value head: " + (ppo ? "ret, v_old and grad_value_out" : "value_out") + " must be NULL");
    if (v.wv && ppo && !c.ret && c.rows > 0) return fail(GAQ_ERR_INVALID, who + "the policy has a value head: its loss needs ret");
  }
  // (GRAD_PPO leaves vclip and the coefficients 0: only its clip can be refused)
  if (ppo)
    if (int rc = check_ppo_hyper(who, c.clip, c.vclip, c.vf_coef, c.ent_coef, grad_base(c.mode) == GRAD_PPO_AC && (!c.wide || v.wv), c.v_old,
                                 c.rows > 0))
      return rc;
  if (grad_is_ac(c.mode) && !c.wide && !v.wv)
    return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head): the actor-critic passes need V on the policy's trunk");
  if ((ppo || grad_is_forward(c.mode)) && !v.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no log-probability");
  if (misaligned) return fail(GAQ_ERR_INVALID, who + "pointers must be 4-byte aligned" + (wide ? " (stats_out: 8)" : ""));
  if (int rc = check_overlap(c.who, in, out)) return rc;
  return grad_run(v, c, (hipStream_t)stream);
}

// The three loss gradients, each the body of its contiguous entry point (idx = nullptr, src_rows = rows) and of its idx form: the
// inputs span src_rows rows, idx spans `rows` words, and an idx form's stats_out is one double longer.
size_t grad_src(int mode, int64_t src_rows) { return grad_is_idx(mode) && src_rows < 0 ? 0 : (size_t)src_rows; }

int grad_ppo_ac_call(const char* who, int mode, gaq_policy* p, int64_t rows, const int32_t* idx, int64_t src_rows, const float* obs,
                     const float* actions, const float* logp_old, const float* adv, const float* ret, const float* v_old, float clip_eps,
                     float vclip, float vf_coef, float ent_coef, float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out,
                     double* stats_out, void* stream) {
  GradNet v;
  if (int rc = policy_grad_view(p, v)) return rc;
  GradCall c{};
  c.who = who; c.mode = mode; c.rows = rows; c.idx = idx; c.src_rows = src_rows; c.obs = obs; c.a = actions; c.logp_old = logp_old; c.adv = adv;
  c.ret = ret; c.v_old = v_old; c.clip = clip_eps; c.vclip = vclip; c.vf_coef = vf_coef; c.ent_coef = ent_coef; c.scale = scale;
  c.grad_out = grad_out; c.grad_value_out = grad_value_out; c.log_std_out = grad_log_std_out; c.stats_out = stats_out; c.n_stat = 5;
  const size_t r = grad_src(mode, src_rows), nv = (size_t)v.net->pd.width[v.net->pd.n_hidden - 1] + 1;
  std::vector<Span> in = {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {actions, r * 16, SPAN_ROWS}, {logp_old, r * 4, SPAN_ROWS},
                          {adv, r * 4, SPAN_ROWS}, {ret, r * 4, SPAN_ROWS}, {v_old, r * 4, SPAN_OPTIONAL}};
  if (grad_is_idx(mode)) in.push_back({idx, (size_t)(rows > 0 ? rows : 0) * 4, SPAN_ROWS});
  return grad_checked_run(v, c, in,
                          {{grad_out, (size_t)v.net->nw * 4, SPAN_ALWAYS}, {grad_value_out, nv * 4, SPAN_ALWAYS},
                           {grad_log_std_out, 16, SPAN_ALWAYS}, {stats_out, grad_is_idx(mode) ? 56u : 48u, SPAN_ALWAYS, 8}},
                          stream);
}

int grad_ppo_call(const char* who, int mode, gaq_policy* p, int64_t rows, const int32_t* idx, int64_t src_rows, const float* obs,
                  const float* actions, const float* logp_old, const float* adv, float clip_eps, float scale, float* grad_out,
                  float* grad_log_std_out, double* stats_out, void* stream) {
  GradNet v;
  if (int rc = policy_grad_view(p, v)) return rc;
  GradCall c{};
  c.who = who; c.mode = mode; c.rows = rows; c.idx = idx; c.src_rows = src_rows; c.obs = obs; c.a = actions; c.logp_old = logp_old; c.adv = adv;
  c.clip = clip_eps; c.scale = scale; c.grad_out = grad_out; c.log_std_out = grad_log_std_out; c.stats_out = stats_out; c.n_stat = 3;
  const size_t r = grad_src(mode, src_rows);
  std::vector<Span> in = {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {actions, r * 16, SPAN_ROWS}, {logp_old, r * 4, SPAN_ROWS},
                          {adv, r * 4, SPAN_ROWS}};
  if (grad_is_idx(mode)) in.push_back({idx, (size_t)(rows > 0 ? rows : 0) * 4, SPAN_ROWS});
  return grad_checked_run(v, c, in,
                          {{grad_out, (size_t)v.net->nw * 4, SPAN_ALWAYS}, {grad_log_std_out, 16, SPAN_ALWAYS},
                           {stats_out, grad_is_idx(mode) ? 40u : 32u, SPAN_ALWAYS, 8}},
                          stream);
}

int grad_mse_call(const char* who, int mode, gaq_critic* cr, int64_t rows, const int32_t* idx, int64_t src_rows, const float* obs,
                  const float* target, float scale, float* grad_out, double* stats_out, void* stream) {
  GradNet v;
  if (int rc = critic_grad_view(cr, v)) return rc;
  GradCall c{};
  c.who = who; c.mode = mode; c.rows = rows; c.idx = idx; c.src_rows = src_rows; c.obs = obs; c.a = target; c.scale = scale;
  c.grad_out = grad_out; c.stats_out = stats_out; c.n_stat = 1;
  const size_t r = grad_src(mode, src_rows);
  std::vector<Span> in = {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {target, r * 4, SPAN_ROWS}};
  if (grad_is_idx(mode)) in.push_back({idx, (size_t)(rows > 0 ? rows : 0) * 4, SPAN_ROWS});
  return grad_checked_run(v, c, in, {{grad_out, (size_t)v.net->nw * 4, SPAN_ALWAYS}, {stats_out, grad_is_idx(mode) ? 24u : 16u, SPAN_ALWAYS, 8}},
                          stream);
}

}  // namespace

// gaq_grad.hpp: the reduce, for this unit and for gaq_policy_grad_seq.hip
int grad_reduce(const GradReduce& r, hipStream_t st) {
  hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)((r.nw + r.nv + 255) / 256)), dim3(256), 0, st, r);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

// ---- the encoder in front of a recurrent cell: its backward over stored rows (gaq_grad.hpp GradFeatCall) -----------------------------
// A trunk without an output layer whose last layer's gradient is GIVEN: dfeat [., E], which the sequence kernel wrote (dfeat_t = W_ih^T
// planes).  A kernel of its own, built from grad_kernel's pieces, and not two more Modes of grad_kernel: that kernel has a head, a row
// stage and statistics in every Mode, and its nine instantiations keep their instructions only while its text stays what it is
// (DESIGN.md 4a).  Per 64-row tile: the observation is staged as grad_kernel stages it (through the normaliser), the hidden layers are
// recomputed with grad_fwd_layer into rows of their own, the tile's dfeat rows are staged into the last layer's rows times act'(h), then
// grad_kernel's hidden-layer loop runs: dW_l (grad_dw), db_l (grad_row_sum), delta_{l-1} = (W_l^T delta_l) act'(h_{l-1}).  Partials and
// their ownership as in grad_kernel; no statistics, no atomics.  Idx: row j of the call is row rowidx[j] of obs and dfeat, a negative
// entry a dead lane from which no address is formed.  LDS = 272 B x (in_dim rounded up to 16 + the widths) (+ 256 B).
namespace {

struct GradFeatArgs {
  PolicyDev net;                  // the encoder: w, in_dim, n_hidden (1 or 2), hidden_act, width, off
  PolObsNorm nm;
  int64_t rows, ntiles;
  const float* obs;               // [., D]
  const float* dfeat;             // [., E]
  const int32_t* rowidx;          // Idx: [rows]
  float* part;                    // [G][pstride]
  int64_t pstride;
};

template <bool Idx>
__global__ __launch_bounds__(kGradBlock) void grad_feat_kernel(GradFeatArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  [[maybe_unused]] int* sidx = reinterpret_cast<int*>(smem);      // Idx: [64] the tile's source rows (or < 0)
  float* X = reinterpret_cast<float*>(smem + (Idx ? kGradIdxBytes : 0));
  const PolicyDev& net = g.net;
  const int D = net.in_dim, kin = (D + 3) & ~3, kx = (D + 15) & ~15, nh = net.n_hidden, act = net.hidden_act;
  const uint32_t lane = threadIdx.x & 63u;
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w0 = net.width[0];
  auto Hl = [&](int l) { return X + (kx + (l > 0 ? w0 : 0)) * kGradStride; };
  const int G = (int)gridDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * g.ntiles / G, t1 = ((int64_t)blockIdx.x + 1) * g.ntiles / G;
  float* part = g.part + (int64_t)blockIdx.x * g.pstride;
  const int E = net.width[nh - 1];

#pragma unroll 1
  for (int64_t tile = t0; tile < t1; ++tile) {
    const bool first = tile == t0;
    const int64_t row0 = tile * kTile;
    const int nlive = (int)((g.rows - row0) < kTile ? (g.rows - row0) : kTile);
    if constexpr (Idx) {
      if (tid < kTile) sidx[tid] = tid < nlive ? g.rowidx[row0 + tid] : kGradIdxDead;
      __syncthreads();
    }
    auto src_of = [&](int e, int64_t& src) -> bool {
      if constexpr (Idx) {
        src = sidx[e];
        return src >= 0;
      } else {
        src = row0 + e;
        return e < nlive;
      }
    };
    for (int f = tid; f < kTile * kx; f += kGradBlock) {
      const int e = f / kx, k = f - e * kx;
      float v = k >= kin ? 0.0f : -0.0f;
      if (k < D) {
        v = 0.0f;
        int64_t src;
        if (src_of(e, src)) {
          v = g.obs[src * D + k];
          if (g.nm.tab) v = g.nm(v, k);
        }
      }
      X[k * kGradStride + grad_col(e)] = v;
    }
    __syncthreads();
    {
      const float* A = X;
      int in = D;
#pragma unroll 1
      for (int l = 0; l < nh; ++l) {
        const int width = net.width[l];
        const int nc = (width / 16 - wave + 3) / 4;
        if (nc == 1) grad_fwd_layer<1>(net.w + net.off[l], in, width, act, wave, A, Hl(l), lane);
        else if (nc == 2) grad_fwd_layer<2>(net.w + net.off[l], in, width, act, wave, A, Hl(l), lane);
        __syncthreads();
        A = Hl(l);
        in = width;
      }
    }
    // delta of the last layer: the given dfeat times act'(h), dead rows exactly 0
    {
      float* Y = Hl(nh - 1);
      for (int f = tid; f < kTile * E; f += kGradBlock) {
        const int e = f / E, k = f - e * E;
        float* pos = Y + k * kGradStride + grad_col(e);
        int64_t src;
        *pos = src_of(e, src) ? g.dfeat[src * E + k] * grad_actd(act, *pos) : 0.0f;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int l = nh - 1; l >= 0; --l) {
      const int width = net.width[l], in = l ? net.width[l - 1] : D;
      float* A = l ? Hl(l - 1) : X;
      const float* dl = Hl(l);
      const float* wl = net.w + net.off[l];
      float* pw = part + net.off[l];
#pragma unroll 1
      for (int uc = wave; uc < width / 16; uc += kGradWaves) grad_dw(dl + uc * 16 * kGradStride, A, in, uc, lane, pw, first);
      if (tid < width) grad_put(pw + width * in + tid, grad_row_sum(dl + tid * kGradStride), first);
      __syncthreads();                                            // dW_l has consumed the layer's input
      if (l > 0) {
        const int n = (int)(lane & 15), kk = (int)(lane >> 4);
#pragma unroll 1
        for (int kc = wave; kc < in / 16; kc += kGradWaves) {
          f32x4 acc[4];
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) acc[eb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          for (int uch = 0; uch < width / 16; ++uch) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + ((int64_t)uch * in + kc * 16 + n) * 16 + 4 * kk);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(dl + (uch * 16 + 4 * kk + i) * kGradStride + n * 4);
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            f32x4* pos = reinterpret_cast<f32x4*>(A + (kc * 16 + 4 * kk + r) * kGradStride + n * 4);
            const f32x4 hv = *pos;
            const f32x4 nv = {acc[0][r] * grad_actd(act, hv[0]), acc[1][r] * grad_actd(act, hv[1]), acc[2][r] * grad_actd(act, hv[2]),
                              acc[3][r] * grad_actd(act, hv[3])};
            *pos = nv;
          }
        }
        __syncthreads();
      }
    }
    // (the last barrier above -- dW_0's, or the delta's -- stands between this tile's readers of X and the next tile's staging)
  }
}

// rowidx[t S + j] = t S_src + idx[j], or kGradIdxSkipped for an index outside [0, S_src); list[t S + j] the same row for the encoder's
// gathered forward, which has no dead slots: a skipped entry names column 0 of its step (a valid row, encoded once more to the same
// bits), so no address is formed from the index.  *count = T S.
__global__ __launch_bounds__(256) void grad_rowidx_kernel(int32_t T, int64_t S, const int32_t* idx, int64_t S_src, int32_t* rowidx,
                                                          uint32_t* list, uint32_t* count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *count = (uint32_t)((int64_t)T * S);
  if (i >= (int64_t)T * S) return;
  const int64_t t = i / S, j = i - t * S;
  const int64_t v = idx[j];
  const bool ok = v >= 0 && v < S_src;
  rowidx[i] = ok ? (int32_t)(t * S_src + v) : kGradIdxSkipped;
  list[i] = (uint32_t)(t * S_src + (ok ? v : 0));
}

}  // namespace

size_t grad_feat_lds(const PolicyDev& trunk, bool idx) {
  int rows = (trunk.in_dim + 15) & ~15;
  for (int l = 0; l < trunk.n_hidden; ++l) rows += trunk.width[l];
  return (size_t)rows * kGradStride * 4 + (idx ? kGradIdxBytes : 0);
}

int grad_feat_run(const GradFeatCall& c, hipStream_t st) {
  GradFeatArgs g{};
  g.net = c.trunk; g.nm = PolObsNorm{c.nm_tab, c.nm_dim}; g.rows = c.rows; g.ntiles = (c.rows + kTile - 1) / kTile;
  g.obs = c.obs; g.dfeat = c.dfeat; g.rowidx = c.rowidx; g.part = c.part; g.pstride = c.pstride;
  const size_t lds = grad_feat_lds(c.trunk, c.rowidx != nullptr);
  return c.rowidx ? grad_launch(grad_feat_kernel<true>, g, c.G, lds, st) : grad_launch(grad_feat_kernel<false>, g, c.G, lds, st);
}

int grad_rowidx_run(int32_t T, int64_t S, const int32_t* idx, int64_t S_src, int32_t* rowidx, uint32_t* list, uint32_t* count, hipStream_t st) {
  const int64_t n = (int64_t)T * S;
  hipLaunchKernelGGL(grad_rowidx_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T, S, idx, S_src, rowidx, list, count);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

extern "C" {

int gaq_policy_eval_wide_dev(gaq_policy* p, int64_t rows, const float* obs, const float* actions, float* logp_out, float* value_out,
                             float* mean_out, void* stream) {
  GradNet v;
  if (int rc = policy_grad_wide_view(p, v)) return rc;
  GradCall c{};
  c.who = "gaq_policy_eval_wide_dev"; c.mode = GRAD_EVAL_AC; c.wide = true; c.rows = rows; c.obs = obs; c.a = actions; c.logp_out = logp_out;
  c.value_out = value_out; c.mean_out = mean_out;
  const size_t r = (size_t)rows;
  return grad_checked_run(v, c, {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {actions, r * 16, SPAN_ROWS}},
                          {{logp_out, r * 4, SPAN_ROWS}, {value_out, r * 4, v.wv ? SPAN_ROWS : SPAN_OPTIONAL}, {mean_out, r * 16, SPAN_OPTIONAL}},
                          stream);
}

int gaq_policy_grad_ppo_wide_dev(gaq_policy* p, int64_t rows, const int32_t* idx, int64_t src_rows, const float* obs, const float* actions,
                                 const float* logp_old, const float* adv, const float* ret, const float* v_old, float clip_eps, float vclip,
                                 float vf_coef, float ent_coef, float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out,
                                 double* stats_out, void* stream) {
  GradNet v;
  if (int rc = policy_grad_wide_view(p, v)) return rc;
  const int mode = idx ? GRAD_PPO_AC_IDX : GRAD_PPO_AC;
  if (!idx) src_rows = rows;
  GradCall c{};
  c.who = "gaq_policy_grad_ppo_wide_dev"; c.mode = mode; c.wide = true; c.rows = rows; c.idx = idx; c.src_rows = src_rows; c.obs = obs;
  c.a = actions; c.logp_old = logp_old; c.adv = adv; c.ret = ret; c.v_old = v_old; c.clip = clip_eps; c.vclip = vclip; c.vf_coef = vf_coef;
  c.ent_coef = ent_coef; c.scale = scale; c.grad_out = grad_out; c.grad_value_out = grad_value_out; c.log_std_out = grad_log_std_out;
  c.stats_out = stats_out; c.n_stat = 5;
  const size_t r = grad_src(mode, src_rows), nv = (size_t)v.net->pd.width[v.net->pd.n_hidden - 1] + 1;
  // (ret is refused by grad_checked_run with a text of its own, with a head and without)
  std::vector<Span> in = {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {actions, r * 16, SPAN_ROWS}, {logp_old, r * 4, SPAN_ROWS},
                          {adv, r * 4, SPAN_ROWS}, {ret, r * 4, SPAN_OPTIONAL}, {v_old, r * 4, SPAN_OPTIONAL}};
  if (idx) in.push_back({idx, (size_t)(rows > 0 ? rows : 0) * 4, SPAN_ROWS});
  return grad_checked_run(v, c, in,
                          {{grad_out, (size_t)v.net->nw * 4, SPAN_ALWAYS}, {grad_value_out, nv * 4, v.wv ? SPAN_ALWAYS : SPAN_OPTIONAL},
                           {grad_log_std_out, 16, SPAN_ALWAYS}, {stats_out, idx ? 56u : 48u, SPAN_ALWAYS, 8}},
                          stream);
}

int gaq_critic_grad_mse_wide_dev(gaq_critic* cr, int64_t rows, const int32_t* idx, int64_t src_rows, const float* obs, const float* target,
                                 float scale, float* grad_out, double* stats_out, void* stream) {
  GradNet v;
  if (int rc = critic_grad_wide_view(cr, v)) return rc;
  const int mode = idx ? GRAD_MSE_IDX : GRAD_MSE;
  if (!idx) src_rows = rows;
  GradCall c{};
  c.who = "gaq_critic_grad_mse_wide_dev"; c.mode = mode; c.wide = true; c.rows = rows; c.idx = idx; c.src_rows = src_rows; c.obs = obs;
  c.a = target; c.scale = scale; c.grad_out = grad_out; c.stats_out = stats_out; c.n_stat = 1;
  const size_t r = grad_src(mode, src_rows);
  std::vector<Span> in = {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {target, r * 4, SPAN_ROWS}};
  if (idx) in.push_back({idx, (size_t)(rows > 0 ? rows : 0) * 4, SPAN_ROWS});
  return grad_checked_run(v, c, in, {{grad_out, (size_t)v.net->nw * 4, SPAN_ALWAYS}, {stats_out, idx ? 24u : 16u, SPAN_ALWAYS, 8}}, stream);
}

int gaq_policy_eval_ac_dev(gaq_policy* p, int64_t rows, const float* obs, const float* actions, float* logp_out, float* value_out,
                           float* mean_out, void* stream) {
  GradNet v;
  if (int rc = policy_grad_view(p, v)) return rc;
  GradCall c{};
  c.who = "gaq_policy_eval_ac_dev"; c.mode = GRAD_EVAL_AC; c.rows = rows; c.obs = obs; c.a = actions; c.logp_out = logp_out;
  c.value_out = value_out; c.mean_out = mean_out;
  const size_t r = (size_t)rows;
  return grad_checked_run(v, c, {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {actions, r * 16, SPAN_ROWS}},
                          {{logp_out, r * 4, SPAN_ROWS}, {value_out, r * 4, SPAN_ROWS}, {mean_out, r * 16, SPAN_OPTIONAL}}, stream);
}

int gaq_policy_grad_ppo_ac_dev(gaq_policy* p, int64_t rows, const float* obs, const float* actions, const float* logp_old, const float* adv,
                               const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                               float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  return grad_ppo_ac_call("gaq_policy_grad_ppo_ac_dev", GRAD_PPO_AC, p, rows, nullptr, rows, obs, actions, logp_old, adv, ret, v_old, clip_eps,
                          vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

int gaq_policy_grad_ppo_ac_idx_dev(gaq_policy* p, int64_t rows, const int32_t* idx, int64_t src_rows, const float* obs, const float* actions,
                                   const float* logp_old, const float* adv, const float* ret, const float* v_old, float clip_eps, float vclip,
                                   float vf_coef, float ent_coef, float scale, float* grad_out, float* grad_value_out,
                                   float* grad_log_std_out, double* stats_out, void* stream) {
  return grad_ppo_ac_call("gaq_policy_grad_ppo_ac_idx_dev", GRAD_PPO_AC_IDX, p, rows, idx, src_rows, obs, actions, logp_old, adv, ret, v_old,
                          clip_eps, vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

int gaq_policy_logp_dev(gaq_policy* p, int64_t rows, const float* obs, const float* actions, float* logp_out, float* mean_out,
                        void* stream) {
  GradNet v;
  if (int rc = policy_grad_view(p, v)) return rc;
  GradCall c{};
  c.who = "gaq_policy_logp_dev"; c.mode = GRAD_LOGP; c.rows = rows; c.obs = obs; c.a = actions; c.logp_out = logp_out; c.mean_out = mean_out;
  const size_t r = (size_t)rows;
  return grad_checked_run(v, c, {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {actions, r * 16, SPAN_ROWS}},
                          {{logp_out, r * 4, SPAN_ROWS}, {mean_out, r * 16, SPAN_OPTIONAL}}, stream);
}

int gaq_policy_backward_dev(gaq_policy* p, int64_t rows, const float* obs, const float* dout, float scale, float* grad_out, void* stream) {
  GradNet v;
  if (int rc = policy_grad_view(p, v)) return rc;
  GradCall c{};
  c.who = "gaq_policy_backward_dev"; c.mode = GRAD_BACKWARD; c.rows = rows; c.obs = obs; c.a = dout; c.scale = scale; c.grad_out = grad_out;
  const size_t r = (size_t)rows;
  return grad_checked_run(v, c, {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {dout, r * 16, SPAN_ROWS}},
                          {{grad_out, (size_t)v.net->nw * 4, SPAN_ALWAYS}}, stream);
}

int gaq_policy_grad_ppo_dev(gaq_policy* p, int64_t rows, const float* obs, const float* actions, const float* logp_old, const float* adv,
                            float clip_eps, float scale, float* grad_out, float* grad_log_std_out, double* stats_out, void* stream) {
  return grad_ppo_call("gaq_policy_grad_ppo_dev", GRAD_PPO, p, rows, nullptr, rows, obs, actions, logp_old, adv, clip_eps, scale, grad_out,
                       grad_log_std_out, stats_out, stream);
}

int gaq_policy_grad_ppo_idx_dev(gaq_policy* p, int64_t rows, const int32_t* idx, int64_t src_rows, const float* obs, const float* actions,
                                const float* logp_old, const float* adv, float clip_eps, float scale, float* grad_out,
                                float* grad_log_std_out, double* stats_out, void* stream) {
  return grad_ppo_call("gaq_policy_grad_ppo_idx_dev", GRAD_PPO_IDX, p, rows, idx, src_rows, obs, actions, logp_old, adv, clip_eps, scale,
                       grad_out, grad_log_std_out, stats_out, stream);
}

int gaq_critic_backward_dev(gaq_critic* cr, int64_t rows, const float* obs, const float* dout, float scale, float* grad_out, void* stream) {
  GradNet v;
  if (int rc = critic_grad_view(cr, v)) return rc;
  GradCall c{};
  c.who = "gaq_critic_backward_dev"; c.mode = GRAD_BACKWARD; c.rows = rows; c.obs = obs; c.a = dout; c.scale = scale; c.grad_out = grad_out;
  const size_t r = (size_t)rows;
  return grad_checked_run(v, c, {{obs, r * v.net->pd.in_dim * 4, SPAN_ROWS}, {dout, r * 4, SPAN_ROWS}},
                          {{grad_out, (size_t)v.net->nw * 4, SPAN_ALWAYS}}, stream);
}

int gaq_critic_grad_mse_dev(gaq_critic* cr, int64_t rows, const float* obs, const float* target, float scale, float* grad_out,
                            double* stats_out, void* stream) {
  return grad_mse_call("gaq_critic_grad_mse_dev", GRAD_MSE, cr, rows, nullptr, rows, obs, target, scale, grad_out, stats_out, stream);
}

int gaq_critic_grad_mse_idx_dev(gaq_critic* cr, int64_t rows, const int32_t* idx, int64_t src_rows, const float* obs, const float* target,
                                float scale, float* grad_out, double* stats_out, void* stream) {
  return grad_mse_call("gaq_critic_grad_mse_idx_dev", GRAD_MSE_IDX, cr, rows, idx, src_rows, obs, target, scale, grad_out, stats_out, stream);
}

}  // extern "C"
