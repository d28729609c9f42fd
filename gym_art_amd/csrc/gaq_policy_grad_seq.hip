// gaq_policy_grad_seq.hip -- the learner's passes over stored SEQUENCES for a recurrent policy (include/gaq.h "gradients of a recurrent
// policy" and "gradients of an LSTM policy"), once for both cells:
//   GRU   gaq_policy_eval_seq_dev       gaq_policy_grad_ppo_seq_dev       gaq_policy_grad_ppo_seq_idx_dev
//   LSTM  gaq_policy_eval_lstm_seq_dev  gaq_policy_grad_ppo_lstm_seq_dev  gaq_policy_grad_ppo_lstm_seq_idx_dev
// the forward pass (log-probabilities, V, means and the final state of T steps of S sequences, the rollout's bits), the truncated-BPTT
// gradient of gaq_policy_grad_ppo_ac_dev's loss, and that gradient over the columns an index vector names -- and, for a policy with an
// ENCODER in front of its cell (gaq.h "sequences through an encoder"), the same three under names that take both cells:
//   gaq_policy_eval_enc_seq_dev  gaq_policy_grad_ppo_enc_seq_dev  gaq_policy_grad_ppo_enc_seq_idx_dev
// and, for a GRU of more than 64 and up to 128 units (gaq.h "the wide recurrent learner"), grad_seq_wide_kernel further down under
//   gaq_policy_eval_seq_wide_dev  gaq_policy_grad_ppo_seq_wide_dev  (idx or NULL)
// as split passes: gaq_policy.hip's encoder kernel over the stored rows (policy_encode_rows / _list), the kernels below on the features
// (the gradient: with Dx, which also writes dfeat_t = W_ih^T planes beside the dW stage), gaq_policy_grad.hip's grad_feat_kernel for
// the encoder's backward over the rows, and the one reduce twice.  Of gaq_policy.hip it uses the
// net record gaq_grad.hpp declares (policy_grad_seq_view) and what that header holds for both gradient units: the span checks, the split
// into workgroups, the scratch, the PPO refusals, the launch and the reduce.
//
// One kernel template, grad_seq_kernel<L, Bwd, Idx, Dx> (L: the LSTM), ten kernels: 4 waves per workgroup,
// one 64-sequence tile at a time; sequence e of the tile lives in column grad_col(e) = pol_col(e) of every LDS row (stride 68 floats, as
// in gaq_policy_grad.hip).  What the feed-forward gradient kernel and this one have in common -- the layout, the partial's words, dW,
// the row sum -- is gaq_grad_dev.hpp; the stages themselves are restated here, not shared: that kernel keeps its recorded resource
// lines.  The LDS head, the staging of observations and of [., H] rows and one head layer's forward are gaq_grad_seq_dev.hpp.
// The frame -- the LDS head, the column layout, the idx rules, the staging, the head's forward and backward, the row stage, dW, the
// W_hh^T product -- is written once; what is the cell's own (below: the lines GRU and LSTM) stands under `if constexpr (L)` ... else.
// Idx (with Bwd): sequence e of a tile is column sidx[e] = idx[row0 + e] of every input; only the addresses of the loads differ, and a
// column whose index is out of range is a dead lane.
//   forward   t ascending: the observation is staged as pol_stage_obs stages it; hin_t = h_{t-1} (an LSTM's cin_t = c_{t-1} too) with
//             the rows of done[t-1] (and dead lanes) 0 by select; then the cell, chunk by chunk, each gate sum an ascending k-ordered
//             MFMA chain over the x products then the h products, so h_t (and c_t) are the rollout's bits:
//               GRU   gru_cell's arithmetic: r and z start at b_i + b_h, n_x and n_h stay apart, n = tanhf(fmaf(r, n_h, n_x)),
//                     h' = fmaf(z, hin - n, n)
//               LSTM  lstm_cell's: i, f, g, o start at b_ih + b_hh, i, f, o sigmoids, g = tanhf, c' = fmaf(f, cin, i g), h' = o tanhf(c').
//                     At H <= 64 a wave owns one 16-unit chunk, and the lane that owns 4 units x 4 column blocks of it owns them at
//                     every t: c is carried in 16 registers and takes no LDS.
//             <Bwd = false> (eval) then runs the head and the row stage; <true> writes h_t to the workgroup's tape [T][64][H] (the LSTM:
//             [T][64][2][H], a sequence's h_t and c_t side by side).
//   backward  t descending (<true>): h_t and hin_t come back from the tape, the head is recomputed, the row stage forms the five deltas
//             of gaq_policy_grad_ppo_ac_dev's loss, the head is backpropagated with that kernel's code shape down to dh_t (no activation
//             derivative on the cell's output); the gates are recomputed with the forward's code and, in the accumulator registers,
//               GRU   da_n = dh (1 - z)(1 - n^2), da_z = dh (hin - n) z (1 - z), da_r = da_n n_h r (1 - r), dn_h = da_n r, direct = dh z
//                     go to four planes of LDS (over the rows the head used) and to the carried dh; dW_ih = [da_r; da_z; da_n] x^T and
//                     dW_hh = [da_r; da_z; dn_h] hin^T; dh_{t-1} = direct + W_hh^T [da_r; da_z; dn_h]
//               LSTM  cin_t is read from the tape by the owning lane (four 16-byte loads under the select that cuts the carried
//                     gradients; c0 at t = 0) and c_t recomputed from it; with tc = tanhf(c_t) and dh = dh_t + carried:
//                     da_o = dh tc o (1 - o), dc = dc_carried + dh o (1 - tc^2), da_i = dc g i (1 - i), da_f = dc cin f (1 - f),
//                     da_g = dc i (1 - g^2), dc_carried <- dc f; the four planes [da_i; da_f; da_g; da_o] are contiguous in the packed
//                     row order, so dW_ih = planes x^T, dW_hh = planes hin^T and dh_{t-1} = W_hh^T planes; b_ih and b_hh take the
//                     same sum.  The carried dc has H LDS rows of its own beside the carried dh's.
//             dW are MFMAs over the tile's 64 columns, the biases row sums in ascending column order, the packed W_hh is read 16 bytes
//             per lane; what is carried to t - 1 is 0 by select where done[t-1] and in dead columns.
// LDS = 8.25 KiB + 272 B x (kx + carried H + max(4 H, H + head widths)) for <true>, carried = 2 (hin, dh; the LSTM 3: dc) (+ 256 B for
// the idx form): 118.75 KiB at 18-GRU64-64-64, 135.75 KiB at 18-LSTM64-64-64; 8.25 KiB + 272 B x (kx + 2 H + head widths) for <false>.
// Partials: every word of the workgroup's partial is owned by one lane for every (tile, t); the first (tile, t) stores, the others add;
// grad_reduce (gaq_grad.hpp: gaq_policy_grad.hip's grad_reduce_kernel) sums the G partials in ascending order in fp64 and rounds once.  No atomics; dead lanes contribute exactly 0
// (their deltas are 0 and every activation is finite); nothing is read past S or through an index out of range.
#include "gaq_host.hpp"
#include "gaq_norm.hpp"
#include "gaq_grad.hpp"
#include "gaq_grad_dev.hpp"
#include "gaq_grad_seq_dev.hpp"

namespace {

// One argument record for both cells: the LSTM's has c0 right after h0 and c_out right after h_out, the GRU's has neither (an empty
// member takes no room), so each keeps the layout its kernels were recorded with.
struct SeqNone {};
template <bool L>
struct SeqArgsT {
  PolicyDev net;                  // width[0] = H (the cell), width[1 ..] the head's layers
  int32_t off_hh;                 // float offset of W_hh' in net.w
  PolObsNorm nm;                  // tab = nullptr: no normaliser
  int32_t T;
  int64_t S, ntiles;
  const float* obs;               // [T, S, D]
  const float* a;                 // [T, S, 4] or nullptr (eval without logp)
  const uint8_t* done;            // [T, S]
  const float* h0;                // [S, H]
  [[no_unique_address]] std::conditional_t<L, const float*, SeqNone> c0;   // [S, H]
  const float *logp_old, *adv;    // [T, S]
  const float *ret, *v_old;       // [T, S] or nullptr
  const float* wv;                // the value head (last width weights, bias) or nullptr
  float clip, scale, vclip, vf_coef;
  float log_std[4], inv_std[4];
  float *logp_out, *value_out, *mean_out, *h_out;   // eval
  [[no_unique_address]] std::conditional_t<L, float*, SeqNone> c_out;
  float* part;                    // [G][pstride]
  double* spart;                  // [G][kGradStatsAc]
  float* tape;                    // [G][T][64][H], the LSTM's [G][T][64][2][H]
  int64_t pstride;
  // the idx form (at the end: every offset above stays); the [T, S, ...] inputs are then [T, S_src, ...], h0 and c0 [S_src, H]
  const int32_t* idx;             // [S] source columns
  int64_t S_src;
  // device mode (after everything else): the policy's table log_std[4] | std[4] | inv_std[4], read by the row stage in place of
  // log_std and inv_std above, which are then 0
  const float* explore_tab;
};

// the chunks c, c + cs, ... c + (NG-1) cs -- one per gate -- of one product of the cell (`in` inputs: the rows of A, zero-padded to a
// multiple of 4) into acc[0 .. NG-2] and, the last gate, acc[JL]: cell_kloop<NG, JL>'s order of operations (k ascending, each MFMA a
// k-ordered fmaf chain) over this unit's LDS rows.  (GRU: <3, 2> for the x product and <3, 3> for the h product; LSTM: <4, 3>.)
template <int NG, int JL>
__device__ __forceinline__ void seq_kloop(const float* __restrict__ wl, int in, int c, int cs, const float* A, uint32_t lane,
                                          f32x4 (&acc)[4][4]) {
  const int h = (int)(lane >> 4);
  const float* arow = A + h * kGradStride + (lane & 15) * 4;
  const int kfull = in & ~3;
  for (int k0 = 0; k0 < kfull; k0 += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + k0 * kGradStride);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int s = j == NG - 1 ? JL : j;
      const float a = wl[((c + j * cs) * in + k0) * 16 + lane];
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[s][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[s][eb], 0, 0, 0);
    }
  }
  if (kfull < in) {                                               // the x product's last, partial k-step: no weight past in - 1 is read
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + kfull * kGradStride);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int s = j == NG - 1 ? JL : j;
      const float a = kfull + h < in ? wl[((c + j * cs) * in + kfull) * 16 + lane] : 0.0f;
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[s][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[s][eb], 0, 0, 0);
    }
  }
}

// chunk c's gate sums of this lane's 4 units x 4 column blocks: r, z (from b_i + b_h), n_x, n_h -- gru_cell's accumulators
__device__ __forceinline__ void seq_gates(const PolicyDev& net, int off_hh, int c, const float* X, const float* Hin, uint32_t lane,
                                          f32x4 (&acc)[4][4]) {
  const int hid = net.width[0], hc = hid / 16, D = net.in_dim;
  const float* wih = net.w + net.off[0];
  const float* bih = wih + 3 * hid * D;
  const float* whh = net.w + off_hh;
  const float* bhh = whh + 3 * hid * hid;
  const int u0 = c * 16 + 4 * (int)(lane >> 4);
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
  seq_kloop<3, 2>(wih, D, c, hc, X, lane, acc);
  seq_kloop<3, 3>(whh, hid, c, hc, Hin, lane, acc);
}

// the same for the LSTM: i, f, g, o, each from b_ih + b_hh -- lstm_cell's accumulators
__device__ __forceinline__ void lstm_gates(const PolicyDev& net, int off_hh, int c, const float* X, const float* Hin, uint32_t lane,
                                           f32x4 (&acc)[4][4]) {
  const int hid = net.width[0], hc = hid / 16, D = net.in_dim;
  const float* wih = net.w + net.off[0];
  const float* bih = wih + 4 * hid * D;
  const float* whh = net.w + off_hh;
  const float* bhh = whh + 4 * hid * hid;
  const int u0 = c * 16 + 4 * (int)(lane >> 4);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    f32x4 b;
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = bih[s * hid + u0 + r] + bhh[s * hid + u0 + r];
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[s][eb] = b;
  }
  seq_kloop<4, 3>(wih, D, c, hc, X, lane, acc);
  seq_kloop<4, 3>(whh, hid, c, hc, Hin, lane, acc);
}

// The encoder forms' record (gaq.h "sequences through an encoder"): the gradient kernel then also writes dfeat_t = W_ih^T planes, the
// gradient of the loss in the cell's input (the encoder's features), to dfeat [T, S, E] (the idx form: [T, S_src, E], row = source row).
// The base comes first, so every member keeps its offset, and the kernels without Dx keep their record and their argument segment.
template <bool L>
struct SeqArgsDx : SeqArgsT<L> {
  float* dfeat;
};

// `g` must stay the kernel's first and only argument: the row stage reads its own members of it at offset 0 of the kernel-argument
// segment, as grad_kernel's does.  The ten kernels are <L, false, false> (eval), <L, true, false>, <L, true, true> (the idx form) and
// the last two with Dx.  The body must not become a function called from here: one call below its __global__ entry point, even
// force-inlined, it gets another register allocation, and these kernels keep their recorded resource lines.
template <bool L, bool Bwd, bool Idx, bool Dx = false>
__global__ __launch_bounds__(kGradBlock) void grad_seq_kernel(std::conditional_t<Dx, SeqArgsDx<L>, SeqArgsT<L>> g) {
  static_assert(!Dx || Bwd);
  constexpr int NG = L ? 4 : 3;                                   // gates
  constexpr int TS = L ? 2 : 1;                                   // [., H] rows of a sequence's tape entry: h_t (and c_t)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dlt = reinterpret_cast<float*>(smem);                    // [5][64] the head's delta, sequence e at column grad_col(e)
  float* outs = dlt + kSeqND * kTile;                             // [4][64] the head's sums, sequence e at e
  float* vsum = outs + 4 * kTile;                                 // [4][64] the waves' parts of V
  double* red = reinterpret_cast<double*>(smem + (kSeqND + 8) * kTile * 4);   // [kGradStatsAc][64]
  [[maybe_unused]] int* sidx = reinterpret_cast<int*>(smem + kSeqHeadBytes);   // Idx: [64] the tile's source columns (or < 0)
  float* X = reinterpret_cast<float*>(smem + kSeqHeadBytes + (Idx ? kGradIdxBytes : 0));   // [kx][68] the observation
  const PolicyDev& net = g.net;
  const int D = net.in_dim, kx = (D + 15) & ~15, nh = net.n_hidden, act = net.hidden_act, H = net.width[0], hc = H / 16;
  const int w1 = nh > 1 ? net.width[1] : 0;
  float* Hin = X + kx * kGradStride;                              // [H][68] hin_t
  [[maybe_unused]] float* DH = Hin + H * kGradStride;             // Bwd: [H][68] the carried dh
  [[maybe_unused]] float* DC = DH + H * kGradStride;              // Bwd, L: [H][68] the carried dc
  float* P = Hin + (Bwd ? (L ? 3 : 2) : 1) * H * kGradStride;     // h_t, then the head's layers; Bwd: then the four delta planes of H rows
  auto Hl = [&](int l) { return P + ((l > 0 ? H : 0) + (l > 1 ? w1 : 0)) * kGradStride; };   // layer l's rows (0: the cell's h_t)
  const uint32_t lane = threadIdx.x & 63u;
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int G = (int)gridDim.x, T = g.T;
  const int64_t S = g.S;
  const int64_t t0 = (int64_t)blockIdx.x * g.ntiles / G, t1 = ((int64_t)blockIdx.x + 1) * g.ntiles / G;
  [[maybe_unused]] float* part = g.part + (int64_t)blockIdx.x * g.pstride;
  [[maybe_unused]] float* tape = g.tape + (int64_t)blockIdx.x * T * kTile * TS * H;
  const bool hasv = g.wv != nullptr;
  const int lw = net.width[nh - 1];                               // what the 4-output layer reads
  const float* wo = net.w + net.off[nh];                          // [lw][4], then bias[4]
  const int h4 = (int)(lane >> 4), n16 = (int)(lane & 15);
  // u0, this lane's first unit of its wave's chunk (wave < hc), and done[t-1]'s address below are each written per cell: where such a sum
  // is formed moves the kernels' instructions.  The LSTM's kernels were recorded with u0 formed here and dprev once per
  // step, the GRU's with both formed where they are used -- and a copy up here, even a dead one, is what the compiler would use.
  [[maybe_unused]] int u0_lstm = 0;
  if constexpr (L) u0_lstm = wave * 16 + 4 * h4;
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (Bwd && wave == 0) {
#pragma unroll
    for (int s = 0; s < kGradStatsAc; ++s) red[s * kTile + lane] = 0.0;
  }

  // the head over h_t in Hl(0): its layers, the 4 sums and V's parts; ends after the barrier that follows them
  auto head_forward = [&]() {
#pragma unroll 1
    for (int l = 1; l < nh; ++l) {
      seq_fwd_layer(net.w + net.off[l], net.width[l - 1], net.width[l], act, wave, Hl(l - 1), Hl(l), lane);
      __syncthreads();
    }
    const float* ycol = Hl(nh - 1) + grad_col((int)lane);
    {
      float s = wo[lw * 4 + wave];
#pragma unroll 8
      for (int u = 0; u < lw; ++u) s = __builtin_fmaf(wo[u * 4 + wave], ycol[u * kGradStride], s);
      outs[wave * kTile + lane] = s;
    }
    if (hasv) {                                                   // this wave's quarter of V: policy_value_part's chain
      const int q = lw / kGradWaves;
      float v = 0.0f;
#pragma unroll 8
      for (int u = wave * q; u < (wave + 1) * q; ++u) v = __builtin_fmaf(g.wv[u], ycol[u * kGradStride], v);
      vsum[wave * kTile + lane] = v;
    }
    __syncthreads();
  };

#pragma unroll 1
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t row0 = tile * kTile;
    const int nlive = (int)((S - row0) < kTile ? (S - row0) : kTile);
    if constexpr (Idx) {
      // the tile's indices, read once: an index outside [0, S_src) makes its lane a dead one (no address is ever formed from it) and
      // is counted by the row stage.  (The last readers of sidx, the previous tile's last step, stand behind a barrier.)
      if (tid < kTile) {
        const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<L>*)__builtin_amdgcn_kernarg_segment_ptr();
        int s = kGradIdxDead;
        if (tid < nlive) {
          const int64_t v = r.idx[row0 + tid];
          s = v >= 0 && v < r.S_src ? (int)v : kGradIdxSkipped;
        }
        sidx[tid] = s;
      }
      __syncthreads();
    }
    // Idx: lane e's source column (0 where it has none: then nothing is read through it), and whether it has one
    [[maybe_unused]] auto scol = [&](int e) -> int64_t { const int s = sidx[e]; return s >= 0 ? s : 0; };
    [[maybe_unused]] auto shas = [&](int e) -> bool { return sidx[e] >= 0; };
    bool live_;
    if constexpr (Idx) live_ = shas((int)lane);
    else live_ = (int)lane < nlive;
    const bool live = live_;
    // whether e is a live column, and its row of an [S (S_src), .] input
    auto has = [&](int e) -> bool {
      if constexpr (Idx) return shas(e);
      else return e < nlive;
    };
    auto srow = [&](int e) -> int64_t {
      if constexpr (Idx) return scol(e);
      else return row0 + e;
    };
    // done[t-1] of sequence e (base, tsrc, dprev: step t's; dprev is where step t-1's row of done starts)
    auto pdone = [&](int64_t base, [[maybe_unused]] int64_t tsrc, [[maybe_unused]] int64_t dprev, auto e) -> bool {
      if constexpr (L) return g.done[dprev + srow((int)e)] != 0;
      else if constexpr (Idx) return g.done[tsrc - g.S_src + scol((int)e)] != 0;
      else return g.done[base - S + e] != 0;
    };
    // ---- the forward sweep -------------------------------------------------------------------------------------------------------------
    [[maybe_unused]] f32x4 cst[4];                                // L, wave < hc: c of this lane's 4 units, one vector per column block
    if constexpr (L) {
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) cst[eb] = zero4;
    }
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      const int64_t base = (int64_t)t * S + row0;
      [[maybe_unused]] const int64_t tsrc = (int64_t)t * g.S_src;   // Idx: the step's first row in a [T, S_src, ...] input
      [[maybe_unused]] const int64_t dprev = Idx ? tsrc - g.S_src : base - S - row0;   // L
      seq_stage_obs<Idx>(X, g.obs, g.nm, Idx ? tsrc : base, nlive, sidx, D, tid);
      if (t == 0) {
        seq_stage_rows(Hin, g.h0 + srow((int)lane) * H, live, H, lane, wave);
      } else {                                                    // hin_t = h_{t-1} (still in Hl(0)), 0 where done[t-1] and in dead columns
        for (int f = tid; f < H * kTile; f += kGradBlock) {
          const int u = f >> 6, col = f & 63, e = grad_env(col);
          const bool keep = has(e) && !pdone(base, tsrc, dprev, e);
          Hin[u * kGradStride + col] = keep ? P[u * kGradStride + col] : 0.0f;
        }
      }
      if constexpr (L) {
        if (wave < hc) {                                          // cin_t, by the same select
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) {
            const int e = eb * 16 + n16;
            if (t == 0) cst[eb] = has(e) ? *reinterpret_cast<const f32x4*>(g.c0 + srow(e) * H + u0_lstm) : zero4;
            else cst[eb] = has(e) && !pdone(base, tsrc, dprev, e) ? cst[eb] : zero4;
          }
        }
      }
      __syncthreads();
      if (wave < hc) {
        const int u0 = L ? u0_lstm : wave * 16 + 4 * h4;
        f32x4 acc[4][4];
        f32x4 hn[4];
        if constexpr (L) lstm_gates(net, g.off_hh, wave, X, Hin, lane, acc);
        else seq_gates(net, g.off_hh, wave, X, Hin, lane, acc);
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (L) {
              const float ig = seq_sigmoid(acc[0][eb][r]), fg = seq_sigmoid(acc[1][eb][r]);
              const float gg = tanhf(acc[2][eb][r]), og = seq_sigmoid(acc[3][eb][r]);
              cst[eb][r] = __builtin_fmaf(fg, cst[eb][r], ig * gg);
              hn[eb][r] = og * tanhf(cst[eb][r]);
            } else {
              const float hold = Hin[(u0 + r) * kGradStride + n16 * 4 + eb];
              const float rg = seq_sigmoid(acc[0][eb][r]), zg = seq_sigmoid(acc[1][eb][r]);
              const float n = tanhf(__builtin_fmaf(rg, acc[3][eb][r], acc[2][eb][r]));
              hn[eb][r] = __builtin_fmaf(zg, hold - n, n);
            }
          }
          const int e = eb * 16 + n16;
          if (e < nlive) {
            if constexpr (Bwd) {
              float* row = tape + ((int64_t)t * kTile + e) * TS * H + u0;
              *reinterpret_cast<f32x4*>(row) = hn[eb];
              if constexpr (L) *reinterpret_cast<f32x4*>(row + H) = cst[eb];
            } else if (t == T - 1 && (L || g.h_out)) {
              const bool z = g.done[base + e] != 0;
              if (g.h_out) *reinterpret_cast<f32x4*>(g.h_out + (row0 + e) * H + u0) = z ? zero4 : hn[eb];
              if constexpr (L) {
                if (g.c_out) *reinterpret_cast<f32x4*>(g.c_out + (row0 + e) * H + u0) = z ? zero4 : cst[eb];
              }
            }
          }
        }
        if (!Bwd || t + 1 < T) {                                   // (the backward sweep reloads h_{T-1} from the tape)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 v = {hn[0][r], hn[1][r], hn[2][r], hn[3][r]};
            *reinterpret_cast<f32x4*>(P + (u0 + r) * kGradStride + n16 * 4) = v;
          }
        }
      }
      __syncthreads();
      if constexpr (!Bwd) {
        head_forward();
        if (wave == 0 && live) {                                  // lane = sequence
          const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<L>*)__builtin_amdgcn_kernarg_segment_ptr();
          const int e = (int)lane;
          const int64_t i = base + e;
          float m[4];
#pragma unroll
          for (int o = 0; o < 4; ++o) {
            m[o] = outs[o * kTile + e];
            if (net.out_tanh) m[o] = tanhf(m[o]);
          }
          if (r.logp_out) {
            float z[4], lp = 0.0f, ls[4], is[4];
            grad_explore(r, ls, is);
#pragma unroll
            for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * is[o];
#pragma unroll
            for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
            r.logp_out[i] = lp - kGradTwoLn2Pi;
          }
          if (r.value_out) r.value_out[i] = ((vsum[e] + vsum[kTile + e]) + (vsum[2 * kTile + e] + vsum[3 * kTile + e])) + r.wv[lw];
          if (r.mean_out) {
#pragma unroll
            for (int o = 0; o < 4; ++o) r.mean_out[i * 4 + o] = m[o];
          }
        }
        // (no barrier: the next writers of outs and vsum stand behind the next step's two)
      }
    }
    // ---- the backward sweep ------------------------------------------------------------------------------------------------------------
    if constexpr (Bwd) {
#pragma unroll 1
      for (int t = T - 1; t >= 0; --t) {
        const bool first = tile == t0 && t == T - 1, last_t = t == T - 1;
        const int64_t base = (int64_t)t * S + row0;
        [[maybe_unused]] const int64_t tsrc = (int64_t)t * g.S_src;
        [[maybe_unused]] const int64_t dprev = Idx ? tsrc - g.S_src : base - S - row0;   // L
        seq_stage_obs<Idx>(X, g.obs, g.nm, Idx ? tsrc : base, nlive, sidx, D, tid);
        if (t == 0) seq_stage_rows(Hin, g.h0 + srow((int)lane) * H, live, H, lane, wave);
        else seq_stage_rows(Hin, tape + ((int64_t)(t - 1) * kTile + lane) * TS * H, live && !pdone(base, tsrc, dprev, lane), H, lane, wave);
        seq_stage_rows(P, tape + ((int64_t)t * kTile + lane) * TS * H, live, H, lane, wave);
        __syncthreads();
        head_forward();
        if (wave == 0) {                                          // lane = sequence: gaq_policy_grad_ppo_ac_dev's row stage
          const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<L>*)__builtin_amdgcn_kernarg_segment_ptr();
          const int e = (int)lane;
          int64_t i_;
          if constexpr (Idx) i_ = tsrc + scol(e);
          else i_ = base + e;
          const int64_t i = i_;
          if constexpr (Idx) {                                    // a skipped index is counted once, in the spare statistic
            if (last_t && sidx[e] == kGradIdxSkipped) red[(kGradStatsAc - 1) * kTile + e] += 1.0;
          }
          float d[kSeqND];                                        // the head's delta (already times scale)
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) d[o] = 0.0f;
          if (live) {
            float m[4], dm[4], z[4], lp = 0.0f, ls[4], is[4];
            grad_explore(r, ls, is);
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              m[o] = outs[o * kTile + e];
              if (net.out_tanh) m[o] = tanhf(m[o]);
              dm[o] = net.out_tanh ? __builtin_fmaf(-m[o], m[o], 1.0f) : 1.0f;
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * is[o];
#pragma unroll
            for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
            lp -= kGradTwoLn2Pi;
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
            if (r.wv) {                                           // L_V = 1/2 max(e1^2, e2^2); dL_V / dV = e1 unless the clipped error is larger
              const float V = ((vsum[e] + vsum[kTile + e]) + (vsum[2 * kTile + e] + vsum[3 * kTile + e])) + r.wv[lw];
              const float ret = r.ret[i], e1 = V - ret;
              float lv = e1 * e1, dv = e1;
              if (r.vclip > 0.0f) {                               // (where the clamp does not bind, e2 is e1 itself: a tie)
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
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) dlt[o * kTile + grad_col(e)] = d[o];
        }
        __syncthreads();
        // the 4-output layer and the value head: thread u owns unit u of what they read -- dWo[u][:] and dwv[u], then its row becomes
        // delta (with the activation's derivative only where the row is a head layer's, not the cell's h_t); 5 more threads sum dbo, dbv
        float* pv = part + net.off[nh] + (lw + 1) * 4;             // the value head's words follow the packed weights
        if (tid < lw) {
          float* yrow = Hl(nh - 1) + tid * kGradStride;
          float w4[kSeqND], gw[kSeqND];
#pragma unroll
          for (int o = 0; o < 4; ++o) w4[o] = wo[tid * 4 + o];
          w4[4] = hasv ? g.wv[tid] : 0.0f;
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) gw[o] = 0.0f;
#pragma unroll 4
          for (int q = 0; q < kTile / 4; ++q) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(yrow + 4 * q);
            f32x4 dv[kSeqND], nv;
#pragma unroll
            for (int o = 0; o < kSeqND; ++o) dv[o] = *reinterpret_cast<const f32x4*>(dlt + o * kTile + 4 * q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              float s = 0.0f;
#pragma unroll
              for (int o = 0; o < kSeqND; ++o) {
                gw[o] = __builtin_fmaf(dv[o][c], hv[c], gw[o]);
                s = __builtin_fmaf(w4[o], dv[o][c], s);
              }
              nv[c] = nh > 1 ? s * grad_actd(act, hv[c]) : s;
            }
            *reinterpret_cast<f32x4*>(yrow + 4 * q) = nv;
          }
#pragma unroll
          for (int o = 0; o < 4; ++o) grad_put(part + net.off[nh] + tid * 4 + o, gw[o], first);
          if (hasv) grad_put(pv + tid, gw[4], first);
        } else if (tid >= kGradBlock - kSeqND && (tid < kGradBlock - 1 || hasv)) {
          const int o = tid - (kGradBlock - kSeqND);
          float s = 0.0f;
          for (int c = 0; c < kTile; ++c) s += dlt[o * kTile + c];
          grad_put(o < 4 ? part + net.off[nh] + lw * 4 + o : pv + lw, s, first);
        }
        __syncthreads();
        // the head's layers, from the last down to the first: dW_l and db_l, then the delta of the layer's input in place
#pragma unroll 1
        for (int l = nh - 1; l >= 1; --l) {
          const int width = net.width[l], in = net.width[l - 1];
          float* A = Hl(l - 1);
          const float* dl = Hl(l);
          const float* wl = net.w + net.off[l];
          float* pw = part + net.off[l];
          if (wave < width / 16) grad_dw(dl + wave * 16 * kGradStride, A, in, wave, lane, pw, first);
          if (tid < width) grad_put(pw + width * in + tid, grad_row_sum(dl + tid * kGradStride), first);
          __syncthreads();                                        // dW_l has consumed the layer's input
          if (wave < in / 16) {
            const int kc = wave;
            f32x4 acc[4];
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) acc[eb] = zero4;
            for (int uch = 0; uch < width / 16; ++uch) {
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + ((int64_t)uch * in + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(dl + (uch * 16 + 4 * h4 + i) * kGradStride + n16 * 4);
#pragma unroll
                for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              f32x4* pos = reinterpret_cast<f32x4*>(A + (kc * 16 + 4 * h4 + r) * kGradStride + n16 * 4);
              if (l > 1) {
                const f32x4 hv = *pos;
                const f32x4 nv = {acc[0][r] * grad_actd(act, hv[0]), acc[1][r] * grad_actd(act, hv[1]), acc[2][r] * grad_actd(act, hv[2]),
                                  acc[3][r] * grad_actd(act, hv[3])};
                *pos = nv;
              } else {
                const f32x4 nv = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
                *pos = nv;
              }
            }
          }
          __syncthreads();
        }
        // the cell: Hl(0) now holds the head's dh_t.  Each lane reads its 16 words of it (and of what is carried) before it writes the
        // planes, whose first H rows are those very rows; the other planes lie over the head's layers, which are spent.
        bool cut[4];                                              // done[t-1] or a dead column: nothing is carried in or out
        if constexpr (L) {                                        // (cin_t needs it; the GRU not before dh_{t-1})
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) {
            const int e = eb * 16 + n16;
            cut[eb] = !has(e) || (t > 0 && pdone(base, tsrc, dprev, e));
          }
        }
        if (wave < hc) {
          const int u0 = L ? u0_lstm : wave * 16 + 4 * h4;
          f32x4 acc[4][4];
          if constexpr (L) {
            lstm_gates(net, g.off_hh, wave, X, Hin, lane, acc);
            f32x4 cin[4];                                         // cin_t of the column blocks: c_{t-1} from the tape (c0 at t = 0) or 0
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) {
              const int e = eb * 16 + n16;
              const float* crow = t == 0 ? g.c0 + srow(e) * H + u0 : tape + (((int64_t)(t - 1) * kTile + e) * 2 + 1) * H + u0;
              cin[eb] = cut[eb] ? zero4 : *reinterpret_cast<const f32x4*>(crow);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int off = (u0 + r) * kGradStride + n16 * 4;
              f32x4 dh = *reinterpret_cast<const f32x4*>(P + off);
              f32x4 dcc = zero4;
              if (!last_t) {
                dh += *reinterpret_cast<const f32x4*>(DH + off);
                dcc = *reinterpret_cast<const f32x4*>(DC + off);
              }
              f32x4 dai, daf, dag, dao, dcn;
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) {
                const float ig = seq_sigmoid(acc[0][eb][r]), fg = seq_sigmoid(acc[1][eb][r]);
                const float gg = tanhf(acc[2][eb][r]), og = seq_sigmoid(acc[3][eb][r]);
                const float ci = cin[eb][r];
                const float tc = tanhf(__builtin_fmaf(fg, ci, ig * gg));
                const float dc = dcc[eb] + dh[eb] * og * __builtin_fmaf(-tc, tc, 1.0f);
                dao[eb] = dh[eb] * tc * og * (1.0f - og);
                dai[eb] = dc * gg * ig * (1.0f - ig);
                daf[eb] = dc * ci * fg * (1.0f - fg);
                dag[eb] = dc * ig * __builtin_fmaf(-gg, gg, 1.0f);
                dcn[eb] = cut[eb] ? 0.0f : dc * fg;
              }
              *reinterpret_cast<f32x4*>(P + off) = dai;
              *reinterpret_cast<f32x4*>(P + H * kGradStride + off) = daf;
              *reinterpret_cast<f32x4*>(P + 2 * H * kGradStride + off) = dag;
              *reinterpret_cast<f32x4*>(P + 3 * H * kGradStride + off) = dao;
              *reinterpret_cast<f32x4*>(DC + off) = dcn;
            }
          } else {
            seq_gates(net, g.off_hh, wave, X, Hin, lane, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int off = (u0 + r) * kGradStride + n16 * 4;
              const f32x4 hold = *reinterpret_cast<const f32x4*>(Hin + off);
              f32x4 dh = *reinterpret_cast<const f32x4*>(P + off);
              if (!last_t) dh += *reinterpret_cast<const f32x4*>(DH + off);
              f32x4 dar, daz, dan, dnh, dir;
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) {
                const float rg = seq_sigmoid(acc[0][eb][r]), zg = seq_sigmoid(acc[1][eb][r]), nhh = acc[3][eb][r];
                const float n = tanhf(__builtin_fmaf(rg, nhh, acc[2][eb][r]));
                dan[eb] = dh[eb] * (1.0f - zg) * __builtin_fmaf(-n, n, 1.0f);
                daz[eb] = dh[eb] * (hold[eb] - n) * zg * (1.0f - zg);
                dar[eb] = dan[eb] * nhh * rg * (1.0f - rg);
                dnh[eb] = dan[eb] * rg;
                dir[eb] = dh[eb] * zg;
              }
              *reinterpret_cast<f32x4*>(P + off) = dar;
              *reinterpret_cast<f32x4*>(P + H * kGradStride + off) = daz;
              *reinterpret_cast<f32x4*>(P + 2 * H * kGradStride + off) = dan;
              *reinterpret_cast<f32x4*>(P + 3 * H * kGradStride + off) = dnh;
              *reinterpret_cast<f32x4*>(DH + off) = dir;
            }
          }
        }
        __syncthreads();
        // dW_ih = planes x^T and dW_hh = planes hin^T in the packed layout (chunk uc = gate * H/16 + c).  The LSTM's four planes serve
        // both and b_ih and b_hh take the same sum; the GRU's W_hh skips the plane da_n for dn_h, and its n words of b_ih and b_hh are
        // those two planes' sums
        auto hplane = [&](int uc) {
          if constexpr (L) return uc;
          else return uc < 2 * hc ? uc : uc + hc;
        };
        {
          float* pih = part + net.off[0];
          float* phh = part + g.off_hh;
#pragma unroll 1
          for (int uc = wave; uc < NG * hc; uc += kGradWaves) {
            grad_dw(P + uc * 16 * kGradStride, X, D, uc, lane, pih, first);
            grad_dw(P + hplane(uc) * 16 * kGradStride, Hin, H, uc, lane, phh, first);
          }
          if (tid < 4 * H) {
            const float s = grad_row_sum(P + tid * kGradStride);
            if constexpr (L) {
              grad_put(pih + 4 * H * D + tid, s, first);
              grad_put(phh + 4 * H * H + tid, s, first);
            } else {
              if (tid < 3 * H) grad_put(pih + 3 * H * D + tid, s, first);
              if (tid < 2 * H) grad_put(phh + 3 * H * H + tid, s, first);
              if (tid >= 3 * H) grad_put(phh + 3 * H * H + tid - H, s, first);
            }
          }
        }
        // Dx: dfeat_t = W_ih^T planes (the GRU: da_r, da_z, da_n; the LSTM: all four) -- the W_hh^T product's code shape below with
        // in = D, this wave's input chunks wave, wave + 4, ...  The lane that holds 4 consecutive inputs of a sequence stores them as
        // one 16-byte store to the sequence's row of dfeat [T, S (S_src), D] (enc_store_feat's pattern); a dead column has no row, a
        // live one whose deltas are 0 writes zeros.
        if constexpr (Dx) {
          const float* wih = net.w + net.off[0];
#pragma unroll 1
          for (int kc = wave; kc < D / 16; kc += kGradWaves) {
            f32x4 acc[4];
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) acc[eb] = zero4;
            for (int uch = 0; uch < NG * hc; ++uch) {
              const float* drows = P + uch * 16 * kGradStride;
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wih + ((int64_t)uch * D + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(drows + (4 * h4 + i) * kGradStride + n16 * 4);
#pragma unroll
                for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
              }
            }
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) {
              const int e = eb * 16 + n16;
              if (has(e)) {
                int64_t row;
                if constexpr (Idx) row = tsrc + scol(e);
                else row = base + e;
                *reinterpret_cast<f32x4*>(g.dfeat + row * D + kc * 16 + 4 * h4) = acc[eb];
              }
            }
          }
        }
        // dh_{t-1} = W_hh^T planes (the GRU: + direct), 0 where done[t-1] (and in dead columns); nothing flows into h0
        if (t > 0 && wave < hc) {
          const float* whh = net.w + g.off_hh;
          const int kc = wave;
          f32x4 acc[4];
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) acc[eb] = zero4;
          for (int uch = 0; uch < NG * hc; ++uch) {
            const float* drows = P + hplane(uch) * 16 * kGradStride;
            const f32x4 wv = *reinterpret_cast<const f32x4*>(whh + ((int64_t)uch * H + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(drows + (4 * h4 + i) * kGradStride + n16 * 4);
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
            }
          }
          if constexpr (!L) {
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) {
              const int e = eb * 16 + n16;
              cut[eb] = !has(e) || pdone(base, tsrc, dprev, e);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            f32x4* pos = reinterpret_cast<f32x4*>(DH + (kc * 16 + 4 * h4 + r) * kGradStride + n16 * 4);
            if constexpr (L) {
              const f32x4 nv = {cut[0] ? 0.0f : acc[0][r], cut[1] ? 0.0f : acc[1][r], cut[2] ? 0.0f : acc[2][r], cut[3] ? 0.0f : acc[3][r]};
              *pos = nv;
            } else {                                              // + the direct term dh z, which the cell left here
              const f32x4 dir = *pos;
              const f32x4 nv = {cut[0] ? 0.0f : acc[0][r] + dir[0], cut[1] ? 0.0f : acc[1][r] + dir[1], cut[2] ? 0.0f : acc[2][r] + dir[2],
                                cut[3] ? 0.0f : acc[3][r] + dir[3]};
              *pos = nv;
            }
          }
        }
        __syncthreads();                                          // X, hin and the planes are read before the next step is staged
      }
    }
  }

  if constexpr (Bwd) {
    if (tid < kGradStatsAc) {                                     // the 64 lanes in ascending order
      double s = 0.0;
      for (int e = 0; e < kTile; ++e) s += red[tid * kTile + e];
      g.spart[(int64_t)blockIdx.x * kGradStatsAc + tid] = s;
    }
  }
}

// ---- the wide recurrent learner (gaq.h "the wide recurrent learner"): a GRU of up to kGradSeqWideMaxWidth = 128 units ------------------
// grad_seq_wide_kernel<Bwd, Idx>, three kernels (eval, the gradient, its idx form): grad_seq_kernel<false, ...>'s frame -- the LDS head,
// the 64-sequence tile, the idx rules, the staging, the head, the row stage, the partial and the tape -- with the cell's UNITS IN GROUPS OF
// 64.  A sibling of that kernel, not more parameters of it: its ten kernels keep their text.
//   forward   wave w runs the chunks w, w + 4 one after the other (64 accumulator registers at a time), each with seq_gates: gru_cell's
//             chain, so h_t is the rollout's bits at every H.  h_t goes to P's rows (no wave reads them before the barrier) and the tape.
//   backward  after the head's backward Hl(0) holds dh_t.  The owning lanes add the carried dh into the DH rows in place (the one fp32 add
//             of the narrow kernel).  Then per group g of 64 units (chunks 4g + wave): the gates recomputed, da_r, da_z, da_n, dn_h to the
//             group's four planes of min(H, 64) rows (over the rows the head used -- a lane overwrites only words of dh_t it has itself
//             consumed), dh z back into the lane's own words of DH, barrier; the group's dW_ih and dW_hh chunks and bias row sums to the
//             partial; this group's part of W_hh^T [da_r; da_z; dn_h] into 2 x 16 accumulator registers per lane (wave w: the outputs of
//             the chunks w and w + 4); barrier.  After the last group dh_{t-1} = direct + product, 0 by select where done[t-1] and in dead
//             columns.
// At one group (H <= 64) every sum has grad_seq_kernel's order: the results are that kernel's bits.
// LDS = 8.25 KiB + 272 B x (kx + 2 H + max(4 min(H, 64), H + head widths)) (+ 256 B for the idx form) for <true>: 156 416 B at
// 18-GRU128-64-64; 8.25 KiB + 272 B x (kx + 2 H + head widths) for <false>.
template <bool Bwd, bool Idx>
__global__ __launch_bounds__(kGradBlock) void grad_seq_wide_kernel(SeqArgsT<false> g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dlt = reinterpret_cast<float*>(smem);                    // [5][64] the head's delta, sequence e at column grad_col(e)
  float* outs = dlt + kSeqND * kTile;                             // [4][64] the head's sums, sequence e at e
  float* vsum = outs + 4 * kTile;                                 // [4][64] the waves' parts of V
  double* red = reinterpret_cast<double*>(smem + (kSeqND + 8) * kTile * 4);   // [kGradStatsAc][64]
  [[maybe_unused]] int* sidx = reinterpret_cast<int*>(smem + kSeqHeadBytes);   // Idx: [64] the tile's source columns (or < 0)
  float* X = reinterpret_cast<float*>(smem + kSeqHeadBytes + (Idx ? kGradIdxBytes : 0));   // [kx][68] the observation
  const PolicyDev& net = g.net;
  const int D = net.in_dim, kx = (D + 15) & ~15, nh = net.n_hidden, act = net.hidden_act, H = net.width[0], hc = H / 16;
  const int w1 = nh > 1 ? net.width[1] : 0;
  [[maybe_unused]] const int GH = H < 64 ? H : 64;                // the units of a group: the rows of one delta plane
  float* Hin = X + kx * kGradStride;                              // [H][68] hin_t
  [[maybe_unused]] float* DH = Hin + H * kGradStride;             // Bwd: [H][68] the carried dh, then the step's total dh, then dh z
  float* P = Hin + (Bwd ? 2 : 1) * H * kGradStride;               // h_t, then the head's layers; Bwd: then a group's four planes of GH rows
  auto Hl = [&](int l) { return P + ((l > 0 ? H : 0) + (l > 1 ? w1 : 0)) * kGradStride; };   // layer l's rows (0: the cell's h_t)
  const uint32_t lane = threadIdx.x & 63u;
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int G = (int)gridDim.x, T = g.T;
  const int64_t S = g.S;
  const int64_t t0 = (int64_t)blockIdx.x * g.ntiles / G, t1 = ((int64_t)blockIdx.x + 1) * g.ntiles / G;
  [[maybe_unused]] float* part = g.part + (int64_t)blockIdx.x * g.pstride;
  [[maybe_unused]] float* tape = g.tape + (int64_t)blockIdx.x * T * kTile * H;
  const bool hasv = g.wv != nullptr;
  const int lw = net.width[nh - 1];                               // what the 4-output layer reads
  const float* wo = net.w + net.off[nh];                          // [lw][4], then bias[4]
  const int h4 = (int)(lane >> 4), n16 = (int)(lane & 15);
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (Bwd && wave == 0) {
#pragma unroll
    for (int s = 0; s < kGradStatsAc; ++s) red[s * kTile + lane] = 0.0;
  }

  // the head over h_t in Hl(0): its layers, the 4 sums and V's parts; ends after the barrier that follows them
  auto head_forward = [&]() {
#pragma unroll 1
    for (int l = 1; l < nh; ++l) {
      seq_fwd_layer(net.w + net.off[l], net.width[l - 1], net.width[l], act, wave, Hl(l - 1), Hl(l), lane);
      __syncthreads();
    }
    const float* ycol = Hl(nh - 1) + grad_col((int)lane);
    {
      float s = wo[lw * 4 + wave];
#pragma unroll 8
      for (int u = 0; u < lw; ++u) s = __builtin_fmaf(wo[u * 4 + wave], ycol[u * kGradStride], s);
      outs[wave * kTile + lane] = s;
    }
    if (hasv) {                                                   // this wave's quarter of V: policy_value_part's chain
      const int q = lw / kGradWaves;
      float v = 0.0f;
#pragma unroll 8
      for (int u = wave * q; u < (wave + 1) * q; ++u) v = __builtin_fmaf(g.wv[u], ycol[u * kGradStride], v);
      vsum[wave * kTile + lane] = v;
    }
    __syncthreads();
  };

#pragma unroll 1
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t row0 = tile * kTile;
    const int nlive = (int)((S - row0) < kTile ? (S - row0) : kTile);
    if constexpr (Idx) {
      // the tile's indices, read once: an index outside [0, S_src) makes its lane a dead one (no address is ever formed from it) and
      // is counted by the row stage.  (The last readers of sidx, the previous tile's last step, stand behind a barrier.)
      if (tid < kTile) {
        const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<false>*)__builtin_amdgcn_kernarg_segment_ptr();
        int s = kGradIdxDead;
        if (tid < nlive) {
          const int64_t v = r.idx[row0 + tid];
          s = v >= 0 && v < r.S_src ? (int)v : kGradIdxSkipped;
        }
        sidx[tid] = s;
      }
      __syncthreads();
    }
    // Idx: lane e's source column (0 where it has none: then nothing is read through it), and whether it has one
    [[maybe_unused]] auto scol = [&](int e) -> int64_t { const int s = sidx[e]; return s >= 0 ? s : 0; };
    [[maybe_unused]] auto shas = [&](int e) -> bool { return sidx[e] >= 0; };
    bool live_;
    if constexpr (Idx) live_ = shas((int)lane);
    else live_ = (int)lane < nlive;
    const bool live = live_;
    // whether e is a live column, and its row of an [S (S_src), .] input
    auto has = [&](int e) -> bool {
      if constexpr (Idx) return shas(e);
      else return e < nlive;
    };
    auto srow = [&](int e) -> int64_t {
      if constexpr (Idx) return scol(e);
      else return row0 + e;
    };
    // done[t-1] of sequence e (base, tsrc: step t's)
    auto pdone = [&](int64_t base, [[maybe_unused]] int64_t tsrc, auto e) -> bool {
      if constexpr (Idx) return g.done[tsrc - g.S_src + scol((int)e)] != 0;
      else return g.done[base - S + e] != 0;
    };
    // ---- the forward sweep -------------------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      const int64_t base = (int64_t)t * S + row0;
      [[maybe_unused]] const int64_t tsrc = (int64_t)t * g.S_src;   // Idx: the step's first row in a [T, S_src, ...] input
      seq_stage_obs<Idx>(X, g.obs, g.nm, Idx ? tsrc : base, nlive, sidx, D, tid);
      if (t == 0) {
        seq_stage_rows(Hin, g.h0 + srow((int)lane) * H, live, H, lane, wave);
      } else {                                                    // hin_t = h_{t-1} (still in Hl(0)), 0 where done[t-1] and in dead columns
        for (int f = tid; f < H * kTile; f += kGradBlock) {
          const int u = f >> 6, col = f & 63, e = grad_env(col);
          const bool keep = has(e) && !pdone(base, tsrc, e);
          Hin[u * kGradStride + col] = keep ? P[u * kGradStride + col] : 0.0f;
        }
      }
      __syncthreads();
#pragma unroll 1
      for (int c = wave; c < hc; c += kGradWaves) {               // this wave's chunks, one after the other
        const int u0 = c * 16 + 4 * h4;
        f32x4 acc[4][4];
        f32x4 hn[4];
        seq_gates(net, g.off_hh, c, X, Hin, lane, acc);
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float hold = Hin[(u0 + r) * kGradStride + n16 * 4 + eb];
            const float rg = seq_sigmoid(acc[0][eb][r]), zg = seq_sigmoid(acc[1][eb][r]);
            const float n = tanhf(__builtin_fmaf(rg, acc[3][eb][r], acc[2][eb][r]));
            hn[eb][r] = __builtin_fmaf(zg, hold - n, n);
          }
          const int e = eb * 16 + n16;
          if (e < nlive) {
            if constexpr (Bwd) {
              *reinterpret_cast<f32x4*>(tape + ((int64_t)t * kTile + e) * H + u0) = hn[eb];
            } else if (t == T - 1 && g.h_out) {
              const bool z = g.done[base + e] != 0;
              *reinterpret_cast<f32x4*>(g.h_out + (row0 + e) * H + u0) = z ? zero4 : hn[eb];
            }
          }
        }
        if (!Bwd || t + 1 < T) {                                   // (the backward sweep reloads h_{T-1} from the tape)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 v = {hn[0][r], hn[1][r], hn[2][r], hn[3][r]};
            *reinterpret_cast<f32x4*>(P + (u0 + r) * kGradStride + n16 * 4) = v;
          }
        }
      }
      __syncthreads();
      if constexpr (!Bwd) {
        head_forward();
        if (wave == 0 && live) {                                  // lane = sequence
          const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<false>*)__builtin_amdgcn_kernarg_segment_ptr();
          const int e = (int)lane;
          const int64_t i = base + e;
          float m[4];
#pragma unroll
          for (int o = 0; o < 4; ++o) {
            m[o] = outs[o * kTile + e];
            if (net.out_tanh) m[o] = tanhf(m[o]);
          }
          if (r.logp_out) {
            float z[4], lp = 0.0f, ls[4], is[4];
            grad_explore(r, ls, is);
#pragma unroll
            for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * is[o];
#pragma unroll
            for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
            r.logp_out[i] = lp - kGradTwoLn2Pi;
          }
          if (r.value_out) r.value_out[i] = ((vsum[e] + vsum[kTile + e]) + (vsum[2 * kTile + e] + vsum[3 * kTile + e])) + r.wv[lw];
          if (r.mean_out) {
#pragma unroll
            for (int o = 0; o < 4; ++o) r.mean_out[i * 4 + o] = m[o];
          }
        }
        // (no barrier: the next writers of outs and vsum stand behind the next step's two)
      }
    }
    // ---- the backward sweep ------------------------------------------------------------------------------------------------------------
    if constexpr (Bwd) {
#pragma unroll 1
      for (int t = T - 1; t >= 0; --t) {
        const bool first = tile == t0 && t == T - 1, last_t = t == T - 1;
        const int64_t base = (int64_t)t * S + row0;
        [[maybe_unused]] const int64_t tsrc = (int64_t)t * g.S_src;
        seq_stage_obs<Idx>(X, g.obs, g.nm, Idx ? tsrc : base, nlive, sidx, D, tid);
        if (t == 0) seq_stage_rows(Hin, g.h0 + srow((int)lane) * H, live, H, lane, wave);
        else seq_stage_rows(Hin, tape + ((int64_t)(t - 1) * kTile + lane) * H, live && !pdone(base, tsrc, lane), H, lane, wave);
        seq_stage_rows(P, tape + ((int64_t)t * kTile + lane) * H, live, H, lane, wave);
        __syncthreads();
        head_forward();
        if (wave == 0) {                                          // lane = sequence: gaq_policy_grad_ppo_ac_dev's row stage
          const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<false>*)__builtin_amdgcn_kernarg_segment_ptr();
          const int e = (int)lane;
          int64_t i_;
          if constexpr (Idx) i_ = tsrc + scol(e);
          else i_ = base + e;
          const int64_t i = i_;
          if constexpr (Idx) {                                    // a skipped index is counted once, in the spare statistic
            if (last_t && sidx[e] == kGradIdxSkipped) red[(kGradStatsAc - 1) * kTile + e] += 1.0;
          }
          float d[kSeqND];                                        // the head's delta (already times scale)
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) d[o] = 0.0f;
          if (live) {
            float m[4], dm[4], z[4], lp = 0.0f, ls[4], is[4];
            grad_explore(r, ls, is);
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              m[o] = outs[o * kTile + e];
              if (net.out_tanh) m[o] = tanhf(m[o]);
              dm[o] = net.out_tanh ? __builtin_fmaf(-m[o], m[o], 1.0f) : 1.0f;
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * is[o];
#pragma unroll
            for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
            lp -= kGradTwoLn2Pi;
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
            if (r.wv) {                                           // L_V = 1/2 max(e1^2, e2^2); dL_V / dV = e1 unless the clipped error is larger
              const float V = ((vsum[e] + vsum[kTile + e]) + (vsum[2 * kTile + e] + vsum[3 * kTile + e])) + r.wv[lw];
              const float ret = r.ret[i], e1 = V - ret;
              float lv = e1 * e1, dv = e1;
              if (r.vclip > 0.0f) {                               // (where the clamp does not bind, e2 is e1 itself: a tie)
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
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) dlt[o * kTile + grad_col(e)] = d[o];
        }
        __syncthreads();
        // the 4-output layer and the value head: thread u owns unit u of what they read (at most 128: the cell itself) -- dWo[u][:] and
        // dwv[u], then its row becomes delta (with the activation's derivative only where the row is a head layer's, not the cell's
        // h_t); 5 more threads sum dbo, dbv
        float* pv = part + net.off[nh] + (lw + 1) * 4;             // the value head's words follow the packed weights
        if (tid < lw) {
          float* yrow = Hl(nh - 1) + tid * kGradStride;
          float w4[kSeqND], gw[kSeqND];
#pragma unroll
          for (int o = 0; o < 4; ++o) w4[o] = wo[tid * 4 + o];
          w4[4] = hasv ? g.wv[tid] : 0.0f;
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) gw[o] = 0.0f;
#pragma unroll 4
          for (int q = 0; q < kTile / 4; ++q) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(yrow + 4 * q);
            f32x4 dv[kSeqND], nv;
#pragma unroll
            for (int o = 0; o < kSeqND; ++o) dv[o] = *reinterpret_cast<const f32x4*>(dlt + o * kTile + 4 * q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              float s = 0.0f;
#pragma unroll
              for (int o = 0; o < kSeqND; ++o) {
                gw[o] = __builtin_fmaf(dv[o][c], hv[c], gw[o]);
                s = __builtin_fmaf(w4[o], dv[o][c], s);
              }
              nv[c] = nh > 1 ? s * grad_actd(act, hv[c]) : s;
            }
            *reinterpret_cast<f32x4*>(yrow + 4 * q) = nv;
          }
#pragma unroll
          for (int o = 0; o < 4; ++o) grad_put(part + net.off[nh] + tid * 4 + o, gw[o], first);
          if (hasv) grad_put(pv + tid, gw[4], first);
        } else if (tid >= kGradBlock - kSeqND && (tid < kGradBlock - 1 || hasv)) {
          const int o = tid - (kGradBlock - kSeqND);
          float s = 0.0f;
          for (int c = 0; c < kTile; ++c) s += dlt[o * kTile + c];
          grad_put(o < 4 ? part + net.off[nh] + lw * 4 + o : pv + lw, s, first);
        }
        __syncthreads();
        // the head's layers, from the last down to the first: dW_l and db_l, then the delta of the layer's input in place (the first
        // layer's input is the cell's h_t: up to 8 chunks, this wave's one after the other)
#pragma unroll 1
        for (int l = nh - 1; l >= 1; --l) {
          const int width = net.width[l], in = net.width[l - 1];
          float* A = Hl(l - 1);
          const float* dl = Hl(l);
          const float* wl = net.w + net.off[l];
          float* pw = part + net.off[l];
          if (wave < width / 16) grad_dw(dl + wave * 16 * kGradStride, A, in, wave, lane, pw, first);
          if (tid < width) grad_put(pw + width * in + tid, grad_row_sum(dl + tid * kGradStride), first);
          __syncthreads();                                        // dW_l has consumed the layer's input
#pragma unroll 1
          for (int kc = wave; kc < in / 16; kc += kGradWaves) {
            f32x4 acc[4];
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) acc[eb] = zero4;
            for (int uch = 0; uch < width / 16; ++uch) {
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + ((int64_t)uch * in + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(dl + (uch * 16 + 4 * h4 + i) * kGradStride + n16 * 4);
#pragma unroll
                for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              f32x4* pos = reinterpret_cast<f32x4*>(A + (kc * 16 + 4 * h4 + r) * kGradStride + n16 * 4);
              if (l > 1) {
                const f32x4 hv = *pos;
                const f32x4 nv = {acc[0][r] * grad_actd(act, hv[0]), acc[1][r] * grad_actd(act, hv[1]), acc[2][r] * grad_actd(act, hv[2]),
                                  acc[3][r] * grad_actd(act, hv[3])};
                *pos = nv;
              } else {
                const f32x4 nv = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
                *pos = nv;
              }
            }
          }
          __syncthreads();
        }
        // the cell: Hl(0) now holds the head's dh_t.  The total dh = dh_t + carried goes to DH in place, by the lane that owns the words
        // in every later stage of the step.  No barrier: a group's planes lie over P's rows, and plane j's rows of this wave's chunk are,
        // where they are rows of dh_t at all (j GH a multiple of 64), words of a chunk this same lane has just consumed; the rows behind
        // dh_t are the head's layers, which are spent.
#pragma unroll 1
        for (int c = wave; c < hc; c += kGradWaves) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int off = (c * 16 + 4 * h4 + r) * kGradStride + n16 * 4;
            f32x4 dh = *reinterpret_cast<const f32x4*>(P + off);
            if (!last_t) dh += *reinterpret_cast<const f32x4*>(DH + off);
            *reinterpret_cast<f32x4*>(DH + off) = dh;
          }
        }
        float* pih = part + net.off[0];
        float* phh = part + g.off_hh;
        const float* whh = net.w + g.off_hh;
        f32x4 dacc[2][4];                                         // W_hh^T [da_r; da_z; dn_h]: the outputs of the chunks wave and wave + 4
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) dacc[kk][eb] = zero4;
#pragma unroll 1
        for (int ub = 0; ub < H; ub += 64) {                      // the group of the units ub .. ub + 63: the chunks c0 .. c0 + gc - 1
          const int c0 = ub / 16, gc = hc - c0 < kGradWaves ? hc - c0 : kGradWaves;
          if (wave < gc) {
            const int c = c0 + wave, u0 = c * 16 + 4 * h4;
            f32x4 acc[4][4];
            seq_gates(net, g.off_hh, c, X, Hin, lane, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int off = (u0 + r) * kGradStride + n16 * 4;   // the unit's row of Hin and DH
              const int poff = (wave * 16 + 4 * h4 + r) * kGradStride + n16 * 4;   // ... and of a plane
              const f32x4 hold = *reinterpret_cast<const f32x4*>(Hin + off);
              const f32x4 dh = *reinterpret_cast<const f32x4*>(DH + off);
              f32x4 dar, daz, dan, dnh, dir;
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) {
                const float rg = seq_sigmoid(acc[0][eb][r]), zg = seq_sigmoid(acc[1][eb][r]), nhh = acc[3][eb][r];
                const float n = tanhf(__builtin_fmaf(rg, nhh, acc[2][eb][r]));
                dan[eb] = dh[eb] * (1.0f - zg) * __builtin_fmaf(-n, n, 1.0f);
                daz[eb] = dh[eb] * (hold[eb] - n) * zg * (1.0f - zg);
                dar[eb] = dan[eb] * nhh * rg * (1.0f - rg);
                dnh[eb] = dan[eb] * rg;
                dir[eb] = dh[eb] * zg;
              }
              *reinterpret_cast<f32x4*>(P + poff) = dar;
              *reinterpret_cast<f32x4*>(P + GH * kGradStride + poff) = daz;
              *reinterpret_cast<f32x4*>(P + 2 * GH * kGradStride + poff) = dan;
              *reinterpret_cast<f32x4*>(P + 3 * GH * kGradStride + poff) = dnh;
              *reinterpret_cast<f32x4*>(DH + off) = dir;
            }
          }
          __syncthreads();
          // the group's chunks of dW_ih = [da_r; da_z; da_n] x^T and dW_hh = [da_r; da_z; dn_h] hin^T in the packed layout (chunk
          // uc = gate * H/16 + c); item q = gate * gc + local chunk, so at one group q is uc and the planes' rows are 16 uc
#pragma unroll 1
          for (int q = wave; q < 3 * gc; q += kGradWaves) {
            const int j = q / gc, lc = q - j * gc, uc = j * hc + c0 + lc;
            grad_dw(P + (j * GH + lc * 16) * kGradStride, X, D, uc, lane, pih, first);
            grad_dw(P + ((j < 2 ? j : 3) * GH + lc * 16) * kGradStride, Hin, H, uc, lane, phh, first);
          }
          if (tid < 4 * GH) {                                      // the bias words: row sums in ascending column order
            const int j = tid / GH, u = ub + tid - j * GH;
            if (u < H) {
              const float s = grad_row_sum(P + tid * kGradStride);
              if (j < 3) grad_put(pih + 3 * H * D + j * H + u, s, first);
              if (j < 2) grad_put(phh + 3 * H * H + j * H + u, s, first);
              if (j == 3) grad_put(phh + 3 * H * H + 2 * H + u, s, first);
            }
          }
          // this group's part of W_hh^T [da_r; da_z; dn_h]: gate by gate, the group's chunks ascending (at one group: all of them in
          // the packed order); nothing flows into h0
          if (t > 0) {
#pragma unroll 1
            for (int q = 0; q < 3 * gc; ++q) {
              const int j = q / gc, lc = q - j * gc, uch = j * hc + c0 + lc;
              const float* drows = P + ((j < 2 ? j : 3) * GH + lc * 16) * kGradStride;
              f32x4 x[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const f32x4*>(drows + (4 * h4 + i) * kGradStride + n16 * 4);
#pragma unroll
              for (int kk = 0; kk < 2; ++kk) {
                const int kc = wave + kk * kGradWaves;
                if (kc < hc) {
                  const f32x4 wv = *reinterpret_cast<const f32x4*>(whh + ((int64_t)uch * H + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
                  for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int eb = 0; eb < 4; ++eb) dacc[kk][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[i][eb], dacc[kk][eb], 0, 0, 0);
                  }
                }
              }
            }
          }
          __syncthreads();                                        // the planes (and, after the last group, X and hin) are read
        }
        // dh_{t-1} = direct + product, 0 where done[t-1] (and in dead columns), into the lane's own words of DH
        if (t > 0) {
          bool cut[4];
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) {
            const int e = eb * 16 + n16;
            cut[eb] = !has(e) || pdone(base, tsrc, e);
          }
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const int kc = wave + kk * kGradWaves;
            if (kc < hc) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                f32x4* pos = reinterpret_cast<f32x4*>(DH + (kc * 16 + 4 * h4 + r) * kGradStride + n16 * 4);
                const f32x4 dir = *pos;
                const f32x4 nv = {cut[0] ? 0.0f : dacc[kk][0][r] + dir[0], cut[1] ? 0.0f : dacc[kk][1][r] + dir[1],
                                  cut[2] ? 0.0f : dacc[kk][2][r] + dir[2], cut[3] ? 0.0f : dacc[kk][3][r] + dir[3]};
                *pos = nv;
              }
            }
          }
        }
        // (no barrier: these words of DH are this lane's own until the next step's cell, and the group loop's last barrier stands
        // between this step's readers of X, hin and the planes and the next step's staging)
      }
    }
  }

  if constexpr (Bwd) {
    if (tid < kGradStatsAc) {                                     // the 64 lanes in ascending order
      double s = 0.0;
      for (int e = 0; e < kTile; ++e) s += red[tid * kTile + e];
      g.spart[(int64_t)blockIdx.x * kGradStatsAc + tid] = s;
    }
  }
}

// gaq.h's formula for the wide kernels: a group's four planes of min(H, 64) rows in place of four planes of H rows
size_t seq_wide_lds(const PolicyDev& pd, bool bwd) {
  const int H = pd.width[0];
  int head = H;
  for (int l = 1; l < pd.n_hidden; ++l) head += pd.width[l];
  const int rows = ((pd.in_dim + 15) & ~15) + (bwd ? 2 : 1) * H + (bwd ? std::max(4 * std::min(H, 64), head) : head);
  return (size_t)kSeqHeadBytes + (size_t)rows * kGradStride * 4;
}
// An example, not the guard: the largest net the view accepts on an 18-wide observation (kx = 32), in the idx form, 18-GRU128-64-64,
// is 156 672 B.  The ceiling over every in_dim (kx = 48 at H = 128: 161 024 B with an index vector) is held per call by seq_ready and by
// the idx form's re-check in seq_grad_call.
static_assert((size_t)kSeqHeadBytes + kGradIdxBytes + (size_t)(32 + 2 * kGradSeqWideMaxWidth + 4 * 64) * kGradStride * 4 <= kGradLdsMax,
              "the wide sequence kernel's largest form must fit the LDS a workgroup may ask for");

// gaq.h's formula: the backward pass carries dh (the LSTM: and dc) beside hin
size_t seq_lds(const PolicyDev& pd, bool lstm, bool bwd) {
  const int H = pd.width[0];
  int head = H;
  for (int l = 1; l < pd.n_hidden; ++l) head += pd.width[l];
  const int rows = ((pd.in_dim + 15) & ~15) + (bwd ? (lstm ? 3 : 2) : 1) * H + (bwd ? std::max(4 * H, head) : head);
  return (size_t)kSeqHeadBytes + (size_t)rows * kGradStride * 4;
}

// One call of any of the nine entry points: every argument one of them takes, by name; what a form does not have stays 0
struct SeqIn {
  const char* who;
  int32_t T;
  int64_t S, S_src;               // S_src: the columns the inputs span -- S, but for the idx forms
  bool gather;                    // the idx forms: idx [S] names the columns
  const int32_t* idx;
  const float *obs, *actions, *h0, *c0;                           // c0 and c_out: an LSTM's
  const uint8_t* done;
  const float *logp_old, *adv, *ret, *v_old;                      // the PPO gradient's inputs and hyper-parameters
  float clip_eps, vclip, vf_coef, ent_coef, scale;
  float *logp_out, *value_out, *mean_out, *h_out, *c_out;         // what eval writes
  float *grad_out, *grad_enc_out, *grad_value_out, *grad_log_std_out;   // what the gradient writes (grad_enc_out: the encoder forms)
  double* stats_out;
  void* stream;
  // the encoder forms (policy_grad_enc_seq_view's): obs is [., the env's obs_dim], the encoder's kernel writes the features [., E] to the
  // handle's scratch and the sequence kernel reads those as its observation (net.in_dim = E; the encoder's launch has normalised)
  const GradNet* view;
  const GradEnc* enc;
  bool wide_form;                 // the wide recurrent learner's calls (a GRU of up to 128 units): its view, its LDS figure, its kernels
};

// the arguments the calls share, checked: T, S, the handle's view (the encoder forms: the caller's), log_std
template <bool L>
struct SeqCall { GradNet v; SeqArgsT<L> g{}; };

template <bool L>
int seq_begin(SeqCall<L>& c, gaq_policy* p, const SeqIn& in) {
  const std::string who = std::string(in.who) + ": ";
  if (in.enc) c.v = *in.view;
  else if (in.wide_form) { if (int rc = policy_grad_seq_wide_view(p, c.v)) return rc; }
  else if (int rc = policy_grad_seq_view(p, L ? GAQ_POLICY_CELL_LSTM : GAQ_POLICY_CELL_GRU, c.v)) return rc;
  if (in.T < 1) return fail(GAQ_ERR_INVALID, who + "T must be at least 1");
  if (in.S < 0) return fail(GAQ_ERR_INVALID, who + "S must not be negative");
  const PolicyNet& net = *c.v.net;
  SeqArgsT<L>& g = c.g;
  g.net = net.pd; g.off_hh = c.v.off_hh; g.nm = policy_norm_dev(in.enc ? nullptr : net.norm);
  g.T = in.T; g.S = in.S; g.ntiles = (in.S + kTile - 1) / kTile;
  grad_fill_std(c.v, g.log_std, g.inv_std);
  g.explore_tab = c.v.tab;
  g.wv = c.v.wv;
  return GAQ_OK;
}

// the checks every call ends with (alignment, overlaps, sizes), then the device
template <bool L>
int seq_ready(const SeqCall<L>& c, const char* name, bool bwd, bool wide, bool misaligned, const std::vector<Span>& in,
              const std::vector<Span>& out, size_t& lds, bool wide_form = false) {
  const std::string who = std::string(name) + ": ";
  if (misaligned)
    return fail(GAQ_ERR_INVALID, who + "pointers must be 4-byte aligned (h0" + (L ? ", c0" : "") + (bwd ? "" : L ? ", h_out, c_out" : ", h_out") +
                                     ": 16" + (wide && bwd ? ", stats_out: 8" : "") + ")");
  if (int rc = check_overlap(name, in, out)) return rc;
  lds = wide_form ? seq_wide_lds(c.g.net, bwd) : seq_lds(c.g.net, L, bwd);
  if (lds > kGradLdsMax) return fail(GAQ_ERR_INVALID, who + "in_dim too large for the sequence kernel's LDS");
  if (c.g.ntiles > ((int64_t)1 << 31) - 1 || (int64_t)c.g.T * c.g.S > ((int64_t)1 << 40))
    return fail(GAQ_ERR_INVALID, who + "too many sequences or steps for one launch");
  HIP_TRY(hipSetDevice(c.v.net->device));
  return GAQ_OK;
}

// What a gradient call of an encoder form keeps behind the tape in the handle's scratch: feat and dfeat [T S_src, E], the encoder's
// partials [Gf][estride], and for the idx form the row indices [T S] twice (signed for the encoder's backward, a list for its gathered
// forward) and the list's count.  Without an encoder it is 0 bytes.
struct SeqEncPlan {
  int64_t rows = 0, estride = 0;  // T S: what the encoder's passes work on; floats of one partial of its backward
  int Gf = 0;                     // that pass's workgroups
  size_t feat_bytes = 0, epart_bytes = 0, ridx_bytes = 0, bytes = 0;   // bytes: all of it, what the call asks grad_scratch for beyond the tape
  float *feat = nullptr, *dfeat = nullptr, *epart = nullptr;
  int32_t* rowidx = nullptr;
  uint32_t *rowlist = nullptr, *rowcount = nullptr;
  void place(char* at) {          // at: the tape's end
    feat = reinterpret_cast<float*>(at);
    dfeat = reinterpret_cast<float*>(at += feat_bytes);
    epart = reinterpret_cast<float*>(at += feat_bytes);
    rowidx = reinterpret_cast<int32_t*>(at += epart_bytes);
    rowlist = reinterpret_cast<uint32_t*>(at += ridx_bytes);
    rowcount = reinterpret_cast<uint32_t*>(at += ridx_bytes);
  }
};
SeqEncPlan seq_enc_plan(int32_t T, int64_t S, int64_t S_src, bool gather, const GradEnc* enc) {
  SeqEncPlan pl;
  pl.rows = (int64_t)T * S;
  if (!enc) return pl;
  pl.Gf = grad_groups((pl.rows + kTile - 1) / kTile);
  pl.estride = (enc->nw + 15) & ~(int64_t)15;
  pl.feat_bytes = (size_t)T * (size_t)S_src * (size_t)enc->width * sizeof(float);
  pl.epart_bytes = (size_t)pl.Gf * (size_t)pl.estride * sizeof(float);
  pl.ridx_bytes = gather ? (((size_t)pl.rows * 4 + 15) & ~(size_t)15) : 0;
  pl.bytes = 2 * pl.feat_bytes + pl.epart_bytes + 2 * pl.ridx_bytes + (pl.ridx_bytes ? 16 : 0);
  return pl;
}

// the encoder's forward, the rollout's bits: the stored rows -> pl.feat, all of them or (the idx form) those the index vector names
int seq_encode(const SeqIn& in, const SeqEncPlan& pl, hipStream_t st) {
  if (!in.gather) return policy_encode_rows(*in.enc, pl.rows, in.obs, pl.feat, st);
  if (int rc = grad_rowidx_run(in.T, in.S, in.idx, in.S_src, pl.rowidx, pl.rowlist, pl.rowcount, st)) return rc;
  return policy_encode_list(*in.enc, pl.rows, pl.rowlist, pl.rowcount, in.obs, pl.feat, st);
}

// the encoder's backward over the stored rows from pl.dfeat (gaq_policy_grad.hip grad_feat_kernel: batch work, T times the parallelism
// of the sequence kernel), then its partials summed like every other: ascending in fp64, no statistics
int seq_encode_backward(const SeqIn& in, const SeqEncPlan& pl, const PolicyNet& net, const double* spart, hipStream_t st) {
  GradFeatCall f{};
  const PolObsNorm enm = policy_norm_dev(net.norm);
  f.trunk = in.enc->trunk; f.nm_tab = enm.tab; f.nm_dim = enm.dim; f.rows = pl.rows;
  f.obs = in.obs; f.dfeat = pl.dfeat; f.rowidx = in.gather ? pl.rowidx : nullptr; f.part = pl.epart; f.pstride = pl.estride; f.G = pl.Gf;
  if (int rc = grad_feat_run(f, st)) return rc;
  GradReduce re{};
  re.part = pl.epart; re.spart = spart; re.G = pl.Gf; re.ns = 0; re.pstride = pl.estride; re.nw = in.enc->nw; re.nv = 0; re.rows = pl.rows;
  re.grad_out = in.grad_enc_out;
  return grad_reduce(re, st);
}

// the forward pass of either cell
template <bool L>
int seq_eval_call(gaq_policy* p, const SeqIn& in) {
  const GradEnc* enc = in.enc;
  const int64_t S = in.S;
  SeqCall<L> c;
  if (int rc = seq_begin(c, p, in)) return rc;
  SeqArgsT<L>& g = c.g;
  const size_t n = (size_t)in.T * (size_t)S, H = (size_t)g.net.width[0];
  std::vector<Span> ins = {{in.obs, n * (enc ? enc->in_dim : g.net.in_dim) * 4, SPAN_ROWS}, {in.actions, n * 16, in.logp_out ? SPAN_ROWS : SPAN_OPTIONAL},
                           {in.done, n, SPAN_ROWS, 1}, {in.h0, (size_t)S * H * 4, SPAN_ROWS, 16}};
  std::vector<Span> outs = {{in.logp_out, n * 4, SPAN_OPTIONAL}, {in.value_out, n * 4, SPAN_OPTIONAL}, {in.mean_out, n * 16, SPAN_OPTIONAL},
                            {in.h_out, (size_t)S * H * 4, SPAN_OPTIONAL, 16}};
  if (L) {
    ins.push_back({in.c0, (size_t)S * H * 4, SPAN_ROWS, 16});
    outs.push_back({in.c_out, (size_t)S * H * 4, SPAN_OPTIONAL, 16});
  }
  bool wide = false, misaligned = false;
  if (int rc = check_span_nulls(ins, outs, S > 0, wide, misaligned)) return rc;
  if (in.value_out && !c.v.wv)
    return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head): the actor-critic passes need V on the policy's trunk");
  if (in.logp_out && !c.v.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no log-probability");
  size_t lds = 0;
  if (int rc = seq_ready(c, in.who, false, wide, misaligned, ins, outs, lds, in.wide_form)) return rc;
  if (enc && (int64_t)in.T * S > ((int64_t)1 << 31) - 1)
    return fail(GAQ_ERR_INVALID, std::string(in.who) + ": T x S must not exceed 2^31 - 1 rows for the encoder's launch");
  if (S == 0) return GAQ_OK;
  hipStream_t st = (hipStream_t)in.stream;
  g.obs = in.obs;
  if (enc) {
    // the features live in the handle's gradient scratch where a gradient call keeps its tape (grad_scratch's rule: the pointers move
    // only when a call needs more than every call before it)
    SeqEncPlan pl;
    pl.rows = (int64_t)n;
    double* spart; float* part;
    if (int rc = grad_scratch(*c.v.net, 1, n * (size_t)enc->width * sizeof(float), spart, part, pl.feat)) return rc;
    if (int rc = seq_encode(in, pl, st)) return rc;
    g.obs = pl.feat;
  }
  g.a = in.actions; g.done = in.done; g.h0 = in.h0;
  g.logp_out = in.logp_out; g.value_out = in.value_out; g.mean_out = in.mean_out; g.h_out = in.h_out;
  if constexpr (L) { g.c0 = in.c0; g.c_out = in.c_out; }
  g.S_src = S;
  if (!in.value_out) g.wv = nullptr;                              // V's parts are not summed where nobody reads them
  if constexpr (!L) {
    if (in.wide_form) return grad_launch(grad_seq_wide_kernel<false, false>, g, (int)std::min<int64_t>(g.ntiles, (int64_t)1 << 20), lds, st);
  }
  return grad_launch(grad_seq_kernel<L, false, false>, g, (int)std::min<int64_t>(g.ntiles, (int64_t)1 << 20), lds, st);
}

// the gradient of either cell and its idx form (the inputs span S_src columns, idx spans S words, stats_out is one double longer):
// checks, the plan of the scratch, [the encoder's forward,] the sequence kernel, the reduce [, the encoder's backward]
template <bool L>
int seq_grad_call(gaq_policy* p, const SeqIn& in) {
  const GradEnc* enc = in.enc;
  const bool gather = in.gather;
  const int32_t T = in.T;
  const int64_t S = in.S;
  int64_t S_src = in.S_src;
  SeqCall<L> c;
  if (int rc = seq_begin(c, p, in)) return rc;
  const std::string who = std::string(in.who) + ": ";
  SeqArgsT<L>& g = c.g;
  PolicyNet& net = *c.v.net;
  if (in.scale != in.scale) return fail(GAQ_ERR_INVALID, who + "scale is NaN");
  if (gather) {
    if (S > 0 && S_src < 1) return fail(GAQ_ERR_INVALID, who + "S_src must be at least 1");
    if (S_src > ((int64_t)1 << 31) - 1) return fail(GAQ_ERR_INVALID, who + "S_src must not exceed 2^31 - 1");
    if (S_src < 0) S_src = 0;                                     // (only with S = 0: sizes the spans below, nothing is launched)
  }
  // (the idx form's S may exceed S_src: repeated indices; the row list and its 32-bit count span T x S)
  if (enc && ((int64_t)T * S_src > ((int64_t)1 << 31) - 1 || (int64_t)T * S > ((int64_t)1 << 31) - 1))
    return fail(GAQ_ERR_INVALID, who + "T x S and T x S_src must not exceed 2^31 - 1 rows for the encoder's passes");
  const bool hasv = c.v.wv != nullptr;
  const size_t n = (size_t)T * (size_t)S_src, H = (size_t)g.net.width[0];
  const int64_t nv = hasv ? g.net.width[g.net.n_hidden - 1] + 1 : 0;
  std::vector<Span> ins = {{in.obs, n * (enc ? enc->in_dim : g.net.in_dim) * 4, SPAN_ROWS}, {in.actions, n * 16, SPAN_ROWS},
                           {in.done, n, SPAN_ROWS, 1}, {in.h0, (size_t)S_src * H * 4, SPAN_ROWS, 16}, {in.logp_old, n * 4, SPAN_ROWS},
                           {in.adv, n * 4, SPAN_ROWS}, {in.ret, n * 4, hasv ? SPAN_ROWS : SPAN_OPTIONAL}, {in.v_old, n * 4, SPAN_OPTIONAL}};
  if (L) ins.push_back({in.c0, (size_t)S_src * H * 4, SPAN_ROWS, 16});
  if (gather) ins.push_back({in.idx, (size_t)S * 4, SPAN_ROWS});
  std::vector<Span> outs = {{in.grad_out, (size_t)net.nw * 4, SPAN_ALWAYS}, {in.grad_value_out, (size_t)nv * 4, hasv ? SPAN_ALWAYS : SPAN_OPTIONAL},
                            {in.grad_log_std_out, 16, SPAN_ALWAYS}, {in.stats_out, gather ? 56u : 48u, SPAN_ALWAYS, 8}};
  if (enc) outs.push_back({in.grad_enc_out, (size_t)enc->nw * 4, SPAN_ALWAYS});
  bool wide = false, misaligned = false;
  if (int rc = check_span_nulls(ins, outs, S > 0, wide, misaligned)) return rc;
  // (a missing v_old is refused only with a value head, the pointers below only without one: the two never meet, in either order)
  if (int rc = check_ppo_hyper(who, in.clip_eps, in.vclip, in.vf_coef, in.ent_coef, hasv, in.v_old, S > 0)) return rc;
  if (!hasv && (in.ret || in.v_old || in.grad_value_out))
    return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head): ret, v_old and grad_value_out must be NULL without one");
  if (!c.v.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no log-probability");
  size_t lds = 0;
  if (int rc = seq_ready(c, in.who, true, wide, misaligned, ins, outs, lds, in.wide_form)) return rc;
  if (gather) {
    lds += kGradIdxBytes;
    if (lds > kGradLdsMax) return fail(GAQ_ERR_INVALID, who + "in_dim too large for the sequence kernel's LDS");
    if ((int64_t)T * S_src > ((int64_t)1 << 40)) return fail(GAQ_ERR_INVALID, who + "too many sequences or steps for one launch");
  }
  if (enc && grad_feat_lds(enc->trunk, gather) > kGradLdsMax)
    return fail(GAQ_ERR_INVALID, who + "obs_dim too large for the encoder gradient kernel's LDS");
  hipStream_t st = (hipStream_t)in.stream;
  if (S == 0) {                                                   // zeros to every output, no tile work
    HIP_TRY(hipMemsetAsync(in.grad_out, 0, sizeof(float) * (size_t)net.nw, st));
    if (in.grad_value_out) HIP_TRY(hipMemsetAsync(in.grad_value_out, 0, sizeof(float) * (size_t)nv, st));
    HIP_TRY(hipMemsetAsync(in.grad_log_std_out, 0, sizeof(float) * 4, st));
    HIP_TRY(hipMemsetAsync(in.stats_out, 0, sizeof(double) * (gather ? 7 : 6), st));
    if (enc) HIP_TRY(hipMemsetAsync(in.grad_enc_out, 0, sizeof(float) * (size_t)enc->nw, st));
    return GAQ_OK;
  }
  const int G = grad_groups(g.ntiles);
  // the scratch (grad_scratch) with the tape [G][T][64][H] (the LSTM: [2][H]) behind its fixed part and the encoder's plan behind the
  // tape: a graph captured after a call with the largest T (and S) stays valid
  g.pstride = grad_stride_max(net);
  const size_t tape_bytes = (size_t)G * (size_t)T * kTile * (L ? 2 : 1) * H * sizeof(float);
  SeqEncPlan pl = seq_enc_plan(T, S, S_src, gather, enc);
  if (int rc = grad_scratch(net, G, tape_bytes + pl.bytes, g.spart, g.part, g.tape)) return rc;
  pl.place(reinterpret_cast<char*>(g.tape) + tape_bytes);
  g.obs = in.obs;
  if (enc) {
    if (int rc = seq_encode(in, pl, st)) return rc;
    g.obs = pl.feat;
  }
  g.a = in.actions; g.done = in.done; g.h0 = in.h0; g.logp_old = in.logp_old; g.adv = in.adv; g.ret = in.ret; g.v_old = in.v_old;
  if constexpr (L) g.c0 = in.c0;
  g.clip = in.clip_eps; g.scale = in.scale; g.vclip = hasv ? in.vclip : 0.0f; g.vf_coef = hasv ? in.vf_coef : 0.0f;
  g.idx = in.idx; g.S_src = S_src;
  auto wide_launch = [&]() -> int {                              // (the wide form has a GRU's entry points only)
    if constexpr (L) return fail(GAQ_ERR_INVALID, who + "no wide form for the LSTM");
    else return grad_launch(gather ? grad_seq_wide_kernel<true, true> : grad_seq_wide_kernel<true, false>, g, G, lds, st);
  };
  if (in.wide_form) {
    if (int rc = wide_launch()) return rc;
  } else if (enc) {
    SeqArgsDx<L> gx{};
    static_cast<SeqArgsT<L>&>(gx) = g;
    gx.dfeat = pl.dfeat;
    if (int rc = grad_launch(gather ? grad_seq_kernel<L, true, true, true> : grad_seq_kernel<L, true, false, true>, gx, G, lds, st)) return rc;
  } else if (int rc = grad_launch(gather ? grad_seq_kernel<L, true, true> : grad_seq_kernel<L, true, false>, g, G, lds, st)) return rc;
  GradReduce r{};
  r.part = g.part; r.spart = g.spart; r.G = G; r.pstride = g.pstride; r.nw = net.nw; r.nv = nv; r.rows = (int64_t)T * S;
  r.ent = -(double)in.ent_coef * (double)in.scale * (double)T * (double)S;
  r.grad_out = in.grad_out; r.value_out = in.grad_value_out; r.stats_out = in.stats_out; r.log_std_out = in.grad_log_std_out;
  grad_route(r, true, 5, gather);
  if (int rc = grad_reduce(r, st)) return rc;
  return enc ? seq_encode_backward(in, pl, net, g.spart, st) : GAQ_OK;
}

// the encoder forms take either cell: the handle's view and its encoder into the record, and the handle's cell picks the call
template <bool Grad>
int seq_enc_call(gaq_policy* p, SeqIn& in) {
  GradNet v;
  GradEnc e;
  if (int rc = policy_grad_enc_seq_view(p, in.c0 || in.c_out, v, e)) return rc;
  in.view = &v; in.enc = &e;
  const auto call = Grad ? (e.lstm ? seq_grad_call<true> : seq_grad_call<false>) : (e.lstm ? seq_eval_call<true> : seq_eval_call<false>);
  return call(p, in);
}

}  // namespace

extern "C" {

int gaq_policy_eval_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done, const float* h0,
                            float* logp_out, float* value_out, float* mean_out, float* h_out, void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_eval_seq_dev"; in.T = T; in.S = S; in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0;
  in.logp_out = logp_out; in.value_out = value_out; in.mean_out = mean_out; in.h_out = h_out; in.stream = stream;
  return seq_eval_call<false>(p, in);
}

int gaq_policy_grad_ppo_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                const float* h0, const float* logp_old, const float* adv, const float* ret, const float* v_old,
                                float clip_eps, float vclip, float vf_coef, float ent_coef, float scale, float* grad_out,
                                float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_grad_ppo_seq_dev"; in.T = T; in.S = S; in.S_src = S; in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0;
  in.logp_old = logp_old; in.adv = adv; in.ret = ret; in.v_old = v_old;
  in.clip_eps = clip_eps; in.vclip = vclip; in.vf_coef = vf_coef; in.ent_coef = ent_coef; in.scale = scale;
  in.grad_out = grad_out; in.grad_value_out = grad_value_out; in.grad_log_std_out = grad_log_std_out; in.stats_out = stats_out; in.stream = stream;
  return seq_grad_call<false>(p, in);
}

int gaq_policy_grad_ppo_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                    const float* actions, const uint8_t* done, const float* h0, const float* logp_old, const float* adv,
                                    const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef,
                                    float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out,
                                    void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_grad_ppo_seq_idx_dev"; in.T = T; in.S = S; in.gather = true; in.idx = idx; in.S_src = S_src;
  in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0;
  in.logp_old = logp_old; in.adv = adv; in.ret = ret; in.v_old = v_old;
  in.clip_eps = clip_eps; in.vclip = vclip; in.vf_coef = vf_coef; in.ent_coef = ent_coef; in.scale = scale;
  in.grad_out = grad_out; in.grad_value_out = grad_value_out; in.grad_log_std_out = grad_log_std_out; in.stats_out = stats_out; in.stream = stream;
  return seq_grad_call<false>(p, in);
}

int gaq_policy_eval_lstm_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                 const float* h0, const float* c0, float* logp_out, float* value_out, float* mean_out, float* h_out,
                                 float* c_out, void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_eval_lstm_seq_dev"; in.T = T; in.S = S; in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0; in.c0 = c0;
  in.logp_out = logp_out; in.value_out = value_out; in.mean_out = mean_out; in.h_out = h_out; in.c_out = c_out; in.stream = stream;
  return seq_eval_call<true>(p, in);
}

int gaq_policy_grad_ppo_lstm_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                     const float* h0, const float* c0, const float* logp_old, const float* adv, const float* ret,
                                     const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                                     float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_grad_ppo_lstm_seq_dev"; in.T = T; in.S = S; in.S_src = S;
  in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0; in.c0 = c0;
  in.logp_old = logp_old; in.adv = adv; in.ret = ret; in.v_old = v_old;
  in.clip_eps = clip_eps; in.vclip = vclip; in.vf_coef = vf_coef; in.ent_coef = ent_coef; in.scale = scale;
  in.grad_out = grad_out; in.grad_value_out = grad_value_out; in.grad_log_std_out = grad_log_std_out; in.stats_out = stats_out; in.stream = stream;
  return seq_grad_call<true>(p, in);
}

int gaq_policy_grad_ppo_lstm_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                         const float* actions, const uint8_t* done, const float* h0, const float* c0, const float* logp_old,
                                         const float* adv, const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef,
                                         float ent_coef, float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out,
                                         double* stats_out, void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_grad_ppo_lstm_seq_idx_dev"; in.T = T; in.S = S; in.gather = true; in.idx = idx; in.S_src = S_src;
  in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0; in.c0 = c0;
  in.logp_old = logp_old; in.adv = adv; in.ret = ret; in.v_old = v_old;
  in.clip_eps = clip_eps; in.vclip = vclip; in.vf_coef = vf_coef; in.ent_coef = ent_coef; in.scale = scale;
  in.grad_out = grad_out; in.grad_value_out = grad_value_out; in.grad_log_std_out = grad_log_std_out; in.stats_out = stats_out; in.stream = stream;
  return seq_grad_call<true>(p, in);
}

// the wide recurrent learner: a GRU of up to 128 units; idx == NULL: contiguous columns (S_src is then S, stats_out 6 doubles)
int gaq_policy_eval_seq_wide_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                 const float* h0, float* logp_out, float* value_out, float* mean_out, float* h_out, void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_eval_seq_wide_dev"; in.wide_form = true; in.T = T; in.S = S; in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0;
  in.logp_out = logp_out; in.value_out = value_out; in.mean_out = mean_out; in.h_out = h_out; in.stream = stream;
  return seq_eval_call<false>(p, in);
}

int gaq_policy_grad_ppo_seq_wide_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                     const float* actions, const uint8_t* done, const float* h0, const float* logp_old, const float* adv,
                                     const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef,
                                     float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out,
                                     void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_grad_ppo_seq_wide_dev"; in.wide_form = true; in.T = T; in.S = S; in.gather = idx != nullptr; in.idx = idx;
  in.S_src = idx ? S_src : S;
  in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0;
  in.logp_old = logp_old; in.adv = adv; in.ret = ret; in.v_old = v_old;
  in.clip_eps = clip_eps; in.vclip = vclip; in.vf_coef = vf_coef; in.ent_coef = ent_coef; in.scale = scale;
  in.grad_out = grad_out; in.grad_value_out = grad_value_out; in.grad_log_std_out = grad_log_std_out; in.stats_out = stats_out; in.stream = stream;
  return seq_grad_call<false>(p, in);
}

// either cell behind an encoder
int gaq_policy_eval_enc_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                const float* h0, const float* c0, float* logp_out, float* value_out, float* mean_out, float* h_out,
                                float* c_out, void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_eval_enc_seq_dev"; in.T = T; in.S = S; in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0; in.c0 = c0;
  in.logp_out = logp_out; in.value_out = value_out; in.mean_out = mean_out; in.h_out = h_out; in.c_out = c_out; in.stream = stream;
  return seq_enc_call<false>(p, in);
}

int gaq_policy_grad_ppo_enc_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                    const float* h0, const float* c0, const float* logp_old, const float* adv, const float* ret,
                                    const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                                    float* grad_out, float* grad_enc_out, float* grad_value_out, float* grad_log_std_out, double* stats_out,
                                    void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_grad_ppo_enc_seq_dev"; in.T = T; in.S = S; in.S_src = S;
  in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0; in.c0 = c0;
  in.logp_old = logp_old; in.adv = adv; in.ret = ret; in.v_old = v_old;
  in.clip_eps = clip_eps; in.vclip = vclip; in.vf_coef = vf_coef; in.ent_coef = ent_coef; in.scale = scale;
  in.grad_out = grad_out; in.grad_enc_out = grad_enc_out; in.grad_value_out = grad_value_out; in.grad_log_std_out = grad_log_std_out;
  in.stats_out = stats_out; in.stream = stream;
  return seq_enc_call<true>(p, in);
}

int gaq_policy_grad_ppo_enc_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                        const float* actions, const uint8_t* done, const float* h0, const float* c0, const float* logp_old,
                                        const float* adv, const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef,
                                        float ent_coef, float scale, float* grad_out, float* grad_enc_out, float* grad_value_out,
                                        float* grad_log_std_out, double* stats_out, void* stream) {
  SeqIn in{};
  in.who = "gaq_policy_grad_ppo_enc_seq_idx_dev"; in.T = T; in.S = S; in.gather = true; in.idx = idx; in.S_src = S_src;
  in.obs = obs; in.actions = actions; in.done = done; in.h0 = h0; in.c0 = c0;
  in.logp_old = logp_old; in.adv = adv; in.ret = ret; in.v_old = v_old;
  in.clip_eps = clip_eps; in.vclip = vclip; in.vf_coef = vf_coef; in.ent_coef = ent_coef; in.scale = scale;
  in.grad_out = grad_out; in.grad_enc_out = grad_enc_out; in.grad_value_out = grad_value_out; in.grad_log_std_out = grad_log_std_out;
  in.stats_out = stats_out; in.stream = stream;
  return seq_enc_call<true>(p, in);
}

}  // extern "C"

