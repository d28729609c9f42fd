// gaq_policy_grad_seq.hip -- the learner's passes over stored SEQUENCES for a GRU policy (include/gaq.h "gradients of a recurrent policy"):
// gaq_policy_eval_seq_dev (log-probabilities, V, means and the final state of T steps of S sequences, the rollout's bits) and
// gaq_policy_grad_ppo_seq_dev (the truncated-BPTT gradient of gaq_policy_grad_ppo_ac_dev's loss).  Of gaq_policy.hip it uses the net
// record gaq_grad.hpp declares (policy_grad_seq_view), of gaq_policy_grad.hip the span checks and the split into workgroups.
//
// One kernel template, grad_seq_kernel<Bwd>, 4 waves per workgroup, one 64-sequence tile at a time; sequence e of the tile lives in
// column seq_col(e) = pol_col(e) of every LDS row (stride 68 floats, as in gaq_policy_grad.hip).  The stages of the feed-forward
// gradient kernel are restated here, not shared: that kernel keeps its recorded resource lines.
//   forward   t ascending: the observation is staged as pol_stage_obs stages it; hin_t = h_{t-1} with the rows of done[t-1] (and dead
//             lanes) 0 by select; the cell is gru_cell's arithmetic chunk by chunk -- r and z start at b_i + b_h and take the x products
//             then the h products, n_x and n_h apart, n = tanhf(fmaf(r, n_h, n_x)), h' = fmaf(z, hin - n, n) -- so h_t is the rollout's
//             bits.  <false> (eval) then runs the head and the row stage; <true> writes h_t to the workgroup's tape [T][64][H].
//   backward  t descending (<true>): h_t and hin_t come back from the tape, the head is recomputed, the row stage forms the five deltas
//             of gaq_policy_grad_ppo_ac_dev's loss, the head is backpropagated with that kernel's code shape down to dh_t (no activation
//             derivative on the cell's output); the gates are recomputed with the forward's code and, in the accumulator registers,
//               da_n = dh (1 - z)(1 - n^2), da_z = dh (hin - n) z (1 - z), da_r = da_n n_h r (1 - r), dn_h = da_n r, direct = dh z
//             go to four planes of LDS (over the rows the head used) and to the carried dh; dW_ih = [da_r; da_z; da_n] x^T and
//             dW_hh = [da_r; da_z; dn_h] hin^T are MFMAs over the tile's 64 columns, the biases row sums in ascending column order; then
//             dh_{t-1} = direct + W_hh^T [da_r; da_z; dn_h] (the packed W_hh read 16 bytes per lane), 0 by select where done[t-1].
// LDS = 8.25 KiB + 272 B x (kx + 2 H + max(4 H, H + head widths)) for <true>: 118.75 KiB at 18-GRU64-64-64.
// Partials: every word of the workgroup's partial is owned by one lane for every (tile, t); the first (tile, t) stores, the others add;
// grad_seq_reduce_kernel sums the G partials in ascending order in fp64 and rounds once.  No atomics; dead lanes contribute exactly 0
// (their deltas are 0 and every activation is finite); nothing is read past S.
#include "gaq_host.hpp"
#include "gaq_norm.hpp"
#include "gaq_grad.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kSeqWaves = 4;
constexpr int kSeqBlock = kSeqWaves * kTile;
constexpr int kSeqStride = 68;                                    // floats per LDS row
constexpr int kSeqStats = 10;                                     // doubles per workgroup, gaq_policy_grad.hip's kGradStatsAc
constexpr int kSeqND = 5;                                         // rows of dlt: the 4 outputs' deltas and V's
constexpr int kSeqHeadBytes = (kSeqND + 4 + 4) * kTile * 4 + kSeqStats * kTile * 8;   // dlt, outs, V's parts, the statistics' lanes
constexpr size_t kSeqLdsMax = 160 * 1024;
constexpr float kSeqTwoLn2Pi = 3.67575413281869f;

struct SeqArgs {
  PolicyDev net;                  // width[0] = H (the cell), width[1 ..] the head's layers
  int32_t off_hh;                 // float offset of W_hh' in net.w
  PolObsNorm nm;                  // tab = nullptr: no normaliser
  int32_t T;
  int64_t S, ntiles;
  const float* obs;               // [T, S, D]
  const float* a;                 // [T, S, 4] or nullptr (eval without logp)
  const uint8_t* done;            // [T, S]
  const float* h0;                // [S, H]
  const float *logp_old, *adv;    // [T, S]
  const float *ret, *v_old;       // [T, S] or nullptr
  const float* wv;                // the value head (last width weights, bias) or nullptr
  float clip, scale, vclip, vf_coef;
  float log_std[4], inv_std[4];
  float *logp_out, *value_out, *mean_out, *h_out;   // eval
  float* part;                    // [G][pstride]
  double* spart;                  // [G][kSeqStats]
  float* tape;                    // [G][T][64][H]
  int64_t pstride;
};

__device__ __forceinline__ int seq_col(int e) { return (e & 15) * 4 + (e >> 4); }
__device__ __forceinline__ int seq_env(int col) { return (col & 3) * 16 + (col >> 2); }
__device__ __forceinline__ float seq_actd(int act, float h) { return act == 0 ? __builtin_fmaf(-h, h, 1.0f) : (h > 0.0f ? 1.0f : 0.0f); }
__device__ __forceinline__ float seq_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ void seq_put(float* p, float v, bool first) { *p = first ? v : *p + v; }
__device__ __forceinline__ void seq_put4(float* p, const f32x4& v, bool first) {
  f32x4* q = reinterpret_cast<f32x4*>(p);
  *q = first ? v : *q + v;
}

// the observations of step-row `base` .. + nlive - 1 -> X: dead columns 0, padded inputs -0, the rows up to a multiple of 16 0
__device__ __forceinline__ void seq_stage_obs(float* X, const float* obs, const PolObsNorm& nm, int64_t base, int nlive, int D, int tid) {
  const int kin = (D + 3) & ~3, kx = (D + 15) & ~15;
  for (int f = tid; f < kTile * kx; f += kSeqBlock) {
    const int e = f / kx, k = f - e * kx;
    float v = k >= kin ? 0.0f : -0.0f;
    if (k < D) {
      v = 0.0f;
      if (e < nlive) {
        v = obs[(base + e) * D + k];
        if (nm.tab) v = nm(v, k);
      }
    }
    X[k * kSeqStride + seq_col(e)] = v;
  }
}

// this lane's row of an [., H] array (keep = false: read as 0) -> the H rows of R, lane = sequence, 4 units per 16-byte load
__device__ __forceinline__ void seq_stage_rows(float* R, const float* row, bool keep, int hid, uint32_t lane, int wave) {
  for (int q = wave; q < hid / 4; q += kSeqWaves) {
    const f32x4 v = keep ? *reinterpret_cast<const f32x4*>(row + 4 * q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r) R[(4 * q + r) * kSeqStride + seq_col((int)lane)] = v[r];
  }
}

// the chunks c, c + cs, c + 2 cs -- one per gate -- of one product of the cell (`in` inputs: the rows of A, zero-padded to a multiple
// of 4) into acc[0], acc[1] and acc[JL]: cell_kloop's order of operations (k ascending, each MFMA a k-ordered fmaf chain)
template <int JL>
__device__ __forceinline__ void seq_kloop(const float* __restrict__ wl, int in, int c, int cs, const float* A, uint32_t lane,
                                          f32x4 (&acc)[4][4]) {
  const int h = (int)(lane >> 4);
  const float* arow = A + h * kSeqStride + (lane & 15) * 4;
  const int kfull = in & ~3;
  for (int k0 = 0; k0 < kfull; k0 += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + k0 * kSeqStride);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int s = j == 2 ? JL : j;
      const float a = wl[((c + j * cs) * in + k0) * 16 + lane];
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[s][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[s][eb], 0, 0, 0);
    }
  }
  if (kfull < in) {                                               // the x product's last, partial k-step: no weight past in - 1 is read
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + kfull * kSeqStride);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int s = j == 2 ? JL : j;
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
  seq_kloop<2>(wih, D, c, hc, X, lane, acc);
  seq_kloop<3>(whh, hid, c, hc, Hin, lane, acc);
}

// this wave's chunk (widths <= 64: at most one) of one head layer: rows 0 .. in-1 of A -> act(bias + W a) in the rows of O
__device__ __forceinline__ void seq_fwd_layer(const float* __restrict__ wl, int in, int width, int act, int wave, const float* A, float* O,
                                              uint32_t lane) {
  if (wave >= width / 16) return;
  const int h = (int)(lane >> 4);
  const float* b = wl + width * in + wave * 16 + 4 * h;
  const f32x4 b4 = {b[0], b[1], b[2], b[3]};
  f32x4 acc[4] = {b4, b4, b4, b4};
  const float* arow = A + h * kSeqStride + (lane & 15) * 4;
  for (int k0 = 0; k0 < in; k0 += 4) {                            // (in is H or a head width: a multiple of 16)
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + k0 * kSeqStride);
    const float a = wl[(wave * in + k0) * 16 + lane];
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[eb], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const f32x4 v = {pol_act(act, acc[0][r]), pol_act(act, acc[1][r]), pol_act(act, acc[2][r]), pol_act(act, acc[3][r])};
    *reinterpret_cast<f32x4*>(O + (wave * 16 + 4 * h + r) * kSeqStride + (lane & 15) * 4) = v;
  }
}

// NK blocks of dW: the 16 delta rows at `drows` (chunk uc of the packed layout) x inputs 16 (kc0 + t) .. + 15 (rows of A), summed over
// the tile's 64 columns, into the partial's packed layout [uc][k][16]; inputs >= in (the observation's padding) are left out
template <int NK>
__device__ __forceinline__ void seq_dw_blocks(const float* drows, const float* A, int in, int uc, int kc0, uint32_t lane, float* pw,
                                              bool first) {
  const int n = (int)(lane & 15), kk = (int)(lane >> 4);
  f32x4 acc[NK];
#pragma unroll
  for (int t = 0; t < NK; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* drow = drows + n * kSeqStride + 4 * kk;
  const float* arow = A + (kc0 * 16 + n) * kSeqStride + 4 * kk;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(drow + 16 * j);
    f32x4 bv[NK];
#pragma unroll
    for (int t = 0; t < NK; ++t) bv[t] = *reinterpret_cast<const f32x4*>(arow + t * 16 * kSeqStride + 16 * j);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int t = 0; t < NK; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[t][i], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < NK; ++t) {
    const int k = (kc0 + t) * 16 + n;
    if (k < in) seq_put4(pw + ((int64_t)uc * in + k) * 16 + 4 * kk, acc[t], first);
  }
}
__device__ __forceinline__ void seq_dw(const float* drows, const float* A, int in, int uc, uint32_t lane, float* pw, bool first) {
  const int nkc = (in + 15) / 16;
#pragma unroll 1
  for (int kc0 = 0; kc0 < nkc; kc0 += 4) {
    switch (nkc - kc0 < 4 ? nkc - kc0 : 4) {
      case 1: seq_dw_blocks<1>(drows, A, in, uc, kc0, lane, pw, first); break;
      case 2: seq_dw_blocks<2>(drows, A, in, uc, kc0, lane, pw, first); break;
      case 3: seq_dw_blocks<3>(drows, A, in, uc, kc0, lane, pw, first); break;
      default: seq_dw_blocks<4>(drows, A, in, uc, kc0, lane, pw, first); break;
    }
  }
}
// the sum of an LDS row's 64 columns in ascending order
__device__ __forceinline__ float seq_row_sum(const float* row) {
  float s = 0.0f;
#pragma unroll 4
  for (int q = 0; q < kTile / 4; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
    s = ((s + v[0]) + v[1]) + v[2] + v[3];
  }
  return s;
}

// `g` must stay the kernel's first and only argument: the row stage reads its own members of it at offset 0 of the kernel-argument
// segment, as grad_kernel's does.
template <bool Bwd>
__global__ __launch_bounds__(kSeqBlock) void grad_seq_kernel(SeqArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dlt = reinterpret_cast<float*>(smem);                    // [5][64] the head's delta, sequence e at column seq_col(e)
  float* outs = dlt + kSeqND * kTile;                             // [4][64] the head's sums, sequence e at e
  float* vsum = outs + 4 * kTile;                                 // [4][64] the waves' parts of V
  double* red = reinterpret_cast<double*>(smem + (kSeqND + 8) * kTile * 4);   // [kSeqStats][64]
  float* X = reinterpret_cast<float*>(smem + kSeqHeadBytes);      // [kx][68] the observation
  const PolicyDev& net = g.net;
  const int D = net.in_dim, kx = (D + 15) & ~15, nh = net.n_hidden, act = net.hidden_act, H = net.width[0], hc = H / 16;
  const int w1 = nh > 1 ? net.width[1] : 0;
  float* Hin = X + kx * kSeqStride;                               // [H][68] hin_t
  [[maybe_unused]] float* DH = Hin + H * kSeqStride;              // Bwd: [H][68] the carried dh
  float* P = Hin + (Bwd ? 2 : 1) * H * kSeqStride;                // h_t, then the head's layers; Bwd: then the four delta planes of H rows
  auto Hl = [&](int l) { return P + ((l > 0 ? H : 0) + (l > 1 ? w1 : 0)) * kSeqStride; };   // layer l's rows (0: the cell's h_t)
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
  if (Bwd && wave == 0) {
#pragma unroll
    for (int s = 0; s < kSeqStats; ++s) red[s * kTile + lane] = 0.0;
  }

  // the head over h_t in Hl(0): its layers, the 4 sums and V's parts; ends after the barrier that follows them
  auto head_forward = [&]() {
#pragma unroll 1
    for (int l = 1; l < nh; ++l) {
      seq_fwd_layer(net.w + net.off[l], net.width[l - 1], net.width[l], act, wave, Hl(l - 1), Hl(l), lane);
      __syncthreads();
    }
    const float* ycol = Hl(nh - 1) + seq_col((int)lane);
    {
      float s = wo[lw * 4 + wave];
#pragma unroll 8
      for (int u = 0; u < lw; ++u) s = __builtin_fmaf(wo[u * 4 + wave], ycol[u * kSeqStride], s);
      outs[wave * kTile + lane] = s;
    }
    if (hasv) {                                                   // this wave's quarter of V: policy_value_part's chain
      const int q = lw / kSeqWaves;
      float v = 0.0f;
#pragma unroll 8
      for (int u = wave * q; u < (wave + 1) * q; ++u) v = __builtin_fmaf(g.wv[u], ycol[u * kSeqStride], v);
      vsum[wave * kTile + lane] = v;
    }
    __syncthreads();
  };

#pragma unroll 1
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t row0 = tile * kTile;
    const int nlive = (int)((S - row0) < kTile ? (S - row0) : kTile);
    const bool live = (int)lane < nlive;
    // ---- the forward sweep -------------------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      const int64_t base = (int64_t)t * S + row0;
      seq_stage_obs(X, g.obs, g.nm, base, nlive, D, tid);
      if (t == 0) {
        seq_stage_rows(Hin, g.h0 + (row0 + lane) * H, live, H, lane, wave);
      } else {                                                    // hin_t = h_{t-1} (still in Hl(0)), 0 where done[t-1] and in dead columns
        for (int f = tid; f < H * kTile; f += kSeqBlock) {
          const int u = f >> 6, col = f & 63, e = seq_env(col);
          const bool keep = e < nlive && !g.done[base - S + e];
          Hin[u * kSeqStride + col] = keep ? P[u * kSeqStride + col] : 0.0f;
        }
      }
      __syncthreads();
      if (wave < hc) {
        const int u0 = wave * 16 + 4 * h4;
        f32x4 acc[4][4];
        seq_gates(net, g.off_hh, wave, X, Hin, lane, acc);
        f32x4 hn[4];
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float hold = Hin[(u0 + r) * kSeqStride + n16 * 4 + eb];
            const float rg = seq_sigmoid(acc[0][eb][r]), zg = seq_sigmoid(acc[1][eb][r]);
            const float n = tanhf(__builtin_fmaf(rg, acc[3][eb][r], acc[2][eb][r]));
            hn[eb][r] = __builtin_fmaf(zg, hold - n, n);
          }
          const int e = eb * 16 + n16;
          if (e < nlive) {
            if constexpr (Bwd) {
              *reinterpret_cast<f32x4*>(tape + ((int64_t)t * kTile + e) * H + u0) = hn[eb];
            } else if (t == T - 1 && g.h_out) {
              const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
              *reinterpret_cast<f32x4*>(g.h_out + (row0 + e) * H + u0) = g.done[base + e] ? zero : hn[eb];
            }
          }
        }
        if (!Bwd || t + 1 < T) {                                   // (the backward sweep reloads h_{T-1} from the tape)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 v = {hn[0][r], hn[1][r], hn[2][r], hn[3][r]};
            *reinterpret_cast<f32x4*>(P + (u0 + r) * kSeqStride + n16 * 4) = v;
          }
        }
      }
      __syncthreads();
      if constexpr (!Bwd) {
        head_forward();
        if (wave == 0 && live) {                                  // lane = sequence
          const auto& r = *(const __attribute__((address_space(4))) SeqArgs*)__builtin_amdgcn_kernarg_segment_ptr();
          const int e = (int)lane;
          const int64_t i = base + e;
          float m[4];
#pragma unroll
          for (int o = 0; o < 4; ++o) {
            m[o] = outs[o * kTile + e];
            if (net.out_tanh) m[o] = tanhf(m[o]);
          }
          if (r.logp_out) {
            float z[4], lp = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * r.inv_std[o];
#pragma unroll
            for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -r.log_std[o]);
            r.logp_out[i] = lp - kSeqTwoLn2Pi;
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
        seq_stage_obs(X, g.obs, g.nm, base, nlive, D, tid);
        if (t == 0) seq_stage_rows(Hin, g.h0 + (row0 + lane) * H, live, H, lane, wave);
        else seq_stage_rows(Hin, tape + ((int64_t)(t - 1) * kTile + lane) * H, live && !g.done[base - S + lane], H, lane, wave);
        seq_stage_rows(P, tape + ((int64_t)t * kTile + lane) * H, live, H, lane, wave);
        __syncthreads();
        head_forward();
        if (wave == 0) {                                          // lane = sequence: gaq_policy_grad_ppo_ac_dev's row stage
          const auto& r = *(const __attribute__((address_space(4))) SeqArgs*)__builtin_amdgcn_kernarg_segment_ptr();
          const int e = (int)lane;
          const int64_t i = base + e;
          float d[kSeqND];                                        // the head's delta (already times scale)
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) d[o] = 0.0f;
          if (live) {
            float m[4], dm[4], z[4], lp = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              m[o] = outs[o * kTile + e];
              if (net.out_tanh) m[o] = tanhf(m[o]);
              dm[o] = net.out_tanh ? __builtin_fmaf(-m[o], m[o], 1.0f) : 1.0f;
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * r.inv_std[o];
#pragma unroll
            for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -r.log_std[o]);
            lp -= kSeqTwoLn2Pi;
            const float x = lp - r.logp_old[i], rt = expf(x), adv = r.adv[i];
            const float s1 = rt * adv, s2 = fminf(fmaxf(rt, 1.0f - r.clip), 1.0f + r.clip) * adv;
            const float dl = s1 <= s2 ? -adv * rt : 0.0f;          // dL / dlogp
            red[e] += (double)-fminf(s1, s2);
            red[kTile + e] += s2 < s1 ? 1.0 : 0.0;
            red[2 * kTile + e] += (double)rt - 1.0 - (double)x;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              d[o] = r.scale * dl * z[o] * r.inv_std[o] * dm[o];
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
          for (int o = 0; o < kSeqND; ++o) dlt[o * kTile + seq_col(e)] = d[o];
        }
        __syncthreads();
        // the 4-output layer and the value head: thread u owns unit u of what they read -- dWo[u][:] and dwv[u], then its row becomes
        // delta (with the activation's derivative only where the row is a head layer's, not the cell's h_t); 5 more threads sum dbo, dbv
        float* pv = part + net.off[nh] + (lw + 1) * 4;             // the value head's words follow the packed weights
        if (tid < lw) {
          float* yrow = Hl(nh - 1) + tid * kSeqStride;
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
              nv[c] = nh > 1 ? s * seq_actd(act, hv[c]) : s;
            }
            *reinterpret_cast<f32x4*>(yrow + 4 * q) = nv;
          }
#pragma unroll
          for (int o = 0; o < 4; ++o) seq_put(part + net.off[nh] + tid * 4 + o, gw[o], first);
          if (hasv) seq_put(pv + tid, gw[4], first);
        } else if (tid >= kSeqBlock - kSeqND && (tid < kSeqBlock - 1 || hasv)) {
          const int o = tid - (kSeqBlock - kSeqND);
          float s = 0.0f;
          for (int c = 0; c < kTile; ++c) s += dlt[o * kTile + c];
          seq_put(o < 4 ? part + net.off[nh] + lw * 4 + o : pv + lw, s, first);
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
          if (wave < width / 16) seq_dw(dl + wave * 16 * kSeqStride, A, in, wave, lane, pw, first);
          if (tid < width) seq_put(pw + width * in + tid, seq_row_sum(dl + tid * kSeqStride), first);
          __syncthreads();                                        // dW_l has consumed the layer's input
          if (wave < in / 16) {
            const int kc = wave;
            f32x4 acc[4];
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) acc[eb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            for (int uch = 0; uch < width / 16; ++uch) {
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + ((int64_t)uch * in + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(dl + (uch * 16 + 4 * h4 + i) * kSeqStride + n16 * 4);
#pragma unroll
                for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              f32x4* pos = reinterpret_cast<f32x4*>(A + (kc * 16 + 4 * h4 + r) * kSeqStride + n16 * 4);
              if (l > 1) {
                const f32x4 hv = *pos;
                const f32x4 nv = {acc[0][r] * seq_actd(act, hv[0]), acc[1][r] * seq_actd(act, hv[1]), acc[2][r] * seq_actd(act, hv[2]),
                                  acc[3][r] * seq_actd(act, hv[3])};
                *pos = nv;
              } else {
                const f32x4 nv = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
                *pos = nv;
              }
            }
          }
          __syncthreads();
        }
        // the cell: Hl(0) now holds the head's dh_t.  Each lane reads its 16 words of it (and of the carried dh) before it writes the
        // planes, whose first H rows are those very rows; the other planes lie over the head's layers, which are spent.
        if (wave < hc) {
          const int u0 = wave * 16 + 4 * h4;
          f32x4 acc[4][4];
          seq_gates(net, g.off_hh, wave, X, Hin, lane, acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int off = (u0 + r) * kSeqStride + n16 * 4;
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
            *reinterpret_cast<f32x4*>(P + H * kSeqStride + off) = daz;
            *reinterpret_cast<f32x4*>(P + 2 * H * kSeqStride + off) = dan;
            *reinterpret_cast<f32x4*>(P + 3 * H * kSeqStride + off) = dnh;
            *reinterpret_cast<f32x4*>(DH + off) = dir;
          }
        }
        __syncthreads();
        // dW_ih = [da_r; da_z; da_n] x^T and dW_hh = [da_r; da_z; dn_h] hin^T in the packed layout (chunk uc = gate * H/16 + c), the
        // biases: b_ih's and b_hh's r and z words take the same sum, the n words those of da_n and of dn_h
        {
          float* pih = part + net.off[0];
          float* phh = part + g.off_hh;
#pragma unroll 1
          for (int uc = wave; uc < 3 * hc; uc += kSeqWaves) {
            seq_dw(P + uc * 16 * kSeqStride, X, D, uc, lane, pih, first);
            seq_dw(P + (uc < 2 * hc ? uc : uc + hc) * 16 * kSeqStride, Hin, H, uc, lane, phh, first);
          }
          if (tid < 4 * H) {
            const float s = seq_row_sum(P + tid * kSeqStride);
            if (tid < 3 * H) seq_put(pih + 3 * H * D + tid, s, first);
            if (tid < 2 * H) seq_put(phh + 3 * H * H + tid, s, first);
            if (tid >= 3 * H) seq_put(phh + 3 * H * H + tid - H, s, first);
          }
        }
        // dh_{t-1} = direct + W_hh^T [da_r; da_z; dn_h], 0 where done[t-1] (and in dead columns); nothing flows into h0
        if (t > 0 && wave < hc) {
          const float* whh = net.w + g.off_hh;
          const int kc = wave;
          f32x4 acc[4];
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) acc[eb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          for (int uch = 0; uch < 3 * hc; ++uch) {
            const float* drows = P + (uch < 2 * hc ? uch : uch + hc) * 16 * kSeqStride;
            const f32x4 wv = *reinterpret_cast<const f32x4*>(whh + ((int64_t)uch * H + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(drows + (4 * h4 + i) * kSeqStride + n16 * 4);
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
            }
          }
          bool cut[4];
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) {
            const int e = eb * 16 + n16;
            cut[eb] = e >= nlive || g.done[base - S + e] != 0;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            f32x4* pos = reinterpret_cast<f32x4*>(DH + (kc * 16 + 4 * h4 + r) * kSeqStride + n16 * 4);
            const f32x4 dir = *pos;
            const f32x4 nv = {cut[0] ? 0.0f : acc[0][r] + dir[0], cut[1] ? 0.0f : acc[1][r] + dir[1], cut[2] ? 0.0f : acc[2][r] + dir[2],
                              cut[3] ? 0.0f : acc[3][r] + dir[3]};
            *pos = nv;
          }
        }
        __syncthreads();                                          // X, hin and the planes are read before the next step is staged
      }
    }
  }

  if constexpr (Bwd) {
    if (tid < kSeqStats) {                                        // the 64 lanes in ascending order
      double s = 0.0;
      for (int e = 0; e < kTile; ++e) s += red[tid * kTile + e];
      g.spart[(int64_t)blockIdx.x * kSeqStats + tid] = s;
    }
  }
}

// grad_reduce_ac_kernel's twin: grad_out[j] = the G partials of word j summed in ascending order in fp64, rounded once; the words
// nw .. nw + nv - 1 are the value head's (nv = 0: none).  stats_out = the sums 0 .. 2, 7, 8, then `rows`; log_std_out = the sums 3 .. 6
// plus the entropy bonus's -ent_coef * scale * rows (`ent`, formed in fp64 by the host), added in fp64 before the one rounding
__global__ __launch_bounds__(256) void grad_seq_reduce_kernel(const float* __restrict__ part, const double* __restrict__ spart, int G,
                                                              int64_t pstride, int64_t nw, int64_t nv, int64_t rows, double ent,
                                                              float* __restrict__ grad_out, float* __restrict__ value_out,
                                                              double* __restrict__ stats_out, float* __restrict__ log_std_out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < nw + nv) {
    double s = 0.0;
    for (int gi = 0; gi < G; ++gi) s += (double)part[(int64_t)gi * pstride + j];
    if (j < nw) grad_out[j] = (float)s;
    else value_out[j - nw] = (float)s;
  }
  if (blockIdx.x == 0 && threadIdx.x < kSeqStats) {
    const int k = (int)threadIdx.x;
    double s = 0.0;
    for (int gi = 0; gi < G; ++gi) s += spart[(int64_t)gi * kSeqStats + k];
    if (k < 3) stats_out[k] = s;
    else if (k < 7) log_std_out[k - 3] = (float)(s + ent);
    else if (k < 9) stats_out[k - 4] = s;
    else stats_out[5] = (double)rows;
  }
}

size_t seq_lds(const PolicyDev& pd, bool bwd) {
  const int H = pd.width[0];
  int head = H;
  for (int l = 1; l < pd.n_hidden; ++l) head += pd.width[l];
  const int rows = ((pd.in_dim + 15) & ~15) + (bwd ? 2 : 1) * H + (bwd ? std::max(4 * H, head) : head);
  return (size_t)kSeqHeadBytes + (size_t)rows * kSeqStride * 4;
}

// the arguments both calls share, checked: T, S, the handle's view, log_std
struct SeqCall {
  const char* who;
  GradNet v;
  SeqArgs g{};
};

int seq_begin(SeqCall& c, gaq_policy* p, int32_t T, int64_t S) {
  const std::string who = std::string(c.who) + ": ";
  if (int rc = policy_grad_seq_view(p, c.v)) return rc;
  if (T < 1) return fail(GAQ_ERR_INVALID, who + "T must be at least 1");
  if (S < 0) return fail(GAQ_ERR_INVALID, who + "S must not be negative");
  const PolicyNet& net = *c.v.net;
  SeqArgs& g = c.g;
  g.net = net.pd; g.off_hh = c.v.off_hh; g.nm = policy_norm_dev(net.norm);
  g.T = T; g.S = S; g.ntiles = (S + kTile - 1) / kTile;
  for (int k = 0; k < 4; ++k) {
    g.log_std[k] = c.v.log_std ? c.v.log_std[k] : 0.0f;
    g.inv_std[k] = (float)std::exp(-(double)g.log_std[k]);
  }
  g.wv = c.v.wv;
  return GAQ_OK;
}

// the checks every call ends with (alignment, overlaps, sizes), then the device
int seq_ready(const SeqCall& c, bool bwd, bool wide, bool misaligned, const std::vector<Span>& in, const std::vector<Span>& out, size_t& lds) {
  const std::string who = std::string(c.who) + ": ";
  if (misaligned)
    return fail(GAQ_ERR_INVALID, who + "pointers must be 4-byte aligned (h0" + (bwd ? "" : ", h_out") + ": 16" + (wide && bwd ? ", stats_out: 8" : "") + ")");
  if (int rc = check_overlap(c.who, in, out)) return rc;
  lds = seq_lds(c.g.net, bwd);
  if (lds > kSeqLdsMax) return fail(GAQ_ERR_INVALID, who + "in_dim too large for the sequence kernel's LDS");
  if (c.g.ntiles > ((int64_t)1 << 31) - 1 || (int64_t)c.g.T * c.g.S > ((int64_t)1 << 40))
    return fail(GAQ_ERR_INVALID, who + "too many sequences or steps for one launch");
  HIP_TRY(hipSetDevice(c.v.net->device));
  return GAQ_OK;
}

template <bool Bwd>
int seq_launch(const SeqArgs& g, int G, size_t lds, hipStream_t st) {
  if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void*)&grad_seq_kernel<Bwd>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(grad_seq_kernel<Bwd>, dim3((unsigned)G), dim3(kSeqBlock), lds, st, g);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

}  // namespace

extern "C" {

int gaq_policy_eval_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done, const float* h0,
                            float* logp_out, float* value_out, float* mean_out, float* h_out, void* stream) {
  SeqCall c{"gaq_policy_eval_seq_dev"};
  if (int rc = seq_begin(c, p, T, S)) return rc;
  SeqArgs& g = c.g;
  const size_t n = (size_t)T * (size_t)S, H = (size_t)g.net.width[0];
  const std::vector<Span> in = {{obs, n * g.net.in_dim * 4, SPAN_ROWS}, {actions, n * 16, logp_out ? SPAN_ROWS : SPAN_OPTIONAL},
                                {done, n, SPAN_ROWS, 1}, {h0, (size_t)S * H * 4, SPAN_ROWS, 16}};
  const std::vector<Span> out = {{logp_out, n * 4, SPAN_OPTIONAL}, {value_out, n * 4, SPAN_OPTIONAL}, {mean_out, n * 16, SPAN_OPTIONAL},
                                 {h_out, (size_t)S * H * 4, SPAN_OPTIONAL, 16}};
  bool wide = false, misaligned = false;
  if (int rc = check_span_nulls(in, out, S > 0, wide, misaligned)) return rc;
  if (value_out && !c.v.wv)
    return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head): the actor-critic passes need V on the policy's trunk");
  if (logp_out && !c.v.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no log-probability");
  size_t lds = 0;
  if (int rc = seq_ready(c, false, wide, misaligned, in, out, lds)) return rc;
  if (S == 0) return GAQ_OK;
  g.obs = obs; g.a = actions; g.done = done; g.h0 = h0;
  g.logp_out = logp_out; g.value_out = value_out; g.mean_out = mean_out; g.h_out = h_out;
  if (!value_out) g.wv = nullptr;                                 // V's parts are not summed where nobody reads them
  return seq_launch<false>(g, (int)std::min<int64_t>(g.ntiles, (int64_t)1 << 20), lds, (hipStream_t)stream);
}

int gaq_policy_grad_ppo_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                const float* h0, const float* logp_old, const float* adv, const float* ret, const float* v_old,
                                float clip_eps, float vclip, float vf_coef, float ent_coef, float scale, float* grad_out,
                                float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  SeqCall c{"gaq_policy_grad_ppo_seq_dev"};
  if (int rc = seq_begin(c, p, T, S)) return rc;
  const std::string who = std::string(c.who) + ": ";
  SeqArgs& g = c.g;
  PolicyNet& net = *c.v.net;
  if (scale != scale) return fail(GAQ_ERR_INVALID, who + "scale is NaN");
  const bool hasv = c.v.wv != nullptr;
  const size_t n = (size_t)T * (size_t)S, H = (size_t)g.net.width[0];
  const int64_t nv = hasv ? g.net.width[g.net.n_hidden - 1] + 1 : 0;
  const std::vector<Span> in = {{obs, n * g.net.in_dim * 4, SPAN_ROWS}, {actions, n * 16, SPAN_ROWS}, {done, n, SPAN_ROWS, 1},
                                {h0, (size_t)S * H * 4, SPAN_ROWS, 16}, {logp_old, n * 4, SPAN_ROWS}, {adv, n * 4, SPAN_ROWS},
                                {ret, n * 4, hasv ? SPAN_ROWS : SPAN_OPTIONAL}, {v_old, n * 4, SPAN_OPTIONAL}};
  const std::vector<Span> out = {{grad_out, (size_t)net.nw * 4, SPAN_ALWAYS}, {grad_value_out, (size_t)nv * 4, hasv ? SPAN_ALWAYS : SPAN_OPTIONAL},
                                 {grad_log_std_out, 16, SPAN_ALWAYS}, {stats_out, 48, SPAN_ALWAYS, 8}};
  bool wide = false, misaligned = false;
  if (int rc = check_span_nulls(in, out, S > 0, wide, misaligned)) return rc;
  if (!(clip_eps > 0.0f && clip_eps < 1.0f)) return fail(GAQ_ERR_INVALID, who + "clip_eps must be in (0, 1)");
  if (!(vclip >= 0.0f)) return fail(GAQ_ERR_INVALID, who + "vclip must not be negative or NaN");
  if (vf_coef != vf_coef || ent_coef != ent_coef) return fail(GAQ_ERR_INVALID, who + "vf_coef or ent_coef is NaN");
  if (!hasv && (ret || v_old || grad_value_out))
    return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head): ret, v_old and grad_value_out must be NULL without one");
  if (vclip > 0.0f && hasv && !v_old && S > 0) return fail(GAQ_ERR_INVALID, who + "vclip > 0 needs v_old");
  if (!c.v.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no log-probability");
  size_t lds = 0;
  if (int rc = seq_ready(c, true, wide, misaligned, in, out, lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {                                                   // zeros to every output, no tile work
    HIP_TRY(hipMemsetAsync(grad_out, 0, sizeof(float) * (size_t)net.nw, st));
    if (grad_value_out) HIP_TRY(hipMemsetAsync(grad_value_out, 0, sizeof(float) * (size_t)nv, st));
    HIP_TRY(hipMemsetAsync(grad_log_std_out, 0, sizeof(float) * 4, st));
    HIP_TRY(hipMemsetAsync(stats_out, 0, sizeof(double) * 6, st));
    return GAQ_OK;
  }
  const int G = grad_groups(g.ntiles);
  // the scratch: the statistics and the partials, sized for the default number of workgroups and for the stride with a value head
  // whatever this call needs, then the tape [G][T][64][H].  It grows when a call needs more than every call before it, and only then
  // do its pointers move: a graph captured after a call with the largest T (and S) stays valid.
  const int64_t nvmax = g.net.width[g.net.n_hidden - 1] + 1;
  g.pstride = (net.nw + nvmax + 15) & ~(int64_t)15;
  const size_t fixed = (size_t)std::max(G, kGradGroups) * ((size_t)g.pstride * sizeof(float) + kSeqStats * sizeof(double));
  const size_t need = fixed + (size_t)G * (size_t)T * kTile * H * sizeof(float);
  if (net.grad_scratch_bytes < need) {
    if (net.grad_scratch) { HIP_TRY(hipFree(net.grad_scratch)); net.grad_scratch = nullptr; net.grad_scratch_bytes = 0; }
    HIP_TRY(hipMalloc(&net.grad_scratch, need));
    net.grad_scratch_bytes = need;
  }
  g.spart = reinterpret_cast<double*>(net.grad_scratch);
  g.part = reinterpret_cast<float*>(g.spart + (size_t)std::max(G, kGradGroups) * kSeqStats);
  g.tape = reinterpret_cast<float*>(reinterpret_cast<char*>(net.grad_scratch) + fixed);
  g.obs = obs; g.a = actions; g.done = done; g.h0 = h0; g.logp_old = logp_old; g.adv = adv; g.ret = ret; g.v_old = v_old;
  g.clip = clip_eps; g.scale = scale; g.vclip = hasv ? vclip : 0.0f; g.vf_coef = hasv ? vf_coef : 0.0f;
  if (int rc = seq_launch<true>(g, G, lds, st)) return rc;
  const double ent = -(double)ent_coef * (double)scale * (double)T * (double)S;
  hipLaunchKernelGGL(grad_seq_reduce_kernel, dim3((unsigned)((net.nw + nv + 255) / 256)), dim3(256), 0, st, g.part, g.spart, G, g.pstride,
                     net.nw, nv, (int64_t)T * S, ent, grad_out, grad_value_out, stats_out, grad_log_std_out);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

}  // extern "C"
