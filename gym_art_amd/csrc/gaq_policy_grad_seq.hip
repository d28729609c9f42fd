// gaq_policy_grad_seq.hip -- the learner's passes over stored SEQUENCES for a GRU policy (include/gaq.h "gradients of a recurrent policy"):
// gaq_policy_eval_seq_dev (log-probabilities, V, means and the final state of T steps of S sequences, the rollout's bits) and
// gaq_policy_grad_ppo_seq_dev (the truncated-BPTT gradient of gaq_policy_grad_ppo_ac_dev's loss) with its index-gathered form
// gaq_policy_grad_ppo_seq_idx_dev (grad_seq_idx_kernel: the same body, the columns read through an index vector).  Of gaq_policy.hip it uses the net
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
  // the idx form (at the end: every offset above stays); the [T, S, ...] inputs are then [T, S_src, ...], h0 [S_src, H]
  const int32_t* idx;             // [S] source columns
  int64_t S_src;
};
constexpr int kSeqIdxBytes = kTile * 4;                           // the idx form: the tile's 64 source columns, between the head region and X
constexpr int kSeqIdxDead = -1, kSeqIdxSkipped = -2;              // what they hold for a dead lane / for an index out of range

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
// its idx twin: sequence e's observation is step-row tsrc + sidx[e] (tsrc = t S_src) where sidx[e] >= 0, else a dead column's zeros
__device__ __forceinline__ void seq_stage_obs_idx(float* X, const float* obs, const PolObsNorm& nm, int64_t tsrc, const int* sidx, int D,
                                                  int tid) {
  const int kin = (D + 3) & ~3, kx = (D + 15) & ~15;
  for (int f = tid; f < kTile * kx; f += kSeqBlock) {
    const int e = f / kx, k = f - e * kx;
    float v = k >= kin ? 0.0f : -0.0f;
    if (k < D) {
      v = 0.0f;
      const int s = sidx[e];
      if (s >= 0) {
        v = obs[(tsrc + s) * D + k];
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

// `g` must stay the kernels' first and only argument: the row stage reads its own members of it at offset 0 of the kernel-argument
// segment, as grad_kernel's does.
template <bool Bwd>
__global__ __launch_bounds__(kSeqBlock) void grad_seq_kernel(SeqArgs g) {
  constexpr bool Idx = false;
#include "gaq_policy_grad_seq_body.inc"
}
// gaq_policy_grad_ppo_seq_idx_dev's: grad_seq_kernel<true> over the columns idx names
__global__ __launch_bounds__(kSeqBlock) void grad_seq_idx_kernel(SeqArgs g) {
  constexpr bool Bwd = true, Idx = true;
#include "gaq_policy_grad_seq_body.inc"
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

// grad_seq_reduce_kernel's twin for the idx form: the same sums in the same order, and one more statistic after `rows`: the
// workgroups' last word, the indices skipped
__global__ __launch_bounds__(256) void grad_seq_reduce_idx_kernel(const float* __restrict__ part, const double* __restrict__ spart, int G,
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
    else { stats_out[5] = (double)rows; stats_out[6] = s; }
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

int seq_idx_launch(const SeqArgs& g, int G, size_t lds, hipStream_t st) {
  if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void*)&grad_seq_idx_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(grad_seq_idx_kernel, dim3((unsigned)G), dim3(kSeqBlock), lds, st, g);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

// gaq_policy_grad_ppo_seq_dev (gather = false, S_src = S) and its idx form: the inputs span S_src columns, idx spans S words, and the idx
// form's stats_out is one double longer
int seq_grad_call(const char* name, bool gather, gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                  const float* actions, const uint8_t* done, const float* h0, const float* logp_old, const float* adv, const float* ret,
                  const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale, float* grad_out,
                  float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  SeqCall c{name};
  if (int rc = seq_begin(c, p, T, S)) return rc;
  const std::string who = std::string(c.who) + ": ";
  SeqArgs& g = c.g;
  PolicyNet& net = *c.v.net;
  if (scale != scale) return fail(GAQ_ERR_INVALID, who + "scale is NaN");
  if (gather) {
    if (S > 0 && S_src < 1) return fail(GAQ_ERR_INVALID, who + "S_src must be at least 1");
    if (S_src > ((int64_t)1 << 31) - 1) return fail(GAQ_ERR_INVALID, who + "S_src must not exceed 2^31 - 1");
    if (S_src < 0) S_src = 0;
  }
  const bool hasv = c.v.wv != nullptr;
  const size_t n = (size_t)T * (size_t)S_src, H = (size_t)g.net.width[0];
  const int64_t nv = hasv ? g.net.width[g.net.n_hidden - 1] + 1 : 0;
  std::vector<Span> in = {{obs, n * g.net.in_dim * 4, SPAN_ROWS}, {actions, n * 16, SPAN_ROWS}, {done, n, SPAN_ROWS, 1},
                          {h0, (size_t)S_src * H * 4, SPAN_ROWS, 16}, {logp_old, n * 4, SPAN_ROWS}, {adv, n * 4, SPAN_ROWS},
                          {ret, n * 4, hasv ? SPAN_ROWS : SPAN_OPTIONAL}, {v_old, n * 4, SPAN_OPTIONAL}};
  if (gather) in.push_back({idx, (size_t)S * 4, SPAN_ROWS});
  const std::vector<Span> out = {{grad_out, (size_t)net.nw * 4, SPAN_ALWAYS}, {grad_value_out, (size_t)nv * 4, hasv ? SPAN_ALWAYS : SPAN_OPTIONAL},
                                 {grad_log_std_out, 16, SPAN_ALWAYS}, {stats_out, gather ? 56u : 48u, SPAN_ALWAYS, 8}};
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
  if (gather) {
    lds += kSeqIdxBytes;
    if (lds > kSeqLdsMax) return fail(GAQ_ERR_INVALID, who + "in_dim too large for the sequence kernel's LDS");
    if ((int64_t)T * S_src > ((int64_t)1 << 40)) return fail(GAQ_ERR_INVALID, who + "too many sequences or steps for one launch");
  }
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {                                                   // zeros to every output, no tile work
    HIP_TRY(hipMemsetAsync(grad_out, 0, sizeof(float) * (size_t)net.nw, st));
    if (grad_value_out) HIP_TRY(hipMemsetAsync(grad_value_out, 0, sizeof(float) * (size_t)nv, st));
    HIP_TRY(hipMemsetAsync(grad_log_std_out, 0, sizeof(float) * 4, st));
    HIP_TRY(hipMemsetAsync(stats_out, 0, sizeof(double) * (gather ? 7 : 6), st));
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
  g.idx = idx; g.S_src = S_src;
  if (int rc = gather ? seq_idx_launch(g, G, lds, st) : seq_launch<true>(g, G, lds, st)) return rc;
  const double ent = -(double)ent_coef * (double)scale * (double)T * (double)S;
  if (gather)
    hipLaunchKernelGGL(grad_seq_reduce_idx_kernel, dim3((unsigned)((net.nw + nv + 255) / 256)), dim3(256), 0, st, g.part, g.spart, G,
                       g.pstride, net.nw, nv, (int64_t)T * S, ent, grad_out, grad_value_out, stats_out, grad_log_std_out);
  else
    hipLaunchKernelGGL(grad_seq_reduce_kernel, dim3((unsigned)((net.nw + nv + 255) / 256)), dim3(256), 0, st, g.part, g.spart, G, g.pstride,
                       net.nw, nv, (int64_t)T * S, ent, grad_out, grad_value_out, stats_out, grad_log_std_out);
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
  return seq_grad_call("gaq_policy_grad_ppo_seq_dev", false, p, T, S, nullptr, S, obs, actions, done, h0, logp_old, adv, ret, v_old, clip_eps,
                       vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

int gaq_policy_grad_ppo_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                    const float* actions, const uint8_t* done, const float* h0, const float* logp_old, const float* adv,
                                    const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef,
                                    float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out,
                                    void* stream) {
  return seq_grad_call("gaq_policy_grad_ppo_seq_idx_dev", true, p, T, S, idx, S_src, obs, actions, done, h0, logp_old, adv, ret, v_old,
                       clip_eps, vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

}  // extern "C"
