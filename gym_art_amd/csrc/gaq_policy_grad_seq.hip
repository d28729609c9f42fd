// gaq_policy_grad_seq.hip -- the learner's passes over stored SEQUENCES for a recurrent policy (include/gaq.h "gradients of a recurrent
// policy" and "gradients of an LSTM policy"), once for both cells:
//   GRU   gaq_policy_eval_seq_dev       gaq_policy_grad_ppo_seq_dev       gaq_policy_grad_ppo_seq_idx_dev
//   LSTM  gaq_policy_eval_lstm_seq_dev  gaq_policy_grad_ppo_lstm_seq_dev  gaq_policy_grad_ppo_lstm_seq_idx_dev
// the forward pass (log-probabilities, V, means and the final state of T steps of S sequences, the rollout's bits), the truncated-BPTT
// gradient of gaq_policy_grad_ppo_ac_dev's loss, and that gradient over the columns an index vector names -- and, for a policy with an
// ENCODER in front of its cell (gaq.h "sequences through an encoder"), the same three under names that take both cells:
//   gaq_policy_eval_enc_seq_dev  gaq_policy_grad_ppo_enc_seq_dev  gaq_policy_grad_ppo_enc_seq_idx_dev
// as split passes: gaq_policy.hip's encoder kernel over the stored rows (policy_encode_rows / _list), the kernels below on the features
// (the gradient: grad_seq_dx_kernel, which also writes dfeat_t = W_ih^T planes), gaq_policy_grad.hip's grad_feat_kernel for the
// encoder's backward over the rows, and the one reduce twice.  Of gaq_policy.hip it uses the
// net record gaq_grad.hpp declares (policy_grad_seq_view) and what that header holds for both gradient units: the span checks, the split
// into workgroups, the scratch, the PPO refusals, the launch and the reduce.
//
// One kernel template, grad_seq_kernel<L, Bwd, Idx> (L: the LSTM), whose text is gaq_policy_grad_seq_body.inc: 4 waves per workgroup,
// one 64-sequence tile at a time; sequence e of the tile lives in column grad_col(e) = pol_col(e) of every LDS row (stride 68 floats, as
// in gaq_policy_grad.hip).  What the feed-forward gradient kernel and this one have in common -- the layout, the partial's words, dW,
// the row sum -- is gaq_grad_dev.hpp; the stages themselves are restated here, not shared: that kernel keeps its recorded resource
// lines.  The LDS head, the staging of observations and of [., H] rows and one head layer's forward are gaq_grad_seq_dev.hpp.
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

// `g` must stay the kernels' first and only argument: the row stage reads its own members of it at offset 0 of the kernel-argument
// segment, as grad_kernel's does.  The six kernels are <L, false, false> (eval), <L, true, false> and <L, true, true> (the idx form).
template <bool L, bool Bwd, bool Idx>
__global__ __launch_bounds__(kGradBlock) void grad_seq_kernel(SeqArgsT<L> g) {
#include "gaq_policy_grad_seq_body.inc"
}

// The encoder forms' gradient kernels (gaq.h "sequences through an encoder"): the backward kernels above -- the same text, Bwd = true --
// which also write dfeat_t = W_ih^T planes, the gradient of the loss in the cell's input (the encoder's features), to dfeat [T, S, E]
// (the idx form: [T, S_src, E], row = source row).  Kernels of their own name with a record of their own (the base first, so the row
// stage's reads at offset 0 hold): the six kernels above keep their symbols, their argument segment and their instructions.
template <bool L>
struct SeqArgsDx : SeqArgsT<L> {
  float* dfeat;
};
template <bool L, bool Idx>
__global__ __launch_bounds__(kGradBlock) void grad_seq_dx_kernel(SeqArgsDx<L> g) {
  constexpr bool Bwd = true;
#include "gaq_policy_grad_seq_body.inc"
}

// gaq.h's formula: the backward pass carries dh (the LSTM: and dc) beside hin
size_t seq_lds(const PolicyDev& pd, bool lstm, bool bwd) {
  const int H = pd.width[0];
  int head = H;
  for (int l = 1; l < pd.n_hidden; ++l) head += pd.width[l];
  const int rows = ((pd.in_dim + 15) & ~15) + (bwd ? (lstm ? 3 : 2) : 1) * H + (bwd ? std::max(4 * H, head) : head);
  return (size_t)kSeqHeadBytes + (size_t)rows * kGradStride * 4;
}

// the arguments the calls share, checked: T, S, the handle's view, log_std
template <bool L>
struct SeqCall {
  const char* who;
  GradNet v;
  SeqArgsT<L> g{};
  const GradEnc* enc = nullptr;   // the encoder forms: v is the caller's (policy_grad_enc_seq_view), the kernel reads features
};

template <bool L>
int seq_begin(SeqCall<L>& c, gaq_policy* p, int32_t T, int64_t S) {
  const std::string who = std::string(c.who) + ": ";
  if (!c.enc)
    if (int rc = policy_grad_seq_view(p, L ? GAQ_POLICY_CELL_LSTM : GAQ_POLICY_CELL_GRU, c.v)) return rc;
  if (T < 1) return fail(GAQ_ERR_INVALID, who + "T must be at least 1");
  if (S < 0) return fail(GAQ_ERR_INVALID, who + "S must not be negative");
  const PolicyNet& net = *c.v.net;
  SeqArgsT<L>& g = c.g;
  g.net = net.pd; g.off_hh = c.v.off_hh; g.nm = policy_norm_dev(c.enc ? nullptr : net.norm);
  g.T = T; g.S = S; g.ntiles = (S + kTile - 1) / kTile;
  grad_fill_std(c.v, g.log_std, g.inv_std);
  g.explore_tab = c.v.tab;
  g.wv = c.v.wv;
  return GAQ_OK;
}

// the checks every call ends with (alignment, overlaps, sizes), then the device
template <bool L>
int seq_ready(const SeqCall<L>& c, bool bwd, bool wide, bool misaligned, const std::vector<Span>& in, const std::vector<Span>& out, size_t& lds) {
  const std::string who = std::string(c.who) + ": ";
  if (misaligned)
    return fail(GAQ_ERR_INVALID, who + "pointers must be 4-byte aligned (h0" + (L ? ", c0" : "") + (bwd ? "" : L ? ", h_out, c_out" : ", h_out") +
                                     ": 16" + (wide && bwd ? ", stats_out: 8" : "") + ")");
  if (int rc = check_overlap(c.who, in, out)) return rc;
  lds = seq_lds(c.g.net, L, bwd);
  if (lds > kGradLdsMax) return fail(GAQ_ERR_INVALID, who + "in_dim too large for the sequence kernel's LDS");
  if (c.g.ntiles > ((int64_t)1 << 31) - 1 || (int64_t)c.g.T * c.g.S > ((int64_t)1 << 40))
    return fail(GAQ_ERR_INVALID, who + "too many sequences or steps for one launch");
  HIP_TRY(hipSetDevice(c.v.net->device));
  return GAQ_OK;
}

// the forward pass of either cell (c0 and c_out: the LSTM's, else nullptr).  view / enc: the encoder form (gaq_policy_eval_enc_seq_dev) --
// obs is [T, S, the env's obs_dim], one launch of the rollout's encoder kernel writes the features [T S, E] to the handle's scratch and
// the sequence kernel reads those as its observation (net.in_dim = E, no normaliser: the encoder's launch has applied it)
template <bool L>
int seq_eval_call(const char* name, gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                  const float* h0, const float* c0, float* logp_out, float* value_out, float* mean_out, float* h_out, float* c_out,
                  void* stream, const GradNet* view = nullptr, const GradEnc* enc = nullptr) {
  SeqCall<L> c{name};
  if (enc) { c.v = *view; c.enc = enc; }
  if (int rc = seq_begin(c, p, T, S)) return rc;
  SeqArgsT<L>& g = c.g;
  const size_t n = (size_t)T * (size_t)S, H = (size_t)g.net.width[0];
  std::vector<Span> in = {{obs, n * (enc ? enc->in_dim : g.net.in_dim) * 4, SPAN_ROWS}, {actions, n * 16, logp_out ? SPAN_ROWS : SPAN_OPTIONAL},
                          {done, n, SPAN_ROWS, 1}, {h0, (size_t)S * H * 4, SPAN_ROWS, 16}};
  std::vector<Span> out = {{logp_out, n * 4, SPAN_OPTIONAL}, {value_out, n * 4, SPAN_OPTIONAL}, {mean_out, n * 16, SPAN_OPTIONAL},
                           {h_out, (size_t)S * H * 4, SPAN_OPTIONAL, 16}};
  if (L) {
    in.push_back({c0, (size_t)S * H * 4, SPAN_ROWS, 16});
    out.push_back({c_out, (size_t)S * H * 4, SPAN_OPTIONAL, 16});
  }
  bool wide = false, misaligned = false;
  if (int rc = check_span_nulls(in, out, S > 0, wide, misaligned)) return rc;
  if (value_out && !c.v.wv)
    return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head): the actor-critic passes need V on the policy's trunk");
  if (logp_out && !c.v.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no log-probability");
  size_t lds = 0;
  if (int rc = seq_ready(c, false, wide, misaligned, in, out, lds)) return rc;
  if (enc && (int64_t)T * S > ((int64_t)1 << 31) - 1)
    return fail(GAQ_ERR_INVALID, std::string(name) + ": T x S must not exceed 2^31 - 1 rows for the encoder's launch");
  if (S == 0) return GAQ_OK;
  if (enc) {
    // the features live in the handle's gradient scratch where a gradient call keeps its tape (grad_scratch's rule: the pointers move
    // only when a call needs more than every call before it)
    double* spart; float *part, *feat;
    if (int rc = grad_scratch(*c.v.net, 1, n * (size_t)enc->width * sizeof(float), spart, part, feat)) return rc;
    if (int rc = policy_encode_rows(*enc, (int64_t)n, obs, feat, (hipStream_t)stream)) return rc;
    obs = feat;
  }
  g.obs = obs; g.a = actions; g.done = done; g.h0 = h0;
  g.logp_out = logp_out; g.value_out = value_out; g.mean_out = mean_out; g.h_out = h_out;
  if constexpr (L) { g.c0 = c0; g.c_out = c_out; }
  g.S_src = S;
  if (!value_out) g.wv = nullptr;                                 // V's parts are not summed where nobody reads them
  return grad_launch(grad_seq_kernel<L, false, false>, g, (int)std::min<int64_t>(g.ntiles, (int64_t)1 << 20), lds, (hipStream_t)stream);
}

// the gradient of either cell (gather = false, S_src = S) and its idx form: the inputs span S_src columns, idx spans S words, and the idx
// form's stats_out is one double longer
template <bool L>
int seq_grad_call(const char* name, bool gather, gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                  const float* actions, const uint8_t* done, const float* h0, const float* c0, const float* logp_old, const float* adv,
                  const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                  float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream,
                  const GradNet* view = nullptr, const GradEnc* enc = nullptr, float* grad_enc_out = nullptr) {
  SeqCall<L> c{name};
  if (enc) { c.v = *view; c.enc = enc; }
  const float* enc_obs = obs;                                     // (obs becomes the features below)
  if (int rc = seq_begin(c, p, T, S)) return rc;
  const std::string who = std::string(c.who) + ": ";
  SeqArgsT<L>& g = c.g;
  PolicyNet& net = *c.v.net;
  if (scale != scale) return fail(GAQ_ERR_INVALID, who + "scale is NaN");
  if (gather) {
    if (S > 0 && S_src < 1) return fail(GAQ_ERR_INVALID, who + "S_src must be at least 1");
    if (S_src > ((int64_t)1 << 31) - 1) return fail(GAQ_ERR_INVALID, who + "S_src must not exceed 2^31 - 1");
    if (S_src < 0) S_src = 0;
  }
  // (the idx form's S may exceed S_src: repeated indices; the row list and its 32-bit count span T x S)
  if (enc && ((int64_t)T * S_src > ((int64_t)1 << 31) - 1 || (int64_t)T * S > ((int64_t)1 << 31) - 1))
    return fail(GAQ_ERR_INVALID, who + "T x S and T x S_src must not exceed 2^31 - 1 rows for the encoder's passes");
  const bool hasv = c.v.wv != nullptr;
  const size_t n = (size_t)T * (size_t)S_src, H = (size_t)g.net.width[0];
  const int64_t nv = hasv ? g.net.width[g.net.n_hidden - 1] + 1 : 0;
  std::vector<Span> in = {{obs, n * (enc ? enc->in_dim : g.net.in_dim) * 4, SPAN_ROWS}, {actions, n * 16, SPAN_ROWS}, {done, n, SPAN_ROWS, 1},
                          {h0, (size_t)S_src * H * 4, SPAN_ROWS, 16}, {logp_old, n * 4, SPAN_ROWS}, {adv, n * 4, SPAN_ROWS},
                          {ret, n * 4, hasv ? SPAN_ROWS : SPAN_OPTIONAL}, {v_old, n * 4, SPAN_OPTIONAL}};
  if (L) in.push_back({c0, (size_t)S_src * H * 4, SPAN_ROWS, 16});
  if (gather) in.push_back({idx, (size_t)S * 4, SPAN_ROWS});
  std::vector<Span> out = {{grad_out, (size_t)net.nw * 4, SPAN_ALWAYS}, {grad_value_out, (size_t)nv * 4, hasv ? SPAN_ALWAYS : SPAN_OPTIONAL},
                           {grad_log_std_out, 16, SPAN_ALWAYS}, {stats_out, gather ? 56u : 48u, SPAN_ALWAYS, 8}};
  if (enc) out.push_back({grad_enc_out, (size_t)enc->nw * 4, SPAN_ALWAYS});
  bool wide = false, misaligned = false;
  if (int rc = check_span_nulls(in, out, S > 0, wide, misaligned)) return rc;
  // (a missing v_old is refused only with a value head, the pointers below only without one: the two never meet, in either order)
  if (int rc = check_ppo_hyper(who, clip_eps, vclip, vf_coef, ent_coef, hasv, v_old, S > 0)) return rc;
  if (!hasv && (ret || v_old || grad_value_out))
    return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head): ret, v_old and grad_value_out must be NULL without one");
  if (!c.v.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no log-probability");
  size_t lds = 0;
  if (int rc = seq_ready(c, true, wide, misaligned, in, out, lds)) return rc;
  if (gather) {
    lds += kGradIdxBytes;
    if (lds > kGradLdsMax) return fail(GAQ_ERR_INVALID, who + "in_dim too large for the sequence kernel's LDS");
    if ((int64_t)T * S_src > ((int64_t)1 << 40)) return fail(GAQ_ERR_INVALID, who + "too many sequences or steps for one launch");
  }
  if (enc) {
    if (grad_feat_lds(enc->trunk, gather) > kGradLdsMax) return fail(GAQ_ERR_INVALID, who + "obs_dim too large for the encoder gradient kernel's LDS");
  }
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {                                                   // zeros to every output, no tile work
    HIP_TRY(hipMemsetAsync(grad_out, 0, sizeof(float) * (size_t)net.nw, st));
    if (grad_value_out) HIP_TRY(hipMemsetAsync(grad_value_out, 0, sizeof(float) * (size_t)nv, st));
    HIP_TRY(hipMemsetAsync(grad_log_std_out, 0, sizeof(float) * 4, st));
    HIP_TRY(hipMemsetAsync(stats_out, 0, sizeof(double) * (gather ? 7 : 6), st));
    if (enc) HIP_TRY(hipMemsetAsync(grad_enc_out, 0, sizeof(float) * (size_t)enc->nw, st));
    return GAQ_OK;
  }
  const int G = grad_groups(g.ntiles);
  // the scratch (grad_scratch) with the tape [G][T][64][H] (the LSTM: [2][H]) behind its fixed part: a graph captured after a call with
  // the largest T (and S) stays valid
  g.pstride = grad_stride_max(net);
  const size_t tape_bytes = (size_t)G * (size_t)T * kTile * (L ? 2 : 1) * H * sizeof(float);
  // the encoder forms keep, behind the tape: feat and dfeat [T S_src, E], the encoder's partials [Gf][its stride], and for the idx form
  // the row indices [T S] twice (signed for the encoder's backward, a list for its gathered forward) and the list's count
  const int64_t rows = (int64_t)T * S;
  const int Gf = enc ? grad_groups((rows + kTile - 1) / kTile) : 0;
  const int64_t estride = enc ? (enc->nw + 15) & ~(int64_t)15 : 0;
  const size_t feat_bytes = enc ? n * (size_t)enc->width * sizeof(float) : 0;
  const size_t epart_bytes = (size_t)Gf * (size_t)estride * sizeof(float);
  const size_t ridx_bytes = enc && gather ? (((size_t)rows * 4 + 15) & ~(size_t)15) : 0;
  if (int rc = grad_scratch(net, G, tape_bytes + 2 * feat_bytes + epart_bytes + 2 * ridx_bytes + (ridx_bytes ? 16 : 0), g.spart, g.part, g.tape))
    return rc;
  char* behind = reinterpret_cast<char*>(g.tape) + tape_bytes;
  float* feat = reinterpret_cast<float*>(behind);
  float* dfeat = reinterpret_cast<float*>(behind + feat_bytes);
  float* epart = reinterpret_cast<float*>(behind + 2 * feat_bytes);
  int32_t* rowidx = reinterpret_cast<int32_t*>(behind + 2 * feat_bytes + epart_bytes);
  uint32_t* rowlist = reinterpret_cast<uint32_t*>(behind + 2 * feat_bytes + epart_bytes + ridx_bytes);
  uint32_t* rowcount = reinterpret_cast<uint32_t*>(behind + 2 * feat_bytes + epart_bytes + 2 * ridx_bytes);
  if (enc) {
    if (gather) {
      if (int rc = grad_rowidx_run(T, S, idx, S_src, rowidx, rowlist, rowcount, st)) return rc;
      if (int rc = policy_encode_list(*enc, rows, rowlist, rowcount, obs, feat, st)) return rc;
    } else if (int rc = policy_encode_rows(*enc, rows, obs, feat, st)) return rc;
    obs = feat;
  }
  g.obs = obs; g.a = actions; g.done = done; g.h0 = h0; g.logp_old = logp_old; g.adv = adv; g.ret = ret; g.v_old = v_old;
  if constexpr (L) g.c0 = c0;
  g.clip = clip_eps; g.scale = scale; g.vclip = hasv ? vclip : 0.0f; g.vf_coef = hasv ? vf_coef : 0.0f;
  g.idx = idx; g.S_src = S_src;
  if (enc) {
    SeqArgsDx<L> gx{};
    static_cast<SeqArgsT<L>&>(gx) = g;
    gx.dfeat = dfeat;
    if (int rc = grad_launch(gather ? grad_seq_dx_kernel<L, true> : grad_seq_dx_kernel<L, false>, gx, G, lds, st)) return rc;
  } else if (int rc = grad_launch(gather ? grad_seq_kernel<L, true, true> : grad_seq_kernel<L, true, false>, g, G, lds, st)) return rc;
  GradReduce r{};
  r.part = g.part; r.spart = g.spart; r.G = G; r.pstride = g.pstride; r.nw = net.nw; r.nv = nv; r.rows = (int64_t)T * S;
  r.ent = -(double)ent_coef * (double)scale * (double)T * (double)S;
  r.grad_out = grad_out; r.value_out = grad_value_out; r.stats_out = stats_out; r.log_std_out = grad_log_std_out;
  grad_route(r, true, 5, gather);
  if (!enc) return grad_reduce(r, st);
  if (int rc = grad_reduce(r, st)) return rc;
  // the encoder's backward over the stored rows (gaq_policy_grad.hip grad_feat_kernel: batch work, T times the parallelism of the
  // kernel above), then its partials summed like every other: ascending in fp64, no statistics
  GradFeatCall f{};
  const PolObsNorm enm = policy_norm_dev(net.norm);
  f.trunk = enc->trunk; f.nm_tab = enm.tab; f.nm_dim = enm.dim; f.rows = rows;
  f.obs = enc_obs; f.dfeat = dfeat; f.rowidx = gather ? rowidx : nullptr; f.part = epart; f.pstride = estride; f.G = Gf;
  if (int rc = grad_feat_run(f, st)) return rc;
  GradReduce re{};
  re.part = epart; re.spart = g.spart; re.G = Gf; re.ns = 0; re.pstride = estride; re.nw = enc->nw; re.nv = 0; re.rows = rows;
  re.grad_out = grad_enc_out;
  return grad_reduce(re, st);
}

}  // namespace

extern "C" {

int gaq_policy_eval_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done, const float* h0,
                            float* logp_out, float* value_out, float* mean_out, float* h_out, void* stream) {
  return seq_eval_call<false>("gaq_policy_eval_seq_dev", p, T, S, obs, actions, done, h0, nullptr, logp_out, value_out, mean_out, h_out,
                              nullptr, stream);
}

int gaq_policy_grad_ppo_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                const float* h0, const float* logp_old, const float* adv, const float* ret, const float* v_old,
                                float clip_eps, float vclip, float vf_coef, float ent_coef, float scale, float* grad_out,
                                float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  return seq_grad_call<false>("gaq_policy_grad_ppo_seq_dev", false, p, T, S, nullptr, S, obs, actions, done, h0, nullptr, logp_old, adv, ret,
                              v_old, clip_eps, vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

int gaq_policy_grad_ppo_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                    const float* actions, const uint8_t* done, const float* h0, const float* logp_old, const float* adv,
                                    const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef,
                                    float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out,
                                    void* stream) {
  return seq_grad_call<false>("gaq_policy_grad_ppo_seq_idx_dev", true, p, T, S, idx, S_src, obs, actions, done, h0, nullptr, logp_old, adv, ret,
                              v_old, clip_eps, vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

int gaq_policy_eval_lstm_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                 const float* h0, const float* c0, float* logp_out, float* value_out, float* mean_out, float* h_out,
                                 float* c_out, void* stream) {
  return seq_eval_call<true>("gaq_policy_eval_lstm_seq_dev", p, T, S, obs, actions, done, h0, c0, logp_out, value_out, mean_out, h_out, c_out,
                             stream);
}

int gaq_policy_grad_ppo_lstm_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                     const float* h0, const float* c0, const float* logp_old, const float* adv, const float* ret,
                                     const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                                     float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  return seq_grad_call<true>("gaq_policy_grad_ppo_lstm_seq_dev", false, p, T, S, nullptr, S, obs, actions, done, h0, c0, logp_old, adv, ret,
                             v_old, clip_eps, vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

int gaq_policy_grad_ppo_lstm_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                         const float* actions, const uint8_t* done, const float* h0, const float* c0, const float* logp_old,
                                         const float* adv, const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef,
                                         float ent_coef, float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out,
                                         double* stats_out, void* stream) {
  return seq_grad_call<true>("gaq_policy_grad_ppo_lstm_seq_idx_dev", true, p, T, S, idx, S_src, obs, actions, done, h0, c0, logp_old, adv, ret,
                             v_old, clip_eps, vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

// either cell behind an encoder: the handle's cell picks the kernel
int gaq_policy_eval_enc_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                const float* h0, const float* c0, float* logp_out, float* value_out, float* mean_out, float* h_out,
                                float* c_out, void* stream) {
  const char* name = "gaq_policy_eval_enc_seq_dev";
  GradNet v;
  GradEnc e;
  if (int rc = policy_grad_enc_seq_view(p, c0 || c_out, v, e)) return rc;
  if (e.lstm)
    return seq_eval_call<true>(name, p, T, S, obs, actions, done, h0, c0, logp_out, value_out, mean_out, h_out, c_out, stream, &v, &e);
  return seq_eval_call<false>(name, p, T, S, obs, actions, done, h0, nullptr, logp_out, value_out, mean_out, h_out, nullptr, stream, &v, &e);
}

int gaq_policy_grad_ppo_enc_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                    const float* h0, const float* c0, const float* logp_old, const float* adv, const float* ret,
                                    const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                                    float* grad_out, float* grad_enc_out, float* grad_value_out, float* grad_log_std_out, double* stats_out,
                                    void* stream) {
  const char* name = "gaq_policy_grad_ppo_enc_seq_dev";
  GradNet v;
  GradEnc e;
  if (int rc = policy_grad_enc_seq_view(p, c0 != nullptr, v, e)) return rc;
  if (e.lstm)
    return seq_grad_call<true>(name, false, p, T, S, nullptr, S, obs, actions, done, h0, c0, logp_old, adv, ret, v_old, clip_eps, vclip, vf_coef,
                               ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream, &v, &e, grad_enc_out);
  return seq_grad_call<false>(name, false, p, T, S, nullptr, S, obs, actions, done, h0, nullptr, logp_old, adv, ret, v_old, clip_eps, vclip,
                              vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream, &v, &e, grad_enc_out);
}

int gaq_policy_grad_ppo_enc_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                        const float* actions, const uint8_t* done, const float* h0, const float* c0, const float* logp_old,
                                        const float* adv, const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef,
                                        float ent_coef, float scale, float* grad_out, float* grad_enc_out, float* grad_value_out,
                                        float* grad_log_std_out, double* stats_out, void* stream) {
  const char* name = "gaq_policy_grad_ppo_enc_seq_idx_dev";
  GradNet v;
  GradEnc e;
  if (int rc = policy_grad_enc_seq_view(p, c0 != nullptr, v, e)) return rc;
  if (e.lstm)
    return seq_grad_call<true>(name, true, p, T, S, idx, S_src, obs, actions, done, h0, c0, logp_old, adv, ret, v_old, clip_eps, vclip, vf_coef,
                               ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream, &v, &e, grad_enc_out);
  return seq_grad_call<false>(name, true, p, T, S, idx, S_src, obs, actions, done, h0, nullptr, logp_old, adv, ret, v_old, clip_eps, vclip,
                              vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream, &v, &e, grad_enc_out);
}

}  // extern "C"
