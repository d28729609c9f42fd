// gaq_policy_grad_seq.hip -- the learner's passes over stored SEQUENCES for a GRU policy (include/gaq.h "gradients of a recurrent policy"):
// gaq_policy_eval_seq_dev (log-probabilities, V, means and the final state of T steps of S sequences, the rollout's bits) and
// gaq_policy_grad_ppo_seq_dev (the truncated-BPTT gradient of gaq_policy_grad_ppo_ac_dev's loss) with its index-gathered form
// gaq_policy_grad_ppo_seq_idx_dev (grad_seq_idx_kernel: the same body, the columns read through an index vector).  Of gaq_policy.hip it uses the net
// record gaq_grad.hpp declares (policy_grad_seq_view) and what that header holds for both gradient units: the span checks, the split
// into workgroups, the scratch, the PPO refusals, the launch and the reduce.
//
// One kernel template, grad_seq_kernel<Bwd>, 4 waves per workgroup, one 64-sequence tile at a time; sequence e of the tile lives in
// column grad_col(e) = pol_col(e) of every LDS row (stride 68 floats, as in gaq_policy_grad.hip).  What the feed-forward gradient
// kernel and this one have in common -- the layout, the partial's words, dW, the row sum -- is gaq_grad_dev.hpp; the stages themselves
// are restated here, not shared: that kernel keeps its recorded resource lines.
// What this unit and the LSTM's (gaq_policy_grad_lstm.hip) have in common on the device -- the LDS head, the staging of observations and
// of [., H] rows, one head layer's forward -- is gaq_grad_seq_dev.hpp.
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
// grad_reduce (gaq_grad.hpp: gaq_policy_grad.hip's grad_reduce_kernel) sums the G partials in ascending order in fp64 and rounds once.  No atomics; dead lanes contribute exactly 0
// (their deltas are 0 and every activation is finite); nothing is read past S.
#include "gaq_host.hpp"
#include "gaq_norm.hpp"
#include "gaq_grad.hpp"
#include "gaq_grad_dev.hpp"
#include "gaq_grad_seq_dev.hpp"

namespace {

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
  double* spart;                  // [G][kGradStatsAc]
  float* tape;                    // [G][T][64][H]
  int64_t pstride;
  // the idx form (at the end: every offset above stays); the [T, S, ...] inputs are then [T, S_src, ...], h0 [S_src, H]
  const int32_t* idx;             // [S] source columns
  int64_t S_src;
};

// the chunks c, c + cs, c + 2 cs -- one per gate -- of one product of the cell (`in` inputs: the rows of A, zero-padded to a multiple
// of 4) into acc[0], acc[1] and acc[JL]: cell_kloop's order of operations (k ascending, each MFMA a k-ordered fmaf chain)
template <int JL>
__device__ __forceinline__ void seq_kloop(const float* __restrict__ wl, int in, int c, int cs, const float* A, uint32_t lane,
                                          f32x4 (&acc)[4][4]) {
  const int h = (int)(lane >> 4);
  const float* arow = A + h * kGradStride + (lane & 15) * 4;
  const int kfull = in & ~3;
  for (int k0 = 0; k0 < kfull; k0 += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + k0 * kGradStride);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int s = j == 2 ? JL : j;
      const float a = wl[((c + j * cs) * in + k0) * 16 + lane];
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[s][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[s][eb], 0, 0, 0);
    }
  }
  if (kfull < in) {                                               // the x product's last, partial k-step: no weight past in - 1 is read
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + kfull * kGradStride);
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
// `g` must stay the kernels' first and only argument: the row stage reads its own members of it at offset 0 of the kernel-argument
// segment, as grad_kernel's does.
template <bool Bwd>
__global__ __launch_bounds__(kGradBlock) void grad_seq_kernel(SeqArgs g) {
  constexpr bool Idx = false;
#include "gaq_policy_grad_seq_body.inc"
}
// gaq_policy_grad_ppo_seq_idx_dev's: grad_seq_kernel<true> over the columns idx names
__global__ __launch_bounds__(kGradBlock) void grad_seq_idx_kernel(SeqArgs g) {
  constexpr bool Bwd = true, Idx = true;
#include "gaq_policy_grad_seq_body.inc"
}

size_t seq_lds(const PolicyDev& pd, bool bwd) {
  const int H = pd.width[0];
  int head = H;
  for (int l = 1; l < pd.n_hidden; ++l) head += pd.width[l];
  const int rows = ((pd.in_dim + 15) & ~15) + (bwd ? 2 : 1) * H + (bwd ? std::max(4 * H, head) : head);
  return (size_t)kSeqHeadBytes + (size_t)rows * kGradStride * 4;
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
  grad_fill_std(c.v, g.log_std, g.inv_std);
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
  if (lds > kGradLdsMax) return fail(GAQ_ERR_INVALID, who + "in_dim too large for the sequence kernel's LDS");
  if (c.g.ntiles > ((int64_t)1 << 31) - 1 || (int64_t)c.g.T * c.g.S > ((int64_t)1 << 40))
    return fail(GAQ_ERR_INVALID, who + "too many sequences or steps for one launch");
  HIP_TRY(hipSetDevice(c.v.net->device));
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
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {                                                   // zeros to every output, no tile work
    HIP_TRY(hipMemsetAsync(grad_out, 0, sizeof(float) * (size_t)net.nw, st));
    if (grad_value_out) HIP_TRY(hipMemsetAsync(grad_value_out, 0, sizeof(float) * (size_t)nv, st));
    HIP_TRY(hipMemsetAsync(grad_log_std_out, 0, sizeof(float) * 4, st));
    HIP_TRY(hipMemsetAsync(stats_out, 0, sizeof(double) * (gather ? 7 : 6), st));
    return GAQ_OK;
  }
  const int G = grad_groups(g.ntiles);
  // the scratch (grad_scratch) with the tape [G][T][64][H] behind its fixed part: a graph captured after a call with the largest T
  // (and S) stays valid
  g.pstride = grad_stride_max(net);
  if (int rc = grad_scratch(net, G, (size_t)G * (size_t)T * kTile * H * sizeof(float), g.spart, g.part, g.tape)) return rc;
  g.obs = obs; g.a = actions; g.done = done; g.h0 = h0; g.logp_old = logp_old; g.adv = adv; g.ret = ret; g.v_old = v_old;
  g.clip = clip_eps; g.scale = scale; g.vclip = hasv ? vclip : 0.0f; g.vf_coef = hasv ? vf_coef : 0.0f;
  g.idx = idx; g.S_src = S_src;
  if (int rc = grad_launch(gather ? grad_seq_idx_kernel : grad_seq_kernel<true>, g, G, lds, st)) return rc;
  GradReduce r{};
  r.part = g.part; r.spart = g.spart; r.G = G; r.pstride = g.pstride; r.nw = net.nw; r.nv = nv; r.rows = (int64_t)T * S;
  r.ent = -(double)ent_coef * (double)scale * (double)T * (double)S;
  r.grad_out = grad_out; r.value_out = grad_value_out; r.stats_out = stats_out; r.log_std_out = grad_log_std_out;
  grad_route(r, true, 5, gather);
  return grad_reduce(r, st);
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
  return grad_launch(grad_seq_kernel<false>, g, (int)std::min<int64_t>(g.ntiles, (int64_t)1 << 20), lds, (hipStream_t)stream);
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
