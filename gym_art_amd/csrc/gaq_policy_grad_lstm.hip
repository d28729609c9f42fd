// gaq_policy_grad_lstm.hip -- the learner's passes over stored SEQUENCES for an LSTM policy (include/gaq.h "gradients of an LSTM policy"):
// gaq_policy_eval_lstm_seq_dev (log-probabilities, V, means and the final h and c of T steps of S sequences, the rollout's bits) and
// gaq_policy_grad_ppo_lstm_seq_dev (the truncated-BPTT gradient of gaq_policy_grad_ppo_ac_dev's loss) with its index-gathered form
// gaq_policy_grad_ppo_lstm_seq_idx_dev.  A unit of its own beside gaq_policy_grad_seq.hip (the GRU's), whose kernels keep their
// instructions; the two share gaq_grad_seq_dev.hpp on the device and gaq_grad.hpp on the host (the span checks, the split into
// workgroups, the scratch, the PPO refusals, the launch and the reduce).
//
// One kernel template, grad_lstm_kernel<Bwd>, and grad_lstm_idx_kernel, in the GRU kernels' frame: 4 waves per workgroup, one
// 64-sequence tile at a time, LDS rows of 68 floats, sequence e at column grad_col(e).
//   forward   t ascending: the observation staged as pol_stage_obs stages it; (hin, cin)_t = (h, c)_{t-1} with the rows of done[t-1]
//             (and dead lanes) 0 by select; the cell is lstm_cell's arithmetic -- each of the four gate sums (i, f, g, o) starts at
//             b_ih + b_hh and takes the x products then the h products as ascending k-ordered MFMA chains, i, f, o sigmoids, g = tanhf,
//             c' = fmaf(f, cin, i g), h' = o tanhf(c') -- so h_t and c_t are the rollout's bits.  At H <= 64 a wave owns one 16-unit
//             chunk, and the lane that owns 4 units x 4 column blocks of it owns them at every t: c is carried in 16 registers and
//             takes no LDS.  <false> (eval) then runs the head and the row stage; <true> writes h_t and c_t to the workgroup's tape
//             [T][64][2][H] (a sequence's h_t and c_t side by side).
//   backward  t descending (<true>): hin_t and h_t are staged from the tape, the head is recomputed and backpropagated down to dh_t with
//             the GRU body's code shape, the gates are recomputed with the forward's code; cin_t is read from the tape by the owning lane
//             (four 16-byte loads under the select that cuts the carried gradients; c0 at t = 0) and c_t recomputed from it.  In the
//             accumulator registers, with tc = tanhf(c_t) and dh = dh_t + carried:
//               da_o = dh tc o (1 - o), dc = dc_carried + dh o (1 - tc^2), da_i = dc g i (1 - i), da_f = dc cin f (1 - f),
//               da_g = dc i (1 - g^2), dc_carried <- dc f
//             the four planes [da_i; da_f; da_g; da_o] go to LDS over the rows the head used -- contiguous in the packed row order, so
//             dW_ih = planes x^T and dW_hh = planes hin^T are both grad_dw over the chunks 0 .. 4H/16 - 1 -- the biases are row sums in
//             ascending column order (b_ih and b_hh take the same sum), dh_{t-1} = W_hh^T planes (the packed W_hh read 16 bytes per
//             lane); dh_{t-1} and dc_carried are 0 by select where done[t-1] and in dead columns.  The carried dh and dc each have H
//             LDS rows of their own.
// LDS = 8.25 KiB + 272 B x (kx + 3 H + max(4 H, H + head widths)) for <true> (+ 256 B for the idx form): 135.75 KiB at 18-LSTM64-64-64;
// 8.25 KiB + 272 B x (kx + 2 H + head widths) for <false>.
// Partials: every word of the workgroup's partial is owned by one lane for every (tile, t); the first (tile, t) stores, the others add;
// grad_reduce sums the G partials in ascending order in fp64 and rounds once.  No atomics; dead lanes contribute exactly 0 (their deltas
// are 0 and every activation is finite); nothing is read past S or through an index out of range.
#include "gaq_host.hpp"
#include "gaq_norm.hpp"
#include "gaq_grad.hpp"
#include "gaq_grad_dev.hpp"
#include "gaq_grad_seq_dev.hpp"

namespace {

struct LstmArgs {
  PolicyDev net;                  // width[0] = H (the cell), width[1 ..] the head's layers
  int32_t off_hh;                 // float offset of W_hh' in net.w
  PolObsNorm nm;                  // tab = nullptr: no normaliser
  int32_t T;
  int64_t S, ntiles;
  const float* obs;               // [T, S, D]
  const float* a;                 // [T, S, 4] or nullptr (eval without logp)
  const uint8_t* done;            // [T, S]
  const float *h0, *c0;           // [S, H]
  const float *logp_old, *adv;    // [T, S]
  const float *ret, *v_old;       // [T, S] or nullptr
  const float* wv;                // the value head (last width weights, bias) or nullptr
  float clip, scale, vclip, vf_coef;
  float log_std[4], inv_std[4];
  float *logp_out, *value_out, *mean_out, *h_out, *c_out;   // eval
  float* part;                    // [G][pstride]
  double* spart;                  // [G][kGradStatsAc]
  float* tape;                    // [G][T][64][2][H]
  int64_t pstride;
  // the idx form: the [T, S, ...] inputs are then [T, S_src, ...], h0 and c0 [S_src, H]
  const int32_t* idx;             // [S] source columns
  int64_t S_src;
};

// the chunks c, c + cs, c + 2 cs, c + 3 cs -- one per gate -- of one product of the cell (`in` inputs: the rows of A, zero-padded to a
// multiple of 4) into acc[0 .. 3]: cell_kloop<4, 3>'s order of operations (k ascending, each MFMA a k-ordered fmaf chain)
__device__ __forceinline__ void lstm_kloop(const float* __restrict__ wl, int in, int c, int cs, const float* A, uint32_t lane,
                                           f32x4 (&acc)[4][4]) {
  const int h = (int)(lane >> 4);
  const float* arow = A + h * kGradStride + (lane & 15) * 4;
  const int kfull = in & ~3;
  for (int k0 = 0; k0 < kfull; k0 += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + k0 * kGradStride);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = wl[((c + j * cs) * in + k0) * 16 + lane];
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[j][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[j][eb], 0, 0, 0);
    }
  }
  if (kfull < in) {                                               // the x product's last, partial k-step: no weight past in - 1 is read
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + kfull * kGradStride);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = kfull + h < in ? wl[((c + j * cs) * in + kfull) * 16 + lane] : 0.0f;
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) acc[j][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[j][eb], 0, 0, 0);
    }
  }
}

// chunk c's gate sums of this lane's 4 units x 4 column blocks: i, f, g, o, each from b_ih + b_hh -- lstm_cell's accumulators
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
  lstm_kloop(wih, D, c, hc, X, lane, acc);
  lstm_kloop(whh, hid, c, hc, Hin, lane, acc);
}

// `g` must stay the kernels' first and only argument: the row stage reads its own members of it at offset 0 of the kernel-argument
// segment, as grad_seq_kernel's does.
template <bool Bwd>
__global__ __launch_bounds__(kGradBlock) void grad_lstm_kernel(LstmArgs g) {
  constexpr bool Idx = false;
#include "gaq_policy_grad_lstm_body.inc"
}
// gaq_policy_grad_ppo_lstm_seq_idx_dev's: grad_lstm_kernel<true> over the columns idx names
__global__ __launch_bounds__(kGradBlock) void grad_lstm_idx_kernel(LstmArgs g) {
  constexpr bool Bwd = true, Idx = true;
#include "gaq_policy_grad_lstm_body.inc"
}

// gaq.h's formula
size_t lstm_lds(const PolicyDev& pd, bool bwd) {
  const int H = pd.width[0];
  int head = H;
  for (int l = 1; l < pd.n_hidden; ++l) head += pd.width[l];
  const int rows = ((pd.in_dim + 15) & ~15) + (bwd ? 3 : 1) * H + (bwd ? std::max(4 * H, head) : head);
  return (size_t)kSeqHeadBytes + (size_t)rows * kGradStride * 4;
}

// the arguments the calls share, checked: T, S, the handle's view, log_std
struct LstmCall {
  const char* who;
  GradNet v;
  LstmArgs g{};
};

int lstm_begin(LstmCall& c, gaq_policy* p, int32_t T, int64_t S) {
  const std::string who = std::string(c.who) + ": ";
  if (int rc = policy_grad_lstm_view(p, c.v)) return rc;
  if (T < 1) return fail(GAQ_ERR_INVALID, who + "T must be at least 1");
  if (S < 0) return fail(GAQ_ERR_INVALID, who + "S must not be negative");
  const PolicyNet& net = *c.v.net;
  LstmArgs& g = c.g;
  g.net = net.pd; g.off_hh = c.v.off_hh; g.nm = policy_norm_dev(net.norm);
  g.T = T; g.S = S; g.ntiles = (S + kTile - 1) / kTile;
  grad_fill_std(c.v, g.log_std, g.inv_std);
  g.wv = c.v.wv;
  return GAQ_OK;
}

// the checks every call ends with (alignment, overlaps, sizes), then the device
int lstm_ready(const LstmCall& c, bool bwd, bool wide, bool misaligned, const std::vector<Span>& in, const std::vector<Span>& out, size_t& lds) {
  const std::string who = std::string(c.who) + ": ";
  if (misaligned)
    return fail(GAQ_ERR_INVALID, who + "pointers must be 4-byte aligned (h0, c0" + (bwd ? "" : ", h_out, c_out") + ": 16" +
                                     (wide && bwd ? ", stats_out: 8" : "") + ")");
  if (int rc = check_overlap(c.who, in, out)) return rc;
  lds = lstm_lds(c.g.net, bwd);
  if (lds > kGradLdsMax) return fail(GAQ_ERR_INVALID, who + "in_dim too large for the sequence kernel's LDS");
  if (c.g.ntiles > ((int64_t)1 << 31) - 1 || (int64_t)c.g.T * c.g.S > ((int64_t)1 << 40))
    return fail(GAQ_ERR_INVALID, who + "too many sequences or steps for one launch");
  HIP_TRY(hipSetDevice(c.v.net->device));
  return GAQ_OK;
}

// gaq_policy_grad_ppo_lstm_seq_dev (gather = false, S_src = S) and its idx form: the inputs span S_src columns, idx spans S words, and
// the idx form's stats_out is one double longer
int lstm_grad_call(const char* name, bool gather, gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                   const float* actions, const uint8_t* done, const float* h0, const float* c0, const float* logp_old, const float* adv,
                   const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                   float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  LstmCall c{name};
  if (int rc = lstm_begin(c, p, T, S)) return rc;
  const std::string who = std::string(c.who) + ": ";
  LstmArgs& g = c.g;
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
                          {h0, (size_t)S_src * H * 4, SPAN_ROWS, 16}, {c0, (size_t)S_src * H * 4, SPAN_ROWS, 16},
                          {logp_old, n * 4, SPAN_ROWS}, {adv, n * 4, SPAN_ROWS}, {ret, n * 4, hasv ? SPAN_ROWS : SPAN_OPTIONAL},
                          {v_old, n * 4, SPAN_OPTIONAL}};
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
  if (int rc = lstm_ready(c, true, wide, misaligned, in, out, lds)) return rc;
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
  // the scratch (grad_scratch) with the tape [G][T][64][2][H] behind its fixed part: a graph captured after a call with the largest T
  // (and S) stays valid
  g.pstride = grad_stride_max(net);
  if (int rc = grad_scratch(net, G, (size_t)G * (size_t)T * kTile * 2 * H * sizeof(float), g.spart, g.part, g.tape)) return rc;
  g.obs = obs; g.a = actions; g.done = done; g.h0 = h0; g.c0 = c0; g.logp_old = logp_old; g.adv = adv; g.ret = ret; g.v_old = v_old;
  g.clip = clip_eps; g.scale = scale; g.vclip = hasv ? vclip : 0.0f; g.vf_coef = hasv ? vf_coef : 0.0f;
  g.idx = idx; g.S_src = S_src;
  if (int rc = grad_launch(gather ? grad_lstm_idx_kernel : grad_lstm_kernel<true>, g, G, lds, st)) return rc;
  GradReduce r{};
  r.part = g.part; r.spart = g.spart; r.G = G; r.pstride = g.pstride; r.nw = net.nw; r.nv = nv; r.rows = (int64_t)T * S;
  r.ent = -(double)ent_coef * (double)scale * (double)T * (double)S;
  r.grad_out = grad_out; r.value_out = grad_value_out; r.stats_out = stats_out; r.log_std_out = grad_log_std_out;
  grad_route(r, true, 5, gather);
  return grad_reduce(r, st);
}

}  // namespace

extern "C" {

int gaq_policy_eval_lstm_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                 const float* h0, const float* c0, float* logp_out, float* value_out, float* mean_out, float* h_out,
                                 float* c_out, void* stream) {
  LstmCall c{"gaq_policy_eval_lstm_seq_dev"};
  if (int rc = lstm_begin(c, p, T, S)) return rc;
  LstmArgs& g = c.g;
  const size_t n = (size_t)T * (size_t)S, H = (size_t)g.net.width[0];
  const std::vector<Span> in = {{obs, n * g.net.in_dim * 4, SPAN_ROWS}, {actions, n * 16, logp_out ? SPAN_ROWS : SPAN_OPTIONAL},
                                {done, n, SPAN_ROWS, 1}, {h0, (size_t)S * H * 4, SPAN_ROWS, 16}, {c0, (size_t)S * H * 4, SPAN_ROWS, 16}};
  const std::vector<Span> out = {{logp_out, n * 4, SPAN_OPTIONAL}, {value_out, n * 4, SPAN_OPTIONAL}, {mean_out, n * 16, SPAN_OPTIONAL},
                                 {h_out, (size_t)S * H * 4, SPAN_OPTIONAL, 16}, {c_out, (size_t)S * H * 4, SPAN_OPTIONAL, 16}};
  bool wide = false, misaligned = false;
  if (int rc = check_span_nulls(in, out, S > 0, wide, misaligned)) return rc;
  if (value_out && !c.v.wv)
    return fail(GAQ_ERR_STATE, "policy: no value head set (gaq_policy_set_value_head): the actor-critic passes need V on the policy's trunk");
  if (logp_out && !c.v.explore)
    return fail(GAQ_ERR_STATE, "policy: no log_std set (gaq_policy_set_explore): a deterministic policy has no log-probability");
  size_t lds = 0;
  if (int rc = lstm_ready(c, false, wide, misaligned, in, out, lds)) return rc;
  if (S == 0) return GAQ_OK;
  g.obs = obs; g.a = actions; g.done = done; g.h0 = h0; g.c0 = c0;
  g.logp_out = logp_out; g.value_out = value_out; g.mean_out = mean_out; g.h_out = h_out; g.c_out = c_out;
  g.S_src = S;
  if (!value_out) g.wv = nullptr;                                 // V's parts are not summed where nobody reads them
  return grad_launch(grad_lstm_kernel<false>, g, (int)std::min<int64_t>(g.ntiles, (int64_t)1 << 20), lds, (hipStream_t)stream);
}

int gaq_policy_grad_ppo_lstm_seq_dev(gaq_policy* p, int32_t T, int64_t S, const float* obs, const float* actions, const uint8_t* done,
                                     const float* h0, const float* c0, const float* logp_old, const float* adv, const float* ret,
                                     const float* v_old, float clip_eps, float vclip, float vf_coef, float ent_coef, float scale,
                                     float* grad_out, float* grad_value_out, float* grad_log_std_out, double* stats_out, void* stream) {
  return lstm_grad_call("gaq_policy_grad_ppo_lstm_seq_dev", false, p, T, S, nullptr, S, obs, actions, done, h0, c0, logp_old, adv, ret, v_old,
                        clip_eps, vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

int gaq_policy_grad_ppo_lstm_seq_idx_dev(gaq_policy* p, int32_t T, int64_t S, const int32_t* idx, int64_t S_src, const float* obs,
                                         const float* actions, const uint8_t* done, const float* h0, const float* c0, const float* logp_old,
                                         const float* adv, const float* ret, const float* v_old, float clip_eps, float vclip, float vf_coef,
                                         float ent_coef, float scale, float* grad_out, float* grad_value_out, float* grad_log_std_out,
                                         double* stats_out, void* stream) {
  return lstm_grad_call("gaq_policy_grad_ppo_lstm_seq_idx_dev", true, p, T, S, idx, S_src, obs, actions, done, h0, c0, logp_old, adv, ret,
                        v_old, clip_eps, vclip, vf_coef, ent_coef, scale, grad_out, grad_value_out, grad_log_std_out, stats_out, stream);
}

}  // extern "C"
