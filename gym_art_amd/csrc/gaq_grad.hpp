// gaq_grad.hpp -- the record a policy handle and a critic handle have in common (both are defined in gaq_policy.hip and embed one), and
// what gaq_policy_grad.hip and gaq_policy_grad_seq.hip (the learner's forward-on-stored-rows and backward passes) need besides it: the
// host side of a gradient call, one of each (their device side is gaq_grad_dev.hpp).  Included after gaq_host.hpp and gaq_norm.hpp;
// internal to csrc/ like them.
#pragma once

#pragma GCC visibility push(hidden)

constexpr int kGradMaxWidth = 128;   // hidden widths the gradient kernel takes (gaq.h "gradients on the device")

// One feed-forward trunk with packed weights on one device, validated against one env.  Host-only: never a kernel argument (the kernels
// take its `pd`, or a PolicyCriticDev filled from it).
struct PolicyNet {
  int device = 0;
  const gaq_env* env = nullptr;   // the handle it was validated against (compared, never dereferenced after create)
  PolicyDev pd{};                 // the trunk in PolicyDev's terms (pd.w = w_dev; a critic's out_tanh, explore and scratch_bytes stay 0)
  int n_out = 0;                  // 4: a policy (output layer [in][4], bias[4]); 1: a critic (w[in], bias)
  int64_t nw = 0;                 // floats of the packed layout (net_layout)
  float* w_dev = nullptr;
  bool weights_set = false;
  int rows = 0;                   // activation rows of a tile (net_act_rows)
  const gaq_obs_norm* norm = nullptr;   // the attached normaliser, the caller's: it outlives the handle
  void* grad_scratch = nullptr; size_t grad_scratch_bytes = 0;   // gaq_policy_grad.hip: the workgroups' partial gradients, allocated on first use
};

// what a gradient pass takes of a handle: its record and, of a policy, the caller's log_std (nullptr: a critic), whether it explores
// and its value head
struct GradNet {
  PolicyNet* net = nullptr;
  const float* log_std = nullptr;
  bool explore = false;
  const float* wv = nullptr;      // a policy's value head on the device (last width weights, bias), nullptr while none is set
  int32_t off_hh = 0;             // policy_grad_seq_view: float offset of W_hh' in the packed weights
  const float* tab = nullptr;     // device mode (gaq_policy_set_explore_dev): the table log_std[4] | std[4] | inv_std[4] the kernels read
};

// gaq_policy.hip: GAQ_ERR_INVALID (the text names the engine or the width) unless p is a feed-forward fp32 MFMA policy of widths <= 128
// with weights set; the same for a critic
int policy_grad_view(gaq_policy* p, GradNet& v);
int critic_grad_view(gaq_critic* c, GradNet& v);
// gaq_policy.hip, for the wide forms (gaq.h "the wide learner"): the same views without the width limit -- hidden widths up to 256, as
// the handles are created -- under the one LDS rule instead: in_dim rounded up to 16 + the sum of the hidden widths <= kGradWideRows
// (the text names LDS and the sum).  Three layers of 256 do not pass: their activations do not fit a 64-row tile's LDS.
constexpr int kGradWideRows = 560;
int policy_grad_wide_view(gaq_policy* p, GradNet& v);
int critic_grad_wide_view(gaq_critic* c, GradNet& v);
// gaq_policy.hip, for gaq_policy_grad_seq.hip: GAQ_ERR_INVALID unless p is a policy with the cell `cell` (GAQ_POLICY_CELL_GRU or _LSTM;
// the text says that a recurrent cell is required, or names the other cell) of H and head widths <= 64 ("width") with weights set;
// v.off_hh is then W_hh's offset in the packed weights
constexpr int kGradSeqMaxWidth = 64;
int policy_grad_seq_view(gaq_policy* p, int cell, GradNet& v);
// gaq_policy.hip, for the wide recurrent learner (gaq.h "the wide recurrent learner"): GAQ_ERR_INVALID, each with a text of its own,
// unless p is a GRU policy without an encoder (a feed-forward policy, the LSTM -- named -- and "encoder" are refused) of H <=
// kGradSeqWideMaxWidth and head widths <= kGradSeqMaxWidth ("width") with weights set; v.off_hh as above
constexpr int kGradSeqWideMaxWidth = 128;
int policy_grad_seq_wide_view(gaq_policy* p, GradNet& v);
// gaq_policy.hip, for gaq_policy_grad_seq.hip's calls on a policy with an ENCODER in front of the cell (gaq.h "sequences through an
// encoder"): the view above of either cell -- v.net->pd.in_dim is then E, the encoder's last width -- and the encoder.  cell_args:
// whether the caller passed an LSTM's c0 or c_out.  GAQ_ERR_INVALID, each with a text of its own: a policy without an encoder
// ("encoder"), c0 / c_out on a GRU, an encoder or cell or head layer wider than the gradient kernels take ("width"), encoder weights
// or weights never set.
struct GradEnc {
  const gaq_policy* p = nullptr;
  bool lstm = false;              // the handle's cell
  int32_t in_dim = 0, width = 0;  // the env's obs_dim; E
  PolicyDev trunk{};              // the encoder's layers (w = the block the rollout reads and the optimiser would step)
  int64_t nw = 0;                 // floats of its block (gaq_policy_encoder_weight_count)
};
int policy_grad_enc_seq_view(gaq_policy* p, bool cell_args, GradNet& v, GradEnc& e);
// gaq_policy.hip: one launch of the rollout's policy_encode_kernel on st -- obs [rows, e.in_dim], through the policy's normaliser where
// one is attached, -> feat [rows, e.width] (16-byte aligned), the rollout's bits.  rows >= 1.
int policy_encode_rows(const GradEnc& e, int64_t rows, const float* obs, float* feat, hipStream_t st);
// the gathered form (policy_encode_term_kernel): row list[j] of obs -> row list[j] of feat, j < *count; `slots` >= *count sizes the grid
int policy_encode_list(const GradEnc& e, int64_t slots, const uint32_t* list, const uint32_t* count, const float* obs, float* feat, hipStream_t st);

// what the optimiser (gaq_optim.hip) takes of a handle: the record whose w_dev it steps in place, and of a policy the value head as it
// stands now (head = its W + 1 floats, 0 while none is set) and the caller's log_std on the host (explore: whether it is in use)
struct OptimView {
  PolicyNet* net = nullptr;
  float* wv = nullptr;
  int head = 0;
  bool explore = false;
  const float* log_std = nullptr;
  float* tab = nullptr;           // the exploration table registered with the policy (nullptr: host mode), whether it explores or not
  float* enc_w = nullptr;         // policy_optim_enc_view: the encoder's block, where the rollout's encoder kernel reads it
  int64_t enc_nw = 0;             // ... and its floats (0: no fourth group)
};
// gaq_policy.hip: GAQ_ERR_INVALID for the bf16 engine (the text names it: its repacked fragments would go stale) and for weights never set
int policy_optim_view(gaq_policy* p, OptimView& v);
// the same for a recurrent policy WITH an encoder (gaq_optim_create_policy_enc): GAQ_ERR_INVALID for a policy without one ("encoder"),
// for encoder weights or weights never set
int policy_optim_enc_view(gaq_policy* p, OptimView& v);
int critic_optim_view(gaq_critic* c, OptimView& v);

// ---- what the two gradient units share of a call's checks and of its split into workgroups ------------------------------------------
constexpr int kGradGroups = 512;                                  // G's default, by measurement (DESIGN.md 4a "Gradients on the device")
// one input or output of an entry point: its bytes, the alignment the kernels need, and when a null pointer is refused
enum SpanNeed { SPAN_ROWS, SPAN_ALWAYS, SPAN_OPTIONAL };              // required when rows > 0 / always / never
struct Span { const void* p; size_t bytes; SpanNeed need; size_t align = 4; };
inline bool spans_overlap(const Span& a, const Span& b) {
  if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
// GAQ_ERR_INVALID if an output overlaps an input or another output
inline int check_overlap(const char* who, const std::vector<Span>& in, const std::vector<Span>& out) {
  for (size_t i = 0; i < out.size(); ++i) {
    for (const Span& s : in)
      if (spans_overlap(out[i], s)) return fail(GAQ_ERR_INVALID, std::string(who) + ": an output overlaps an input");
    for (size_t j = i + 1; j < out.size(); ++j)
      if (spans_overlap(out[i], out[j])) return fail(GAQ_ERR_INVALID, std::string(who) + ": two outputs overlap");
  }
  return GAQ_OK;
}
// GAQ_ERR_INVALID for a null pointer that the call needs (have_rows: the call has rows to work on); else whether any span asks for more
// than a float's alignment and whether any pointer misses its own
inline int check_span_nulls(const std::vector<Span>& in, const std::vector<Span>& out, bool have_rows, bool& wide, bool& misaligned) {
  wide = misaligned = false;
  for (const std::vector<Span>* spans : {&in, &out})
    for (const Span& s : *spans) {
      if (!s.p && (s.need == SPAN_ALWAYS || (s.need == SPAN_ROWS && have_rows))) return fail(GAQ_ERR_INVALID, "null argument");
      wide |= s.align > 4;
      misaligned |= (reinterpret_cast<uintptr_t>(s.p) & (s.align - 1)) != 0;
    }
  return GAQ_OK;
}
// the number of workgroups: min(tiles, GAQ_GRAD_GROUPS or kGradGroups) -- a function of the tile count and the environment alone
inline int grad_groups(int64_t ntiles) {
  int64_t G = kGradGroups;
  if (const char* s = std::getenv("GAQ_GRAD_GROUPS")) {
    const long v = std::strtol(s, nullptr, 10);
    if (v >= 1 && v <= 65536) G = v;
  }
  return (int)std::min<int64_t>(G, ntiles);
}

// ---- one of each for the two gradient units: the scratch, log_std, the PPO refusals, the launch, the reduce ----------------------------
constexpr int kGradStats = 8;      // doubles per workgroup of the narrow forms: 3 sums of the loss's statistics, 4 of dlog_std, 1 spare
constexpr int kGradStatsAc = 10;   // the wide forms (shared trunk, sequences): those 7, the value loss, the rows its clip cut, 1 spare

// The handle's scratch, one layout for every form: the statistics [max(G, kGradGroups)][kGradStatsAc] at the base, the partials
// [G][stride] behind them, `tape_bytes` (the sequence unit's tape) behind those.  The fixed part is sized for the default number of
// workgroups and for the stride with a value head whatever this call needs, so `part` moves with no call's G or form.  The scratch grows
// when a call needs more than every call before it (a GAQ_GRAD_GROUPS above the default, a longer tape), and only then do its pointers
// move: a captured graph keeps its own.
inline int64_t grad_stride_max(const PolicyNet& net) {   // floats of a workgroup's partial with a value head's words
  return (net.nw + net.pd.width[net.pd.n_hidden - 1] + 1 + 15) & ~(int64_t)15;
}
inline int grad_scratch(PolicyNet& net, int G, size_t tape_bytes, double*& spart, float*& part, float*& tape) {
  const int64_t stride = grad_stride_max(net);
  const size_t groups = (size_t)std::max(G, kGradGroups);
  const size_t fixed = groups * ((size_t)stride * sizeof(float) + kGradStatsAc * sizeof(double));
  if (net.grad_scratch_bytes < fixed + tape_bytes) {
    if (net.grad_scratch) { HIP_TRY(hipFree(net.grad_scratch)); net.grad_scratch = nullptr; net.grad_scratch_bytes = 0; }
    HIP_TRY(hipMalloc(&net.grad_scratch, fixed + tape_bytes));
    net.grad_scratch_bytes = fixed + tape_bytes;
  }
  spart = reinterpret_cast<double*>(net.grad_scratch);
  part = reinterpret_cast<float*>(spart + groups * kGradStatsAc);
  tape = reinterpret_cast<float*>(reinterpret_cast<char*>(net.grad_scratch) + fixed);
  return GAQ_OK;
}

// the caller's log_std (0 where the handle has none, or keeps it in a table on the device: the kernels then read that) and
// exp(-log_std), as the row stages take them
inline void grad_fill_std(const GradNet& v, float (&log_std)[4], float (&inv_std)[4]) {
  for (int k = 0; k < 4; ++k) {
    log_std[k] = v.log_std && !v.tab ? v.log_std[k] : 0.0f;
    inv_std[k] = (float)std::exp(-(double)log_std[k]);
  }
}

// the refusals every PPO gradient shares, in the order they are reported (has_value: the form has a value loss)
inline int check_ppo_hyper(const std::string& who, float clip, float vclip, float vf_coef, float ent_coef, bool has_value, const float* v_old,
                           bool have_rows) {
  if (!(clip > 0.0f && clip < 1.0f)) return fail(GAQ_ERR_INVALID, who + "clip_eps must be in (0, 1)");
  if (!(vclip >= 0.0f)) return fail(GAQ_ERR_INVALID, who + "vclip must not be negative or NaN");
  if (vf_coef != vf_coef || ent_coef != ent_coef) return fail(GAQ_ERR_INVALID, who + "vf_coef or ent_coef is NaN");
  if (vclip > 0.0f && has_value && !v_old && have_rows) return fail(GAQ_ERR_INVALID, who + "vclip > 0 needs v_old");
  return GAQ_OK;
}

// one tile kernel on G workgroups of 256 threads: LDS above 64 KiB is asked for first
template <class Args>
int grad_launch(void (*kernel)(Args), const Args& g, int G, size_t lds, hipStream_t st) {
  if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)G), dim3(256), lds, st, g);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

// What grad_reduce_kernel (gaq_policy_grad.hip) takes.  grad_out[j] = the G partials of word j summed in ascending order in fp64 and
// rounded once, the words nw .. nw + nv - 1 going to value_out; block 0 sums the workgroups' `ns` statistics the same way.  Sum k goes
// to stats_out[slot[k]] (slot < 0: nowhere), `rows` to stats_out[rows_slot]; the sums 3 .. 6 go to log_std_out as (float)(sum + ent).
struct GradReduce {
  const float* part;
  const double* spart;
  int32_t G, ns;                  // ns: kGradStats or kGradStatsAc
  int64_t pstride, nw, nv, rows;
  double ent;                     // the entropy bonus's -ent_coef * scale * rows, formed in fp64 by the host (the narrow forms: 0)
  float *grad_out, *value_out;
  double* stats_out;              // nullptr (with log_std_out): no statistics (gaq_policy_backward_dev)
  float* log_std_out;
  int8_t slot[kGradStatsAc], rows_slot;
};
// The routing of the five layouts.  Narrow (wide = false): the sums 0 .. n_stat - 1 to the slots of the same number, `rows` to slot
// n_stat, the idx forms' skipped indices (the last sum, 7) to slot n_stat + 1.  Wide: the sums 0, 1, 2, 7, 8 to the slots 0 .. 4,
// `rows` to slot 5, the skipped indices (sum 9) to slot 6.
inline void grad_route(GradReduce& r, bool wide, int n_stat, bool idx) {
  r.ns = wide ? kGradStatsAc : kGradStats;
  for (int k = 0; k < kGradStatsAc; ++k) r.slot[k] = -1;
  if (wide) n_stat = 5;
  for (int k = 0; k < n_stat; ++k) r.slot[wide && k >= 3 ? k + 4 : k] = (int8_t)k;
  r.rows_slot = (int8_t)n_stat;
  if (idx) r.slot[r.ns - 1] = (int8_t)(n_stat + 1);
}
// gaq_policy_grad.hip: launches grad_reduce_kernel on st
int grad_reduce(const GradReduce& r, hipStream_t st);

// gaq_policy_grad.hip, for gaq_policy_grad_seq.hip's encoder forms: the backward of a trunk without an output layer over `rows` stored
// rows, from the gradient in its last layer's output dfeat [., E] (grad_feat_kernel) -> the G workgroups' partials [G][pstride] in the
// trunk's packed layout, which grad_reduce then sums.  rowidx (nullptr: row j is row j): [rows] source rows of obs and dfeat, negative
// entries dead.  grad_feat_lds: its LDS.  grad_rowidx_run: one elementwise launch, rowidx[t S + j] = t S_src + idx[j] (an index outside
// [0, S_src): negative), list[t S + j] the same with column 0 in a bad index's place, *count = T S.
struct GradFeatCall {
  PolicyDev trunk;
  const float* nm_tab;            // the attached normaliser's table (PolObsNorm's two words; nullptr: none)
  int32_t nm_dim;
  int64_t rows;
  const float *obs, *dfeat;
  const int32_t* rowidx;
  float* part;
  int64_t pstride;
  int G;
};
size_t grad_feat_lds(const PolicyDev& trunk, bool idx);
int grad_feat_run(const GradFeatCall& c, hipStream_t st);
int grad_rowidx_run(int32_t T, int64_t S, const int32_t* idx, int64_t S_src, int32_t* rowidx, uint32_t* list, uint32_t* count, hipStream_t st);

#pragma GCC visibility pop
