// gaq_grad.hpp -- the record a policy handle and a critic handle have in common (both are defined in gaq_policy.hip and embed one), and
// what gaq_policy_grad.hip (the learner's forward-on-stored-rows and backward passes) needs besides it.  Included after gaq_host.hpp and
// gaq_norm.hpp by those two units; internal to csrc/ like them.
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
};

// gaq_policy.hip: GAQ_ERR_INVALID (the text names the engine or the width) unless p is a feed-forward fp32 MFMA policy of widths <= 128
// with weights set; the same for a critic
int policy_grad_view(gaq_policy* p, GradNet& v);
int critic_grad_view(gaq_critic* c, GradNet& v);
// gaq_policy.hip, for gaq_policy_grad_seq.hip: GAQ_ERR_INVALID unless p is a GRU policy (the text says that a recurrent cell is required,
// or names the LSTM) of H and head widths <= 64 ("width") with weights set; v.off_hh is then W_hh's offset in the packed weights
constexpr int kGradSeqMaxWidth = 64;
int policy_grad_seq_view(gaq_policy* p, GradNet& v);

// what the optimiser (gaq_optim.hip) takes of a handle: the record whose w_dev it steps in place, and of a policy the value head as it
// stands now (head = its W + 1 floats, 0 while none is set) and the caller's log_std on the host (explore: whether it is in use)
struct OptimView {
  PolicyNet* net = nullptr;
  float* wv = nullptr;
  int head = 0;
  bool explore = false;
  const float* log_std = nullptr;
};
// gaq_policy.hip: GAQ_ERR_INVALID for the bf16 engine (the text names it: its repacked fragments would go stale) and for weights never set
int policy_optim_view(gaq_policy* p, OptimView& v);
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

#pragma GCC visibility pop
