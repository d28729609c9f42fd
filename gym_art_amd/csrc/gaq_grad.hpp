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
};

// gaq_policy.hip: GAQ_ERR_INVALID (the text names the engine or the width) unless p is a feed-forward fp32 MFMA policy of widths <= 128
// with weights set; the same for a critic
int policy_grad_view(gaq_policy* p, GradNet& v);
int critic_grad_view(gaq_critic* c, GradNet& v);

#pragma GCC visibility pop
