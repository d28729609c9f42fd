// gaq_grad.hpp -- what gaq_policy_grad.hip (the learner's forward-on-stored-rows and backward passes) needs of the policy and critic
// handles, whose definitions stay in gaq_policy.hip: one plain view of a feed-forward fp32 MFMA net, filled by that unit.  Included after
// gaq_host.hpp by those two units; internal to csrc/ like it.
#pragma once

#pragma GCC visibility push(hidden)

constexpr int kGradMaxWidth = 128;   // hidden widths the gradient kernel takes (gaq.h "gradients on the device")

struct GradView {
  PolicyDev net;                  // the trunk in PolicyDev's terms (w, in_dim, n_hidden, hidden_act, out_tanh, width, off)
  int n_out = 0;                  // 4: a policy (output layer [in][4], bias[4]); 1: a critic (w[in], bias)
  int device = 0;
  int64_t nw = 0;                 // floats of the packed layout
  const float* norm_tab = nullptr;   // the attached normaliser's published table (nullptr: none) and its D
  int norm_dim = 0;
  bool explore = false;           // a policy with log_std set
  float log_std[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  void** scratch = nullptr;       // the handle's partial-gradient scratch (library-owned, freed with the handle) and its size
  size_t* scratch_bytes = nullptr;
};

// gaq_policy.hip: GAQ_ERR_INVALID (the text names the engine or the width) unless p is a feed-forward fp32 MFMA policy of widths <= 128
// with weights set; the same for a critic
int policy_grad_view(gaq_policy* p, GradView& v);
int critic_grad_view(gaq_critic* c, GradView& v);

#pragma GCC visibility pop
