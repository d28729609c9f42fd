// gaq_optim.hip -- Adam / AdamW on the device (include/gaq.h "the optimiser on the device"): clips the gradient buffers the gradient calls
// write by their global norm and steps a policy's or a critic's weights in place, in the buffers the rollout and gradient kernels read,
// with no host synchronisation and nothing in the kernel arguments that changes from step to step -- a captured step replays.
// What it needs of the two handles is gaq_grad.hpp's OptimView (gaq_policy.hip fills it).
#include "gaq_host.hpp"
#include "gaq_grad.hpp"

namespace {
constexpr int kOptBlock = 256;                    // threads of a workgroup of the two-launch form
constexpr int kOptPer = 8;                        // elements per thread: a chunk is kOptBlock * kOptPer consecutive elements
constexpr int kOptChunk = kOptBlock * kOptPer;
constexpr int kOptOneBlock = 1024;                // threads of the one workgroup of the one-launch form
constexpr int kOptGroups = 3;                     // the packed weights, the value head, log_std
constexpr int kOptGroupsEnc = 4;                  // ... and, for a recurrent policy with an encoder, the encoder's block (after log_std)
constexpr int kOptLogStd = 2;
constexpr int kOptTabStd = 4, kOptTabInvStd = 8;  // float offsets of std[4] and inv_std[4] in a policy's exploration table

// what lives in device memory so that a replayed step sees it: the hyper-parameters and the counters.  Each counter is two words: the
// sum-of-squares launch copies `commit` to `read`, every workgroup of the update launch reads `read`, and one of them writes `commit` --
// no workgroup of a launch reads a word another workgroup of that launch writes.
struct OptimHyper { double lr, beta1, beta2, eps, weight_decay, max_grad_norm; };
struct OptimCtl {
  OptimHyper hp;
  uint64_t t_read, t_commit;                      // steps taken
  uint64_t skipped_read, skipped_commit;          // steps refused for a non-finite gradient norm
};

// one step's arguments: the groups as one index space [0, end[last]), group k being [end[k-1], end[k]).  OptimDev, three groups, is the
// record every handle but an encoder policy's steps with; OptimDevEnc has the encoder's block as group 3, after log_std
// (gaq_optim_create_policy_enc).
template <int NG>
struct OptimDevT {
  float* theta[NG];
  const float* grad[NG];
  int32_t end[NG];
  float* m; float* v;         // [end[NG-1]] each, the groups concatenated
  double* partial;            // [nchunks]: each chunk's sum of squares
  OptimCtl* ctl;
  double* stats;              // 4 doubles of the caller's, or nullptr
  int32_t nchunks;
  // a device-mode policy (gaq_policy_set_explore_dev): its table log_std[4] | std[4] | inv_std[4]; theta[kOptLogStd] is then
  // the table's log_std, and the lane that steps element k publishes std[k] and inv_std[k] beside it.  nullptr: a master copy
  float* tab;
};
using OptimDev = OptimDevT<kOptGroups>;
using OptimDevEnc = OptimDevT<kOptGroupsEnc>;

// the scalars of one step, formed in fp64 by one lane and rounded once for the fp32 work on the elements
struct OptimScal {
  float coef, omb1, b2, omb2, decay, step, bc2s, eps;
  int32_t skip;
};

__device__ inline double optim_pow(double b, uint64_t t) {      // b^t by squaring: a function of (b, t) alone
  double r = 1.0;
  while (t) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// the scalars from the squared norm and the step count; the lane that calls it also writes the caller's statistics
__device__ inline OptimScal optim_scalars(const OptimHyper& c, double sumsq, uint64_t t0, double* stats) {
  OptimScal s;
  const bool finite = sumsq - sumsq == 0.0;       // false for Inf and NaN
  const double norm = sqrt(sumsq);
  double coef = 1.0;
  if (c.max_grad_norm > 0.0) coef = fmin(1.0, c.max_grad_norm / (norm + 1e-6));
  const uint64_t t = t0 + 1;
  s.skip = finite ? 0 : 1;
  s.coef = (float)coef;
  s.omb1 = (float)(1.0 - c.beta1);
  s.b2 = (float)c.beta2;
  s.omb2 = (float)(1.0 - c.beta2);
  s.decay = (float)(1.0 - c.lr * c.weight_decay);
  s.step = (float)(c.lr / (1.0 - optim_pow(c.beta1, t)));
  s.bc2s = (float)sqrt(1.0 - optim_pow(c.beta2, t));
  s.eps = (float)c.eps;
  if (stats) {
    stats[0] = norm;
    stats[1] = finite ? coef : 0.0;
    stats[2] = (double)(finite ? t : t0);
    stats[3] = finite ? 0.0 : 1.0;
  }
  return s;
}

// the sum of a workgroup's values in a fixed tree; every lane calls it, lane 0 holds the result.  (Dev: the record of the kernel that
// calls it, OptimDevT<NG>, and nothing else -- it makes an instantiation per kernel, each with its one caller.  Shared between the
// three- and the four-group kernels it is not inlined the same way, and the sum-of-squares and one-launch kernels get other
// instructions: this argument is what keeps them.)
template <int B, class Dev> __device__ inline double optim_block_sum(double x, double* red) {
  red[threadIdx.x] = x;
  __syncthreads();
  for (int w = B / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// The element helpers (optim_group, optim_base, optim_square; optim_element: m, v and theta of index i, gaq_policy_set_explore's formula
// for a device-mode log_std by the lane that owns the word, decoupled weight decay never on log_std) and the three step kernels, as
// templates over the group count NG: three for every handle but an encoder policy's, that one's four (the encoder's block as group 3).
//   optim_sumsq_kernel     launch 1 of 2: partial[c] = the sum of squares of chunk c, each lane its elements in ascending order, then
//                          the tree
//   optim_update_kernel    launch 2 of 2: every workgroup adds the partials in ascending order, forms the scalars and updates its chunk;
//                          workgroup 0 commits (only the hyper-parameters and the two "read" words are loaded in this launch)
//   optim_step_one_kernel  the one-launch form: one workgroup takes the norm (each lane its elements in ascending order, then the tree)
//                          and updates everything (one workgroup: nobody else reads or writes the record in this launch)
template <int NG> __device__ inline int optim_group(const OptimDevT<NG>& d, int i) {
  return i < d.end[0] ? 0 : i < d.end[1] ? 1 : NG == kOptGroups || i < d.end[2] ? 2 : 3;
}
template <int NG> __device__ inline int optim_base(const OptimDevT<NG>& d, int g) { return g ? d.end[g - 1] : 0; }
template <int NG> __device__ inline double optim_square(const OptimDevT<NG>& d, int i) {
  const int g = optim_group(d, i);
  const double x = (double)d.grad[g][i - optim_base(d, g)];
  return x * x;
}
template <int NG> __device__ inline void optim_element(const OptimDevT<NG>& d, const OptimScal& s, int i) {
  const int g = optim_group(d, i);
  const int k = i - optim_base(d, g);
  const float gr = s.coef * d.grad[g][k];
  float m = d.m[i], v = d.v[i];
  m = m + s.omb1 * (gr - m);
  v = s.b2 * v + s.omb2 * (gr * gr);
  const float denom = sqrtf(v) / s.bc2s + s.eps;
  const float decay = g == kOptLogStd ? 1.0f : s.decay;
  const float x = d.theta[g][k] * decay - s.step * (m / denom);
  d.theta[g][k] = x;
  d.m[i] = m;
  d.v[i] = v;
  if (g == kOptLogStd && d.tab) {
    d.tab[kOptTabStd + k] = (float)exp((double)x);
    d.tab[kOptTabInvStd + k] = (float)exp(-(double)x);
  }
}
template <int NG> __global__ __launch_bounds__(kOptBlock) void optim_sumsq_kernel(OptimDevT<NG> d) {
  __shared__ double red[kOptBlock];
  const int total = d.end[NG - 1];
  const int base = (int)blockIdx.x * kOptChunk;
  double acc = 0.0;
  for (int k = 0; k < kOptPer; ++k) {
    const int i = base + k * kOptBlock + (int)threadIdx.x;
    if (i < total) acc += optim_square(d, i);
  }
  const double sum = optim_block_sum<kOptBlock, OptimDevT<NG>>(acc, red);
  if (threadIdx.x == 0) {
    d.partial[blockIdx.x] = sum;
    if (blockIdx.x == 0) {
      d.ctl->t_read = d.ctl->t_commit;
      d.ctl->skipped_read = d.ctl->skipped_commit;
    }
  }
}
template <int NG> __global__ __launch_bounds__(kOptBlock) void optim_update_kernel(OptimDevT<NG> d) {
  __shared__ double stage[kOptBlock];
  __shared__ OptimScal scal;
  double sumsq = 0.0;
  for (int c0 = 0; c0 < d.nchunks; c0 += kOptBlock) {
    const int c = c0 + (int)threadIdx.x;
    stage[threadIdx.x] = c < d.nchunks ? d.partial[c] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = min(kOptBlock, d.nchunks - c0);
      for (int k = 0; k < n; ++k) sumsq += stage[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const OptimHyper hp = d.ctl->hp;
    const uint64_t t0 = d.ctl->t_read;
    const OptimScal s = optim_scalars(hp, sumsq, t0, blockIdx.x == 0 ? d.stats : nullptr);
    scal = s;
    if (blockIdx.x == 0) {
      if (s.skip) d.ctl->skipped_commit = d.ctl->skipped_read + 1;
      else d.ctl->t_commit = t0 + 1;
    }
  }
  __syncthreads();
  const OptimScal s = scal;
  if (s.skip) return;
  const int total = d.end[NG - 1];
  const int base = (int)blockIdx.x * kOptChunk;
  for (int k = 0; k < kOptPer; ++k) {
    const int i = base + k * kOptBlock + (int)threadIdx.x;
    if (i < total) optim_element(d, s, i);
  }
}
template <int NG> __global__ __launch_bounds__(kOptOneBlock) void optim_step_one_kernel(OptimDevT<NG> d) {
  __shared__ double red[kOptOneBlock];
  __shared__ OptimScal scal;
  const int total = d.end[NG - 1];
  double acc = 0.0;
  for (int i = (int)threadIdx.x; i < total; i += kOptOneBlock) acc += optim_square(d, i);
  const double sumsq = optim_block_sum<kOptOneBlock, OptimDevT<NG>>(acc, red);
  if (threadIdx.x == 0) {
    const uint64_t t0 = d.ctl->t_commit;
    const OptimScal s = optim_scalars(d.ctl->hp, sumsq, t0, d.stats);
    scal = s;
    if (s.skip) d.ctl->skipped_commit += 1;
    else d.ctl->t_commit = t0 + 1;
  }
  __syncthreads();
  const OptimScal s = scal;
  if (s.skip) return;
  for (int i = (int)threadIdx.x; i < total; i += kOptOneBlock) optim_element(d, s, i);
}

__global__ void optim_set_lr_kernel(OptimCtl* ctl, double lr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ctl->hp.lr = lr;
}

int optim_check_desc(const gaq_optim_desc* d) {
  if (!d || d->struct_size != sizeof(gaq_optim_desc)) return fail(GAQ_ERR_INVALID, "gaq_optim_desc: struct_size mismatch (header vs library)");
  if (!(d->lr >= 0.0) || !std::isfinite(d->lr)) return fail(GAQ_ERR_INVALID, "optim: lr must be finite and not negative");
  if (!(d->beta1 >= 0.0 && d->beta1 < 1.0)) return fail(GAQ_ERR_INVALID, "optim: beta1 must be in [0, 1)");
  if (!(d->beta2 >= 0.0 && d->beta2 < 1.0)) return fail(GAQ_ERR_INVALID, "optim: beta2 must be in [0, 1)");
  if (!(d->eps > 0.0) || !std::isfinite(d->eps)) return fail(GAQ_ERR_INVALID, "optim: eps must be positive");
  if (!(d->weight_decay >= 0.0) || !std::isfinite(d->weight_decay)) return fail(GAQ_ERR_INVALID, "optim: weight_decay must be finite and not negative");
  if (!(d->max_grad_norm >= 0.0) || !std::isfinite(d->max_grad_norm))
    return fail(GAQ_ERR_INVALID, "optim: max_grad_norm must be finite and not negative (0: no clipping)");
  if (d->flags & ~(uint32_t)GAQ_OPTIM_STEP_LOG_STD) return fail(GAQ_ERR_INVALID, "optim: unknown flags");
  return GAQ_OK;
}
}  // namespace

extern "C" {

struct gaq_optim {
  gaq_policy* p = nullptr;        // the handle it steps: one of the two
  gaq_critic* c = nullptr;
  int device = 0;
  OptimDevEnc d{};                // grad and stats are filled per call; group 3 (the encoder's block) is empty unless `enc`
  bool enc = false;               // gaq_optim_create_policy_enc: steps the encoder's block too, through gaq_optim_step_enc_dev
  int head = 0;                   // floats of the value-head group (0: the handle had none at creation)
  bool steps_log_std = false;
  int launches = 2;               // 2, or 1 under GAQ_OPTIM_LAUNCHES=1 (DESIGN.md 4a "Adam on the device")
  void* block = nullptr;          // m, v, the master log_std, the partials and the control words: one allocation
  float* log_std_dev = nullptr;
  float log_std[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // the master copy as last synchronised (at creation: the handle's)
  float* tab = nullptr;           // the policy's exploration table at creation (nullptr: host mode): log_std is stepped there
};

namespace {
int optim_view(const gaq_optim* o, OptimView& v) {
  return o->enc ? policy_optim_enc_view(o->p, v) : o->p ? policy_optim_view(o->p, v) : critic_optim_view(o->c, v);
}
extern "C++" {                    // (templates below)
// the first groups of the handle's record as a launch takes them, and the launches
template <class Dev> void optim_launch(const gaq_optim* o, const OptimDevEnc& a, hipStream_t st, void (*sumsq)(Dev), void (*update)(Dev),
                                       void (*one)(Dev)) {
  Dev d{};
  for (size_t k = 0; k < sizeof(d.end) / sizeof(d.end[0]); ++k) { d.theta[k] = a.theta[k]; d.grad[k] = a.grad[k]; d.end[k] = a.end[k]; }
  d.m = a.m; d.v = a.v; d.partial = a.partial; d.ctl = a.ctl; d.stats = a.stats; d.nchunks = a.nchunks; d.tab = a.tab;
  if (o->launches == 1) {
    hipLaunchKernelGGL(one, dim3(1), dim3(kOptOneBlock), 0, st, d);
  } else {
    hipLaunchKernelGGL(sumsq, dim3((unsigned)d.nchunks), dim3(kOptBlock), 0, st, d);
    hipLaunchKernelGGL(update, dim3((unsigned)d.nchunks), dim3(kOptBlock), 0, st, d);
  }
}
}  // extern "C++"

int optim_create(gaq_policy* p, gaq_critic* c, const gaq_optim_desc* desc, gaq_optim** out, bool enc = false) {
  if ((!p && !c) || !desc || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = optim_check_desc(desc)) return rc;
  OptimView v;
  if (int rc = enc ? policy_optim_enc_view(p, v) : p ? policy_optim_view(p, v) : critic_optim_view(c, v)) return rc;
  const bool ls = (desc->flags & GAQ_OPTIM_STEP_LOG_STD) && v.explore;
  const int64_t total = v.net->nw + v.head + (ls ? 4 : 0) + v.enc_nw;
  if (total >= ((int64_t)1 << 31) - kOptChunk) return fail(GAQ_ERR_INVALID, "optim: too many parameters for one launch");
  gaq_optim* o = new (std::nothrow) gaq_optim;
  if (!o) return fail(GAQ_ERR_INVALID, "out of host memory");
  o->p = p; o->c = c; o->device = v.net->device; o->head = v.head; o->steps_log_std = ls; o->enc = enc;
  o->launches = env_override("GAQ_OPTIM_LAUNCHES") == 1 ? 1 : 2;
  OptimDevEnc& d = o->d;
  d.end[0] = (int32_t)v.net->nw; d.end[1] = d.end[0] + v.head; d.end[2] = d.end[1] + (ls ? 4 : 0); d.end[3] = (int32_t)total;
  d.nchunks = (int32_t)((total + kOptChunk - 1) / kOptChunk);
  // [m | v | log_std (4 floats)] then, 8-byte aligned, [partials | ctl]
  const size_t floats = ((size_t)2 * total + 4 + 1) & ~(size_t)1;
  const size_t bytes = floats * sizeof(float) + (size_t)d.nchunks * sizeof(double) + sizeof(OptimCtl);
  hipError_t he = hipSetDevice(o->device);
  if (he == hipSuccess) he = hipMalloc(&o->block, bytes);
  if (he == hipSuccess) he = hipMemset(o->block, 0, bytes);
  if (he != hipSuccess) { (void)gaq_optim_destroy(o); return fail(GAQ_ERR_DEVICE, std::string("optim: ") + hipGetErrorString(he)); }
  d.m = static_cast<float*>(o->block); d.v = d.m + total; o->log_std_dev = d.v + total;
  d.partial = reinterpret_cast<double*>(d.m + floats);
  d.ctl = reinterpret_cast<OptimCtl*>(d.partial + d.nchunks);
  o->tab = v.tab;
  d.tab = ls ? v.tab : nullptr;                   // a device-mode policy's log_std is stepped where its kernels read it
  d.theta[0] = v.net->w_dev; d.theta[1] = v.wv; d.theta[2] = d.tab ? d.tab : o->log_std_dev; d.theta[3] = v.enc_w;
  OptimCtl ctl{{desc->lr, desc->beta1, desc->beta2, desc->eps, desc->weight_decay, desc->max_grad_norm}, 0, 0, 0, 0};
  he = hipMemcpy(d.ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice);
  if (ls) std::memcpy(o->log_std, v.log_std, sizeof(o->log_std));
  if (he == hipSuccess && ls) he = hipMemcpy(o->log_std_dev, o->log_std, sizeof(o->log_std), hipMemcpyHostToDevice);
  if (he != hipSuccess) { (void)gaq_optim_destroy(o); return fail(GAQ_ERR_DEVICE, std::string("optim: ") + hipGetErrorString(he)); }
  *out = o;
  return GAQ_OK;
}

// An optimiser that steps log_std owns it: the handle's host copy must still be what the optimiser last gave it (at creation: took from
// it).  GAQ_ERR_STATE if the caller has switched exploration off or set another log_std since -- the device master copy never saw that,
// and the next synchronisation would silently undo it.
int optim_check_log_std(const gaq_optim* o, const OptimView& v) {
  if (v.tab != o->tab)
    return fail(GAQ_ERR_STATE, o->tab ? "optim: the exploration table the policy had when the optimiser was created is no longer registered "
                                        "(gaq_policy_set_explore_dev): create a new optimiser"
                                      : "optim: the policy has registered an exploration table since the optimiser was created "
                                        "(gaq_policy_set_explore_dev): create a new one");
  if (!o->steps_log_std) return GAQ_OK;
  if (!v.explore)
    return fail(GAQ_ERR_STATE, "optim: the policy has been made deterministic since the optimiser began to step its log_std: set the "
                               "log_std of gaq_optim_get_log_std again, or create a new optimiser");
  if (o->tab) return GAQ_OK;      // device mode: nothing to own -- a gaq_policy_set_explore between steps wrote the table the step reads
  if (std::memcmp(v.log_std, o->log_std, sizeof(o->log_std)) != 0)
    return fail(GAQ_ERR_STATE, "optim: log_std was set on the policy behind the optimiser that steps it (its device copy has not seen "
                               "the new values): create a new optimiser");
  return GAQ_OK;
}

// what the two state calls begin with: everything enqueued on the device has finished, and the control record is on the host
int optim_read_ctl(gaq_optim* o, OptimCtl& ctl) {
  if (!o) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(o->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&ctl, o->d.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
  return GAQ_OK;
}
size_t optim_state_bytes(const gaq_optim* o) { return sizeof(float) * (size_t)o->d.end[kOptGroupsEnc - 1]; }
}  // namespace

int gaq_optim_create_policy(gaq_policy* p, const gaq_optim_desc* desc, gaq_optim** out) { return optim_create(p, nullptr, desc, out); }

int gaq_optim_create_critic(gaq_critic* c, const gaq_optim_desc* desc, gaq_optim** out) { return optim_create(nullptr, c, desc, out); }

int gaq_optim_destroy(gaq_optim* o) {
  if (!o) return GAQ_OK;
  if (o->block) { (void)hipSetDevice(o->device); (void)hipFree(o->block); }
  delete o;
  return GAQ_OK;
}

int gaq_optim_create_policy_enc(gaq_policy* p, const gaq_optim_desc* desc, gaq_optim** out) {
  if (!p) return fail(GAQ_ERR_INVALID, "null argument");
  return optim_create(p, nullptr, desc, out, true);
}

int64_t gaq_optim_state_count(const gaq_optim* o) { return o ? (int64_t)o->d.end[kOptGroupsEnc - 1] : fail(GAQ_ERR_INVALID, "null argument"); }

namespace {
// gaq_optim_step_dev (enc = false, grad_enc = nullptr) and gaq_optim_step_enc_dev
int optim_step(gaq_optim* o, bool enc, const float* grad, const float* grad_enc, const float* grad_value, const float* grad_log_std,
               double* stats_out, void* stream) {
  if (!o || !grad || (enc && !grad_enc)) return fail(GAQ_ERR_INVALID, "null argument");
  if (o->enc != enc)
    return fail(GAQ_ERR_INVALID, o->enc ? "optim: this optimiser steps an encoder's block too: gaq_optim_step_enc_dev takes its gradient"
                                        : "optim: gaq_optim_step_enc_dev takes an optimiser made by gaq_optim_create_policy_enc");
  OptimView v;
  if (int rc = optim_view(o, v)) return rc;
  if ((v.head != 0) != (o->head != 0))
    return fail(GAQ_ERR_STATE, o->head ? "optim: the value head this optimiser steps has been removed from the policy"
                                       : "optim: the policy has gained a value head since the optimiser was created: create a new one");
  if (int rc = optim_check_log_std(o, v)) return rc;
  if (o->head && !grad_value) return fail(GAQ_ERR_INVALID, "optim: grad_value is required: the optimiser steps a value head");
  if (!o->head && grad_value) return fail(GAQ_ERR_INVALID, "optim: grad_value given, but the optimiser steps no value head");
  if (o->steps_log_std && !grad_log_std) return fail(GAQ_ERR_INVALID, "optim: grad_log_std is required: the optimiser steps log_std");
  const float* gls = o->steps_log_std ? grad_log_std : nullptr;
  if ((reinterpret_cast<uintptr_t>(grad) & 3) || (reinterpret_cast<uintptr_t>(grad_value) & 3) || (reinterpret_cast<uintptr_t>(gls) & 3) ||
      (reinterpret_cast<uintptr_t>(grad_enc) & 3) || (reinterpret_cast<uintptr_t>(stats_out) & 7))
    return fail(GAQ_ERR_INVALID, "optim: the gradients must be 4-byte aligned and stats_out 8-byte aligned");
  HIP_TRY(hipSetDevice(o->device));
  OptimDevEnc d = o->d;
  d.grad[0] = grad; d.grad[1] = grad_value; d.grad[2] = gls; d.grad[3] = grad_enc;
  d.stats = stats_out;
  hipStream_t st = (hipStream_t)stream;
  if (enc)
    optim_launch<OptimDevEnc>(o, d, st, optim_sumsq_kernel<kOptGroupsEnc>, optim_update_kernel<kOptGroupsEnc>,
                              optim_step_one_kernel<kOptGroupsEnc>);
  else
    optim_launch<OptimDev>(o, d, st, optim_sumsq_kernel<kOptGroups>, optim_update_kernel<kOptGroups>, optim_step_one_kernel<kOptGroups>);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}
}  // namespace

int gaq_optim_step_dev(gaq_optim* o, const float* grad, const float* grad_value, const float* grad_log_std, double* stats_out, void* stream) {
  return optim_step(o, false, grad, nullptr, grad_value, grad_log_std, stats_out, stream);
}

int gaq_optim_step_enc_dev(gaq_optim* o, const float* grad, const float* grad_enc, const float* grad_value, const float* grad_log_std,
                           double* stats_out, void* stream) {
  return optim_step(o, true, grad, grad_enc, grad_value, grad_log_std, stats_out, stream);
}

int gaq_optim_set_lr_dev(gaq_optim* o, double lr, void* stream) {
  if (!o) return fail(GAQ_ERR_INVALID, "null argument");
  if (!(lr >= 0.0) || !std::isfinite(lr)) return fail(GAQ_ERR_INVALID, "optim: lr must be finite and not negative");
  HIP_TRY(hipSetDevice(o->device));
  hipLaunchKernelGGL(optim_set_lr_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, o->d.ctl, lr);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

int gaq_optim_sync_log_std(gaq_optim* o, void* stream) {
  if (!o) return fail(GAQ_ERR_INVALID, "null argument");
  if (!o->steps_log_std) return GAQ_OK;
  OptimView v;
  if (int rc = optim_view(o, v)) return rc;
  if (int rc = optim_check_log_std(o, v)) return rc;
  if (o->tab) return GAQ_OK;      // device mode: the policy's kernels read what the step wrote
  HIP_TRY(hipSetDevice(o->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipMemcpy(o->log_std, o->log_std_dev, sizeof(o->log_std), hipMemcpyDeviceToHost));
  return gaq_policy_set_explore(o->p, o->log_std);
}

int gaq_optim_get_log_std(const gaq_optim* o, float* log_std4) {
  if (!o || !log_std4) return fail(GAQ_ERR_INVALID, "null argument");
  if (!o->steps_log_std) return fail(GAQ_ERR_STATE, "optim: the optimiser steps no log_std");
  if (o->tab) return gaq_policy_get_log_std(o->p, log_std4);     // device mode: the table's, after everything enqueued
  std::memcpy(log_std4, o->log_std, sizeof(o->log_std));
  return GAQ_OK;
}

int gaq_optim_get_state(gaq_optim* o, uint64_t* step, uint64_t* skipped, float* m_host, float* v_host) {
  OptimCtl ctl;
  if (int rc = optim_read_ctl(o, ctl)) return rc;
  if (step) *step = ctl.t_commit;
  if (skipped) *skipped = ctl.skipped_commit;
  if (m_host) HIP_TRY(hipMemcpy(m_host, o->d.m, optim_state_bytes(o), hipMemcpyDeviceToHost));
  if (v_host) HIP_TRY(hipMemcpy(v_host, o->d.v, optim_state_bytes(o), hipMemcpyDeviceToHost));
  return GAQ_OK;
}

int gaq_optim_set_state(gaq_optim* o, const uint64_t* step, const uint64_t* skipped, const float* m_host, const float* v_host) {
  OptimCtl ctl;
  if (int rc = optim_read_ctl(o, ctl)) return rc;       // (the hyper-parameters stay what they are on the device)
  if (step) ctl.t_read = ctl.t_commit = *step;
  if (skipped) ctl.skipped_read = ctl.skipped_commit = *skipped;
  if (m_host) HIP_TRY(hipMemcpy(o->d.m, m_host, optim_state_bytes(o), hipMemcpyHostToDevice));
  if (v_host) HIP_TRY(hipMemcpy(o->d.v, v_host, optim_state_bytes(o), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(o->d.ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice));
  return GAQ_OK;
}

}  // extern "C"
