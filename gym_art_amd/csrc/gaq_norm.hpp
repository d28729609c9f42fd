// gaq_norm.hpp -- what gaq_policy.hip needs of the observation normaliser, whose kernels and entry points are in gaq_learn.hip: one element
// of the normalisation, the table a normalising kernel takes, and the handle.  Included after gaq_host.hpp by those two units; internal
// to csrc/ like it.
#pragma once

// the running moments of D columns and their published table, in a gaq_obs_norm (D = obs_dim) and a gaq_ret_norm (D = 1): gaq_learn.hip moments_*
struct RunMoments {
  int device = 0, dim = 0;        // dim: D
  float eps = 0.0f, clip = 0.0f;
  double* state = nullptr;        // count, mean[D], M2[D]
  double* part = nullptr;         // [workgroups][D][3]: the workgroups' partial moments of one update
  float* tab = nullptr;           // the published table: mean[D], inv_std[D], clip
  const float* shift = nullptr;   // D floats behind the table: the shift of the update in flight (nullptr: it is the batch's first row)
};

// the observation normaliser (include/gaq.h gaq_obs_norm)
struct gaq_obs_norm {
  RunMoments m;                   // part: [kObsNormMaxBlocks][D][3]
  const gaq_env* env = nullptr;   // the handle it was created for (compared, never dereferenced after create)
};

// (an anonymous namespace in a header, as for gaq_host.hpp's Randomizer: the policy and critic kernels are templates over PolObsNorm and
//  obs_norm_apply_kernel takes it by value, so its linkage is part of their mangled names, which the recorded profiles key on.)
namespace {
// ---- observation normalisation (include/gaq.h gaq_obs_norm) -------------------------------------------------------------------------
// The published table of a normaliser: fp32 mean[D], then inv_std[D], then clip (2 D + 1 floats at an address that never changes; only the
// last launch of gaq_obs_norm_update_dev / gaq_obs_norm_set_stats writes it).  One element is obs_norm_elem, in every place: the apply
// kernel and the staging of every policy and critic kernel, so they agree to the bit.  Two roundings, the subtraction and the product
// (nothing here can contract to an fma; the pragma says so), then the clamp.
__device__ __forceinline__ float obs_norm_elem(float x, float mean, float inv_std, float clip) {
#pragma clang fp contract(off)
  return fminf(fmaxf((x - mean) * inv_std, -clip), clip);
}
// what the staging of a kernel's normalising instantiation does to input k of a live row (the plain instantiation has no such step)
struct PolObsNorm {
  const float* tab;               // mean[D], inv_std[D], clip (nullptr on the host side: no normaliser)
  int32_t dim;                    // D
  __device__ __forceinline__ float operator()(float x, int k) const { return obs_norm_elem(x, tab[k], tab[dim + k], tab[2 * dim]); }
};
// the table of an attached normaliser (nullptr: none)
PolObsNorm policy_norm_dev(const gaq_obs_norm* n) { return n ? PolObsNorm{n->m.tab, (int32_t)n->m.dim} : PolObsNorm{nullptr, 0}; }
}  // namespace
