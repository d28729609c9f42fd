// gaq_learn.hip -- the passes a learner runs over a finished rollout's buffers (include/gaq.h gaq_gae_*, gaq_vtrace_*, gaq_obs_norm,
// gaq_ret_norm, gaq_adv_norm): generalised advantage estimation and V-trace targets, the two running normalisers -- of observations and
// of discounted returns -- the standardisation of a batch of advantages and the permutation of an epoch's minibatches (gaq_perm_dev), with their kernels, the running normalisers' one host path
// for their moments and every entry point but the two attach calls gaq_policy_set_obs_norm / gaq_critic_set_obs_norm (gaq_policy.hip).  Of the env core (gaq.hip) it uses the handle and the error macro (gaq_host.hpp), nothing else;
// with gaq_policy.hip it shares gaq_norm.hpp, so that the apply kernel and the policies' staging normalise an element by one definition.
#include "gaq_host.hpp"
#include "gaq_norm.hpp"

namespace {

// Generalised advantage estimation over a [T, N] rollout (gaq_gae_dev): one lane per env, t descending, every access coalesced along N.
// nd = 1 - done[t]:  delta = r_t + gamma nd V_{t+1} - V_t,  A_t = delta + gamma lambda nd A_{t+1} (A_T = 0),  ret_t = A_t + V_t.
// The mask selects the factor (gamma or 0) instead of multiplying, so a done row is r_t - V_t in one rounding.  21 B per env-step.
__global__ __launch_bounds__(kBlock) void gae_kernel(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                     const float* __restrict__ value, float* __restrict__ adv, float* __restrict__ ret,
                                                     int64_t n, int T, float gamma, float gl) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float a = 0.0f, vn = value[(int64_t)T * n + i];
#pragma unroll 4
  for (int t = T - 1; t >= 0; --t) {
    const int64_t k = (int64_t)t * n + i;
    const float r = reward[k], v = value[k];
    const bool d = done[k] != 0;
    const float delta = __builtin_fmaf(d ? 0.0f : gamma, vn, r) - v;
    a = __builtin_fmaf(d ? 0.0f : gl, a, delta);
    adv[k] = a;
    if (ret) ret[k] = a + v;
    vn = v;
  }
}

// gae_kernel with time-limit bootstrapping (gaq_gae_term_dev): where done[t] is set the next value is term[t] -- V of the finished
// episode's last observation -- instead of nothing, and the advantage chain still cuts there.  A kernel of its own (gae_kernel keeps its
// code); term[t] is loaded for every row (coalesced) and selected, so what a non-done entry holds never reaches a sum.  25 B per env-step.
__global__ __launch_bounds__(kBlock) void gae_term_kernel(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                          const float* __restrict__ value, const float* __restrict__ term,
                                                          float* __restrict__ adv, float* __restrict__ ret, int64_t n, int T, float gamma,
                                                          float gl) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float a = 0.0f, vn = value[(int64_t)T * n + i];
#pragma unroll 4
  for (int t = T - 1; t >= 0; --t) {
    const int64_t k = (int64_t)t * n + i;
    const float r = reward[k], v = value[k], tv = term[k];
    const bool d = done[k] != 0;
    const float delta = __builtin_fmaf(gamma, d ? tv : vn, r) - v;
    a = __builtin_fmaf(d ? 0.0f : gl, a, delta);
    adv[k] = a;
    if (ret) ret[k] = a + v;
    vn = v;
  }
}

// V-trace targets over a [T, N] rollout (gaq_vtrace_dev, gaq_vtrace_term_dev; include/gaq.h has the contract): gae_kernel's scan with the
// importance ratio w = expf(logp_target - logp_behaviour) of each row clipped three ways.  One lane per env, t descending, every access
// coalesced along N; 25 B per env-step with pg (29 B with term), 4 B less without it.  The loop-carried chain is the fma of acc and the
// add of vs; expf of row t does not depend on it, so the unrolled loop has the rows' loads and their expf in flight.  The order of the
// operations is the contract: with w = 1, rho_bar, c_bar >= 1, gamma * c is gae_launch's gl, acc is gae_kernel's a and vs its ret.
struct VtraceClip {
  float gamma, lambda, rho_bar, c_bar, pg_rho_bar;
};
template <bool kTerm>
__device__ __forceinline__ void vtrace_scan(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                            const float* __restrict__ value, const float* __restrict__ logp_b,
                                            const float* __restrict__ logp_t, const float* __restrict__ term, float* __restrict__ vs_out,
                                            float* __restrict__ pg, int64_t n, int T, const VtraceClip& p) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f, vn = value[(int64_t)T * n + i], vsn = vn;
#pragma unroll 4
  for (int t = T - 1; t >= 0; --t) {
    const int64_t k = (int64_t)t * n + i;
    const float r = reward[k], v = value[k], x = logp_t[k] - logp_b[k];
    const float tv = kTerm ? term[k] : 0.0f;
    const bool d = done[k] != 0;
    const float w = expf(x);
    const float rho = fminf(p.rho_bar, w), c = p.lambda * fminf(p.c_bar, w);
    const float td = __builtin_fmaf(p.gamma, d ? tv : vn, r) - v;
    acc = __builtin_fmaf(d ? 0.0f : p.gamma * c, acc, rho * td);
    const float vs = v + acc;
    vs_out[k] = vs;
    if (pg) pg[k] = fminf(p.pg_rho_bar, w) * (__builtin_fmaf(p.gamma, d ? tv : vsn, r) - v);
    vn = v;
    vsn = vs;
  }
}
__global__ __launch_bounds__(kBlock) void vtrace_kernel(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                        const float* __restrict__ value, const float* __restrict__ logp_b,
                                                        const float* __restrict__ logp_t, float* __restrict__ vs_out,
                                                        float* __restrict__ pg, int64_t n, int T, VtraceClip p) {
  vtrace_scan<false>(reward, done, value, logp_b, logp_t, nullptr, vs_out, pg, n, T, p);
}
__global__ __launch_bounds__(kBlock) void vtrace_term_kernel(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                             const float* __restrict__ value, const float* __restrict__ logp_b,
                                                             const float* __restrict__ logp_t, const float* __restrict__ term,
                                                             float* __restrict__ vs_out, float* __restrict__ pg, int64_t n, int T,
                                                             VtraceClip p) {
  vtrace_scan<true>(reward, done, value, logp_b, logp_t, term, vs_out, pg, n, T, p);
}

// ---- the normaliser's own kernels (gaq_obs_norm_update_dev, gaq_obs_norm_set_stats, gaq_obs_norm_apply_dev) ------------------------------
// update: one streaming pass over obs [rows, D] in two launches, no atomics, every order fixed by (rows, D) alone -- the same input gives
// the same bits.  obs_norm_partial_kernel: workgroup b takes the rows [b rpb, (b + 1) rpb) as ONE flat stream of floats, a tile of
// kObsNormTile / D whole rows at a time: 16-byte loads from the first 16-byte boundary on (the base need only be 4-byte aligned and D is
// rarely a multiple of 4, so a tile's first and last up to 3 floats go singly) into LDS at the same offset mod 4, so the LDS stores are
// 16-byte ones too.  Then thread (g, c) = (tid / D, tid % D) sums column c over the tile's rows g, g + G, ... (G = 256 / D row groups;
// consecutive lanes read consecutive LDS words) in fp64, SHIFTED by K = the column's value in the batch's first row (every thread of
// every workgroup uses the same K): d = x - K is exact (or one fp64 rounding), s += d, q += d d, so a column of mean 1e3 and spread 1e-2
// loses nothing to cancellation where sum x^2 would lose ten digits.  Its moments are kept SHIFTED too, (n, s / n, q - s^2 / n): a mean
// stored at its own magnitude would carry an absolute error of ulp(1e3), and the delta^2 terms of the merges would inherit it relative to
// a delta of 1e-2.  Thread c < D merges the G of its column in ascending g (Chan et al.) into part[b][c].
// obs_norm_merge_kernel (one workgroup): thread (g, c) merges a contiguous run of the workgroups' partials in ascending b, thread c < D
// those G in ascending g, adds K to the batch's mean (its only rounding at the column's magnitude), then merges the batch into the
// running state, and PUBLISHES: tab = fp32(mean), fp32(1 / sqrt(M2 / n + eps)) -- the
// division, the square root and the reciprocal in fp64, one rounding to fp32 -- and clip.  With nb = 0 it only publishes (set_stats).
constexpr int kObsNormBlock = 256;
constexpr int kObsNormTile = 8192;                                // floats of a tile: 32 KiB of LDS
constexpr int kObsNormMaxBlocks = 1024;
constexpr int kObsNormMaxDim = kObsNormBlock;
constexpr int kObsNormApplyPer = 4;                               // elements per thread of obs_norm_apply_kernel

struct Moments {
  double n, mean, m2;
};
// Chan, Golub & LeVeque's pairwise update: the moments of the union of two samples
__device__ __forceinline__ Moments moments_merge(const Moments& a, const Moments& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n, delta = b.mean - a.mean;
  return Moments{n, a.mean + delta * (b.n / n), a.m2 + b.m2 + delta * delta * (a.n * b.n / n)};
}
// red[tid] = this thread's moments of column tid % D -> (thread c < D) the column's, merged in ascending row group
__device__ __forceinline__ Moments moments_column(double* red, const Moments& mine, int D, int tid) {
  red[3 * tid] = mine.n; red[3 * tid + 1] = mine.mean; red[3 * tid + 2] = mine.m2;
  __syncthreads();
  Moments acc{0.0, 0.0, 0.0};
  if (tid < D) {
    for (int g = 0; g < kObsNormBlock / D; ++g) {
      const double* r = red + 3 * (g * D + tid);
      acc = moments_merge(acc, Moments{r[0], r[1], r[2]});
    }
  }
  return acc;
}

__global__ __launch_bounds__(kObsNormBlock) void obs_norm_partial_kernel(const float* __restrict__ obs, int64_t rows, int D,
                                                                         int64_t rows_per_block, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float tile[kObsNormTile + 4];
  __shared__ double red[3 * kObsNormBlock];
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  const int c = tid % D, g = tid / D, G = kObsNormBlock / D;       // (threads past G D take no part in the sums)
  const int TR = kObsNormTile / D;
  const double K = (double)obs[c];                                // the shift: the column's value in the batch's first row
  double sum = 0.0, sq = 0.0, cnt = 0.0;
  for (int64_t t0 = r0; t0 < r1; t0 += TR) {
    const int tr = (int)(r1 - t0 < TR ? r1 - t0 : TR);
    const int len = tr * D;                                       // every index below stays inside the tile's [0, len) floats
    const float* src = obs + t0 * D;
    const int a = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    const int lead = ((4 - a) & 3) < len ? ((4 - a) & 3) : len;
    if (tid < lead) tile[a + tid] = src[tid];
    const int nq = (len - lead) >> 2;
    for (int j = tid; j < nq; j += kObsNormBlock)
      *reinterpret_cast<float4*>(tile + a + lead + 4 * j) = *reinterpret_cast<const float4*>(src + lead + 4 * j);
    const int got = lead + 4 * nq;
    if (tid < len - got) tile[a + got + tid] = src[got + tid];
    __syncthreads();
    if (g < G) {
      for (int r = g; r < tr; r += G) {
        const double x = (double)tile[a + r * D + c];
        const double d = x - K;
        sum += d;
        sq = __builtin_fma(d, d, sq);
        cnt += 1.0;
      }
    }
    __syncthreads();
  }
  Moments mine{0.0, 0.0, 0.0};
  if (cnt > 0.0) {
    const double m2 = sq - sum * sum / cnt;
    mine = Moments{cnt, sum / cnt, m2 > 0.0 ? m2 : 0.0};         // (the mean stays shifted by K)
  }
  const Moments col = moments_column(red, mine, D, tid);
  if (tid < D) {
    double* o = part + 3 * ((int64_t)blockIdx.x * D + tid);
    o[0] = col.n; o[1] = col.mean; o[2] = col.m2;
  }
}

// state: count, mean[D], M2[D] (fp64); tab: the published table (PolObsNorm); obs: the batch the nb partials come from (its first row is
// their shift; not read when nb = 0)
__global__ __launch_bounds__(kObsNormBlock) void obs_norm_merge_kernel(const double* __restrict__ part, int nb, int D,
                                                                       const float* __restrict__ obs, double* __restrict__ state,
                                                                       float* __restrict__ tab, float eps, float clip) {
  __shared__ double red[3 * kObsNormBlock];
  const int tid = (int)threadIdx.x;
  const int c = tid % D, g = tid / D, G = kObsNormBlock / D;
  Moments mine{0.0, 0.0, 0.0};
  if (g < G) {
    const int chunk = (nb + G - 1) / G;
    const int b1 = (g + 1) * chunk < nb ? (g + 1) * chunk : nb;
    for (int b = g * chunk; b < b1; ++b) {
      const double* r = part + 3 * ((int64_t)b * D + c);
      mine = moments_merge(mine, Moments{r[0], r[1], r[2]});
    }
  }
  Moments batch = moments_column(red, mine, D, tid);
  if (tid < D && nb > 0) batch.mean += (double)obs[tid];
  Moments tot{0.0, 0.0, 0.0};
  if (tid < D) tot = moments_merge(Moments{state[0], state[1 + tid], state[1 + D + tid]}, batch);
  __syncthreads();                                                // every column has read the count
  if (tid < D) {
    if (tid == 0) { state[0] = tot.n; tab[2 * D] = clip; }
    state[1 + tid] = tot.mean;
    state[1 + D + tid] = tot.m2;
    const double var = tot.n > 0.0 ? tot.m2 / tot.n : 1.0;        // before any update the variance is defined as 1
    tab[tid] = (float)tot.mean;
    tab[D + tid] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// out[i] = obs_norm_elem of obs[i], column i % D, over the flat [rows D] stream: kObsNormApplyPer coalesced dwords per thread.  out may be
// obs itself (each element is read and written by one thread); the column advances by 256 % D instead of a 64-bit remainder per element.
__global__ __launch_bounds__(kObsNormBlock) void obs_norm_apply_kernel(const float* obs, float* out, int64_t total, PolObsNorm nm) {
  const int64_t base = (int64_t)blockIdx.x * (kObsNormBlock * kObsNormApplyPer) + threadIdx.x;
  int k = (int)(base % nm.dim);
  const int step = kObsNormBlock % nm.dim;
#pragma unroll
  for (int j = 0; j < kObsNormApplyPer; ++j) {
    const int64_t i = base + j * kObsNormBlock;
    if (i < total) out[i] = nm(obs[i], k);
    k += step;
    if (k >= nm.dim) k -= nm.dim;
  }
}

// ---- return normalisation (include/gaq.h gaq_ret_norm): the running discounted return of each env and its statistics -----------------
// update: one streaming pass over reward [T, N] and done [T, N] in two launches, no atomics, every order fixed by N alone.
// ret_norm_partial_kernel: one lane per env, t ascending, a dword of reward and a byte of done per env-step, both coalesced along N
// (5 B per env-step, 16 B per env for R); the loop is unrolled so that several rows' loads are in flight, as in gae_kernel.  The lane
// carries R in a register: R = gamma R + r in fp64, product and sum rounded separately (the pragma: no fma), is one sample, then R = 0
// where done is set.  Its T samples are summed in fp64 SHIFTED by one K for every lane of every workgroup -- the running mean rounded to
// fp32, or reward[0] before the first update (so a batch whose samples all equal that value has d = 0 throughout and M2 = 0 exactly) --
// and kept shifted, (T, s / T, q - s^2 / T), for the reason obs_norm_partial_kernel gives.  Lanes merge (Chan et al.) in a fixed shuffle
// tree within the wave (lane l takes l + 1, then l + 2, ... l + 32: lane 0 ends with lanes 0..63 in ascending blocks), the workgroup's
// waves in ascending order through LDS, into part[b].  Workgroup 0 leaves K in `shift` (nobody reads that word in this launch), where
// obs_norm_merge_kernel with D = 1 finds "the batch's first row": it merges the partials in ascending b, adds K back, merges into
// state = (count, mean, M2) and publishes tab = fp32(mean) (the next K), inv_std, clip.
constexpr int kRetNormApplyPer = 4;                               // elements per thread of ret_norm_apply_kernel

__global__ __launch_bounds__(kBlock) void ret_norm_partial_kernel(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                                  int64_t n, int T, float gamma, double* __restrict__ R,
                                                                  const double* __restrict__ state, float* __restrict__ shift,
                                                                  double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[3 * (kBlock / 64)];
  const int tid = (int)threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
  const float kf = state[0] > 0.0 ? (float)state[1] : reward[0];
  if (blockIdx.x == 0 && tid == 0) shift[0] = kf;
  const double K = (double)kf, g = (double)gamma;
  Moments mine{0.0, 0.0, 0.0};
  if (i < n) {
    double r = R[i], sum = 0.0, sq = 0.0;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
      const int64_t k = (int64_t)t * n + i;
      const double x = (double)reward[k];
      const bool d = done[k] != 0;
      r = g * r + x;                                              // two roundings
      const double dev = r - K;
      sum += dev;
      sq = __builtin_fma(dev, dev, sq);
      r = d ? 0.0 : r;
    }
    R[i] = r;
    const double cnt = (double)T, m2 = sq - sum * sum / cnt;
    mine = Moments{cnt, sum / cnt, m2 > 0.0 ? m2 : 0.0};        // (the mean stays shifted by K)
  }
  for (int o = 1; o < 64; o <<= 1) {                              // (a lane past the wave's end reads itself; lane 0 never does)
    const Moments up{__shfl_down(mine.n, o), __shfl_down(mine.mean, o), __shfl_down(mine.m2, o)};
    mine = moments_merge(mine, up);
  }
  if ((tid & 63) == 0) { red[3 * (tid >> 6)] = mine.n; red[3 * (tid >> 6) + 1] = mine.mean; red[3 * (tid >> 6) + 2] = mine.m2; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kBlock / 64; ++w) mine = moments_merge(mine, Moments{red[3 * w], red[3 * w + 1], red[3 * w + 2]});
    double* o = part + 3 * (int64_t)blockIdx.x;
    o[0] = mine.n; o[1] = mine.mean; o[2] = mine.m2;
  }
}

// out[i] = fminf(fmaxf(reward[i] inv_std, -clip), clip) with the published table (the mean is not subtracted): kRetNormApplyPer coalesced
// dwords per thread.  out may be reward itself (each element is read and written by one thread).
__global__ __launch_bounds__(kBlock) void ret_norm_apply_kernel(const float* reward, float* out, int64_t total, const float* __restrict__ tab) {
  const float inv_std = tab[1], clip = tab[2];
  const int64_t base = (int64_t)blockIdx.x * (kBlock * kRetNormApplyPer) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kRetNormApplyPer; ++j) {
    const int64_t i = base + j * kBlock;
    if (i < total) out[i] = fminf(fmaxf(reward[i] * inv_std, -clip), clip);
  }
}

// R[i] <- 0 where mask[i] is non-zero (gaq_ret_norm_reset_returns_dev with a mask)
__global__ __launch_bounds__(kBlock) void ret_norm_zero_kernel(double* __restrict__ R, const uint8_t* __restrict__ mask, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n && mask[i]) R[i] = 0.0;
}

// ---- advantage standardisation (include/gaq.h gaq_adv_norm): (A - mean) / (std + eps) with the statistics of the batch itself ---------
// The moments are obs_norm_partial_kernel's at D = 1 (shift: the batch's first element).  adv_norm_finish_kernel (one workgroup): thread
// g merges the run of kAdvNormRun workgroups' partials [g kAdvNormRun, (g + 1) kAdvNormRun) in ascending b, thread 0 those runs in
// ascending g (a thread past the last run holds n = 0, which moments_merge passes over: the serial chain is one run plus nb / kAdvNormRun
// merges instead of 256), adds the shift back, stores state = (count, mean, M2) and PUBLISHES tab = fp32(mean),
// fp32(1 / (sqrt(M2 / (count - ddof)) + eps)) -- the division, the square root and the reciprocal in fp64, one rounding each, then one
// to fp32.  Nothing is carried from one batch to the next.
constexpr int kAdvNormApplyPer = 4;                               // elements per thread of adv_norm_apply_kernel
constexpr int kAdvNormRun = 32;                                   // partials per thread of adv_norm_finish_kernel
static_assert(kObsNormMaxBlocks <= kAdvNormRun * kObsNormBlock, "every partial needs a thread");

__global__ __launch_bounds__(kObsNormBlock) void adv_norm_finish_kernel(const double* __restrict__ part, int nb,
                                                                        const float* __restrict__ adv, double* __restrict__ state,
                                                                        float* __restrict__ tab, double eps, double ddof) {
  __shared__ double red[3 * kObsNormBlock];
  const int tid = (int)threadIdx.x;
  const int b1 = (tid + 1) * kAdvNormRun < nb ? (tid + 1) * kAdvNormRun : nb;
  Moments mine{0.0, 0.0, 0.0};
  for (int b = tid * kAdvNormRun; b < b1; ++b) {
    const double* r = part + 3 * (int64_t)b;
    mine = moments_merge(mine, Moments{r[0], r[1], r[2]});
  }
  Moments batch = moments_column(red, mine, 1, tid);
  if (tid == 0) {
    batch.mean += (double)adv[0];
    state[0] = batch.n; state[1] = batch.mean; state[2] = batch.m2;
    const double var = batch.m2 / (batch.n - ddof);
    tab[0] = (float)batch.mean;
    tab[1] = (float)(1.0 / (sqrt(var) + eps));
  }
}

// out[i] = (adv[i] - mean) * inv with the published table, the subtraction and the product rounded separately: kAdvNormApplyPer
// coalesced dwords per thread.  out may be adv itself (each element is read and written by one thread).
__global__ __launch_bounds__(kObsNormBlock) void adv_norm_apply_kernel(const float* adv, float* out, int64_t total,
                                                                       const float* __restrict__ tab) {
#pragma clang fp contract(off)
  const float mean = tab[0], inv = tab[1];
  const int64_t base = (int64_t)blockIdx.x * (kObsNormBlock * kAdvNormApplyPer) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kAdvNormApplyPer; ++j) {
    const int64_t i = base + j * kObsNormBlock;
    if (i < total) out[i] = (adv[i] - mean) * inv;
  }
}

// ---- the running moments of a normaliser (RunMoments, gaq_norm.hpp): the one host path of both handles ------------------------------
// (who: the prefix of the handle's messages, "obs_norm: " or "ret_norm: ")
int launched() { HIP_TRY(hipGetLastError()); return GAQ_OK; }     // after a launch
// merge the `nb` workgroups' partials of `batch` (0: none) into the running state and publish the table: the one launch that writes either
int moments_publish(RunMoments& m, int nb, const float* batch, hipStream_t st) {
  hipLaunchKernelGGL(obs_norm_merge_kernel, dim3(1), dim3(kObsNormBlock), 0, st, m.part, nb, m.dim, m.shift ? m.shift : batch, m.state, m.tab,
                     m.eps, m.clip);
  return launched();
}
void moments_free(RunMoments& m) {
  (void)hipSetDevice(m.device);
  (void)hipFree(m.state); (void)hipFree(m.part); (void)hipFree(m.tab);   // (nullptr: nothing to free)
}
// validate, then on `device`: the memory of D columns and `blocks` workgroups' partials, state = 0 (count = 0, mean = 0: the variance reads
// as 1) and the first table.  own_shift: D zeroed floats behind the table for RunMoments::shift.  On failure nothing stays allocated.
int moments_create(RunMoments& m, const char* who, int device, int dim, float eps, float clip, size_t blocks, bool own_shift) {
  if (!(eps >= 0.0f) || !std::isfinite(eps)) return fail(GAQ_ERR_INVALID, std::string(who) + "eps must be finite and >= 0");
  if (!(clip > 0.0f)) return fail(GAQ_ERR_INVALID, std::string(who) + "clip must be > 0 (+inf: no clamp)");
  if (dim > kObsNormMaxDim)
    return fail(GAQ_ERR_INVALID, std::string(who) + "obs_dim " + std::to_string(dim) + " exceeds " + std::to_string(kObsNormMaxDim));
  HIP_TRY(hipSetDevice(device));
  m.device = device; m.dim = dim; m.eps = eps; m.clip = clip;
  const size_t D = (size_t)dim, ns = 1 + 2 * D, nt = 2 * D + 1 + (own_shift ? D : 0);
  hipError_t he = hipMalloc(&m.state, sizeof(double) * ns);
  if (he == hipSuccess) he = hipMalloc(&m.part, sizeof(double) * 3 * D * blocks);
  if (he == hipSuccess) he = hipMalloc(&m.tab, sizeof(float) * nt);
  if (he == hipSuccess) he = hipMemset(m.state, 0, sizeof(double) * ns);
  if (he == hipSuccess) he = hipMemset(m.tab, 0, sizeof(float) * nt);
  if (own_shift) m.shift = m.tab + 2 * D + 1;
  int rc = he == hipSuccess ? GAQ_OK : fail(GAQ_ERR_DEVICE, std::string(who) + hipGetErrorString(he));
  if (!rc) rc = moments_publish(m, 0, nullptr, nullptr);
  if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(GAQ_ERR_DEVICE, std::string(who) + "the first publish failed");
  if (rc) moments_free(m);
  return rc;
}
// count, mean[D], M2[D] once everything queued on any stream has run: one copy of the whole state
int moments_get(RunMoments& m, double* count, double* mean, double* m2) {
  HIP_TRY(hipSetDevice(m.device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t D = (size_t)m.dim;
  double host[1 + 2 * kObsNormMaxDim];
  HIP_TRY(hipMemcpy(host, m.state, sizeof(double) * (1 + 2 * D), hipMemcpyDeviceToHost));
  *count = host[0];
  std::copy(host + 1, host + 1 + D, mean);
  std::copy(host + 1 + D, host + 1 + 2 * D, m2);
  return GAQ_OK;
}
// validate, then replace the state and publish its table.  mean_fp32: the mean must be finite as an fp32 too (ret_norm: it is the next shift)
int moments_set(RunMoments& m, const char* who, double count, const double* mean, const double* m2, bool mean_fp32) {
  if (!(count >= 0.0) || !std::isfinite(count)) return fail(GAQ_ERR_INVALID, std::string(who) + "count must be finite and >= 0");
  for (int k = 0; k < m.dim; ++k)
    if (!std::isfinite(mean_fp32 ? (double)(float)mean[k] : mean[k]) || !(m2[k] >= 0.0) || !std::isfinite(m2[k]))
      return fail(GAQ_ERR_INVALID, std::string(who) + (mean_fp32 ? "mean must be finite (as an fp32 too) and M2 finite and >= 0"
                                                                 : "mean must be finite and M2 finite and >= 0"));
  HIP_TRY(hipSetDevice(m.device));
  HIP_TRY(hipDeviceSynchronize());                                // whatever is queued on any stream has read the old table
  const size_t D = (size_t)m.dim;
  double host[1 + 2 * kObsNormMaxDim];
  host[0] = count;
  std::copy(mean, mean + D, host + 1);
  std::copy(m2, m2 + D, host + 1 + D);
  HIP_TRY(hipMemcpy(m.state, host, sizeof(double) * (1 + 2 * D), hipMemcpyHostToDevice));
  if (int rc = moments_publish(m, 0, nullptr, nullptr)) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  return GAQ_OK;
}
}  // namespace

extern "C" {

// ---- return normaliser (include/gaq.h gaq_ret_norm) ---------------------------------------------------------------------------
struct gaq_ret_norm {
  RunMoments m;                   // D = 1; part: [nb][3]; the shift K of the update in flight stands behind the table, in tab[3]
  int64_t n = 0;                  // the env's N
  int nb = 0;                     // workgroups of ret_norm_partial_kernel: a function of N alone
  float gamma = 0.0f;
  double* ret = nullptr;          // R[N]: the running discounted return of each env
};

namespace {
// true if the byte ranges [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}
// gaq_gae_dev (term = nullptr: gae_kernel, as ever) and gaq_gae_term_dev
int gae_launch(gaq_env* e, int32_t T, const float* reward, const uint8_t* done, const float* value, const float* term, float gamma,
               float lambda, float* adv, float* ret, void* stream) {
  if (!e || !reward || !done || !value || !adv) return fail(GAQ_ERR_INVALID, "null argument");
  if (T <= 0) return fail(GAQ_ERR_INVALID, "T must be positive");
  if (!(gamma >= 0.0f && gamma <= 1.0f) || !(lambda >= 0.0f && lambda <= 1.0f)) return fail(GAQ_ERR_INVALID, "gae: gamma and lambda must be in [0, 1]");
  const int64_t n = e->d.n;
  const size_t tn = (size_t)T * (size_t)n;
  const void* in[4] = {reward, done, value, term};
  const size_t in_bytes[4] = {tn * 4, tn, (tn + (size_t)n) * 4, tn * 4};
  for (float* out : {adv, ret}) {
    if (!out) continue;
    for (int k = 0; k < 4; ++k)
      if (in[k] && ranges_overlap(out, tn * 4, in[k], in_bytes[k])) return fail(GAQ_ERR_INVALID, "gae: an output overlaps an input");
  }
  if (ret && ranges_overlap(adv, tn * 4, ret, tn * 4)) return fail(GAQ_ERR_INVALID, "gae: adv_out and ret_out overlap");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  if (term) {
    hipLaunchKernelGGL(gae_term_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, reward, done, value, term, adv, ret, n, (int)T, gamma,
                       gamma * lambda);
  } else {
    hipLaunchKernelGGL(gae_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, reward, done, value, adv, ret, n, (int)T, gamma, gamma * lambda);
  }
  return launched();
}
// gaq_vtrace_dev (term = nullptr: vtrace_kernel) and gaq_vtrace_term_dev
int vtrace_launch(gaq_env* e, int32_t T, const float* reward, const uint8_t* done, const float* value, const float* logp_b,
                  const float* logp_t, const float* term, float gamma, float lambda, float rho_bar, float c_bar, float pg_rho_bar, float* vs,
                  float* pg, void* stream) {
  if (!e || !reward || !done || !value || !logp_b || !logp_t || !vs) return fail(GAQ_ERR_INVALID, "null argument");
  if (T <= 0) return fail(GAQ_ERR_INVALID, "T must be positive");
  if (!(gamma >= 0.0f && gamma <= 1.0f) || !(lambda >= 0.0f && lambda <= 1.0f))
    return fail(GAQ_ERR_INVALID, "vtrace: gamma and lambda must be in [0, 1]");
  if (!(rho_bar > 0.0f) || !(c_bar > 0.0f) || !(pg_rho_bar > 0.0f))
    return fail(GAQ_ERR_INVALID, "vtrace: rho_bar, c_bar and pg_rho_bar must be > 0 (+inf: no clipping)");
  const int64_t n = e->d.n;
  const size_t tn = (size_t)T * (size_t)n;
  const void* in[6] = {reward, done, value, logp_b, logp_t, term};
  const size_t in_bytes[6] = {tn * 4, tn, (tn + (size_t)n) * 4, tn * 4, tn * 4, tn * 4};
  for (float* out : {vs, pg}) {
    if (!out) continue;
    for (int k = 0; k < 6; ++k)
      if (in[k] && ranges_overlap(out, tn * 4, in[k], in_bytes[k])) return fail(GAQ_ERR_INVALID, "vtrace: an output overlaps an input");
  }
  if (pg && ranges_overlap(vs, tn * 4, pg, tn * 4)) return fail(GAQ_ERR_INVALID, "vtrace: vs_out and pg_adv_out overlap");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  const VtraceClip p{gamma, lambda, rho_bar, c_bar, pg_rho_bar};
  if (term) {
    hipLaunchKernelGGL(vtrace_term_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, reward, done, value, logp_b, logp_t, term, vs, pg, n,
                       (int)T, p);
  } else {
    hipLaunchKernelGGL(vtrace_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, reward, done, value, logp_b, logp_t, vs, pg, n, (int)T, p);
  }
  return launched();
}
int obs_norm_check_rows(const gaq_obs_norm* n, int64_t rows, const void* a, const void* b) {
  if (!n || !a || !b) return fail(GAQ_ERR_INVALID, "null argument");
  if (rows <= 0) return fail(GAQ_ERR_INVALID, "obs_norm: rows must be positive");
  if ((reinterpret_cast<uintptr_t>(a) & 3) || (reinterpret_cast<uintptr_t>(b) & 3))
    return fail(GAQ_ERR_INVALID, "obs_norm: the observation pointers must be 4-byte aligned");
  if (rows > (((int64_t)1 << 31) - 1) * (kObsNormBlock * kObsNormApplyPer) / n->m.dim)
    return fail(GAQ_ERR_INVALID, "obs_norm: too many rows for one launch");
  return GAQ_OK;
}
}  // namespace

int gaq_gae_dev(gaq_env* e, int32_t T, const float* reward, const uint8_t* done, const float* value, float gamma, float lambda, float* adv,
                float* ret, void* stream) {
  return gae_launch(e, T, reward, done, value, nullptr, gamma, lambda, adv, ret, stream);
}

int gaq_gae_term_dev(gaq_env* e, int32_t T, const float* reward, const uint8_t* done, const float* value, const float* term, float gamma,
                     float lambda, float* adv, float* ret, void* stream) {
  return gae_launch(e, T, reward, done, value, term, gamma, lambda, adv, ret, stream);
}

// ---- observation normaliser: the entry points (include/gaq.h gaq_obs_norm) -------------------------------------------------------
int gaq_obs_norm_create(gaq_env* e, float eps, float clip, gaq_obs_norm** out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  gaq_obs_norm* n = new (std::nothrow) gaq_obs_norm;
  if (!n) return fail(GAQ_ERR_INVALID, "out of host memory");
  n->env = e;
  if (int rc = moments_create(n->m, "obs_norm: ", e->cfg.device, e->obs_dim, eps, clip, kObsNormMaxBlocks, false)) { delete n; return rc; }
  *out = n;
  return GAQ_OK;
}

int gaq_obs_norm_update_dev(gaq_obs_norm* n, int64_t rows, const float* obs, void* stream) {
  if (int rc = obs_norm_check_rows(n, rows, obs, obs)) return rc;
  HIP_TRY(hipSetDevice(n->m.device));
  // the split into workgroups is a function of (rows, D) alone: at least one tile of rows each, at most kObsNormMaxBlocks of them
  const int64_t tile_rows = kObsNormTile / n->m.dim;
  const int64_t want = (rows + tile_rows - 1) / tile_rows;
  const int64_t nb0 = want < kObsNormMaxBlocks ? want : kObsNormMaxBlocks;
  const int64_t rpb = (rows + nb0 - 1) / nb0;
  const int nb = (int)((rows + rpb - 1) / rpb);
  hipLaunchKernelGGL(obs_norm_partial_kernel, dim3((unsigned)nb), dim3(kObsNormBlock), 0, (hipStream_t)stream, obs, rows, n->m.dim, rpb,
                     n->m.part);
  HIP_TRY(hipGetLastError());
  return moments_publish(n->m, nb, obs, (hipStream_t)stream);
}

int gaq_obs_norm_apply_dev(gaq_obs_norm* n, int64_t rows, const float* obs, float* out, void* stream) {
  if (int rc = obs_norm_check_rows(n, rows, obs, out)) return rc;
  HIP_TRY(hipSetDevice(n->m.device));
  const int64_t total = rows * n->m.dim, per = kObsNormBlock * kObsNormApplyPer;
  hipLaunchKernelGGL(obs_norm_apply_kernel, dim3((unsigned)((total + per - 1) / per)), dim3(kObsNormBlock), 0, (hipStream_t)stream, obs, out,
                     total, policy_norm_dev(n));
  return launched();
}

int gaq_obs_norm_get_stats(gaq_obs_norm* n, double* count, double* mean, double* m2) {
  if (!n || !count || !mean || !m2) return fail(GAQ_ERR_INVALID, "null argument");
  return moments_get(n->m, count, mean, m2);
}

int gaq_obs_norm_set_stats(gaq_obs_norm* n, double count, const double* mean, const double* m2) {
  if (!n || !mean || !m2) return fail(GAQ_ERR_INVALID, "null argument");
  return moments_set(n->m, "obs_norm: ", count, mean, m2, false);
}

int gaq_obs_norm_destroy(gaq_obs_norm* n) {
  if (n) moments_free(n->m);
  delete n;
  return GAQ_OK;
}

// ---- return normaliser: the entry points (include/gaq.h gaq_ret_norm) ---------------------------------------------------------------
int gaq_ret_norm_create(gaq_env* e, float gamma, float eps, float clip, gaq_ret_norm** out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(GAQ_ERR_INVALID, "ret_norm: gamma must be in [0, 1]");
  gaq_ret_norm* n = new (std::nothrow) gaq_ret_norm;
  if (!n) return fail(GAQ_ERR_INVALID, "out of host memory");
  n->n = e->d.n; n->gamma = gamma; n->nb = (int)((n->n + kBlock - 1) / kBlock);
  if (int rc = moments_create(n->m, "ret_norm: ", e->cfg.device, 1, eps, clip, (size_t)n->nb, true)) { delete n; return rc; }
  hipError_t he = hipMalloc(&n->ret, sizeof(double) * (size_t)n->n);
  if (he == hipSuccess) he = hipMemset(n->ret, 0, sizeof(double) * (size_t)n->n);
  if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
  if (he != hipSuccess) { (void)gaq_ret_norm_destroy(n); return fail(GAQ_ERR_DEVICE, std::string("ret_norm: ") + hipGetErrorString(he)); }
  *out = n;
  return GAQ_OK;
}

int gaq_ret_norm_update_dev(gaq_ret_norm* n, int32_t T, const float* reward, const uint8_t* done, void* stream) {
  if (!n || !reward || !done) return fail(GAQ_ERR_INVALID, "null argument");
  if (T < 1) return fail(GAQ_ERR_INVALID, "ret_norm: T must be positive");
  if (reinterpret_cast<uintptr_t>(reward) & 3) return fail(GAQ_ERR_INVALID, "ret_norm: the reward pointer must be 4-byte aligned");
  HIP_TRY(hipSetDevice(n->m.device));
  hipLaunchKernelGGL(ret_norm_partial_kernel, dim3((unsigned)n->nb), dim3(kBlock), 0, (hipStream_t)stream, reward, done, n->n, (int)T,
                     n->gamma, n->ret, n->m.state, n->m.tab + 3, n->m.part);
  HIP_TRY(hipGetLastError());
  return moments_publish(n->m, n->nb, nullptr, (hipStream_t)stream);
}

int gaq_ret_norm_apply_dev(gaq_ret_norm* n, int64_t count, const float* reward, float* out, void* stream) {
  if (!n || !reward || !out) return fail(GAQ_ERR_INVALID, "null argument");
  if (count < 0) return fail(GAQ_ERR_INVALID, "ret_norm: count must not be negative");
  if ((reinterpret_cast<uintptr_t>(reward) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
    return fail(GAQ_ERR_INVALID, "ret_norm: the reward and out pointers must be 4-byte aligned");
  const int64_t per = kBlock * kRetNormApplyPer;
  if (count > (((int64_t)1 << 31) - 1) * per) return fail(GAQ_ERR_INVALID, "ret_norm: count is too large for one launch");
  if (count == 0) return GAQ_OK;
  HIP_TRY(hipSetDevice(n->m.device));
  hipLaunchKernelGGL(ret_norm_apply_kernel, dim3((unsigned)((count + per - 1) / per)), dim3(kBlock), 0, (hipStream_t)stream, reward, out, count,
                     n->m.tab);
  return launched();
}

int gaq_ret_norm_reset_returns_dev(gaq_ret_norm* n, const uint8_t* mask, void* stream) {
  if (!n) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(n->m.device));
  if (!mask) {
    HIP_TRY(hipMemsetAsync(n->ret, 0, sizeof(double) * (size_t)n->n, (hipStream_t)stream));
    return GAQ_OK;
  }
  hipLaunchKernelGGL(ret_norm_zero_kernel, dim3((unsigned)n->nb), dim3(kBlock), 0, (hipStream_t)stream, n->ret, mask, n->n);
  return launched();
}

int gaq_ret_norm_get_stats(gaq_ret_norm* n, double* count, double* mean, double* m2) {
  if (!n || !count || !mean || !m2) return fail(GAQ_ERR_INVALID, "null argument");
  return moments_get(n->m, count, mean, m2);
}

int gaq_ret_norm_set_stats(gaq_ret_norm* n, double count, double mean, double m2) {
  if (!n) return fail(GAQ_ERR_INVALID, "null argument");
  return moments_set(n->m, "ret_norm: ", count, &mean, &m2, true);
}

int gaq_ret_norm_get_returns(gaq_ret_norm* n, double* host) {
  if (!n || !host) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(n->m.device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, n->ret, sizeof(double) * (size_t)n->n, hipMemcpyDeviceToHost));
  return GAQ_OK;
}

int gaq_ret_norm_set_returns(gaq_ret_norm* n, const double* host) {
  if (!n || !host) return fail(GAQ_ERR_INVALID, "null argument");
  for (int64_t i = 0; i < n->n; ++i)
    if (!std::isfinite(host[i])) return fail(GAQ_ERR_INVALID, "ret_norm: the returns must be finite");
  HIP_TRY(hipSetDevice(n->m.device));
  HIP_TRY(hipDeviceSynchronize());                                // updates queued on any stream have stored their R
  HIP_TRY(hipMemcpy(n->ret, host, sizeof(double) * (size_t)n->n, hipMemcpyHostToDevice));
  return GAQ_OK;
}

int gaq_ret_norm_destroy(gaq_ret_norm* n) {
  if (n) { moments_free(n->m); (void)hipFree(n->ret); }
  delete n;
  return GAQ_OK;
}

// ---- V-trace: the entry points (include/gaq.h gaq_vtrace_dev) ---------------------------------------------------------------------------
int gaq_vtrace_dev(gaq_env* e, int32_t T, const float* reward, const uint8_t* done, const float* value, const float* logp_behaviour,
                   const float* logp_target, float gamma, float lambda, float rho_bar, float c_bar, float pg_rho_bar, float* vs,
                   float* pg_adv, void* stream) {
  return vtrace_launch(e, T, reward, done, value, logp_behaviour, logp_target, nullptr, gamma, lambda, rho_bar, c_bar, pg_rho_bar, vs, pg_adv,
                       stream);
}

int gaq_vtrace_term_dev(gaq_env* e, int32_t T, const float* reward, const uint8_t* done, const float* value, const float* logp_behaviour,
                        const float* logp_target, const float* term, float gamma, float lambda, float rho_bar, float c_bar,
                        float pg_rho_bar, float* vs, float* pg_adv, void* stream) {
  return vtrace_launch(e, T, reward, done, value, logp_behaviour, logp_target, term, gamma, lambda, rho_bar, c_bar, pg_rho_bar, vs, pg_adv,
                       stream);
}

// ---- advantage standardisation: the entry points (include/gaq.h gaq_adv_norm) -----------------------------------------------------------
struct gaq_adv_norm {
  int device = 0, ddof = 0;
  float eps = 0.0f;
  double* part = nullptr;         // [kObsNormMaxBlocks][3]: the workgroups' partial moments of the batch in flight
  double* state = nullptr;        // count, mean, M2 of the last batch
  float* tab = nullptr;           // the published table: mean, inv
};

int gaq_adv_norm_create(gaq_env* e, float eps, int32_t ddof, gaq_adv_norm** out) {
  if (!e || !out) return fail(GAQ_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!(eps >= 0.0f) || !std::isfinite(eps)) return fail(GAQ_ERR_INVALID, "adv_norm: eps must be finite and >= 0");
  if (ddof != 0 && ddof != 1) return fail(GAQ_ERR_INVALID, "adv_norm: ddof must be 0 or 1");
  gaq_adv_norm* n = new (std::nothrow) gaq_adv_norm;
  if (!n) return fail(GAQ_ERR_INVALID, "out of host memory");
  n->device = e->cfg.device; n->eps = eps; n->ddof = (int)ddof;
  hipError_t he = hipSetDevice(n->device);
  if (he == hipSuccess) he = hipMalloc(&n->part, sizeof(double) * 3 * kObsNormMaxBlocks);
  if (he == hipSuccess) he = hipMalloc(&n->state, sizeof(double) * 3);
  if (he == hipSuccess) he = hipMalloc(&n->tab, sizeof(float) * 2);
  if (he == hipSuccess) he = hipMemset(n->state, 0, sizeof(double) * 3);
  if (he == hipSuccess) he = hipMemset(n->tab, 0, sizeof(float) * 2);
  if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
  if (he != hipSuccess) { (void)gaq_adv_norm_destroy(n); return fail(GAQ_ERR_DEVICE, std::string("adv_norm: ") + hipGetErrorString(he)); }
  *out = n;
  return GAQ_OK;
}

int gaq_adv_norm_apply_dev(gaq_adv_norm* n, int64_t count, const float* adv, float* out, void* stream) {
  if (!n || !adv || !out) return fail(GAQ_ERR_INVALID, "null argument");
  if (count < 1 + n->ddof) return fail(GAQ_ERR_INVALID, "adv_norm: count must be at least 1 + ddof");
  if ((reinterpret_cast<uintptr_t>(adv) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
    return fail(GAQ_ERR_INVALID, "adv_norm: the adv and out pointers must be 4-byte aligned");
  const int64_t per = kObsNormBlock * kAdvNormApplyPer;
  if (count > (((int64_t)1 << 31) - 1) * per) return fail(GAQ_ERR_INVALID, "adv_norm: count is too large for one launch");
  HIP_TRY(hipSetDevice(n->device));
  // the split into workgroups is a function of count alone: at least one tile each, at most kObsNormMaxBlocks of them
  const int64_t want = (count + kObsNormTile - 1) / kObsNormTile;
  const int64_t nb0 = want < kObsNormMaxBlocks ? want : kObsNormMaxBlocks;
  const int64_t rpb = (count + nb0 - 1) / nb0;
  const int nb = (int)((count + rpb - 1) / rpb);
  hipLaunchKernelGGL(obs_norm_partial_kernel, dim3((unsigned)nb), dim3(kObsNormBlock), 0, (hipStream_t)stream, adv, count, 1, rpb, n->part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(adv_norm_finish_kernel, dim3(1), dim3(kObsNormBlock), 0, (hipStream_t)stream, n->part, nb, adv, n->state, n->tab,
                     (double)n->eps, (double)n->ddof);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(adv_norm_apply_kernel, dim3((unsigned)((count + per - 1) / per)), dim3(kObsNormBlock), 0, (hipStream_t)stream, adv, out,
                     count, n->tab);
  return launched();
}

int gaq_adv_norm_get_stats(gaq_adv_norm* n, double* count, double* mean, double* m2) {
  if (!n || !count || !mean || !m2) return fail(GAQ_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(n->device));
  HIP_TRY(hipDeviceSynchronize());
  double host[3];
  HIP_TRY(hipMemcpy(host, n->state, sizeof(host), hipMemcpyDeviceToHost));
  *count = host[0]; *mean = host[1]; *m2 = host[2];
  return GAQ_OK;
}

int gaq_adv_norm_destroy(gaq_adv_norm* n) {
  if (n) {
    (void)hipSetDevice(n->device);
    (void)hipFree(n->part); (void)hipFree(n->state); (void)hipFree(n->tab);
  }
  delete n;
  return GAQ_OK;
}

}  // extern "C"

// ---- shuffled minibatches: a pseudo-random permutation in one launch (include/gaq.h gaq_perm_dev, whose formula this restates) --------
namespace {

constexpr int kPermRounds = 8;

// idx_out[i] = P(i): a keyed Feistel network on b = 2 h bits, walked along i's cycle until the value is below n.  Elementwise: a thread
// reads the epoch word (if there is one) and writes its own idx_out[i], nothing else.
// THE WALK TERMINATES for every key: each round (L, R) -> (R, L ^ F(R)) is invertible whatever F is, so P is a bijection of [0, 2^b) and
// the sequence i, P(i), P(P(i)), ... is a cycle that returns to i itself, which is below n -- the loop leaves at the first value below n
// on the way, after at most 2^b - n + 1 applications.  Summed over all i < n the applications number at most 2^b (every element of
// [0, 2^b) is passed at most once), and 2^b <= 4 n (< 4 n for n > 1): at most 4 per thread on average.  Two i never meet: the first value below n after
// i on i's cycle is a different one for each i, which also makes the result a permutation of [0, n).
__global__ __launch_bounds__(kBlock) void perm_kernel(int32_t* __restrict__ out, uint32_t n, int h, uint64_t seed, uint64_t epoch,
                                                      const uint64_t* __restrict__ epoch_dev) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (epoch_dev) epoch = *epoch_dev;
  // the round keys: two Philox4x32-10 blocks of (seed, epoch) -- uniform over the launch
  uint32_t key[kPermRounds];
#pragma unroll
  for (int j = 0; j < kPermRounds / 4; ++j) {
    const gaq::Philox ph(seed, epoch, (uint64_t)j, gaq::RNG_PERM);
#pragma unroll
    for (int q = 0; q < 4; ++q) key[4 * j + q] = ph.c[q];
  }
  const uint32_t mask = (1u << h) - 1u;
  uint32_t x = i;
  do {
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (int r = 0; r < kPermRounds; ++r) {
      const uint64_t p = (uint64_t)0xD2511F53u * (uint64_t)(R ^ key[r]);
      const uint64_t q = (uint64_t)0xCD9E8D57u * (uint64_t)((uint32_t)(p >> 32) ^ (uint32_t)p);
      const uint32_t f = ((uint32_t)(q >> 32) ^ (uint32_t)q) >> (32 - h);
      const uint32_t nr = L ^ f;
      L = R;
      R = nr;
    }
    x = (L << h) | R;
  } while (x >= n);
  out[i] = (int32_t)x;
}

}  // namespace

extern "C" {

int gaq_perm_dev(int64_t n, uint64_t seed, uint64_t epoch, const uint64_t* epoch_dev, int32_t* idx_out, void* stream) {
  if (!idx_out) return fail(GAQ_ERR_INVALID, "null argument");
  if (n < 1 || n > ((int64_t)1 << 31) - 1) return fail(GAQ_ERR_INVALID, "gaq_perm_dev: n must be in [1, 2^31 - 1]");
  if ((reinterpret_cast<uintptr_t>(idx_out) & 3) || (reinterpret_cast<uintptr_t>(epoch_dev) & 7))
    return fail(GAQ_ERR_INVALID, "gaq_perm_dev: idx_out must be 4-byte aligned (epoch_dev: 8)");
  int b = 2;                                                      // the smallest even b with 2^b >= n, at least 2 (so 2^b < 4 n)
  while (((int64_t)1 << b) < n) b += 2;
  hipLaunchKernelGGL(perm_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, idx_out, (uint32_t)n,
                     b / 2, seed, epoch, epoch_dev);
  HIP_TRY(hipGetLastError());
  return GAQ_OK;
}

}  // extern "C"
