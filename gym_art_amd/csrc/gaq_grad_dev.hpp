// gaq_grad_dev.hpp -- the device pieces gaq_policy_grad.hip and gaq_policy_grad_seq.hip have in
// common: a tile's LDS layout (the row stride, the column of a row and its inverse), the activation's derivative, the words of a
// workgroup's partial, dW as MFMAs over the tile's 64 columns, the row sum, and the constants of the row stage and of the idx forms.
// Every function is force-inlined into the tile kernels, which keep the instructions they had when each unit held its own copy
// (tools/kernel_asm_same.py against the parent; DESIGN.md 4a "One reduce kernel, shared pieces").  Included after gaq_grad.hpp by those
// two units only; internal to csrc/.
#pragma once

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kGradWaves = 4;
constexpr int kGradBlock = kGradWaves * kTile;
constexpr int kGradStride = 68;                                   // floats per LDS row
constexpr float kGradTwoLn2Pi = 3.67575413281869f;
constexpr int kGradIdxBytes = kTile * 4;                          // the idx forms: the tile's 64 source rows, between the head region and X
constexpr int kGradIdxDead = -1, kGradIdxSkipped = -2;            // what they hold for a dead lane / for an index out of range
constexpr size_t kGradLdsMax = 160 * 1024;

// row (env, sequence) e of a tile lives in column grad_col(e) = pol_col(e) of every LDS row; grad_env is its inverse
__device__ __forceinline__ int grad_col(int e) { return (e & 15) * 4 + (e >> 4); }
__device__ __forceinline__ int grad_env(int col) { return (col & 3) * 16 + (col >> 2); }
__device__ __forceinline__ float grad_actd(int act, float h) { return act == 0 ? __builtin_fmaf(-h, h, 1.0f) : (h > 0.0f ? 1.0f : 0.0f); }

// one word of the workgroup's partial: the first tile stores, the others add (the same lane owns the word for every tile)
__device__ __forceinline__ void grad_put(float* p, float v, bool first) { *p = first ? v : *p + v; }
__device__ __forceinline__ void grad_put4(float* p, const f32x4& v, bool first) {
  f32x4* q = reinterpret_cast<f32x4*>(p);
  *q = first ? v : *q + v;
}

// NK blocks of dW: the 16 delta rows row0 .. row0 + 15 of dl (chunk uc of the packed layout) x inputs 16 (kc0 + t) .. + 15 (rows of
// A), summed over the tile's 64 columns, into the partial's packed layout [uc][k][16]; inputs >= in (the observation's padding) are left
// out.  (The rows are named by base and offset because each unit keeps the address arithmetic it had: grad_kernel passes its layer's
// rows and 16 uc, the sequence kernels the chunk's own pointer and 0.  With one pointer alone grad_kernel's instructions move.)
template <int NK>
__device__ __forceinline__ void grad_dw_blocks(const float* dl, int row0, const float* A, int in, int uc, int kc0, uint32_t lane, float* pw,
                                               bool first) {
  const int n = (int)(lane & 15), kk = (int)(lane >> 4);
  f32x4 acc[NK];
#pragma unroll
  for (int t = 0; t < NK; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* drow = dl + (row0 + n) * kGradStride + 4 * kk;
  const float* arow = A + (kc0 * 16 + n) * kGradStride + 4 * kk;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(drow + 16 * j);
    f32x4 bv[NK];
#pragma unroll
    for (int t = 0; t < NK; ++t) bv[t] = *reinterpret_cast<const f32x4*>(arow + t * 16 * kGradStride + 16 * j);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int t = 0; t < NK; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[t][i], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < NK; ++t) {
    const int k = (kc0 + t) * 16 + n;                             // this lane's column of the block: input k, units 16 uc + 4 kk .. + 3
    if (k < in) grad_put4(pw + ((int64_t)uc * in + k) * 16 + 4 * kk, acc[t], first);
  }
}
// chunk uc's dW over all `in` inputs, at most 4 blocks of 16 x 16 in registers at a time.  (grad_kernel restates this loop and the
// row sum below in its own body: called as functions they move its instructions.)
__device__ __forceinline__ void grad_dw(const float* drows, const float* A, int in, int uc, uint32_t lane, float* pw, bool first) {
  const int nkc = (in + 15) / 16;
#pragma unroll 1
  for (int kc0 = 0; kc0 < nkc; kc0 += 4) {
    switch (nkc - kc0 < 4 ? nkc - kc0 : 4) {
      case 1: grad_dw_blocks<1>(drows, 0, A, in, uc, kc0, lane, pw, first); break;
      case 2: grad_dw_blocks<2>(drows, 0, A, in, uc, kc0, lane, pw, first); break;
      case 3: grad_dw_blocks<3>(drows, 0, A, in, uc, kc0, lane, pw, first); break;
      default: grad_dw_blocks<4>(drows, 0, A, in, uc, kc0, lane, pw, first); break;
    }
  }
}
// The row stage's log_std and exp(-log_std): the words of the argument record r (GradArgs, SeqArgsT: the host's values), or, for a
// policy that keeps them on the device (r.explore_tab: log_std[4] | std[4] | inv_std[4]), the table's, as wave-uniform loads at the
// point of use -- what an optimiser's earlier launch published is what this launch sees.  The arithmetic that follows is one text.
constexpr int kGradExploreInvStd = 8;
template <class Args>
__device__ __forceinline__ void grad_explore(const Args& r, float (&ls)[4], float (&is)[4]) {
  if (r.explore_tab) {
    const auto* tab = (const __attribute__((address_space(4))) float*)(uintptr_t)r.explore_tab;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      ls[o] = tab[o];
      is[o] = tab[kGradExploreInvStd + o];
    }
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      ls[o] = r.log_std[o];
      is[o] = r.inv_std[o];
    }
  }
}
// the sum of an LDS row's 64 columns in ascending order
__device__ __forceinline__ float grad_row_sum(const float* row) {
  float s = 0.0f;
#pragma unroll 4
  for (int q = 0; q < kTile / 4; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
    s = ((s + v[0]) + v[1]) + v[2] + v[3];
  }
  return s;
}

}  // namespace
