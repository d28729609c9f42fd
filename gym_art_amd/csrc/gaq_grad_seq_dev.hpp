// gaq_grad_seq_dev.hpp -- the device pieces of the sequence unit (gaq_policy_grad_seq.hip) that no cell owns, besides gaq_grad_dev.hpp:
// the head region of the LDS, the gates' sigmoid, the staging of a step's observations and of one [., H] row per sequence, and one
// head layer's forward.  Every function is force-inlined; the kernels keep the instructions they had when the unit held these
// (tools/kernel_asm_same.py against the parent).  Included after gaq_grad_dev.hpp by that unit only; internal to csrc/.
#pragma once

namespace {

constexpr int kSeqND = 5;                                         // rows of dlt: the 4 outputs' deltas and V's
constexpr int kSeqHeadBytes = (kSeqND + 4 + 4) * kTile * 4 + kGradStatsAc * kTile * 8;   // dlt, outs, V's parts, the statistics' lanes

__device__ __forceinline__ float seq_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// a step's observations -> X: dead columns 0, padded inputs -0, the rows up to a multiple of 16 0.  Sequence e's observation is
// step-row row0 + e while e < nlive; Idx: step-row row0 + sidx[e] (row0 = t S_src) where sidx[e] >= 0.  (The row lookup is a
// compile-time switch, not a callable: with a lambda for it the three sequence kernels' instructions move.)
template <bool Idx>
__device__ __forceinline__ void seq_stage_obs(float* X, const float* obs, const PolObsNorm& nm, int64_t row0, int nlive, const int* sidx,
                                              int D, int tid) {
  const int kin = (D + 3) & ~3, kx = (D + 15) & ~15;
  for (int f = tid; f < kTile * kx; f += kGradBlock) {
    const int e = f / kx, k = f - e * kx;
    float v = k >= kin ? 0.0f : -0.0f;
    if (k < D) {
      v = 0.0f;
      const int s = Idx ? sidx[e] : e;
      if (Idx ? s >= 0 : e < nlive) {
        v = obs[(row0 + s) * D + k];
        if (nm.tab) v = nm(v, k);
      }
    }
    X[k * kGradStride + grad_col(e)] = v;
  }
}

// this lane's row of an [., H] array (keep = false: read as 0) -> the H rows of R, lane = sequence, 4 units per 16-byte load
__device__ __forceinline__ void seq_stage_rows(float* R, const float* row, bool keep, int hid, uint32_t lane, int wave) {
  for (int q = wave; q < hid / 4; q += kGradWaves) {
    const f32x4 v = keep ? *reinterpret_cast<const f32x4*>(row + 4 * q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r) R[(4 * q + r) * kGradStride + grad_col((int)lane)] = v[r];
  }
}

// this wave's chunk (widths <= 64: at most one) of one head layer: rows 0 .. in-1 of A -> act(bias + W a) in the rows of O
__device__ __forceinline__ void seq_fwd_layer(const float* __restrict__ wl, int in, int width, int act, int wave, const float* A, float* O,
                                              uint32_t lane) {
  if (wave >= width / 16) return;
  const int h = (int)(lane >> 4);
  const float* b = wl + width * in + wave * 16 + 4 * h;
  const f32x4 b4 = {b[0], b[1], b[2], b[3]};
  f32x4 acc[4] = {b4, b4, b4, b4};
  const float* arow = A + h * kGradStride + (lane & 15) * 4;
  for (int k0 = 0; k0 < in; k0 += 4) {                            // (in is H or a head width: a multiple of 16)
    const f32x4 x = *reinterpret_cast<const f32x4*>(arow + k0 * kGradStride);
    const float a = wl[(wave * in + k0) * 16 + lane];
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[eb], acc[eb], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const f32x4 v = {pol_act(act, acc[0][r]), pol_act(act, acc[1][r]), pol_act(act, acc[2][r]), pol_act(act, acc[3][r])};
    *reinterpret_cast<f32x4*>(O + (wave * 16 + 4 * h + r) * kGradStride + (lane & 15) * 4) = v;
  }
}

}  // namespace
