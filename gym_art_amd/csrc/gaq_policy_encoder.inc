// gaq_policy_encoder.inc -- the device half of "an encoder in front of the cell" (include/gaq.h gaq_policy_desc_rnn_enc): text of
// gaq_policy.hip, included inside its unnamed namespace after every other kernel of the unit, because it is built from that unit's
// stages (PolTile, pol_stage_obs, mfma_layer, mfma_store).
//
// A recurrent policy with an encoder is obs -> [Linear -> hidden_act] x 1..2 -> cell -> head.  The cell's six kernels stay what they
// are: policy_encode_kernel runs in front of each of their launches and writes the encoder's last activations, the features [N, E], to
// a buffer of the handle's; the cell's launch then takes that buffer as its observation, with D = E and no normaliser.
// One workgroup = one tile of 64 envs, 4 waves, policy_mfma_kernel's staging and operand layout: the observation rows go into H
// (through the normaliser's table in the <PolObsNorm> instantiation), every layer is mfma_layer -- accumulators from the bias, ascending
// k-steps, each MFMA a k-ordered fmaf chain, the partial k-step of in_dim padded with +0 x -0 -- so a feature is bit for bit the hidden
// activation policy_mfma_kernel computes from the same weights.  A first layer of two goes through mfma_store into H in place; the last
// layer never touches LDS: the lane that holds 4 consecutive units of an env in an accumulator writes them through pol_act as one
// 16-byte store to the env's feature row (16 envs x 64 B per store instruction, the pattern of gru_cell's write-back of h').
// LDS = 256 B x max(in_dim rounded up to 4, the first width of two): 5 KiB for 18 inputs and one layer of any width.
// Tags 12 and 13 (+ 16 with a normaliser): instantiations of mfma_layer / mfma_store of their own, as every kernel of the unit has.
struct PolicyEncDev {
  PolicyDev trunk;                // the encoder's layers in PolicyDev's terms: w, in_dim, n_hidden, hidden_act, width, off
  float* feat;                    // [N, E] features, E = the last width
};

// this wave's NC chunks of the last layer, through the activation, to the feature rows of the tile's live envs / slots
template <int NC, class Row>
__device__ __forceinline__ void enc_store_feat(const f32x4 (&acc)[4][4], int act, int width, float* feat, const PolTile& t, Row row) {
  const int h = (int)(t.lane >> 4);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int u0 = (t.wave + 4 * j) * 16 + 4 * h;                 // this lane's 4 units of the chunk
#pragma unroll
    for (int eb = 0; eb < 4; ++eb) {
      const int e = eb * 16 + (int)(t.lane & 15);
      const f32x4 v = {pol_act(act, acc[j][eb][0]), pol_act(act, acc[j][eb][1]), pol_act(act, acc[j][eb][2]), pol_act(act, acc[j][eb][3])};
      if (e < t.nlive) *reinterpret_cast<f32x4*>(feat + row(e) * width + u0) = v;
    }
  }
}

// the tile's observations (rows row(e) of obs) -> its rows of en.feat
template <int Kernel, class Row, class... Norm>
__device__ __forceinline__ void policy_encode_tile(const PolicyEncDev& en, float* H, const PolTile& t, Row row, const float* obs, int D,
                                                   Norm... nm) {
  const PolicyDev& pol = en.trunk;
  pol_stage_obs(H, obs, D, t, row, nm...);
  __syncthreads();
  int in = pol.in_dim;
#pragma unroll 1
  for (int l = 0; l < pol.n_hidden; ++l) {
    const int width = pol.width[l];
    const float* wl = pol.w + pol.off[l];
    const int nc = (width / 16 - t.wave + 3) / 4;                 // chunks wave, wave + 4, ... below width / 16 (wave-uniform)
    const bool last = l + 1 == pol.n_hidden;
    f32x4 acc[4][4];
    switch (nc) {
      case 1: mfma_layer<1, Kernel>(wl, in, width, t.wave, H, t.lane, acc); break;
      case 2: mfma_layer<2, Kernel>(wl, in, width, t.wave, H, t.lane, acc); break;
      case 3: mfma_layer<3, Kernel>(wl, in, width, t.wave, H, t.lane, acc); break;
      case 4: mfma_layer<4, Kernel>(wl, in, width, t.wave, H, t.lane, acc); break;
      default: break;
    }
    if (last) {
      switch (nc) {
        case 1: enc_store_feat<1>(acc, pol.hidden_act, width, en.feat, t, row); break;
        case 2: enc_store_feat<2>(acc, pol.hidden_act, width, en.feat, t, row); break;
        case 3: enc_store_feat<3>(acc, pol.hidden_act, width, en.feat, t, row); break;
        case 4: enc_store_feat<4>(acc, pol.hidden_act, width, en.feat, t, row); break;
        default: break;
      }
    } else {                                                      // (last is uniform: every wave meets both barriers)
      __syncthreads();                                            // every wave has read the layer's input
      switch (nc) {
        case 1: mfma_store<1, Kernel>(acc, pol.hidden_act, t.wave, H, t.lane); break;
        case 2: mfma_store<2, Kernel>(acc, pol.hidden_act, t.wave, H, t.lane); break;
        case 3: mfma_store<3, Kernel>(acc, pol.hidden_act, t.wave, H, t.lane); break;
        case 4: mfma_store<4, Kernel>(acc, pol.hidden_act, t.wave, H, t.lane); break;
        default: break;
      }
      __syncthreads();
    }
    in = width;
  }
}

// the batch form: obs [rows, D] -> feat [rows, E], in front of every actor launch of a rollout (the bootstrap launch included)
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_encode_kernel(PolicyEncDev en, int64_t rows, const float* __restrict__ obs, int D, Norm... nm) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PolTile t;
  pol_tile_span(t, rows);
  if (t.first >= rows) return;
  policy_encode_tile<pol_tag<12, Norm...>>(en, reinterpret_cast<float*>(smem), t, PolRowBatch{t.first}, obs, D, nm...);
}

// the gathered form, in front of the cell's terminal-value launch: the terminal observations of the listed envs -> the SAME rows of
// feat (row = env).  The batch launch's features of this step have been consumed by then (the cell's launch of the step is earlier in
// the stream) and the next batch launch overwrites every row, so the handle needs no second buffer.
template <class... Norm>
__global__ __launch_bounds__(kPolMfmaBlock) __attribute__((amdgpu_waves_per_eu(2)))
void policy_encode_term_kernel(PolicyEncDev en, PolicyTermDev tm, int D, Norm... nm) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PolTile t;
  if (!pol_tile_list(t, tm.count)) return;
  policy_encode_tile<pol_tag<13, Norm...>>(en, reinterpret_cast<float*>(smem), t, PolRowList{tm.list, t.first}, tm.term_obs, D, nm...);
}
