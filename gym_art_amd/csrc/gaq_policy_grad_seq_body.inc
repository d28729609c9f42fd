// gaq_policy_grad_seq_body.inc -- the body of grad_seq_kernel<L, Bwd, Idx> and of grad_seq_dx_kernel<L, Idx> (gaq_policy_grad_seq.hip: Bwd,
// with dfeat_t = W_ih^T planes written beside the dW stage under `if constexpr (Dx)`), with `g` in scope.  The frame --
// the LDS head, the column layout, the idx rules, the staging, the head's forward and backward, the row stage, dW, the W_hh^T product --
// is written once; what is the cell's own stands under `if constexpr (L)` (the LSTM) ... else (the GRU).
// It stays included text: a kernel body one call below its __global__ entry point, even force-inlined, gets another register
// allocation (DESIGN.md r15, r35), and these kernels keep their recorded resource lines.
// The LSTM's own: four gate sums per unit, every one over both products; the cell state c, which the lane that owns 4 units x 4 column
// blocks of its wave's chunk carries in 16 registers through the forward sweep (0 by select after a done and in dead columns); the
// tape, [T][64][2][H] per workgroup (h_t then c_t of a sequence side by side); in the backward sweep cin_t read from the tape by the
// owning lane (four 16-byte loads under the select that cuts the carried gradients), the carried dc in LDS rows of its own beside the
// carried dh, four contiguous delta planes in the packed row order.  The GRU's own: n_x and n_h apart, so dW_ih takes the planes
// 0, 1, 2 and dW_hh the planes 0, 1, 3, and a direct term dh z carried beside W_hh^T's.
// Idx (with Bwd): sequence e of a tile is column sidx[e] = idx[row0 + e] of every input; only the addresses of the loads differ, and a
// column whose index is out of range is a dead lane.
  constexpr int NG = L ? 4 : 3;                                   // gates
  // Dx: the kernel also writes dfeat_t, the gradient of the cell's input (grad_seq_dx_kernel, whose record has the pointer)
  constexpr bool Dx = !std::is_same_v<std::remove_cv_t<decltype(g)>, SeqArgsT<L>>;
  constexpr int TS = L ? 2 : 1;                                   // [., H] rows of a sequence's tape entry: h_t (and c_t)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dlt = reinterpret_cast<float*>(smem);                    // [5][64] the head's delta, sequence e at column grad_col(e)
  float* outs = dlt + kSeqND * kTile;                             // [4][64] the head's sums, sequence e at e
  float* vsum = outs + 4 * kTile;                                 // [4][64] the waves' parts of V
  double* red = reinterpret_cast<double*>(smem + (kSeqND + 8) * kTile * 4);   // [kGradStatsAc][64]
  [[maybe_unused]] int* sidx = reinterpret_cast<int*>(smem + kSeqHeadBytes);   // Idx: [64] the tile's source columns (or < 0)
  float* X = reinterpret_cast<float*>(smem + kSeqHeadBytes + (Idx ? kGradIdxBytes : 0));   // [kx][68] the observation
  const PolicyDev& net = g.net;
  const int D = net.in_dim, kx = (D + 15) & ~15, nh = net.n_hidden, act = net.hidden_act, H = net.width[0], hc = H / 16;
  const int w1 = nh > 1 ? net.width[1] : 0;
  float* Hin = X + kx * kGradStride;                              // [H][68] hin_t
  [[maybe_unused]] float* DH = Hin + H * kGradStride;             // Bwd: [H][68] the carried dh
  [[maybe_unused]] float* DC = DH + H * kGradStride;              // Bwd, L: [H][68] the carried dc
  float* P = Hin + (Bwd ? (L ? 3 : 2) : 1) * H * kGradStride;     // h_t, then the head's layers; Bwd: then the four delta planes of H rows
  auto Hl = [&](int l) { return P + ((l > 0 ? H : 0) + (l > 1 ? w1 : 0)) * kGradStride; };   // layer l's rows (0: the cell's h_t)
  const uint32_t lane = threadIdx.x & 63u;
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int G = (int)gridDim.x, T = g.T;
  const int64_t S = g.S;
  const int64_t t0 = (int64_t)blockIdx.x * g.ntiles / G, t1 = ((int64_t)blockIdx.x + 1) * g.ntiles / G;
  [[maybe_unused]] float* part = g.part + (int64_t)blockIdx.x * g.pstride;
  [[maybe_unused]] float* tape = g.tape + (int64_t)blockIdx.x * T * kTile * TS * H;
  const bool hasv = g.wv != nullptr;
  const int lw = net.width[nh - 1];                               // what the 4-output layer reads
  const float* wo = net.w + net.off[nh];                          // [lw][4], then bias[4]
  const int h4 = (int)(lane >> 4), n16 = (int)(lane & 15);
  // u0, this lane's first unit of its wave's chunk (wave < hc), and done[t-1]'s address below are each written per cell: where such a sum
  // is formed moves the kernels' instructions (DESIGN.md r37).  The LSTM's kernels were recorded with u0 formed here and dprev once per
  // step, the GRU's with both formed where they are used -- and a copy up here, even a dead one, is what the compiler would use.
  [[maybe_unused]] int u0_lstm = 0;
  if constexpr (L) u0_lstm = wave * 16 + 4 * h4;
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (Bwd && wave == 0) {
#pragma unroll
    for (int s = 0; s < kGradStatsAc; ++s) red[s * kTile + lane] = 0.0;
  }

  // the head over h_t in Hl(0): its layers, the 4 sums and V's parts; ends after the barrier that follows them
  auto head_forward = [&]() {
#pragma unroll 1
    for (int l = 1; l < nh; ++l) {
      seq_fwd_layer(net.w + net.off[l], net.width[l - 1], net.width[l], act, wave, Hl(l - 1), Hl(l), lane);
      __syncthreads();
    }
    const float* ycol = Hl(nh - 1) + grad_col((int)lane);
    {
      float s = wo[lw * 4 + wave];
#pragma unroll 8
      for (int u = 0; u < lw; ++u) s = __builtin_fmaf(wo[u * 4 + wave], ycol[u * kGradStride], s);
      outs[wave * kTile + lane] = s;
    }
    if (hasv) {                                                   // this wave's quarter of V: policy_value_part's chain
      const int q = lw / kGradWaves;
      float v = 0.0f;
#pragma unroll 8
      for (int u = wave * q; u < (wave + 1) * q; ++u) v = __builtin_fmaf(g.wv[u], ycol[u * kGradStride], v);
      vsum[wave * kTile + lane] = v;
    }
    __syncthreads();
  };

#pragma unroll 1
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t row0 = tile * kTile;
    const int nlive = (int)((S - row0) < kTile ? (S - row0) : kTile);
    if constexpr (Idx) {
      // the tile's indices, read once: an index outside [0, S_src) makes its lane a dead one (no address is ever formed from it) and
      // is counted by the row stage.  (The last readers of sidx, the previous tile's last step, stand behind a barrier.)
      if (tid < kTile) {
        const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<L>*)__builtin_amdgcn_kernarg_segment_ptr();
        int s = kGradIdxDead;
        if (tid < nlive) {
          const int64_t v = r.idx[row0 + tid];
          s = v >= 0 && v < r.S_src ? (int)v : kGradIdxSkipped;
        }
        sidx[tid] = s;
      }
      __syncthreads();
    }
    // Idx: lane e's source column (0 where it has none: then nothing is read through it), and whether it has one
    [[maybe_unused]] auto scol = [&](int e) -> int64_t { const int s = sidx[e]; return s >= 0 ? s : 0; };
    [[maybe_unused]] auto shas = [&](int e) -> bool { return sidx[e] >= 0; };
    bool live_;
    if constexpr (Idx) live_ = shas((int)lane);
    else live_ = (int)lane < nlive;
    const bool live = live_;
    // whether e is a live column, and its row of an [S (S_src), .] input
    auto has = [&](int e) -> bool {
      if constexpr (Idx) return shas(e);
      else return e < nlive;
    };
    auto srow = [&](int e) -> int64_t {
      if constexpr (Idx) return scol(e);
      else return row0 + e;
    };
    // done[t-1] of sequence e (base, tsrc, dprev: step t's; dprev is where step t-1's row of done starts)
    auto pdone = [&](int64_t base, [[maybe_unused]] int64_t tsrc, [[maybe_unused]] int64_t dprev, auto e) -> bool {
      if constexpr (L) return g.done[dprev + srow((int)e)] != 0;
      else if constexpr (Idx) return g.done[tsrc - g.S_src + scol((int)e)] != 0;
      else return g.done[base - S + e] != 0;
    };
    // ---- the forward sweep -------------------------------------------------------------------------------------------------------------
    [[maybe_unused]] f32x4 cst[4];                                // L, wave < hc: c of this lane's 4 units, one vector per column block
    if constexpr (L) {
#pragma unroll
      for (int eb = 0; eb < 4; ++eb) cst[eb] = zero4;
    }
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      const int64_t base = (int64_t)t * S + row0;
      [[maybe_unused]] const int64_t tsrc = (int64_t)t * g.S_src;   // Idx: the step's first row in a [T, S_src, ...] input
      [[maybe_unused]] const int64_t dprev = Idx ? tsrc - g.S_src : base - S - row0;   // L
      seq_stage_obs<Idx>(X, g.obs, g.nm, Idx ? tsrc : base, nlive, sidx, D, tid);
      if (t == 0) {
        seq_stage_rows(Hin, g.h0 + srow((int)lane) * H, live, H, lane, wave);
      } else {                                                    // hin_t = h_{t-1} (still in Hl(0)), 0 where done[t-1] and in dead columns
        for (int f = tid; f < H * kTile; f += kGradBlock) {
          const int u = f >> 6, col = f & 63, e = grad_env(col);
          const bool keep = has(e) && !pdone(base, tsrc, dprev, e);
          Hin[u * kGradStride + col] = keep ? P[u * kGradStride + col] : 0.0f;
        }
      }
      if constexpr (L) {
        if (wave < hc) {                                          // cin_t, by the same select
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) {
            const int e = eb * 16 + n16;
            if (t == 0) cst[eb] = has(e) ? *reinterpret_cast<const f32x4*>(g.c0 + srow(e) * H + u0_lstm) : zero4;
            else cst[eb] = has(e) && !pdone(base, tsrc, dprev, e) ? cst[eb] : zero4;
          }
        }
      }
      __syncthreads();
      if (wave < hc) {
        const int u0 = L ? u0_lstm : wave * 16 + 4 * h4;
        f32x4 acc[4][4];
        f32x4 hn[4];
        if constexpr (L) lstm_gates(net, g.off_hh, wave, X, Hin, lane, acc);
        else seq_gates(net, g.off_hh, wave, X, Hin, lane, acc);
#pragma unroll
        for (int eb = 0; eb < 4; ++eb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (L) {
              const float ig = seq_sigmoid(acc[0][eb][r]), fg = seq_sigmoid(acc[1][eb][r]);
              const float gg = tanhf(acc[2][eb][r]), og = seq_sigmoid(acc[3][eb][r]);
              cst[eb][r] = __builtin_fmaf(fg, cst[eb][r], ig * gg);
              hn[eb][r] = og * tanhf(cst[eb][r]);
            } else {
              const float hold = Hin[(u0 + r) * kGradStride + n16 * 4 + eb];
              const float rg = seq_sigmoid(acc[0][eb][r]), zg = seq_sigmoid(acc[1][eb][r]);
              const float n = tanhf(__builtin_fmaf(rg, acc[3][eb][r], acc[2][eb][r]));
              hn[eb][r] = __builtin_fmaf(zg, hold - n, n);
            }
          }
          const int e = eb * 16 + n16;
          if (e < nlive) {
            if constexpr (Bwd) {
              float* row = tape + ((int64_t)t * kTile + e) * TS * H + u0;
              *reinterpret_cast<f32x4*>(row) = hn[eb];
              if constexpr (L) *reinterpret_cast<f32x4*>(row + H) = cst[eb];
            } else if (t == T - 1 && (L || g.h_out)) {
              const bool z = g.done[base + e] != 0;
              if (g.h_out) *reinterpret_cast<f32x4*>(g.h_out + (row0 + e) * H + u0) = z ? zero4 : hn[eb];
              if constexpr (L) {
                if (g.c_out) *reinterpret_cast<f32x4*>(g.c_out + (row0 + e) * H + u0) = z ? zero4 : cst[eb];
              }
            }
          }
        }
        if (!Bwd || t + 1 < T) {                                   // (the backward sweep reloads h_{T-1} from the tape)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 v = {hn[0][r], hn[1][r], hn[2][r], hn[3][r]};
            *reinterpret_cast<f32x4*>(P + (u0 + r) * kGradStride + n16 * 4) = v;
          }
        }
      }
      __syncthreads();
      if constexpr (!Bwd) {
        head_forward();
        if (wave == 0 && live) {                                  // lane = sequence
          const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<L>*)__builtin_amdgcn_kernarg_segment_ptr();
          const int e = (int)lane;
          const int64_t i = base + e;
          float m[4];
#pragma unroll
          for (int o = 0; o < 4; ++o) {
            m[o] = outs[o * kTile + e];
            if (net.out_tanh) m[o] = tanhf(m[o]);
          }
          if (r.logp_out) {
            float z[4], lp = 0.0f, ls[4], is[4];
            grad_explore(r, ls, is);
#pragma unroll
            for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * is[o];
#pragma unroll
            for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
            r.logp_out[i] = lp - kGradTwoLn2Pi;
          }
          if (r.value_out) r.value_out[i] = ((vsum[e] + vsum[kTile + e]) + (vsum[2 * kTile + e] + vsum[3 * kTile + e])) + r.wv[lw];
          if (r.mean_out) {
#pragma unroll
            for (int o = 0; o < 4; ++o) r.mean_out[i * 4 + o] = m[o];
          }
        }
        // (no barrier: the next writers of outs and vsum stand behind the next step's two)
      }
    }
    // ---- the backward sweep ------------------------------------------------------------------------------------------------------------
    if constexpr (Bwd) {
#pragma unroll 1
      for (int t = T - 1; t >= 0; --t) {
        const bool first = tile == t0 && t == T - 1, last_t = t == T - 1;
        const int64_t base = (int64_t)t * S + row0;
        [[maybe_unused]] const int64_t tsrc = (int64_t)t * g.S_src;
        [[maybe_unused]] const int64_t dprev = Idx ? tsrc - g.S_src : base - S - row0;   // L
        seq_stage_obs<Idx>(X, g.obs, g.nm, Idx ? tsrc : base, nlive, sidx, D, tid);
        if (t == 0) seq_stage_rows(Hin, g.h0 + srow((int)lane) * H, live, H, lane, wave);
        else seq_stage_rows(Hin, tape + ((int64_t)(t - 1) * kTile + lane) * TS * H, live && !pdone(base, tsrc, dprev, lane), H, lane, wave);
        seq_stage_rows(P, tape + ((int64_t)t * kTile + lane) * TS * H, live, H, lane, wave);
        __syncthreads();
        head_forward();
        if (wave == 0) {                                          // lane = sequence: gaq_policy_grad_ppo_ac_dev's row stage
          const auto& r = *(const __attribute__((address_space(4))) SeqArgsT<L>*)__builtin_amdgcn_kernarg_segment_ptr();
          const int e = (int)lane;
          int64_t i_;
          if constexpr (Idx) i_ = tsrc + scol(e);
          else i_ = base + e;
          const int64_t i = i_;
          if constexpr (Idx) {                                    // a skipped index is counted once, in the spare statistic
            if (last_t && sidx[e] == kGradIdxSkipped) red[(kGradStatsAc - 1) * kTile + e] += 1.0;
          }
          float d[kSeqND];                                        // the head's delta (already times scale)
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) d[o] = 0.0f;
          if (live) {
            float m[4], dm[4], z[4], lp = 0.0f, ls[4], is[4];
            grad_explore(r, ls, is);
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              m[o] = outs[o * kTile + e];
              if (net.out_tanh) m[o] = tanhf(m[o]);
              dm[o] = net.out_tanh ? __builtin_fmaf(-m[o], m[o], 1.0f) : 1.0f;
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) z[o] = (r.a[i * 4 + o] - m[o]) * is[o];
#pragma unroll
            for (int o = 0; o < 4; ++o) lp += __builtin_fmaf(-0.5f * z[o], z[o], -ls[o]);
            lp -= kGradTwoLn2Pi;
            const float x = lp - r.logp_old[i], rt = expf(x), adv = r.adv[i];
            const float s1 = rt * adv, s2 = fminf(fmaxf(rt, 1.0f - r.clip), 1.0f + r.clip) * adv;
            const float dl = s1 <= s2 ? -adv * rt : 0.0f;          // dL / dlogp
            red[e] += (double)-fminf(s1, s2);
            red[kTile + e] += s2 < s1 ? 1.0 : 0.0;
            red[2 * kTile + e] += (double)rt - 1.0 - (double)x;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              d[o] = r.scale * dl * z[o] * is[o] * dm[o];
              red[(3 + o) * kTile + e] += (double)(r.scale * dl) * ((double)z[o] * (double)z[o] - 1.0);
            }
            if (r.wv) {                                           // L_V = 1/2 max(e1^2, e2^2); dL_V / dV = e1 unless the clipped error is larger
              const float V = ((vsum[e] + vsum[kTile + e]) + (vsum[2 * kTile + e] + vsum[3 * kTile + e])) + r.wv[lw];
              const float ret = r.ret[i], e1 = V - ret;
              float lv = e1 * e1, dv = e1;
              if (r.vclip > 0.0f) {                               // (where the clamp does not bind, e2 is e1 itself: a tie)
                const float vo = r.v_old[i], dvo = V - vo, cl = fminf(fmaxf(dvo, -r.vclip), r.vclip);
                const float e2 = cl == dvo ? e1 : vo + cl - ret, l2 = e2 * e2;
                if (!(lv >= l2)) {
                  lv = l2;
                  dv = 0.0f;
                  red[8 * kTile + e] += 1.0;
                }
              }
              d[4] = r.scale * r.vf_coef * dv;
              red[7 * kTile + e] += 0.5 * (double)lv;
            }
          }
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) dlt[o * kTile + grad_col(e)] = d[o];
        }
        __syncthreads();
        // the 4-output layer and the value head: thread u owns unit u of what they read -- dWo[u][:] and dwv[u], then its row becomes
        // delta (with the activation's derivative only where the row is a head layer's, not the cell's h_t); 5 more threads sum dbo, dbv
        float* pv = part + net.off[nh] + (lw + 1) * 4;             // the value head's words follow the packed weights
        if (tid < lw) {
          float* yrow = Hl(nh - 1) + tid * kGradStride;
          float w4[kSeqND], gw[kSeqND];
#pragma unroll
          for (int o = 0; o < 4; ++o) w4[o] = wo[tid * 4 + o];
          w4[4] = hasv ? g.wv[tid] : 0.0f;
#pragma unroll
          for (int o = 0; o < kSeqND; ++o) gw[o] = 0.0f;
#pragma unroll 4
          for (int q = 0; q < kTile / 4; ++q) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(yrow + 4 * q);
            f32x4 dv[kSeqND], nv;
#pragma unroll
            for (int o = 0; o < kSeqND; ++o) dv[o] = *reinterpret_cast<const f32x4*>(dlt + o * kTile + 4 * q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              float s = 0.0f;
#pragma unroll
              for (int o = 0; o < kSeqND; ++o) {
                gw[o] = __builtin_fmaf(dv[o][c], hv[c], gw[o]);
                s = __builtin_fmaf(w4[o], dv[o][c], s);
              }
              nv[c] = nh > 1 ? s * grad_actd(act, hv[c]) : s;
            }
            *reinterpret_cast<f32x4*>(yrow + 4 * q) = nv;
          }
#pragma unroll
          for (int o = 0; o < 4; ++o) grad_put(part + net.off[nh] + tid * 4 + o, gw[o], first);
          if (hasv) grad_put(pv + tid, gw[4], first);
        } else if (tid >= kGradBlock - kSeqND && (tid < kGradBlock - 1 || hasv)) {
          const int o = tid - (kGradBlock - kSeqND);
          float s = 0.0f;
          for (int c = 0; c < kTile; ++c) s += dlt[o * kTile + c];
          grad_put(o < 4 ? part + net.off[nh] + lw * 4 + o : pv + lw, s, first);
        }
        __syncthreads();
        // the head's layers, from the last down to the first: dW_l and db_l, then the delta of the layer's input in place
#pragma unroll 1
        for (int l = nh - 1; l >= 1; --l) {
          const int width = net.width[l], in = net.width[l - 1];
          float* A = Hl(l - 1);
          const float* dl = Hl(l);
          const float* wl = net.w + net.off[l];
          float* pw = part + net.off[l];
          if (wave < width / 16) grad_dw(dl + wave * 16 * kGradStride, A, in, wave, lane, pw, first);
          if (tid < width) grad_put(pw + width * in + tid, grad_row_sum(dl + tid * kGradStride), first);
          __syncthreads();                                        // dW_l has consumed the layer's input
          if (wave < in / 16) {
            const int kc = wave;
            f32x4 acc[4];
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) acc[eb] = zero4;
            for (int uch = 0; uch < width / 16; ++uch) {
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + ((int64_t)uch * in + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(dl + (uch * 16 + 4 * h4 + i) * kGradStride + n16 * 4);
#pragma unroll
                for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              f32x4* pos = reinterpret_cast<f32x4*>(A + (kc * 16 + 4 * h4 + r) * kGradStride + n16 * 4);
              if (l > 1) {
                const f32x4 hv = *pos;
                const f32x4 nv = {acc[0][r] * grad_actd(act, hv[0]), acc[1][r] * grad_actd(act, hv[1]), acc[2][r] * grad_actd(act, hv[2]),
                                  acc[3][r] * grad_actd(act, hv[3])};
                *pos = nv;
              } else {
                const f32x4 nv = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
                *pos = nv;
              }
            }
          }
          __syncthreads();
        }
        // the cell: Hl(0) now holds the head's dh_t.  Each lane reads its 16 words of it (and of what is carried) before it writes the
        // planes, whose first H rows are those very rows; the other planes lie over the head's layers, which are spent.
        bool cut[4];                                              // done[t-1] or a dead column: nothing is carried in or out
        if constexpr (L) {                                        // (cin_t needs it; the GRU not before dh_{t-1})
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) {
            const int e = eb * 16 + n16;
            cut[eb] = !has(e) || (t > 0 && pdone(base, tsrc, dprev, e));
          }
        }
        if (wave < hc) {
          const int u0 = L ? u0_lstm : wave * 16 + 4 * h4;
          f32x4 acc[4][4];
          if constexpr (L) {
            lstm_gates(net, g.off_hh, wave, X, Hin, lane, acc);
            f32x4 cin[4];                                         // cin_t of the column blocks: c_{t-1} from the tape (c0 at t = 0) or 0
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) {
              const int e = eb * 16 + n16;
              const float* crow = t == 0 ? g.c0 + srow(e) * H + u0 : tape + (((int64_t)(t - 1) * kTile + e) * 2 + 1) * H + u0;
              cin[eb] = cut[eb] ? zero4 : *reinterpret_cast<const f32x4*>(crow);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int off = (u0 + r) * kGradStride + n16 * 4;
              f32x4 dh = *reinterpret_cast<const f32x4*>(P + off);
              f32x4 dcc = zero4;
              if (!last_t) {
                dh += *reinterpret_cast<const f32x4*>(DH + off);
                dcc = *reinterpret_cast<const f32x4*>(DC + off);
              }
              f32x4 dai, daf, dag, dao, dcn;
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) {
                const float ig = seq_sigmoid(acc[0][eb][r]), fg = seq_sigmoid(acc[1][eb][r]);
                const float gg = tanhf(acc[2][eb][r]), og = seq_sigmoid(acc[3][eb][r]);
                const float ci = cin[eb][r];
                const float tc = tanhf(__builtin_fmaf(fg, ci, ig * gg));
                const float dc = dcc[eb] + dh[eb] * og * __builtin_fmaf(-tc, tc, 1.0f);
                dao[eb] = dh[eb] * tc * og * (1.0f - og);
                dai[eb] = dc * gg * ig * (1.0f - ig);
                daf[eb] = dc * ci * fg * (1.0f - fg);
                dag[eb] = dc * ig * __builtin_fmaf(-gg, gg, 1.0f);
                dcn[eb] = cut[eb] ? 0.0f : dc * fg;
              }
              *reinterpret_cast<f32x4*>(P + off) = dai;
              *reinterpret_cast<f32x4*>(P + H * kGradStride + off) = daf;
              *reinterpret_cast<f32x4*>(P + 2 * H * kGradStride + off) = dag;
              *reinterpret_cast<f32x4*>(P + 3 * H * kGradStride + off) = dao;
              *reinterpret_cast<f32x4*>(DC + off) = dcn;
            }
          } else {
            seq_gates(net, g.off_hh, wave, X, Hin, lane, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int off = (u0 + r) * kGradStride + n16 * 4;
              const f32x4 hold = *reinterpret_cast<const f32x4*>(Hin + off);
              f32x4 dh = *reinterpret_cast<const f32x4*>(P + off);
              if (!last_t) dh += *reinterpret_cast<const f32x4*>(DH + off);
              f32x4 dar, daz, dan, dnh, dir;
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) {
                const float rg = seq_sigmoid(acc[0][eb][r]), zg = seq_sigmoid(acc[1][eb][r]), nhh = acc[3][eb][r];
                const float n = tanhf(__builtin_fmaf(rg, nhh, acc[2][eb][r]));
                dan[eb] = dh[eb] * (1.0f - zg) * __builtin_fmaf(-n, n, 1.0f);
                daz[eb] = dh[eb] * (hold[eb] - n) * zg * (1.0f - zg);
                dar[eb] = dan[eb] * nhh * rg * (1.0f - rg);
                dnh[eb] = dan[eb] * rg;
                dir[eb] = dh[eb] * zg;
              }
              *reinterpret_cast<f32x4*>(P + off) = dar;
              *reinterpret_cast<f32x4*>(P + H * kGradStride + off) = daz;
              *reinterpret_cast<f32x4*>(P + 2 * H * kGradStride + off) = dan;
              *reinterpret_cast<f32x4*>(P + 3 * H * kGradStride + off) = dnh;
              *reinterpret_cast<f32x4*>(DH + off) = dir;
            }
          }
        }
        __syncthreads();
        // dW_ih = planes x^T and dW_hh = planes hin^T in the packed layout (chunk uc = gate * H/16 + c).  The LSTM's four planes serve
        // both and b_ih and b_hh take the same sum; the GRU's W_hh skips the plane da_n for dn_h, and its n words of b_ih and b_hh are
        // those two planes' sums
        auto hplane = [&](int uc) {
          if constexpr (L) return uc;
          else return uc < 2 * hc ? uc : uc + hc;
        };
        {
          float* pih = part + net.off[0];
          float* phh = part + g.off_hh;
#pragma unroll 1
          for (int uc = wave; uc < NG * hc; uc += kGradWaves) {
            grad_dw(P + uc * 16 * kGradStride, X, D, uc, lane, pih, first);
            grad_dw(P + hplane(uc) * 16 * kGradStride, Hin, H, uc, lane, phh, first);
          }
          if (tid < 4 * H) {
            const float s = grad_row_sum(P + tid * kGradStride);
            if constexpr (L) {
              grad_put(pih + 4 * H * D + tid, s, first);
              grad_put(phh + 4 * H * H + tid, s, first);
            } else {
              if (tid < 3 * H) grad_put(pih + 3 * H * D + tid, s, first);
              if (tid < 2 * H) grad_put(phh + 3 * H * H + tid, s, first);
              if (tid >= 3 * H) grad_put(phh + 3 * H * H + tid - H, s, first);
            }
          }
        }
        // Dx: dfeat_t = W_ih^T planes (the GRU: da_r, da_z, da_n; the LSTM: all four) -- the W_hh^T product's code shape below with
        // in = D, this wave's input chunks wave, wave + 4, ...  The lane that holds 4 consecutive inputs of a sequence stores them as
        // one 16-byte store to the sequence's row of dfeat [T, S (S_src), D] (enc_store_feat's pattern); a dead column has no row, a
        // live one whose deltas are 0 writes zeros.
        if constexpr (Dx) {
          const float* wih = net.w + net.off[0];
#pragma unroll 1
          for (int kc = wave; kc < D / 16; kc += kGradWaves) {
            f32x4 acc[4];
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) acc[eb] = zero4;
            for (int uch = 0; uch < NG * hc; ++uch) {
              const float* drows = P + uch * 16 * kGradStride;
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wih + ((int64_t)uch * D + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(drows + (4 * h4 + i) * kGradStride + n16 * 4);
#pragma unroll
                for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
              }
            }
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) {
              const int e = eb * 16 + n16;
              if (has(e)) {
                int64_t row;
                if constexpr (Idx) row = tsrc + scol(e);
                else row = base + e;
                *reinterpret_cast<f32x4*>(g.dfeat + row * D + kc * 16 + 4 * h4) = acc[eb];
              }
            }
          }
        }
        // dh_{t-1} = W_hh^T planes (the GRU: + direct), 0 where done[t-1] (and in dead columns); nothing flows into h0
        if (t > 0 && wave < hc) {
          const float* whh = net.w + g.off_hh;
          const int kc = wave;
          f32x4 acc[4];
#pragma unroll
          for (int eb = 0; eb < 4; ++eb) acc[eb] = zero4;
          for (int uch = 0; uch < NG * hc; ++uch) {
            const float* drows = P + hplane(uch) * 16 * kGradStride;
            const f32x4 wv = *reinterpret_cast<const f32x4*>(whh + ((int64_t)uch * H + kc * 16 + n16) * 16 + 4 * h4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(drows + (4 * h4 + i) * kGradStride + n16 * 4);
#pragma unroll
              for (int eb = 0; eb < 4; ++eb) acc[eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[eb], acc[eb], 0, 0, 0);
            }
          }
          if constexpr (!L) {
#pragma unroll
            for (int eb = 0; eb < 4; ++eb) {
              const int e = eb * 16 + n16;
              cut[eb] = !has(e) || pdone(base, tsrc, dprev, e);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            f32x4* pos = reinterpret_cast<f32x4*>(DH + (kc * 16 + 4 * h4 + r) * kGradStride + n16 * 4);
            if constexpr (L) {
              const f32x4 nv = {cut[0] ? 0.0f : acc[0][r], cut[1] ? 0.0f : acc[1][r], cut[2] ? 0.0f : acc[2][r], cut[3] ? 0.0f : acc[3][r]};
              *pos = nv;
            } else {                                              // + the direct term dh z, which the cell left here
              const f32x4 dir = *pos;
              const f32x4 nv = {cut[0] ? 0.0f : acc[0][r] + dir[0], cut[1] ? 0.0f : acc[1][r] + dir[1], cut[2] ? 0.0f : acc[2][r] + dir[2],
                                cut[3] ? 0.0f : acc[3][r] + dir[3]};
              *pos = nv;
            }
          }
        }
        __syncthreads();                                          // X, hin and the planes are read before the next step is staged
      }
    }
  }

  if constexpr (Bwd) {
    if (tid < kGradStatsAc) {                                     // the 64 lanes in ascending order
      double s = 0.0;
      for (int e = 0; e < kTile; ++e) s += red[tid * kTile + e];
      g.spart[(int64_t)blockIdx.x * kGradStatsAc + tid] = s;
    }
  }
