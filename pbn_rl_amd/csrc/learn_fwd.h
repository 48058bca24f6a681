// learn_fwd.h -- the first of the fused BDQ update's three launches (pbn_learn.hip):
//
//   learn_fwd    3 B/16 blocks.  Block = 16 transitions of one of three row sets (online network
//                on s, online on s', target network on s').  The bilinear layer is a sum of
//                target-table rows (T[t][i][:] = sum_j target_t[j] W[:, i, j], the table the acting
//                kernel reads) over the state's set bits; the trunk and the heads run on
//                v_mfma_f32_16x16x4_f32 with the 16 transitions as the MFMA's columns and the
//                activations in LDS.  Stores the raw head outputs of all three sets and, for the
//                online s rows, every layer's activation (the backward's operands).
#pragma once
#include "learn_args.h"

namespace {

// ---- forward tiles.  Activations in LDS are blocked [K/16][16 rows][16]: the float4 at
// (kb, r, 4g) holds features 16 kb + 4g .. +3 of row r, the B operand of four k-steps of lane
// (g = lane >> 4, r = lane & 15).  D[o][r] = sum_k W[o][k] X[k][r] for the 16 outputs o0..o0+15:
// lane l supplies A[o0 + (l & 15)][k] = one float4 of weight row o0 + (l & 15); its accumulator
// holds D[o0 + 4g + v][r], v = 0..3.
// The weight fragments come in registers, loaded by wfrag before the layer's inputs are ready
// (every layer's fragments are requested at kernel entry: one L2 round trip, not one per layer):
// output tile ot of a layer with K inputs, from its fwd tiles in the image (zero past n_ot tiles)
template <int K>
__device__ __forceinline__ void wfrag(float4 (&w)[K / 16], const float* __restrict__ tiles, int ot, int n_ot, int lane) {
  const bool ok = ot < n_ot;
  const float4* t = reinterpret_cast<const float4*>(tiles) + (size_t)(ok ? ot : 0) * (K / 16) * 64 + lane;
#pragma unroll
  for (int kb = 0; kb < K / 16; ++kb) {
    w[kb] = t[kb * 64];
    if (!ok) w[kb] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

template <int K>
__device__ __forceinline__ f32x4 fwd_tile(const float4 (&wf)[K / 16], const float* __restrict__ Xs, int lane) {
  const int g = lane >> 4, rr = lane & 15;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < K / 16; ++kb) {
    const float4 w = wf[kb];
    const float4 x = *reinterpret_cast<const float4*>(Xs + (kb * 16 + rr) * 16 + 4 * g);
    acc = mfma(w.x, x.x, acc);
    acc = mfma(w.y, x.y, acc);
    acc = mfma(w.z, x.z, acc);
    acc = mfma(w.w, x.w, acc);
  }
  return acc;
}

// bias + LeakyReLU, into the blocked LDS plane (tile o0) and, when `out` is set, the [O][B] plane
__device__ __forceinline__ void fwd_store(f32x4 acc, const float* __restrict__ bias, int o0, float slope,
                                          float* __restrict__ Ys, float* __restrict__ out, int B, int b0, int lane) {
  const int g = lane >> 4, rr = lane & 15;
  float4 y;
  float* yp = &y.x;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int o = o0 + 4 * g + v;
    yp[v] = leaky(acc[v] + bias[o], slope);
    if (out) out[(size_t)o * B + b0 + rr] = yp[v];
  }
  *reinterpret_cast<float4*>(Ys + ((o0 >> 4) * 16 + rr) * 16 + 4 * g) = y;
}

__global__ void __launch_bounds__(kThreads) learn_fwd_kernel(LearnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // carved by FwdLds (bdq_layout.h), which also sizes it
  const FwdLds at(a.H, a.A);
  float* Y1 = lds + at.y1;
  float* X2 = lds + at.x2;
  float* X3 = lds + at.x3;
  float* X4 = lds + at.x4;
  float* XH = lds + at.xh;
  float* tail = lds + at.tail();
  uint32_t* sw = reinterpret_cast<uint32_t*>(tail + at.sw);
  int* stg = reinterpret_cast<int*>(tail + at.stg);
  int* scnt = reinterpret_cast<int*>(tail + at.scnt);
  uint8_t* slist = reinterpret_cast<uint8_t*>(tail + at.slist);
  float* sbias = tail + at.sbias;
  const int tiles = a.B / kRows;
  const int set = blockIdx.x / tiles;
  const int b0 = (blockIdx.x - set * tiles) * kRows;
  const float* P = set == 2 ? a.PT : a.P;
  const float* Tq = set == 2 ? a.TqT : a.Tq;
  PBN_LSTAMP(0, 31);
  PBN_LSTAMP(0, 0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the biases, requested first (unguarded: a clamped index) and stored to LDS before the first
  // barrier
  const int nbias = fwd_bias_floats(a.H, a.A);
  float bv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) bv[k] = P[fwd_bias_src(a.off, a.H, min(tid + kThreads * k, nbias - 1))];
  const int B = a.B;
  float* keep = nullptr;   // the online s rows keep their activations for the backward
  // every layer's weight fragments of this wave, requested at entry (they arrive during the row
  // and bilinear phases: no barrier waits for them)
  const int at16 = a.Apad / 16;
  float4 w2[kD0 / 16], w3[kD1 / 16], w4[kD2 / 16], wh1[2][kD3 / 16], wh2[kDH / 16];
  auto fetch_weights = [&]() {
    wfrag<kD0>(w2, Tq + a.ifw[LY2], wave, kD1 / 16, lane);
    if (wave < kD2 / 16) wfrag<kD1>(w3, Tq + a.ifw[LY3], wave, kD2 / 16, lane);   // (only these waves
    if (wave < kD3 / 16) wfrag<kD2>(w4, Tq + a.ifw[LY4], wave, kD3 / 16, lane);   // compute the layers)
#pragma unroll
    for (int u = 0; u < 2; ++u) wfrag<kD3>(wh1[u], Tq + a.ifw[LYH1], wave + kWaves * u, a.H * kDH / 16, lane);
    wfrag<kDH>(wh2, Tq + a.ifw[LYH2], wave < a.H * at16 ? wave : 0, a.H * at16, lane);
  };
  if (wave != 0) fetch_weights();   // (wave 0 loads the rows first: the load counter is in order)
  if (tid < kRows) {   // the rows' targets, state words and the list of their set bits
    const int64_t j = row_index(a, b0 + tid);
    stg[tid] = a.tgt[j];
    int c = 0;
    for (int w = 0; w < a.W; ++w) {
      uint32_t x = (set == 0 ? a.st : a.nst)[(size_t)w * a.cap + j];
      if (w == a.W - 1 && (a.N & 31)) x &= (1u << (a.N & 31)) - 1u;
      sw[w * kRows + tid] = x;
      while (x) {
        slist[tid * 128 + c++] = (uint8_t)(32 * w + __builtin_ctz(x));
        x &= x - 1u;
      }
    }
    scnt[tid] = c;
  }
  if (wave == 0) fetch_weights();
  // (unconditional: past the biases into a spare slot; a branch here made the wait counter's merge
  // hold the first barrier for every weight fragment)
#pragma unroll
  for (int k = 0; k < 4; ++k) sbias[min(tid + kThreads * k, nbias)] = bv[k];
  lds_barrier();
  PBN_LSTAMP(0, 1);
  // bilinear layer: y[o] = bias[o] + sum over the set bits i of T[t][i][o] (t = the row's target;
  // a row without a target has an all-zero second input: bias only).  Wave w takes rows 2w, 2w+1;
  // lane p reads Tq positions 4p..4p+3 ([t][i][j][q] = T[t][i][16 q + j]: o = 16 q + j): only the
  // table rows of set bits, eight of each row per round trip.
  {
    const float* bias = sbias;
    const int r0 = 2 * wave;
    const int t0 = stg[r0], t1 = stg[r0 + 1];
    const int c0 = t0 < a.n_attr ? scnt[r0] : 0, c1 = t1 < a.n_attr ? scnt[r0 + 1] : 0;
    float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    const int cm = max(c0, c1);
    if (cm > 0) {
      const uint8_t* l0 = slist + r0 * 128;
      const uint8_t* l1 = l0 + 128;
      // buffer loads: a lane past its row's count gets an out-of-range offset, whose load returns
      // zeros without memory traffic (it read table row 0 before: ~35 % of the reads at 14-17 bits)
      const int tb0 = __builtin_amdgcn_readfirstlane(c0 ? t0 : 0), tb1 = __builtin_amdgcn_readfirstlane(c1 ? t1 : 0);
      const int nrec = a.N * 256 * 4;
      __amdgpu_buffer_rsrc_t R0 = __builtin_amdgcn_make_buffer_rsrc((void*)(Tq + (size_t)tb0 * a.N * 256), (short)0, nrec, 0x00020000);
      __amdgpu_buffer_rsrc_t R1 = __builtin_amdgcn_make_buffer_rsrc((void*)(Tq + (size_t)tb1 * a.N * 256), (short)0, nrec, 0x00020000);
      for (int p0 = 0; p0 < cm; p0 += 8) {
        float4 x0[8], x1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int p = p0 + u;
          const int i0 = l0[min(p, 127)], i1 = l1[min(p, 127)];
          const int o0 = p < c0 ? (i0 * 256 + 4 * lane) * 4 : 0x40000000;
          const int o1 = p < c1 ? (i1 * 256 + 4 * lane) * 4 : 0x40000000;
          auto v0 = __builtin_amdgcn_raw_buffer_load_b128(R0, o0, 0, 0);
          auto v1 = __builtin_amdgcn_raw_buffer_load_b128(R1, o1, 0, 0);
          x0[u] = *reinterpret_cast<float4*>(&v0);
          x1[u] = *reinterpret_cast<float4*>(&v1);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const bool on0 = p0 + u < c0, on1 = p0 + u < c1;
          acc[0].x += on0 ? x0[u].x : 0.f;
          acc[0].y += on0 ? x0[u].y : 0.f;
          acc[0].z += on0 ? x0[u].z : 0.f;
          acc[0].w += on0 ? x0[u].w : 0.f;
          acc[1].x += on1 ? x1[u].x : 0.f;
          acc[1].y += on1 ? x1[u].y : 0.f;
          acc[1].z += on1 ? x1[u].z : 0.f;
          acc[1].w += on1 ? x1[u].w : 0.f;
        }
      }
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = r0 + rr;
      const float* ap = &acc[rr].x;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int o = 16 * (4 * (lane & 3) + c) + (lane >> 2);
        const float y = leaky(ap[c] + bias[o], a.slope);
        Y1[((o >> 4) * 16 + r) * 16 + (o & 15)] = y;
        if (set == 0) a.y1[(size_t)o * B + b0 + r] = y;
      }
    }
  }
  PBN_LSTAMP(0, 2);
  lds_barrier();
  PBN_LSTAMP(0, 3);
  if (set == 0) keep = a.h2;
  {   // 256 -> 128: one output tile per wave
    const f32x4 acc = fwd_tile<kD0>(w2, Y1, lane);
    fwd_store(acc, sbias + fwd_bias_at(LY2, a.H), 16 * wave, a.slope, X2, keep, B, b0, lane);
  }
  PBN_LSTAMP(0, 4);
  lds_barrier();
  PBN_LSTAMP(0, 5);
  if (wave < kD2 / 16) {   // 128 -> 64
    const f32x4 acc = fwd_tile<kD1>(w3, X2, lane);
    fwd_store(acc, sbias + fwd_bias_at(LY3, a.H), 16 * wave, a.slope, X3, set == 0 ? a.h3 : nullptr, B, b0, lane);
  }
  lds_barrier();
  PBN_LSTAMP(0, 6);
  if (wave < kD3 / 16) {   // 64 -> 32
    const f32x4 acc = fwd_tile<kD2>(w4, X3, lane);
    fwd_store(acc, sbias + fwd_bias_at(LY4, a.H), 16 * wave, a.slope, X4, set == 0 ? a.h4 : nullptr, B, b0, lane);
  }
  lds_barrier();
  PBN_LSTAMP(0, 7);
  {   // the H first head layers: 32 -> 64 H
    const int n1 = a.H * kDH / 16;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tt = wave + kWaves * u;
      if (tt < n1) {
        const f32x4 acc = fwd_tile<kD3>(wh1[u], X4, lane);
        fwd_store(acc, sbias + fwd_bias_at(LYH1, a.H), 16 * tt, a.slope, XH, set == 0 ? a.hh : nullptr, B, b0, lane);
      }
    }
    for (int tt = wave + 2 * kWaves; tt < n1; tt += kWaves) {
      float4 wl[kD3 / 16];
      wfrag<kD3>(wl, Tq + a.ifw[LYH1], tt, n1, lane);
      const f32x4 acc = fwd_tile<kD3>(wl, X4, lane);
      fwd_store(acc, sbias + fwd_bias_at(LYH1, a.H), 16 * tt, a.slope, XH, set == 0 ? a.hh : nullptr, B, b0, lane);
    }
  }
  lds_barrier();
  PBN_LSTAMP(0, 8);
  // second head layers: head h, outputs 16 at .. (A of them, no activation) -> heads[set][h][b][a]
  auto head_out = [&](const float4 (&wl)[kDH / 16], int tt) {
    const int h = tt / at16, o0 = 16 * (tt - h * at16);
    const f32x4 acc = fwd_tile<kDH>(wl, XH + h * kDH * kRows, lane);
    const int g = lane >> 4, rr = lane & 15;
    const float* b2 = sbias + fwd_bias_at(LYH2, a.H) + h * a.A;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int o = o0 + 4 * g + v;
      if (o < a.A) a.heads[(((size_t)set * a.H + h) * B + b0 + rr) * a.Apad + o] = acc[v] + b2[o];
    }
  };
  if (wave < a.H * at16) head_out(wh2, wave);
  for (int tt = wave + kWaves; tt < a.H * at16; tt += kWaves) {
    float4 wl[kDH / 16];
    wfrag<kDH>(wl, Tq + a.ifw[LYH2], tt, a.H * at16, lane);
    head_out(wl, tt);
  }
  PBN_LSTAMP(0, 9);
}

}  // namespace
