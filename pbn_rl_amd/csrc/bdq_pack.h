// bdq_pack.h -- pbn_bdq_pack's two kernels (pbn_learn.hip): a network's image (bdq_layout.h
// make_image) from its flat parameters.
#pragma once
#include "learn_args.h"

namespace {

// the target table of the bilinear layer, [t][i][j][q] = T[t][i][16 q + j] (the layout the
// acting kernel reads); block (t, i), thread o
__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ P, int64_t w_off, int N, int W,
                                                   const uint32_t* __restrict__ att_first, float* __restrict__ Tq) {
  const int t = blockIdx.x / N, i = blockIdx.x - t * N, o = threadIdx.x;
  const uint32_t* ts = att_first + (size_t)t * W;
  const float* wrow = P + w_off + (int64_t)o * N * N + (int64_t)i * N;
  float s = 0.f;
  for (int j = 0; j < N; ++j) {
    const bool on = (ts[j >> 5] >> (j & 31)) & 1u;
    s += on ? wrow[j] : 0.f;
  }
  Tq[((size_t)t * N + i) * 256 + (o & 15) * 16 + (o >> 4)] = s;
}

// the weight tiles of one network's image from its flat parameters (make_image's layout): thread =
// one lane's float4 of one tile of one order
__global__ void __launch_bounds__(256) pack_tiles_kernel(const float* __restrict__ P, LearnArgs a, int64_t n4) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  // (layer, order, tile, lane) from the flat float4 index over the tiles region
  int64_t r = e;
  int l = 0, bwd = 0;
  int64_t per = 0;
  for (l = 0; l < NLAY; ++l) {
    const int R = layer_rows(l, a.H, a.Apad), C = layer_cols(l);
    per = (int64_t)R * C / 4;   // float4s of one order of this layer
    if (r < 2 * per) break;
    r -= 2 * per;
  }
  bwd = r >= per;
  if (bwd) r -= per;
  const int C = PBN_LAYER_COLS(l);   // (a macro, not layer_cols(l): the call changes the kernel's listing, tools/listing_diff.py)
  const int64_t tile = r >> 6;
  const int lane = (int)(r & 63), g = lane >> 4, rr = lane & 15;
  const int ot = (int)(tile / (C / 16)), kt = (int)(tile - (int64_t)ot * (C / 16));
  float x[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int row = bwd ? 16 * ot + 4 * g + v : 16 * ot + rr;
    const int col = bwd ? 16 * kt + rr : 16 * kt + 4 * g + v;
    float val;
    if (l == LYH2) {
      const int h = row / a.Apad, o = row - h * a.Apad;
      constexpr Layer y = layer(LYH2);
      val = o < a.A ? P[a.off[y.w] + ((int64_t)h * a.A + o) * y.cols + col] : 0.f;
    } else {
      val = P[PBN_LAYER_W_OFF(a.off, l) + (int64_t)row * C + col];   // (a macro: as the columns above)
    }
    x[v] = val;
  }
  reinterpret_cast<float4*>(a.Tq + (bwd ? a.ibw[l] : a.ifw[l]))[tile * 64 + lane] = make_float4(x[0], x[1], x[2], x[3]);
}

}  // namespace
