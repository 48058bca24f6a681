// dqn_forward.h -- the forward of ddqn_per/network.py's DQN (one hidden Linear) for 16 rows on one
// wave, shared by the kernels of pbn_ddqn.hip (acting, the update's three forwards) and the policy
// rollout of step_wave.h (pbn_step_wave with a PolicyArgs): one function, so the policy
// rollout's actions are dqn_act's bit for bit.  Also the shapes and layouts (Dims) of the flat parameter buffer and of
// the network image that forward16 reads (pbn_dqn_pack writes it).
#pragma once
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "dqn_scalar.h"
#include "host_check.h"
#include "wave_util.h"

namespace {

constexpr int kMaxHT = 4;       // hidden widths <= 64: at most four 16-wide tiles
constexpr int kMaxA = 128;      // N + 1 <= 128

enum Seg { BIL_W, BIL_B, L1_W, L1_B, OUT_W, OUT_B, TOTAL };

using pbn::al16;
using pbn::explore_threshold;

// Shapes, the parameter layout (pbn_dqn_layout) and the image layout.  Image (floats):
//   T     [n_attr][N][H0p]   the bilinear layer contracted with each attractor's first state,
//                            zero past h0 (a row without a target reads none of it)
//   b0 [H0p], b1 [H1p], b2 [Ap]   the biases, zero-padded
//   w1f   [H1p/16][H0p/16][64][4]  linears.0: lane 16g + r holds W[16 ot + r][16 kt + 4g + v]
//   w1b   [H1p/16][H0p/16][64][4]  its transpose's operand: W[16 ot + 4g + v][16 kt + r]
//   w2f   [Ap/16][H1p/16][64][4]   output, as w1f
struct Dims {
  int N, W, n_attr, h0, h1, A, H0p, H1p, Ap, H0T, H1T, AT;
  int64_t off[TOTAL + 1], sz[TOTAL];
  int64_t iT, ib0, ib1, ib2, iw1f, iw1b, iw2f, itotal;
};

inline const char* shape_error(int N, int h0, int h1) {
  if (N < 1 || N + 1 > kMaxA) return "n_nodes must be 1..127 (N + 1 <= 128 actions)";
  if (h0 < 1 || h0 > 64 || h1 < 1 || h1 > 64) return "hidden widths must be 1..64";
  return nullptr;
}

inline void make_dims(int N, int W, int n_attr, int h0, int h1, Dims* d) {
  d->N = N;
  d->W = W;
  d->n_attr = n_attr;
  d->h0 = h0;
  d->h1 = h1;
  d->A = N + 1;
  d->H0T = (h0 + 15) / 16;
  d->H1T = (h1 + 15) / 16;
  d->AT = (N + 1 + 15) / 16;
  d->H0p = 16 * d->H0T;
  d->H1p = 16 * d->H1T;
  d->Ap = 16 * d->AT;
  const int64_t sz[TOTAL] = {(int64_t)h0 * N * N, h0, (int64_t)h1 * h0, h1, (int64_t)d->A * h1, d->A};
  int64_t o = 0;
  for (int s = 0; s < TOTAL; ++s) {
    d->sz[s] = sz[s];
    d->off[s] = o;
    o += al16(sz[s]);
  }
  d->off[TOTAL] = o;
  int64_t i = 0;
  d->iT = i;
  i += (int64_t)n_attr * N * d->H0p;
  d->ib0 = i;
  i += d->H0p;
  d->ib1 = i;
  i += d->H1p;
  d->ib2 = i;
  i += d->Ap;
  d->iw1f = i;
  i += (int64_t)d->H1p * d->H0p;
  d->iw1b = i;
  i += (int64_t)d->H1p * d->H0p;
  d->iw2f = i;
  i += (int64_t)d->Ap * d->H1p;
  d->itotal = i;
}

// ---- the forward of 16 rows on one wave --------------------------------------------------------
// Lane 16g + r works on row r.  sw: the row's state words (bits past N cleared), t: its target id.
// y0[kb] / y1[kb] hold features 16 kb + 4g + v of row r after the ReLU (F.relu: a NaN stays; exactly
// zero in the padding, whatever the real features hold);
// qf(at, q) receives Q[16 at + 4g + v][r] tile by tile, at ascending.
// PRELOAD changes when the dense layers' operands are requested, and nothing of the arithmetic:
// linears.0's tiles and bias before the table rows, the output layer's tile row at + 1 before the
// MFMAs of row at (a tile past the shape is the clamped index's, loaded and not used).  For a wave
// that has its SIMD to itself (the policy rollout: nothing else hides a round trip to L2), where
// the default requests each tile next to its MFMAs and leaves the hiding to the other waves.
template <bool PRELOAD = false, class QF>
__device__ __forceinline__ void forward16(const Dims& d, const float* __restrict__ img, const uint32_t (&sw)[4], int t,
                                          int lane, float4 (&y0)[kMaxHT], float4 (&y1)[kMaxHT], QF&& qf) {
  const int g = lane >> 4;
  float4 wl[kMaxHT][kMaxHT], bl[kMaxHT];
  if constexpr (PRELOAD) {
    const float4* w1p = reinterpret_cast<const float4*>(img + d.iw1f) + lane;
#pragma unroll
    for (int ot = 0; ot < kMaxHT; ++ot) {
      const int oc = ot < d.H1T ? ot : 0;
#pragma unroll
      for (int kb = 0; kb < kMaxHT; ++kb) wl[ot][kb] = w1p[(oc * d.H0T + (kb < d.H0T ? kb : 0)) * 64];
      bl[ot] = *reinterpret_cast<const float4*>(img + d.ib1 + 16 * oc + 4 * g);
    }
  }
  // bilinear layer: bias + the table rows of the set bits, i ascending
#pragma unroll
  for (int kb = 0; kb < kMaxHT; ++kb)
    y0[kb] = kb < d.H0T ? *reinterpret_cast<const float4*>(img + d.ib0 + 16 * kb + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < d.n_attr) {
    const float* T = img + d.iT + (int64_t)t * d.N * d.H0p + 4 * g;
    // four set bits a round: their table rows are requested together (one round trip, not four)
    // and added in order; a slot past the last bit reads row 0 and adds zeros
    for (int w = 0; w < d.W; ++w) {
      uint32_t x = sw[w];
      while (x) {
        float4 tv[4][kMaxHT];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          on[u] = x != 0u;
          const int i = on[u] ? 32 * w + __builtin_ctz(x) : 0;
          x &= x - 1u;
          const float* row = T + (int64_t)i * d.H0p;
#pragma unroll
          for (int kb = 0; kb < kMaxHT; ++kb)
            if (kb < d.H0T) tv[u][kb] = *reinterpret_cast<const float4*>(row + 16 * kb);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int kb = 0; kb < kMaxHT; ++kb)
            if (kb < d.H0T) {
              y0[kb].x += on[u] ? tv[u][kb].x : 0.f;
              y0[kb].y += on[u] ? tv[u][kb].y : 0.f;
              y0[kb].z += on[u] ? tv[u][kb].z : 0.f;
              y0[kb].w += on[u] ? tv[u][kb].w : 0.f;
            }
        }
      }
    }
  }
#pragma unroll
  for (int kb = 0; kb < kMaxHT; ++kb) {
    y0[kb].x = pbn::relu(y0[kb].x);   // (a padded feature is 0 + zeros: it stays exactly 0)
    y0[kb].y = pbn::relu(y0[kb].y);
    y0[kb].z = pbn::relu(y0[kb].z);
    y0[kb].w = pbn::relu(y0[kb].w);
  }
  // linears.0
  const float4* w1 = reinterpret_cast<const float4*>(img + d.iw1f) + lane;
  const float4* w2 = reinterpret_cast<const float4*>(img + d.iw2f) + lane;
  // PRELOAD: tile row `at` of the output layer and its bias (here row 0, ahead of linears.0's MFMAs)
  float4 wo[kMaxHT], bo;
  auto load_out = [&](int at) {
#pragma unroll
    for (int kb = 0; kb < kMaxHT; ++kb) wo[kb] = w2[(at * d.H1T + (kb < d.H1T ? kb : 0)) * 64];
    bo = *reinterpret_cast<const float4*>(img + d.ib2 + 16 * at + 4 * g);
  };
  if constexpr (PRELOAD) load_out(0);
#pragma unroll
  for (int ot = 0; ot < kMaxHT; ++ot) {
    y1[ot] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ot < d.H1T) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < kMaxHT; ++kb)
        if (kb < d.H0T) {
          float4 w;
          if constexpr (PRELOAD) w = wl[ot][kb];
          else w = w1[(ot * d.H0T + kb) * 64];
          acc = mfma(w.x, y0[kb].x, acc);
          acc = mfma(w.y, y0[kb].y, acc);
          acc = mfma(w.z, y0[kb].z, acc);
          acc = mfma(w.w, y0[kb].w, acc);
        }
      float4 b;
      if constexpr (PRELOAD) b = bl[ot];
      else b = *reinterpret_cast<const float4*>(img + d.ib1 + 16 * ot + 4 * g);
      y1[ot] = make_float4(pbn::relu(acc[0] + b.x), pbn::relu(acc[1] + b.y), pbn::relu(acc[2] + b.z),
                           pbn::relu(acc[3] + b.w));
      // a padded row's sum is 0 * y0 + 0, which is NaN where a feature is infinite or NaN: the ReLU
      // keeps a NaN, so the padding (the last tile's features 16 ot + 4g + v >= h1) is set to 0 by
      // its index.  (wave-uniform branch: only a ragged last tile pays for it)
      if (ot == d.H1T - 1 && (d.h1 & 15)) {
        const int real = d.h1 - 16 * ot - 4 * g;   // this lane's real features of the tile
        if (real < 1) y1[ot].x = 0.f;
        if (real < 2) y1[ot].y = 0.f;
        if (real < 3) y1[ot].z = 0.f;
        if (real < 4) y1[ot].w = 0.f;
      }
    }
  }
  // output
  for (int at = 0; at < d.AT; ++at) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float4 wc[kMaxHT], b;
    if constexpr (PRELOAD) {   // this row's operands, and the next row's requested under its MFMAs
#pragma unroll
      for (int kb = 0; kb < kMaxHT; ++kb) wc[kb] = wo[kb];
      b = bo;
      load_out(at + 1 < d.AT ? at + 1 : at);
    }
#pragma unroll
    for (int kb = 0; kb < kMaxHT; ++kb)
      if (kb < d.H1T) {
        float4 w;
        if constexpr (PRELOAD) w = wc[kb];
        else w = w2[(at * d.H1T + kb) * 64];
        acc = mfma(w.x, y1[kb].x, acc);
        acc = mfma(w.y, y1[kb].y, acc);
        acc = mfma(w.z, y1[kb].z, acc);
        acc = mfma(w.w, y1[kb].w, acc);
      }
    if constexpr (!PRELOAD) b = *reinterpret_cast<const float4*>(img + d.ib2 + 16 * at + 4 * g);
    const f32x4 q = {acc[0] + b.x, acc[1] + b.y, acc[2] + b.z, acc[3] + b.w};
    qf(at, q);
  }
}

// torch.argmax's order: NaN is the maximum, of equals the lower index wins
__device__ __forceinline__ bool better(float a, int ia, float b, int ib) {
  if (isnan(a)) return isnan(b) ? ia < ib : true;
  if (isnan(b)) return false;
  return a > b || (a == b && ia < ib);
}

// the first maximum of a row whose lanes (g = 0..3) each hold a running (best, index)
__device__ __forceinline__ int row_argmax(float best, int bi) {
#pragma unroll
  for (int m = 16; m <= 32; m <<= 1) {
    const float ob = __shfl_xor(best, m);
    const int oi = __shfl_xor(bi, m);
    if (better(ob, oi, best, bi)) {
      best = ob;
      bi = oi;
    }
  }
  return bi;
}

// the flip-mask word w of action act (0: the no-op; a > 0 flips node a - 1)
__device__ __forceinline__ uint32_t action_mask_word(int act, int N, int w) {
  return (act > 0 && act <= N && ((act - 1) >> 5) == w) ? 1u << ((act - 1) & 31) : 0u;
}

}  // namespace
