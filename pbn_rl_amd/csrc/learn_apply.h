// learn_apply.h -- the third of the fused BDQ update's three launches (pbn_learn.hip):
//
//   learn_apply  one wave per 16 x 16 gradient tile (K = the batch: dW = delta . act^T), the
//                bilinear layer's weight gradient from the packed state and target bits
//                (dW[o][i][j] = sum_r g[o][r] s_i[r] t_j[r]); each wave clamps its tile to
//                [-c, c] (:129-130), takes the Adam step on it, and, for the bilinear layer,
//                recomputes the target-table rows of the weights it just wrote.  Block 0 adds
//                the MSE's partial sums in block order (the loss is reproducible).
//
// The tasks and their order are bdq_layout.h's (apply_tiles, apply_tasks).
#pragma once
#include "learn_args.h"
#include "replay_draw.h"

namespace {

// ---- Adam (torch.optim.Adam, fused, defaults but lr: bdq_model/__init__.py:34) on one element,
// after clamping its gradient to [-c, c] (torch.clamp: NaN stays NaN)
// The element's parameter and moments are loaded ahead (adam_load_ahead, at the task's start: the
// round trip overlaps the gradient loop), adam_apply writes the step and returns the new value.
struct AdamIn {
  float p, m, v;
};

__device__ __forceinline__ float adam_apply(const LearnArgs& a, int64_t i, AdamIn in, float g, float bc1, float bc2s) {
  g = isnan(g) ? g : fminf(fmaxf(g, -a.clampv), a.clampv);
  if (a.grad) a.grad[i] = g;
  const float m = a.b1 * in.m + (1.f - a.b1) * g;
  const float v = a.b2 * in.v + (1.f - a.b2) * g * g;
  a.m[i] = m;
  a.v[i] = v;
  const float denom = sqrtf(v) / bc2s + a.eps;
  const float p = in.p - (a.lr / bc1) * m / denom;
  a.P[i] = p;
  return p;
}

__device__ __forceinline__ uint4 target_words(const LearnArgs& a, int t) {
  uint32_t tw[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) tw[w] = (t < a.n_attr && w < a.W) ? a.att_first[(size_t)t * a.W + w] : 0u;
  return make_uint4(tw[0], tw[1], tw[2], tw[3]);
}

// Loads issued ahead of their use in straight-line code, without a branch or a select at the
// load: a guarded load puts its select right behind the load, and that select's s_waitcnt waits
// out every load issued before it (vmcnt retires in order: learn_apply's ISA had a vmcnt(0)
// behind each of its 16 target-word loads, and its gradient operands queued behind the Adam
// state).  Clamped to a valid element; the callers use only the valid lanes' values.
__device__ __forceinline__ uint4 target_words_ahead(const LearnArgs& a, int t) {
  const uint32_t* af = a.n_attr > 0 ? a.att_first : reinterpret_cast<const uint32_t*>(a.P);   // (no attractors: unused)
  const uint32_t* row = af + (size_t)(t < a.n_attr ? t : (a.n_attr > 0 ? a.n_attr - 1 : 0)) * a.W;
  return make_uint4(row[0], row[a.W > 1 ? 1 : 0], row[a.W > 2 ? 2 : 0], row[a.W > 3 ? 3 : 0]);
}
__device__ __forceinline__ AdamIn adam_load_ahead(const LearnArgs& a, int64_t i) {
  return AdamIn{a.P[i], a.m[i], a.v[i]};
}

struct Dense {
  const float* dY;
  const float* X;
  int64_t w_off, b_off;
  int ldw, o_valid, k_tiles;
  int lay, ot0;   // the layer's tiles in the image; its first output tile there (head h: h Apad/16)
};

template <int NT>
__global__ void __launch_bounds__(64 * kApplyWaves) learn_apply_kernel(LearnArgs a) {
  __shared__ float wsc[kApplyWaves][16][kMaxNT * 16 + 1];   // a bilinear tile's new weights, per wave
  // The extra last block advances the frame's counters and draws the next frame's rows.  This
  // launch reads neither; the earlier launches of the call did.
  if (a.adv_on && blockIdx.x == gridDim.x - 1) {
    const pbn_frame_advance& f = a.adv;
    pbn::frame_advance_block(f.n_store, f.capacity, f.d_pos, f.d_size, f.d_step, f.d_eps64, f.d_eps32,
                             f.eps_final, f.eps_step, f.n_idx, f.seed, f.d_counter, f.d_idx, f.n_store);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, rr = lane & 15;
  const int B = a.B;
  PBN_LSTAMP(2, 31);
  PBN_LSTAMP(2, 0);
  if (blockIdx.x == 0 && wave == 0) {   // the loss: the backward blocks' partial sums, a fixed-order reduction
    float s = 0.f;
    for (int p = lane; p < B / kRows; p += 64) s += a.partial[p];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) a.loss[0] = s / (float)(a.wts ? B : B * a.K);   // (weighted: mean_b w_b l_b, l_b the mean over k)
  }
  const float stepc = a.step[0];
  const float bc1 = 1.f - powf(a.b1, stepc);
  const float bc2s = sqrtf(1.f - powf(a.b2, stepc));
  int task = blockIdx.x * kApplyWaves + wave;
  const int n_bil = apply_bil_tasks(a.N);
  if (task < n_bil) {
    // bilinear weight tile: outputs o0..o0+15 of input i, all j: D[o][j] = sum_r g1[o][r] s_i[r] t_j[r]
    const int ot = task / a.N, i = task - ot * a.N, o0 = 16 * ot;
    const int64_t NN = (int64_t)a.N * a.N;
    const uint32_t* si = a.srow + (size_t)(i >> 5) * B;
    const float* grow = a.g1 + (size_t)(o0 + rr) * B;
    f32x4 acc[NT];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    constexpr int RC = NT <= 2 ? 8 : 4;   // 16-row steps per round of loads
    const uint32_t sh = i & 31;
    float4 y[RC];
    uint4 sv[RC], tv[RC][NT];
    auto round_loads = [&](int r0) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < RC; ++u) {
        const int rb = min(r0 + 16 * u, B - 16) + 4 * g;
        y[u] = *reinterpret_cast<const float4*>(grow + rb);
        sv[u] = *reinterpret_cast<const uint4*>(si + rb);
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
          tv[u][jt] = *reinterpret_cast<const uint4*>(a.trow + (size_t)((16 * jt + rr) >> 5) * B + rb);
      }
    };
    // the first round's gradient operands, then the tile's Adam state and the first four target
    // rows' words of this lane (t = g + 4u) behind them (used after the loop), then the rounds
    round_loads(0);
    __builtin_amdgcn_sched_barrier(0);
    AdamIn pre[NT][4];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int jj = min(16 * jt + rr, a.N - 1);   // (lanes past N: never applied)
        pre[jt][v] = adam_load_ahead(a, a.off[BIL_W] + (o0 + 4 * g + v) * NN + (int64_t)i * a.N + jj);
      }
    const AdamIn preb = adam_load_ahead(a, a.off[BIL_B] + o0 + rr);   // (applied by i == 0, g == 0)
    const uint4 tw0 = target_words_ahead(a, rr);   // target rr's words: the first table tile (t < n_attr)
    __builtin_amdgcn_sched_barrier(0);
    for (int r0 = 0; r0 < B; r0 += 16 * RC) {
      if (r0 > 0) round_loads(r0);
#pragma unroll
      for (int u = 0; u < RC; ++u) {
        if (r0 + 16 * u < B) {
          float4 yy = y[u];
          bsum += (yy.x + yy.y) + (yy.z + yy.w);
          yy.x = (sv[u].x >> sh) & 1u ? yy.x : 0.f;
          yy.y = (sv[u].y >> sh) & 1u ? yy.y : 0.f;
          yy.z = (sv[u].z >> sh) & 1u ? yy.z : 0.f;
          yy.w = (sv[u].w >> sh) & 1u ? yy.w : 0.f;
#pragma unroll
          for (int jt = 0; jt < NT; ++jt) {
            const uint32_t tsh = (16 * jt + rr) & 31;
            acc[jt] = mfma(yy.x, (float)((tv[u][jt].x >> tsh) & 1u), acc[jt]);
            acc[jt] = mfma(yy.y, (float)((tv[u][jt].y >> tsh) & 1u), acc[jt]);
            acc[jt] = mfma(yy.z, (float)((tv[u][jt].z >> tsh) & 1u), acc[jt]);
            acc[jt] = mfma(yy.w, (float)((tv[u][jt].w >> tsh) & 1u), acc[jt]);
          }
        }
      }
    }
    PBN_LSTAMP(2, 1);
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) {
      const int jj = 16 * jt + rr;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int o = o0 + 4 * g + v;
        float nw = 0.f;
        if (jj < a.N) nw = adam_apply(a, a.off[BIL_W] + o * NN + (int64_t)i * a.N + jj, pre[jt][v], acc[jt][v], bc1, bc2s);
        wsc[wave][4 * g + v][jj] = nw;
      }
    }
    if (i == 0) {   // the bilinear bias: sum over the batch of g1 (lane groups added in a fixed order)
      bsum += __shfl_xor(bsum, 16);
      bsum += __shfl_xor(bsum, 32);
      if (g == 0) adam_apply(a, a.off[BIL_B] + o0 + rr, preb, bsum, bc1, bc2s);
    }
    PBN_LSTAMP(2, 2);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the target-table rows of input i for these 16 outputs, from the weights just written, 16
    // targets per MFMA tile: D[o][t] = sum_j W[o][i][j] x_t[j], j ascending through the k-steps
    // (the f32 MFMA is an fmaf chain, and x_t[j] is 0 or 1: pack_kernel's sequential sums bit for
    // bit).  A operand lane (g, r): W[o = r][j = s + g] from this wave's LDS rows; B: x_{t0 + r}[s + g]
    for (int t0 = 0; t0 < a.n_attr; t0 += 16) {
      const int t = t0 + rr;
      const uint4 tw = t0 == 0 ? tw0 : target_words(a, t);
      f32x4 d = {0.f, 0.f, 0.f, 0.f};
      for (int s4 = 0; s4 < a.N; s4 += 4) {
        const int j = s4 + g;
        const uint32_t word = (j >> 5) == 0 ? tw.x : (j >> 5) == 1 ? tw.y : (j >> 5) == 2 ? tw.z : tw.w;
        const bool in = j < a.N;
        d = mfma(in ? wsc[wave][rr][j] : 0.f, (in && t < a.n_attr && ((word >> (j & 31)) & 1u)) ? 1.f : 0.f, d);
      }
      if (t < a.n_attr) {
#pragma unroll
        for (int v = 0; v < 4; ++v) a.Tq[((size_t)t * a.N + i) * 256 + (4 * g + v) * 16 + ot] = d[v];
      }
    }
    PBN_LSTAMP(2, 3);
    return;
  }
  task -= n_bil;
  // dense layers: (layer, output tile, input tile) -> dW[o][k] = sum_r dY[o][r] X[k][r]
  const int H = a.H, at16 = a.Apad / 16;
  Dense L;
  int ot, kt;
  constexpr int n0 = apply_tiles(LY2), n1 = apply_tiles(LY3), n2 = apply_tiles(LY4);   // (the trunk: constants)
  const int n3 = apply_tiles(LYH1, H, at16), n4 = apply_tiles(LYH2, H, at16);
  if (task < n0) {
    constexpr Layer y = layer(LY2);
    L = Dense{a.dh2, a.y1, a.off[y.w], a.off[y.b], y.cols, y.rows, y.cols / 16, LY2, 0};
  } else if ((task -= n0) < n1) {
    constexpr Layer y = layer(LY3);
    L = Dense{a.dh3, a.h2, a.off[y.w], a.off[y.b], y.cols, y.rows, y.cols / 16, LY3, 0};
  } else if ((task -= n1) < n2) {
    constexpr Layer y = layer(LY4);
    L = Dense{a.dh4, a.h3, a.off[y.w], a.off[y.b], y.cols, y.rows, y.cols / 16, LY4, 0};
  } else if ((task -= n2) < n3) {
    const Layer y = layer(LYH1, H);
    L = Dense{a.dhh, a.h4, a.off[y.w], a.off[y.b], y.cols, y.rows, y.cols / 16, LYH1, 0};
  } else if ((task -= n3) < n4) {
    const int per = apply_tiles(LYH2, 1, at16);
    const int h = task / per;
    task -= h * per;
    // head h's second layer: rows are its A outputs (the value head has one real output)
    constexpr Layer y = layer(LYH2);   // (its segments and columns; the rows by hand, per head)
    L = Dense{a.dheads + (size_t)h * a.Apad * B, a.hh + (size_t)h * kDH * B, a.off[y.w] + (int64_t)h * a.A * y.cols,
              a.off[y.b] + (int64_t)h * a.A, y.cols, h == 0 ? 1 : a.A, y.cols / 16, LYH2, h * at16};
  } else {
    return;
  }
  ot = task / L.k_tiles;
  kt = task - ot * L.k_tiles;
  const int o0 = 16 * ot, k0 = 16 * kt;
  const float* yrow = L.dY + (size_t)(o0 + rr) * B;
  const float* xrow = L.X + (size_t)(k0 + rr) * B;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  float4 y[8], x[8];
  auto round_loads = [&](int r0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int rb = min(r0 + 16 * u, B - 16) + 4 * g;
      y[u] = *reinterpret_cast<const float4*>(yrow + rb);
      x[u] = *reinterpret_cast<const float4*>(xrow + rb);
    }
  };
  round_loads(0);   // then the Adam state behind the first round's operands (the bilinear tiles' order)
  __builtin_amdgcn_sched_barrier(0);
  AdamIn pre[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int o = o0 + 4 * g + v;
    pre[v] = adam_load_ahead(a, L.w_off + (int64_t)(o < L.o_valid ? o : 0) * L.ldw + k0 + rr);   // (o < o_valid only)
  }
  const AdamIn preb = adam_load_ahead(a, L.b_off + (o0 + rr < L.o_valid ? o0 + rr : 0));   // (kt, g == 0, valid rows)
  __builtin_amdgcn_sched_barrier(0);
  for (int r0 = 0; r0 < B; r0 += 128) {   // eight 16-row steps per round of loads
    if (r0 > 0) round_loads(r0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (r0 + 16 * u < B) {
        bsum += (y[u].x + y[u].y) + (y[u].z + y[u].w);
        acc = mfma(y[u].x, x[u].x, acc);
        acc = mfma(y[u].y, x[u].y, acc);
        acc = mfma(y[u].z, x[u].z, acc);
        acc = mfma(y[u].w, x[u].w, acc);
      }
    }
  }
  PBN_LSTAMP(2, 4);
  float nw[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int o = o0 + 4 * g + v;
    nw[v] = o < L.o_valid ? adam_apply(a, L.w_off + (int64_t)o * L.ldw + k0 + rr, pre[v], acc[v], bc1, bc2s) : 0.f;
  }
  {   // the tile's new weights into the online image (the learn_fwd / learn_bwd operands of the
      // next update and pbn_bdq_pack's values; rows past o_valid: the flat buffer's zero padding)
    const size_t tix = ((size_t)(L.ot0 + ot) * L.k_tiles + kt) * 64 + lane;
    reinterpret_cast<float4*>(a.Tq + a.ibw[L.lay])[tix] = make_float4(nw[0], nw[1], nw[2], nw[3]);
    float* sc = &wsc[wave][0][0];   // the fwd order is the tile transposed: through this wave's LDS
#pragma unroll
    for (int v = 0; v < 4; ++v) sc[(4 * g + v) * 17 + rr] = nw[v];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    reinterpret_cast<float4*>(a.Tq + a.ifw[L.lay])[tix] =
        make_float4(sc[rr * 17 + 4 * g], sc[rr * 17 + 4 * g + 1], sc[rr * 17 + 4 * g + 2], sc[rr * 17 + 4 * g + 3]);
  }
  if (kt == 0) {
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    if (g == 0 && o0 + rr < L.o_valid) adam_apply(a, L.b_off + o0 + rr, preb, bsum, bc1, bc2s);
  }
  PBN_LSTAMP(2, 5);
}

}  // namespace
