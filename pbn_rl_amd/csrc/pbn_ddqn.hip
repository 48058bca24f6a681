// pbn_ddqn.hip -- the reference's other agent, DDQN / DDQNPER (ddqn_per/__init__.py, driven by
// train_ddqn.py), on the device: batched acting for a whole VectorPBNEnv in one launch and
// _learn_step (:275-278, :468-483) as four launches over one flat parameter buffer.
//
// The network is ddqn_per/network.py's DQN with one hidden Linear: an nn.Bilinear(N, N, h0) input
// layer on (state, target), ReLU, Linear(h0, h1), ReLU, Linear(h1, N + 1).  As in pbn_learn.hip the
// bilinear layer is never evaluated as such: the target half of the input is one of the net's
// attractors' first states, so the layer contracted with each of them is a table
// T[t][i][o] = sum_j x_t[j] W[o][i][j], and a row's first layer is bias + the table rows of its
// state's set bits.  The two dense layers run on v_mfma_f32_16x16x4_f32 with 16 rows (envs or
// transitions) as the MFMA's columns: a lane's accumulator of output tile ot, D[16 ot + 4g + v][r],
// is exactly the B operand of the next layer's k-block ot, so the activations never leave the
// registers.
//
//   dqn_pack     the network image of a flat parameter buffer (below).
//   dqn_act      one wave per 16 envs: packed state + target id -> Q -> epsilon-greedy under the
//                EXPLORE law (pbn_q_to_flipmask's, one branch) -> action and flip-mask words.
//   ddqn_fb      B/16 blocks of three waves: the online network on s, the online network on s'
//                (its first argmax), the target network on s'; then wave 0 takes the TD error, the
//                Huber loss and its gradient and runs the backward, storing the activations and
//                deltas as [feature][B] planes.
//   ddqn_grad    the weight gradients in the parameter layout (the bilinear one from the packed
//                state and target bits, the dense ones as 16 x 16 MFMA tiles with K = the batch) and
//                one sum of squares per block.
//   ddqn_adam    every block adds the blocks' sums in the same fixed order (the total norm of
//                clip_grad_norm_), scales the gradient and takes the Adam step.
//   dqn_pack     again, on the new weights: the online image.
//   ddqn_schedule  a captured frame's _schedule_step: beta's increment and, on the frames where it is
//                due, the hard target copy (parameters and image), decided on the device.
//
// Every reduction runs in a fixed order and nothing is accumulated with atomics: two runs from the
// same state give the same bits.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pbn_env.h"
#include "dqn_forward.h"
#include "host_check.h"
#include "net_view.h"
#include "philox.h"

namespace {

// (Dims, make_dims, forward16 and the argmax: dqn_forward.h, shared with the policy rollout)

constexpr int kActWaves = 4;
constexpr int kGradThreads = 256;

// ---- the image -------------------------------------------------------------------------------
// Element e of the image of parameters P.  A table entry adds its weights by ascending j.
__device__ float image_value(const Dims& d, const float* __restrict__ P, const uint32_t* __restrict__ att_first,
                             int64_t e) {
  if (e < d.ib0) {
    const int o = (int)(e % d.H0p);
    const int64_t ti = e / d.H0p;
    const int i = (int)(ti % d.N), t = (int)(ti / d.N);
    if (o >= d.h0) return 0.f;
    const float* w = P + d.off[BIL_W] + ((int64_t)o * d.N + i) * d.N;
    float s = 0.f;
    for (int j = 0; j < d.N; ++j)
      if ((att_first[(size_t)t * d.W + (j >> 5)] >> (j & 31)) & 1u) s += w[j];
    return s;
  }
  if (e < d.ib1) return e - d.ib0 < d.h0 ? P[d.off[BIL_B] + e - d.ib0] : 0.f;
  if (e < d.ib2) return e - d.ib1 < d.h1 ? P[d.off[L1_B] + e - d.ib1] : 0.f;
  if (e < d.iw1f) return e - d.ib2 < d.A ? P[d.off[OUT_B] + e - d.ib2] : 0.f;
  const bool second = e >= d.iw2f, bwd = !second && e >= d.iw1b;
  const int64_t x = e - (second ? d.iw2f : (bwd ? d.iw1b : d.iw1f));
  const int KT = second ? d.H1T : d.H0T;
  const int tile = (int)(x >> 8), lane = (int)(x >> 2) & 63, v = (int)x & 3;
  const int ot = tile / KT, kt = tile - ot * KT, g = lane >> 4, r = lane & 15;
  const int row = bwd ? 16 * ot + 4 * g + v : 16 * ot + r;
  const int col = bwd ? 16 * kt + r : 16 * kt + 4 * g + v;
  const int rows = second ? d.A : d.h1, cols = second ? d.h1 : d.h0;
  if (row >= rows || col >= cols) return 0.f;
  return P[d.off[second ? OUT_W : L1_W] + (int64_t)row * cols + col];
}

__global__ void __launch_bounds__(256) dqn_pack_kernel(Dims d, const float* __restrict__ P,
                                                        const uint32_t* __restrict__ att_first, float* __restrict__ img) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < d.itotal; e += (int64_t)gridDim.x * 256)
    img[e] = image_value(d, P, att_first, e);
}

__device__ __forceinline__ void load_words(const Dims& d, const uint32_t* __restrict__ st, int64_t stride, int64_t j,
                                           uint32_t (&sw)[4]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t x = w < d.W ? st[(size_t)w * stride + j] : 0u;
    if (w == d.W - 1 && (d.N & 31)) x &= (1u << (d.N & 31)) - 1u;
    sw[w] = x;
  }
}

// ---- acting ------------------------------------------------------------------------------------
struct ActArgs {
  Dims d;
  int64_t n;
  const uint32_t* state;
  const uint8_t* target;
  const float* img;
  uint64_t seed, step, env_offset, eps_u;
  const uint64_t* d_step;
  const float* d_eps;
  float* q;
  uint32_t* flipmask;
  int32_t* actions;
};

__global__ void __launch_bounds__(64 * kActWaves) dqn_act_kernel(ActArgs a) {
  const Dims& d = a.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = (int64_t)blockIdx.x * kActWaves + wave;
  if (tile >= a.n / 16) return;   // (wave-uniform; the kernel has no block barrier)
  const int g = lane >> 4, r = lane & 15;
  const int64_t e = tile * 16 + r;
  uint32_t sw[4];
  load_words(d, a.state, a.n, e, sw);
  const int t = a.target[e];
  float4 y0[kMaxHT], y1[kMaxHT];
  float best = -INFINITY;
  int bi = INT_MAX;
  forward16(d, a.img, sw, t, lane, y0, y1, [&](int at, f32x4 q) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int ai = 16 * at + 4 * g + v;
      if (ai < d.A) {
        if (a.q) a.q[(size_t)e * d.A + ai] = q[v];
        if (better(q[v], ai, best, bi)) {
          best = q[v];
          bi = ai;
        }
      }
    }
  });
  bi = row_argmax(best, bi);
  if (g != 0) return;
  // EXPLORE law (DESIGN.md "Step semantics" 6), one branch: explore iff word 0 < floor(eps 2^32),
  // then word 1 by multiply-high onto [0, N]
  const uint64_t st = a.d_step ? *a.d_step : a.step;
  const pbn::Word4 rw = pbn::draw(a.seed, a.env_offset + (uint64_t)e, st, pbn::kStreamExplore, 0);
  uint64_t eps_u = a.eps_u;
  if (a.d_eps) {   // device epsilon: clamped to [0, 1], NaN -> 0
    const float ef = fminf(fmaxf(*a.d_eps, 0.f), 1.f);
    eps_u = explore_threshold(ef);
  }
  const int act = (uint64_t)rw.x < eps_u ? (int)__umulhi(rw.y, (uint32_t)d.A) : bi;
  if (a.actions) a.actions[e] = act;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (w < d.W) a.flipmask[(size_t)w * a.n + e] = action_mask_word(act, d.N, w);
}

// ---- the update --------------------------------------------------------------------------------
struct Work {   // float offsets into the workspace
  int64_t y0, y1, dz0, dz1, gq, lrow, act, srow, trow, partial, G, total;
  int nb_bil, nb_w1, nb_w2, nblocks;
};

Work make_work(const Dims& d, int64_t B) {
  Work w;
  int64_t o = 0;
  auto take = [&](int64_t n) {
    const int64_t at = o;
    o += al16(n);
    return at;
  };
  w.y0 = take(d.H0p * B);
  w.y1 = take(d.H1p * B);
  w.dz0 = take(d.H0p * B);
  w.dz1 = take(d.H1p * B);
  w.gq = take(B);
  w.lrow = take(B);
  w.act = take(B);
  w.srow = take(4 * B);
  w.trow = take(4 * B);
  w.nb_bil = (int)((d.sz[BIL_W] + kGradThreads - 1) / kGradThreads);
  w.nb_w1 = (d.H1T * d.H0T + 3) / 4;
  w.nb_w2 = (d.AT * d.H1T + 3) / 4;
  w.nblocks = w.nb_bil + 1 + w.nb_w1 + w.nb_w2;
  w.partial = take(w.nblocks);
  w.G = take(d.off[TOTAL]);
  w.total = o;
  return w;
}

struct LearnArgs {
  Dims d;
  Work w;
  int B;
  const int64_t* idx;
  int64_t cap;
  const uint32_t* st;
  const uint32_t* nst;
  const uint8_t* tgt;
  const int32_t* act;
  const float* rew;
  const uint8_t* done;
  const uint32_t* att_first;
  float* P;
  const float* img;
  const float* timg;
  float* m;
  float* v;
  float* step;
  float lr, b1, b2, eps, gamma, max_norm, rconst;
  float* ws;
  float* loss;
  float* grad_norm;
  float* grad;
  const float* wts;
  float* prio;
};

__global__ void __launch_bounds__(192) ddqn_fb_kernel(LearnArgs a) {
  __shared__ int s_ap[16];
  __shared__ float s_qt[kMaxA * 16];
  const Dims& d = a.d;
  const int B = a.B;
  const int lane = threadIdx.x & 63, set = threadIdx.x >> 6;   // 0: Q(s), 1: Q(s'), 2: Q_target(s')
  const int g = lane >> 4, r = lane & 15;
  const int b = blockIdx.x * 16 + r;
  int64_t j = a.idx[b];
  j = j < 0 ? 0 : (j >= a.cap ? a.cap - 1 : j);
  uint32_t sw[4];
  load_words(d, set == 0 ? a.st : a.nst, a.cap, j, sw);
  const int t = a.tgt[j];
  const int act = min(max(a.act[j], 0), d.A - 1);
  float4 y0[kMaxHT], y1[kMaxHT];
  float best = -INFINITY, qsel = 0.f;
  int bi = INT_MAX;
  forward16(d, set == 2 ? a.timg : a.img, sw, t, lane, y0, y1, [&](int at, f32x4 q) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int ai = 16 * at + 4 * g + v;
      if (ai < d.A) {
        if (set == 0 && ai == act) qsel = q[v];
        if (set == 1 && better(q[v], ai, best, bi)) {
          best = q[v];
          bi = ai;
        }
        if (set == 2) s_qt[ai * 16 + r] = q[v];
      }
    }
  });
  if (set == 1) {
    bi = row_argmax(best, bi);
    if (g == 0) s_ap[r] = min(bi, d.A - 1);
  }
  __syncthreads();
  if (set != 0) return;
  // Q(s)[a]: one lane of the row's four holds it, the others add zeros
  qsel += __shfl_xor(qsel, 16);
  qsel += __shfl_xor(qsel, 32);
  const float qt = s_qt[s_ap[r] * 16 + r];
  const float y = a.rew[j] + ((1.f - (a.done[j] ? 1.f : 0.f)) * a.gamma) * qt;
  const float delta = qsel - y;
  const float h = pbn::huber(delta);
  float gq = pbn::huber_grad(delta) * (1.f / (float)B);   // d mean_b h_b / d q_b (a NaN TD error: NaN)
  float l = h;
  if (a.wts) {
    const float wb = a.wts[b];
    gq *= wb;
    l = h * wb;
    if (g == 0) a.prio[b] = fabsf(l) + a.rconst;
  }
  float* ws = a.ws;
  if (g == 0) {
    ws[a.w.gq + b] = gq;
    ws[a.w.lrow + b] = l;
    reinterpret_cast<int*>(ws + a.w.act)[b] = act;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      reinterpret_cast<uint32_t*>(ws + a.w.srow)[w * B + b] = sw[w];
      reinterpret_cast<uint32_t*>(ws + a.w.trow)[w * B + b] =
          (t < d.n_attr && w < d.W) ? a.att_first[(size_t)t * d.W + w] : 0u;
    }
    if (blockIdx.x == 0 && r == 0) a.step[0] += 1.f;   // Adam's step count, read by ddqn_adam
  }
  // backward.  dQ is gq at (a_b, b) alone, so the output layer's transpose is one weight row.
  // The ReLU masks below are y > 0, which is false for a NaN feature, where torch's
  // threshold_backward (x <= 0 ? 0 : g) passes g.  Nothing can tell them apart: a NaN feature makes
  // the row's Q and so gq NaN, the norm NaN, and clip_coef then makes every gradient NaN.
  float4 dz1[kMaxHT], dz0[kMaxHT];
  const float* wo = a.P + d.off[OUT_W] + (int64_t)act * d.h1;
#pragma unroll
  for (int kb = 0; kb < kMaxHT; ++kb) {
    float dv[4];
    const float* yv = &y1[kb].x;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int k = 16 * kb + 4 * g + v;
      dv[v] = (kb < d.H1T && k < d.h1 && yv[v] > 0.f) ? wo[k] * gq : 0.f;
    }
    dz1[kb] = make_float4(dv[0], dv[1], dv[2], dv[3]);
  }
  const float4* w1b = reinterpret_cast<const float4*>(a.img + d.iw1b) + lane;
#pragma unroll
  for (int kt = 0; kt < kMaxHT; ++kt) {
    dz0[kt] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kt < d.H0T) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ot = 0; ot < kMaxHT; ++ot)
        if (ot < d.H1T) {
          const float4 w = w1b[(ot * d.H0T + kt) * 64];
          acc = mfma(w.x, dz1[ot].x, acc);
          acc = mfma(w.y, dz1[ot].y, acc);
          acc = mfma(w.z, dz1[ot].z, acc);
          acc = mfma(w.w, dz1[ot].w, acc);
        }
      dz0[kt] = make_float4(y0[kt].x > 0.f ? acc[0] : 0.f, y0[kt].y > 0.f ? acc[1] : 0.f,
                            y0[kt].z > 0.f ? acc[2] : 0.f, y0[kt].w > 0.f ? acc[3] : 0.f);
    }
  }
#pragma unroll
  for (int kb = 0; kb < kMaxHT; ++kb) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int k = 16 * kb + 4 * g + v;
      if (kb < d.H0T) {
        ws[a.w.y0 + (int64_t)k * B + b] = (&y0[kb].x)[v];
        ws[a.w.dz0 + (int64_t)k * B + b] = (&dz0[kb].x)[v];
      }
      if (kb < d.H1T) {
        ws[a.w.y1 + (int64_t)k * B + b] = (&y1[kb].x)[v];
        ws[a.w.dz1 + (int64_t)k * B + b] = (&dz1[kb].x)[v];
      }
    }
  }
}

// dW[16 ot + 4g + v][16 kt + (lane & 15)] = sum_b X[16 ot + ..][b] Y[16 kt + ..][b], b ascending in
// blocks of 16; xa(o, b4) gives X[16 ot + o][b4 .. b4 + 3]
template <class XA>
__device__ __forceinline__ f32x4 grad_tile(const float* __restrict__ Y, int kt, int B, int lane, XA&& xa) {
  const int g = lane >> 4, c = lane & 15;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < B; b0 += 16) {
    const float4 x = xa(c, b0 + 4 * g);
    const float4 y = *reinterpret_cast<const float4*>(Y + (int64_t)(16 * kt + c) * B + b0 + 4 * g);
    acc = mfma(x.x, y.x, acc);
    acc = mfma(x.y, y.y, acc);
    acc = mfma(x.z, y.z, acc);
    acc = mfma(x.w, y.w, acc);
  }
  return acc;
}

__global__ void __launch_bounds__(kGradThreads) ddqn_grad_kernel(LearnArgs a) {
  __shared__ float red[kGradThreads];
  const Dims& d = a.d;
  const Work& w = a.w;
  const int B = a.B, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* ws = a.ws;
  float* G = a.ws + w.G;
  const float* gq = ws + w.gq;
  const int* act = reinterpret_cast<const int*>(ws + w.act);
  float ss = 0.f;
  int blk = blockIdx.x;
  if (blk < w.nb_bil) {
    // dW[o][i][j] = sum_b dz0[o][b] s_i[b] x_j[b], b ascending
    const int64_t e = (int64_t)blk * kGradThreads + tid;
    if (e < d.sz[BIL_W]) {
      const int jn = (int)(e % d.N), i = (int)((e / d.N) % d.N), o = (int)(e / ((int64_t)d.N * d.N));
      const uint32_t* sr = reinterpret_cast<const uint32_t*>(ws + w.srow) + (i >> 5) * B;
      const uint32_t* tr = reinterpret_cast<const uint32_t*>(ws + w.trow) + (jn >> 5) * B;
      const float* dz = ws + w.dz0 + (int64_t)o * B;
      float s = 0.f;
      for (int b = 0; b < B; ++b)
        if (((sr[b] >> (i & 31)) & (tr[b] >> (jn & 31)) & 1u) != 0u) s += dz[b];
      G[d.off[BIL_W] + e] = s;
      ss = s * s;
    }
  } else if ((blk -= w.nb_bil) == 0) {
    // the three biases: db[o] = sum_b delta[o][b]
    float s = 0.f;
    int64_t at = -1;
    if (tid < d.h0) {
      for (int b = 0; b < B; ++b) s += ws[w.dz0 + (int64_t)tid * B + b];
      at = d.off[BIL_B] + tid;
    } else if (tid - 64 >= 0 && tid - 64 < d.h1) {
      for (int b = 0; b < B; ++b) s += ws[w.dz1 + (int64_t)(tid - 64) * B + b];
      at = d.off[L1_B] + tid - 64;
    } else if (tid - 128 >= 0 && tid - 128 < d.A) {
      for (int b = 0; b < B; ++b) s += act[b] == tid - 128 ? gq[b] : 0.f;
      at = d.off[OUT_B] + tid - 128;
    }
    if (at >= 0) {
      G[at] = s;
      ss = s * s;
    }
  } else if ((blk -= 1) < w.nb_w1) {
    const int tile = blk * 4 + wave;
    if (tile < d.H1T * d.H0T) {   // (wave-uniform)
      const int ot = tile / d.H0T, kt = tile - ot * d.H0T;
      const float* X = ws + w.dz1;
      const f32x4 acc = grad_tile(ws + w.y0, kt, B, lane, [&](int o, int b4) {
        return *reinterpret_cast<const float4*>(X + (int64_t)(16 * ot + o) * B + b4);
      });
      const int col = 16 * kt + (lane & 15);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * ot + 4 * (lane >> 4) + v;
        if (row < d.h1 && col < d.h0) {
          G[d.off[L1_W] + (int64_t)row * d.h0 + col] = acc[v];
          ss += acc[v] * acc[v];
        }
      }
    }
  } else {
    blk -= w.nb_w1;
    const int tile = blk * 4 + wave;
    if (tile < d.AT * d.H1T) {
      const int ot = tile / d.H1T, kt = tile - ot * d.H1T;
      const f32x4 acc = grad_tile(ws + w.y1, kt, B, lane, [&](int o, int b4) {
        const int4 ab = *reinterpret_cast<const int4*>(act + b4);
        const float4 gb = *reinterpret_cast<const float4*>(gq + b4);
        const int ai = 16 * ot + o;
        return make_float4(ab.x == ai ? gb.x : 0.f, ab.y == ai ? gb.y : 0.f, ab.z == ai ? gb.z : 0.f,
                           ab.w == ai ? gb.w : 0.f);
      });
      const int col = 16 * kt + (lane & 15);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * ot + 4 * (lane >> 4) + v;
        if (row < d.A && col < d.h1) {
          G[d.off[OUT_W] + (int64_t)row * d.h1 + col] = acc[v];
          ss += acc[v] * acc[v];
        }
      }
    }
  }
  red[tid] = ss;
  __syncthreads();
  for (int s = kGradThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) a.ws[w.partial + blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kGradThreads) ddqn_adam_kernel(LearnArgs a) {
  __shared__ float red[kGradThreads];
  const Dims& d = a.d;
  const Work& w = a.w;
  const int tid = threadIdx.x;
  // the total norm: every block adds the same sums in the same order
  float s = 0.f;
  for (int k = tid; k < w.nblocks; k += kGradThreads) s += a.ws[w.partial + k];
  red[tid] = s;
  __syncthreads();
  for (int k = kGradThreads / 2; k >= 1; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  const float total = sqrtf(red[0]);
  // clip_grad_norm_: coef = max_norm / (total + 1e-6), at most 1; every gradient is multiplied (by
  // NaN when the norm is NaN)
  const float coef = pbn::clip_coef(total, a.max_norm);
  if (blockIdx.x == 0 && tid == 0) {
    a.grad_norm[0] = total;
    float ls = 0.f;
    for (int b = 0; b < a.B; ++b) ls += a.ws[w.lrow + b];
    a.loss[0] = ls / (float)a.B;
  }
  const float stepc = a.step[0];
  const float bc1 = 1.f - powf(a.b1, stepc);
  const float bc2s = sqrtf(1.f - powf(a.b2, stepc));
  const float* G = a.ws + w.G;
  for (int64_t e = (int64_t)blockIdx.x * kGradThreads + tid; e < d.off[TOTAL]; e += (int64_t)gridDim.x * kGradThreads) {
    int seg = 0;
#pragma unroll
    for (int k = 1; k < TOTAL; ++k) seg += e >= d.off[k] ? 1 : 0;
    if (e - d.off[seg] >= d.sz[seg]) {   // the segment's padding
      if (a.grad) a.grad[e] = 0.f;
      continue;
    }
    const float gv = G[e] * coef;
    if (a.grad) a.grad[e] = gv;
    const pbn::AdamElement n = pbn::adam_element(a.P[e], a.m[e], a.v[e], gv, a.lr, a.b1, a.b2, a.eps, bc1, bc2s);
    a.m[e] = n.m;
    a.v[e] = n.v;
    a.P[e] = n.p;
  }
}

// ---- the schedule step ---------------------------------------------------------------------------
// _schedule_step's beta and hard target copy (ddqn_per/__init__.py:283-290, :488-490) for a frame
// that is replayed from a graph: beta moves in place, and the copy is due when the frames done so
// far, *step - base, are a multiple of `every`.  *step is the env step index that an EARLIER launch
// of the frame advanced (pbn_replay_advance) and nothing here writes, so every block reads the same
// value and takes the same branch; only thread 0 of block 0 touches *beta, which no other thread
// reads.  Not due: a block leaves after that one load.  Due: both ranges as one run of 16-byte
// vectors, grid-stride, plain loads and stores (the target image is read by the next update).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct ScheduleArgs {
  double* beta;
  double beta_inc;
  const int64_t* step;
  int64_t base, every;
  u32x4* t_flat;
  const u32x4* q_flat;
  int64_t n_flat;   // 16-byte vectors
  u32x4* t_img;
  const u32x4* q_img;
  int64_t n_img;
};

__global__ void __launch_bounds__(256) ddqn_schedule_kernel(ScheduleArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double b = *a.beta + a.beta_inc;
    *a.beta = b > 1.0 ? 1.0 : b;   // min(beta + increment, 1)
  }
  if ((*a.step - a.base) % a.every != 0) return;
  const int64_t n = a.n_flat + a.n_img, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    if (i < a.n_flat)
      a.t_flat[i] = a.q_flat[i];
    else
      a.t_img[i - a.n_flat] = a.q_img[i - a.n_flat];
  }
}

bool overlap(const void* p, const void* q, int64_t bytes) {
  const char* a = static_cast<const char*>(p);
  const char* b = static_cast<const char*>(q);
  return a < b + bytes && b < a + bytes;
}

int check_batch(int64_t batch) {
  if (batch < 16 || batch > 1024 || (batch & 15))
    return pbn::set_error(PBN_EINVAL, "batch must be a multiple of 16 in 16..1024");
  return PBN_OK;
}

int net_dims(const pbn_net* net, int h0, int h1, Dims* d) {
  if (const char* msg = shape_error(1, h0, h1)) return pbn::set_error(PBN_EINVAL, msg);
  pbn::NetView nv;
  int rc = pbn::net_view(net, &nv);
  if (rc) return rc;
  if (const char* msg = shape_error(nv.n_nodes, h0, h1)) return pbn::set_error(PBN_EINVAL, msg);
  if (nv.W < 1 || nv.W > 4) return pbn::set_error(PBN_EINVAL, "state words must be 1..4");
  make_dims(nv.n_nodes, nv.W, nv.n_attr, h0, h1, d);
  return PBN_OK;
}

unsigned pack_blocks(const Dims& d) { return (unsigned)std::min<int64_t>((d.itotal + 255) / 256, 4096); }

}  // namespace

extern "C" {

int pbn_dqn_layout(int32_t n_nodes, int32_t h0, int32_t h1, int64_t* offsets) {
  if (const char* msg = shape_error(n_nodes, h0, h1)) return pbn::set_error(PBN_EINVAL, msg);
  if (!offsets) return pbn::set_error(PBN_EINVAL, "null offsets");
  Dims d;
  make_dims(n_nodes, (n_nodes + 31) / 32, 0, h0, h1, &d);
  for (int s = 0; s <= TOTAL; ++s) offsets[s] = d.off[s];
  return PBN_OK;
}

int pbn_dqn_image_floats(const pbn_net* net, int32_t h0, int32_t h1, int64_t* n_floats) {
  if (!n_floats) return pbn::set_error(PBN_EINVAL, "null n_floats");
  Dims d;
  if (int rc = net_dims(net, h0, h1, &d)) return rc;
  *n_floats = d.itotal;
  return PBN_OK;
}

int pbn_dqn_pack(const pbn_net* net, int32_t h0, int32_t h1, const float* d_params, float* d_image, void* stream) {
  Dims d;
  if (int rc = net_dims(net, h0, h1, &d)) return rc;
  if (!d_params || !d_image) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_params, 16) || !pbn::aligned(d_image, 16))
    return pbn::set_error(PBN_EINVAL, "parameter and image buffers: 16-byte aligned");
  if (int rc = pbn::check_device(net)) return rc;
  pbn::NetView nv;
  pbn::net_view(net, &nv);
  hipLaunchKernelGGL(dqn_pack_kernel, dim3(pack_blocks(d)), dim3(256), 0, (hipStream_t)stream, d, d_params,
                     nv.att_first, d_image);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "dqn_pack_kernel launch failed");
  return PBN_OK;
}

int pbn_dqn_flipmask_from_state(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step,
                                uint64_t env_offset, int64_t n_envs, const uint32_t* d_state, const uint8_t* d_target,
                                int32_t h0, int32_t h1, const float* d_image, float epsilon, const float* d_epsilon,
                                float* d_q, uint32_t* d_flipmask, int32_t* d_actions, void* stream) {
  if (n_envs < 0 || (n_envs & 31) || (env_offset & 31))
    return pbn::set_error(PBN_EINVAL, "n_envs and env_offset must be multiples of 32");
  if (const char* msg = pbn::explore_args_error(epsilon, d_step, d_epsilon)) return pbn::set_error(PBN_EINVAL, msg);
  ActArgs a;
  if (int rc = net_dims(net, h0, h1, &a.d)) return rc;
  if (n_envs * (int64_t)a.d.A >= ((int64_t)1 << 31)) return pbn::set_error(PBN_EINVAL, "n_envs * n_actions >= 2^31");
  if (!d_state || !d_target || !d_image || !d_flipmask) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_image, 16)) return pbn::set_error(PBN_EINVAL, "d_image must be 16-byte aligned");
  if (((uintptr_t)d_q | (uintptr_t)d_flipmask | (uintptr_t)d_actions | (uintptr_t)d_state) & 3u)
    return pbn::set_error(PBN_EINVAL, "d_state, d_q, d_flipmask and d_actions must be 4-byte aligned");
  if (int rc = pbn::check_device(net)) return rc;
  if (n_envs == 0) return PBN_OK;
  a.n = n_envs;
  a.state = d_state;
  a.target = d_target;
  a.img = d_image;
  a.seed = seed;
  a.step = step;
  a.env_offset = env_offset;
  // explore iff word 0 < floor(epsilon * 2^32): epsilon = 1 always explores, 0 never
  a.eps_u = explore_threshold(epsilon);
  a.d_step = d_step;
  a.d_eps = d_epsilon;
  a.q = d_q;
  a.flipmask = d_flipmask;
  a.actions = d_actions;
  const int64_t tiles = n_envs / 16;
  hipLaunchKernelGGL(dqn_act_kernel, dim3((unsigned)((tiles + kActWaves - 1) / kActWaves)), dim3(64 * kActWaves), 0,
                     (hipStream_t)stream, a);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "dqn_act_kernel launch failed");
  return PBN_OK;
}

int pbn_ddqn_learn_workspace(int32_t n_nodes, int32_t h0, int32_t h1, int64_t batch, int64_t* bytes) {
  if (const char* msg = shape_error(n_nodes, h0, h1)) return pbn::set_error(PBN_EINVAL, msg);
  if (int rc = check_batch(batch)) return rc;
  if (!bytes) return pbn::set_error(PBN_EINVAL, "null bytes");
  Dims d;
  make_dims(n_nodes, (n_nodes + 31) / 32, 0, h0, h1, &d);
  *bytes = make_work(d, batch).total * (int64_t)sizeof(float);
  return PBN_OK;
}

int pbn_ddqn_learn(const pbn_net* net, int32_t h0, int32_t h1, int64_t batch, const int64_t* d_idx, int64_t capacity,
                   const uint32_t* d_state, const uint32_t* d_next_state, const uint8_t* d_target,
                   const int32_t* d_action, const float* d_reward, const uint8_t* d_done, float* d_params,
                   float* d_image, const float* d_target_image, float* d_adam_m, float* d_adam_v, float* d_adam_step,
                   float lr, float beta1, float beta2, float eps, float gamma, float max_grad_norm, void* d_workspace,
                   int64_t workspace_bytes, float* d_loss, float* d_grad_norm, float* d_grad, const float* d_weights,
                   float replay_constant, float* d_priority, void* stream) {
  if ((d_weights == nullptr) != (d_priority == nullptr))
    return pbn::set_error(PBN_EINVAL, "pbn_ddqn_learn: d_weights and d_priority come together");
  if (((uintptr_t)d_weights | (uintptr_t)d_priority) & 3u)
    return pbn::set_error(PBN_EINVAL, "pbn_ddqn_learn: d_weights and d_priority must be 4-byte aligned");
  if (int rc = check_batch(batch)) return rc;
  LearnArgs a;
  if (int rc = net_dims(net, h0, h1, &a.d)) return rc;
  if (capacity < 1) return pbn::set_error(PBN_EINVAL, "capacity >= 1");
  a.w = make_work(a.d, batch);
  if (workspace_bytes < a.w.total * (int64_t)sizeof(float))
    return pbn::set_error(PBN_EINVAL, "workspace too small (pbn_ddqn_learn_workspace)");
  if (!d_idx || !d_state || !d_next_state || !d_target || !d_action || !d_reward || !d_done || !d_params ||
      !d_adam_m || !d_adam_v || !d_adam_step || !d_workspace || !d_loss || !d_grad_norm)
    return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!d_image || !d_target_image) return pbn::set_error(PBN_EINVAL, "null network image");
  for (const void* p : {(const void*)d_params, (const void*)d_adam_m, (const void*)d_adam_v, (const void*)d_workspace,
                        (const void*)d_image, (const void*)d_target_image, (const void*)d_grad})
    if (!pbn::aligned(p, 16)) return pbn::set_error(PBN_EINVAL, "parameter, image and workspace buffers: 16-byte aligned");
  if (!pbn::aligned(d_idx, 8) || (((uintptr_t)d_state | (uintptr_t)d_next_state | (uintptr_t)d_action |
                                   (uintptr_t)d_reward | (uintptr_t)d_adam_step | (uintptr_t)d_loss |
                                   (uintptr_t)d_grad_norm) & 3u))
    return pbn::set_error(PBN_EINVAL, "d_idx must be 8-byte, the ring and scalar buffers 4-byte aligned");
  if (int rc = pbn::check_device(net)) return rc;
  pbn::NetView nv;
  pbn::net_view(net, &nv);
  a.B = (int)batch;
  a.idx = d_idx;
  a.cap = capacity;
  a.st = d_state;
  a.nst = d_next_state;
  a.tgt = d_target;
  a.act = d_action;
  a.rew = d_reward;
  a.done = d_done;
  a.att_first = nv.att_first;
  a.P = d_params;
  a.img = d_image;
  a.timg = d_target_image;
  a.m = d_adam_m;
  a.v = d_adam_v;
  a.step = d_adam_step;
  a.lr = lr;
  a.b1 = beta1;
  a.b2 = beta2;
  a.eps = eps;
  a.gamma = gamma;
  a.max_norm = max_grad_norm;
  a.rconst = replay_constant;
  a.ws = static_cast<float*>(d_workspace);
  a.loss = d_loss;
  a.grad_norm = d_grad_norm;
  a.grad = d_grad;
  a.wts = d_weights;
  a.prio = d_priority;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ddqn_fb_kernel, dim3((unsigned)(batch / 16)), dim3(192), 0, s, a);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "ddqn_fb_kernel launch failed");
  hipLaunchKernelGGL(ddqn_grad_kernel, dim3((unsigned)a.w.nblocks), dim3(kGradThreads), 0, s, a);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "ddqn_grad_kernel launch failed");
  const unsigned ab = (unsigned)std::min<int64_t>((a.d.off[TOTAL] + kGradThreads - 1) / kGradThreads, 1024);
  hipLaunchKernelGGL(ddqn_adam_kernel, dim3(ab), dim3(kGradThreads), 0, s, a);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "ddqn_adam_kernel launch failed");
  hipLaunchKernelGGL(dqn_pack_kernel, dim3(pack_blocks(a.d)), dim3(256), 0, s, a.d, d_params, nv.att_first, d_image);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "dqn_pack_kernel launch failed");
  return PBN_OK;
}

int pbn_ddqn_schedule(double* d_beta, double beta_increment, const int64_t* d_step, int64_t step_base,
                      int64_t target_update, float* d_target_params, const float* d_params, int64_t n_params,
                      float* d_target_image, const float* d_image, int64_t n_image, void* stream) {
  if (!d_beta || !d_step) return pbn::set_error(PBN_EINVAL, "pbn_ddqn_schedule: null d_beta or d_step");
  if (((uintptr_t)d_beta | (uintptr_t)d_step) & 7u)
    return pbn::set_error(PBN_EINVAL, "pbn_ddqn_schedule: d_beta and d_step must be 8-byte aligned");
  if (target_update < 1) return pbn::set_error(PBN_EINVAL, "pbn_ddqn_schedule: target_update >= 1");
  if (n_params < 4 || n_image < 4 || (n_params & 3) || (n_image & 3))
    return pbn::set_error(PBN_EINVAL, "pbn_ddqn_schedule: n_params and n_image must be positive multiples of 4");
  if (!d_target_params || !d_params || !d_target_image || !d_image)
    return pbn::set_error(PBN_EINVAL, "pbn_ddqn_schedule: null buffer");
  if (!pbn::aligned(d_target_params, 16) || !pbn::aligned(d_params, 16) || !pbn::aligned(d_target_image, 16) ||
      !pbn::aligned(d_image, 16))
    return pbn::set_error(PBN_EINVAL, "pbn_ddqn_schedule: parameter and image buffers: 16-byte aligned");
  if (overlap(d_target_params, d_params, n_params * 4) || overlap(d_target_image, d_image, n_image * 4))
    return pbn::set_error(PBN_EINVAL, "pbn_ddqn_schedule: a target buffer overlaps its source");
  ScheduleArgs a;
  a.beta = d_beta;
  a.beta_inc = beta_increment;
  a.step = d_step;
  a.base = step_base;
  a.every = target_update;
  a.t_flat = reinterpret_cast<u32x4*>(d_target_params);
  a.q_flat = reinterpret_cast<const u32x4*>(d_params);
  a.n_flat = n_params / 4;
  a.t_img = reinterpret_cast<u32x4*>(d_target_image);
  a.q_img = reinterpret_cast<const u32x4*>(d_image);
  a.n_img = n_image / 4;
  // one vector per thread up to 1,024 blocks (a few hundred KB: some tens), grid-stride past that
  const unsigned blocks = (unsigned)std::min<int64_t>((a.n_flat + a.n_img + 255) / 256, 1024);
  hipLaunchKernelGGL(ddqn_schedule_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "ddqn_schedule_kernel launch failed");
  return PBN_OK;
}

}  // extern "C"
