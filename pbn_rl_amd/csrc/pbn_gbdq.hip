// pbn_gbdq.hip -- the GBDQ graph agent's kernels (gbdq_model/network.py:73-79, gbdq_model/__init__.py:
// 183-200; DESIGN.md "GBDQ").
//
//   pbn_gbdq_pack           parameters + the edge list by target node -> the front kernel's image
//   pbn_gbdq_front          the three EdgeConv(add) + BatchNorm1d (per env) + ReLU layers, one launch
//   pbn_replay_store_split  a frame's transitions into the positive and the negative ring
//
// Written literally, EdgeConv forms one row per (env, edge) three times per frame.  The front kernel
// never does: one block works on one env at a time with the (N, N) activations in LDS.
//   layer 1   an edge's input is four bits, so its message is one of 16 precomputed rows (M1); a node
//             sums table rows over its edge list
//   layers 2, 3   with the first Linear split W1 = [A | Bm]:  W1 cat[x_i, x_j - x_i] = (A - Bm) x_i + Bm x_j.
//             u_i = (A - Bm) a_i + b1 and v_j = Bm a_j for all nodes are one MFMA product (rows = nodes,
//             k = features, 128 outputs); an edge is z_e = relu(u_i + v_j), 64 adds and maxes; the
//             second Linear is linear, so it runs once per node on S_i = sum_e z_e, a second MFMA
//             product, plus deg(i) b2
//   BatchNorm per (env, node) row over its N features: one wave per row, butterfly sums (a fixed order)
// v_mfma_f32_16x16x4_f32: exact f32 (an fmaf chain over k).  Lane l gives A[l & 15][k = l >> 4] and
// B[k = l >> 4][l & 15] and holds D[4 (l >> 4) + r][l & 15] in register r.
// No floating-point atomics anywhere: every sum's order is fixed by the thread that owns it.
// Every ReLU is dqn_scalar.h's pbn::relu (x < 0 ? 0 : x), never fmaxf, which drops a NaN: a non-finite
// parameter gives the literal PyTorch forward's NaN rows (DESIGN.md "Non-finite values").  Padding
// needs no mask for it: a 0 * NaN can only land in rows >= N of u / v (never read: the edge list is
// held to [0, N - 1]) and in output tiles' rows / columns >= N (never stored).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pbn_env.h"
#include "dqn_scalar.h"
#include "gbdq_front.h"
#include "host_check.h"
#include "net_view.h"
#include "wave_util.h"

namespace {

using pbn::GbdqConv;
using pbn::GbdqLayout;
using pbn::kGbdqHidden;
using pbn::kGbdqThreads;
using pbn::kGbdqUS;

// a product the compiler cannot contract into an fma with the add that follows it (the M1 table's
// sums are stated as unfused)
__device__ __forceinline__ float mul_rn(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

// ---- pbn_gbdq_pack: one launch, grid-stride over every segment of the image
__global__ void __launch_bounds__(256) gbdq_pack_kernel(GbdqLayout L, GbdqConv C, const float* __restrict__ conv,
                                                        int E, const int32_t* __restrict__ csr_start,
                                                        const int32_t* __restrict__ csr_src, float* __restrict__ image) {
  const int N = L.N;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, dt = (int64_t)gridDim.x * blockDim.x;
  // M1[code][o] = W2 relu(W1 in + b1) + b2, in = (s_i, t_i, s_j - s_i, t_j - t_i): sequential, unfused
  for (int64_t idx = t0; idx < 16 * (int64_t)N; idx += dt) {
    const int code = (int)(idx / N), o = (int)(idx - (int64_t)code * N);
    const float si = (float)(code & 1), ti = (float)((code >> 1) & 1);
    const float in0 = si, in1 = ti, in2 = (float)((code >> 2) & 1) - si, in3 = (float)((code >> 3) & 1) - ti;
    const float* w1 = conv + C.w1[0];
    const float* w2 = conv + C.w2[0] + (int64_t)o * kGbdqHidden;
    float acc = 0.f;
    for (int c = 0; c < kGbdqHidden; ++c) {
      float h = mul_rn(w1[4 * c], in0);
      h = (h + mul_rn(w1[4 * c + 1], in1));
      h = (h + mul_rn(w1[4 * c + 2], in2));
      h = (h + mul_rn(w1[4 * c + 3], in3));
      h = pbn::relu(h + conv[C.b1[0] + c]);
      acc = (acc + mul_rn(w2[c], h));
    }
    image[L.m1 + idx] = (acc + conv[C.b2[0] + o]);
  }
  for (int64_t idx = t0; idx < 6 * (int64_t)N; idx += dt) image[L.bn + idx] = conv[C.bn + idx];
  for (int l = 0; l < 2; ++l) {
    const float* w1 = conv + C.w1[l + 1];     // [64][2 N]
    const float* w2 = conv + C.w2[l + 1];     // [N][64]
    for (int64_t idx = t0; idx < (int64_t)L.Kp * 128; idx += dt) {
      const int k = (int)(idx >> 7), c = (int)(idx & 127);
      float x = 0.f;
      if (k < N) {
        if (c < 64) x = w1[(int64_t)c * 2 * N + k] - w1[(int64_t)c * 2 * N + N + k];
        else x = w1[(int64_t)(c - 64) * 2 * N + N + k];
      }
      image[L.wu[l] + idx] = x;
    }
    for (int64_t idx = t0; idx < kGbdqHidden; idx += dt) image[L.b1[l] + idx] = conv[C.b1[l + 1] + idx];
    for (int64_t idx = t0; idx < (int64_t)kGbdqHidden * L.Np; idx += dt) {
      const int c = (int)(idx / L.Np), o = (int)(idx - (int64_t)c * L.Np);
      image[L.w2t[l] + idx] = o < N ? w2[(int64_t)o * kGbdqHidden + c] : 0.f;
    }
    for (int64_t idx = t0; idx < N; idx += dt) image[L.b2[l] + idx] = conv[C.b2[l + 1] + idx];
  }
  // the edge list, held to its ranges (the front kernel indexes LDS and this list with it)
  int32_t* cs = reinterpret_cast<int32_t*>(image + L.csr_start);
  int32_t* cj = reinterpret_cast<int32_t*>(image + L.csr_src);
  for (int64_t idx = t0; idx <= N; idx += dt) cs[idx] = idx == 0 ? 0 : idx == N ? E : min(max(csr_start[idx], 0), E);
  for (int64_t idx = t0; idx < E; idx += dt) cj[idx] = min(max(csr_src[idx], 0), N - 1);
}

// ---- pbn_gbdq_front
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// BatchNorm1d in training mode on one env: row i over its N features (mean, biased variance, eps
// 1e-5), then gamma_i, beta_i and ReLU.  One wave per row, two features per lane (N <= 128).
__device__ __forceinline__ void bn_relu(float* __restrict__ act, int N, int NS, const float* __restrict__ gb,
                                        int wave, int lane) {
  const float fn = (float)N;   // (divided by, not multiplied with 1 / N: a constant row has zero deviation exactly)
  for (int i = wave; i < N; i += kGbdqThreads / 64) {
    float* row = act + i * NS;
    const bool h0 = lane < N, h1 = lane + 64 < N;
    const float x0 = h0 ? row[lane] : 0.f, x1 = h1 ? row[lane + 64] : 0.f;
    const float mean = wave_sum(x0 + x1) / fn;
    const float d0 = h0 ? x0 - mean : 0.f, d1 = h1 ? x1 - mean : 0.f;
    const float var = wave_sum(d0 * d0 + d1 * d1) / fn;
    const float scale = gb[i] / sqrtf(var + 1e-5f), beta = gb[N + i];
    if (h0) row[lane] = pbn::relu(d0 * scale + beta);
    if (h1) row[lane + 64] = pbn::relu(d1 * scale + beta);
  }
}

__global__ void __launch_bounds__(kGbdqThreads) gbdq_front_kernel(GbdqLayout L, const uint32_t* __restrict__ state,
                                                                  const uint8_t* __restrict__ target,
                                                                  const uint32_t* __restrict__ att_first, int n_attr,
                                                                  int W, uint32_t n, const float* __restrict__ image,
                                                                  float* __restrict__ out) {
  extern __shared__ float lds[];
  float* act = lds + L.lds_act;
  float* u = lds + L.lds_u;
  float* v = lds + L.lds_v;
  float* m1 = lds + L.lds_m1;
  int* code = reinterpret_cast<int*>(lds + L.lds_code);
  const int N = L.N, NS = L.NS, Np = L.Np;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* __restrict__ cs = reinterpret_cast<const int32_t*>(image + L.csr_start);
  const int32_t* __restrict__ cj = reinterpret_cast<const int32_t*>(image + L.csr_src);
  const int RT = Np >> 4;

  // once per block: the padding of act (never written afterwards) and the table
  for (int idx = tid; idx < Np * NS; idx += kGbdqThreads) act[idx] = 0.f;
  for (int idx = tid; idx < 16 * N; idx += kGbdqThreads) m1[idx] = image[L.m1 + idx];

  for (uint32_t env = blockIdx.x; env < n; env += gridDim.x) {
    __syncthreads();
    const uint32_t tg = target[env];
    for (int i = tid; i < N; i += kGbdqThreads) {
      const uint32_t sw = state[(size_t)(i >> 5) * n + env];
      const uint32_t tw = tg < (uint32_t)n_attr ? att_first[(size_t)tg * W + (i >> 5)] : 0u;
      code[i] = (int)(((sw >> (i & 31)) & 1u) | (((tw >> (i & 31)) & 1u) << 1));
    }
    __syncthreads();
    // layer 1: node i's messages are table rows, summed in edge-list order
    for (int idx = tid; idx < N * N; idx += kGbdqThreads) {
      const int i = idx / N, o = idx - i * N;
      const int ci = code[i];
      float s = 0.f;
      for (int e = cs[i]; e < cs[i + 1]; ++e) s += m1[(ci | (code[cj[e]] << 2)) * N + o];
      act[i * NS + o] = s;
    }
    __syncthreads();
    bn_relu(act, N, NS, image + L.bn, wave, lane);
    __syncthreads();

    for (int l = 0; l < 2; ++l) {
      const float* __restrict__ wu = image + L.wu[l];
      const float* __restrict__ b1 = image + L.b1[l];
      const float* __restrict__ w2t = image + L.w2t[l];
      const float* __restrict__ b2 = image + L.b2[l];
      // [u | v] = act [A - Bm | Bm]^T: RT x 8 tiles of 16 x 16, k over the features
      for (int t = wave; t < RT * 8; t += kGbdqThreads / 64) {
        const int rt = t >> 3, ct = t & 7;
        const float* a_ptr = act + (rt * 16 + (lane & 15)) * NS + (lane >> 4);
        const float* b_ptr = wu + (lane >> 4) * 128 + ct * 16 + (lane & 15);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < L.Kp; k0 += 4) acc = mfma(a_ptr[k0], b_ptr[k0 * 128], acc);
        const int col = ct * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rt * 16 + (lane >> 4) * 4 + r;
          if (col < 64) u[row * kGbdqUS + col] = acc[r] + b1[col];
          else v[row * kGbdqUS + col - 64] = acc[r];
        }
      }
      __syncthreads();
      // S_i = sum over node i's edges of relu(u_i + v_j), in edge-list order, in place of u_i
      for (int idx = tid; idx < N * kGbdqHidden; idx += kGbdqThreads) {
        const int i = idx >> 6, c = idx & 63;
        const float ui = u[i * kGbdqUS + c];
        float s = 0.f;
        for (int e = cs[i]; e < cs[i + 1]; ++e) s += pbn::relu(ui + v[cj[e] * kGbdqUS + c]);
        u[i * kGbdqUS + c] = s;
      }
      __syncthreads();
      // out = S W2^T + deg b2: RT x RT tiles, k over the 64 hidden units
      for (int t = wave; t < RT * RT; t += kGbdqThreads / 64) {
        const int rt = t / RT, ct = t - rt * RT;
        const float* a_ptr = u + (rt * 16 + (lane & 15)) * kGbdqUS + (lane >> 4);
        const float* b_ptr = w2t + (lane >> 4) * Np + ct * 16 + (lane & 15);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k0 = 0; k0 < kGbdqHidden; k0 += 4) acc = mfma(a_ptr[k0], b_ptr[k0 * Np], acc);
        const int col = ct * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rt * 16 + (lane >> 4) * 4 + r;
          if (row < N && col < N) act[row * NS + col] = acc[r] + (float)(cs[row + 1] - cs[row]) * b2[col];
        }
      }
      __syncthreads();
      bn_relu(act, N, NS, image + L.bn + (l + 1) * 2 * N, wave, lane);
      __syncthreads();
    }
    float* o_row = out + (size_t)env * N * N;
    for (int idx = tid; idx < N * N; idx += kGbdqThreads) {
      const int i = idx / N;
      o_row[idx] = act[i * NS + (idx - i * N)];
    }
  }
}

// ---- pbn_replay_store_split
constexpr int kSplitThreads = 256;

__global__ void __launch_bounds__(kSplitThreads) split_count_kernel(int64_t n, const uint8_t* __restrict__ flags,
                                                                    uint32_t term_mask, int32_t* __restrict__ counts) {
  const int64_t e = blockIdx.x * (int64_t)kSplitThreads + threadIdx.x;
  const int c = __syncthreads_count(e < n && (flags[e] & term_mask) != 0);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

struct SplitRing {
  int64_t cap;
  const int64_t* pos;
  uint32_t* st;
  uint32_t* nst;
  uint8_t* tgt;
  int32_t* act;
  float* rew;
  uint8_t* done;
};

__global__ void __launch_bounds__(kSplitThreads) split_store_kernel(
    int64_t n, int W, int K, const uint32_t* __restrict__ st, const uint32_t* __restrict__ nst,
    const uint8_t* __restrict__ tgt, const int32_t* __restrict__ act, const float* __restrict__ rew,
    const uint8_t* __restrict__ flags, uint32_t term_mask, uint32_t done_mask, SplitRing rp, SplitRing rn,
    const int32_t* __restrict__ counts) {
  __shared__ int s_part[kSplitThreads / 64];
  __shared__ int s_wave[kSplitThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the terminated envs of the blocks before this one (integers: any order gives the same sum)
  int part = 0;
  for (int b = tid; b < (int)blockIdx.x; b += kSplitThreads) part += counts[b];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
  const int64_t e = blockIdx.x * (int64_t)kSplitThreads + tid;
  const bool live = e < n;
  const uint32_t fl = live ? flags[e] : 0u;
  const bool term = live && (fl & term_mask) != 0;
  const unsigned long long ballot = __ballot(term);
  if (lane == 0) {
    s_part[wave] = part;
    s_wave[wave] = __popcll(ballot);
  }
  __syncthreads();
  int64_t before = 0;     // terminated envs with a lower index than e
  for (int w = 0; w < kSplitThreads / 64; ++w) {
    before += s_part[w];
    if (w < wave) before += s_wave[w];
  }
  before += __popcll(ballot & ((1ull << lane) - 1ull));
  if (!live) return;
  const SplitRing r = term ? rp : rn;
  const int64_t rank = term ? before : e - before;
  const int64_t j = (*r.pos + rank) % r.cap;
  for (int w = 0; w < W; ++w) {
    r.st[(size_t)w * r.cap + j] = st[(size_t)w * n + e];
    r.nst[(size_t)w * r.cap + j] = nst[(size_t)w * n + e];
  }
  r.tgt[j] = tgt[e];
  for (int k = 0; k < K; ++k) r.act[(size_t)j * K + k] = act[(size_t)e * K + k];
  r.rew[j] = rew[e];
  r.done[j] = (fl & done_mask) ? 1 : 0;
}

__global__ void split_tail_kernel(int64_t n, int blocks, const int32_t* __restrict__ counts, int64_t cap_p,
                                  int64_t* __restrict__ pos_p, int64_t* __restrict__ size_p, int64_t cap_n,
                                  int64_t* __restrict__ pos_n, int64_t* __restrict__ size_n,
                                  int64_t* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t p = 0;
  for (int b = 0; b < blocks; ++b) p += counts[b];
  const int64_t q = n - p;
  out[0] = p;
  out[1] = q;
  *pos_p = (*pos_p + p) % cap_p;
  *size_p = *size_p + p < cap_p ? *size_p + p : cap_p;
  *pos_n = (*pos_n + q) % cap_n;
  *size_n = *size_n + q < cap_n ? *size_n + q : cap_n;
}

int launch_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PBN_OK : pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
}

}  // namespace

int pbn_gbdq_image_floats(const pbn_net* net, int32_t n_edges, int64_t* n_floats) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if (n_edges < 0 || !n_floats) return pbn::set_error(PBN_EINVAL, "n_edges >= 0 and a non-null n_floats");
  *n_floats = pbn::gbdq_layout(v.n_nodes).csr_src + pbn::gbdq_al16(n_edges);
  return PBN_OK;
}

int pbn_gbdq_pack(const pbn_net* net, const float* d_conv, int32_t n_edges, const int32_t* d_csr_start,
                  const int32_t* d_csr_src, float* d_image, void* stream) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if ((rc = pbn::check_device(net))) return rc;
  if (n_edges < 0) return pbn::set_error(PBN_EINVAL, "n_edges >= 0");
  if (!d_conv || !d_csr_start || (n_edges > 0 && !d_csr_src) || !d_image) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_conv, 4) || !pbn::aligned(d_csr_start, 4) || !pbn::aligned(d_csr_src, 4) || !pbn::aligned(d_image, 16))
    return pbn::set_error(PBN_EINVAL, "d_image must be 16-byte, the inputs 4-byte aligned");
  const GbdqLayout L = pbn::gbdq_layout(v.n_nodes);
  hipLaunchKernelGGL(gbdq_pack_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, L, pbn::gbdq_conv(v.n_nodes), d_conv,
                     (int)n_edges, d_csr_start, d_csr_src, d_image);
  return launch_error();
}

int pbn_gbdq_front(const pbn_net* net, int64_t n_envs, const uint32_t* d_state, const uint8_t* d_target,
                   const float* d_image, float* d_out, void* stream) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if ((rc = pbn::check_device(net))) return rc;
  if (n_envs < 0 || (n_envs & 31)) return pbn::set_error(PBN_EINVAL, "n_envs must be a non-negative multiple of 32");
  if (n_envs * v.n_nodes * v.n_nodes >= ((int64_t)1 << 31)) return pbn::set_error(PBN_EINVAL, "n_envs too large");
  const GbdqLayout L = pbn::gbdq_layout(v.n_nodes);
  const size_t lds = (size_t)L.lds_floats * sizeof(float);
  if (v.n_nodes > 128 || lds > (size_t)pbn::kGbdqMaxLds)
    return pbn::set_error(PBN_EINVAL, "the front kernel's LDS carving does not fit this node count");
  if (n_envs == 0) return PBN_OK;
  if (!d_state || !d_target || !d_image || !d_out) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_image, 16) || !pbn::aligned(d_out, 16))
    return pbn::set_error(PBN_EINVAL, "d_image and d_out must be 16-byte aligned");
  if (lds > 64 * 1024) {   // beyond the default dynamic-LDS limit
    static bool raised[64] = {};   // per device (a pbn_net is bound to one)
    const int dv = v.device >= 0 && v.device < 64 ? v.device : 0;
    if (!raised[dv]) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(gbdq_front_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, pbn::kGbdqMaxLds) != hipSuccess)
        return pbn::set_error(PBN_EDEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      raised[dv] = true;
    }
  }
  const unsigned blocks = (unsigned)std::min<int64_t>(n_envs, 2048);
  hipLaunchKernelGGL(gbdq_front_kernel, dim3(blocks), dim3(kGbdqThreads), lds, (hipStream_t)stream, L, d_state, d_target,
                     v.att_first, v.n_attr, v.W, (uint32_t)n_envs, d_image, d_out);
  return launch_error();
}

int pbn_replay_store_split(int64_t n, int32_t words, int32_t n_branches, const uint32_t* d_state,
                           const uint32_t* d_next_state, const uint8_t* d_target, const int32_t* d_action,
                           const float* d_reward, const uint8_t* d_flags, uint32_t term_mask, uint32_t done_mask,
                           int64_t capacity_p, int64_t* d_pos_p, int64_t* d_size_p, uint32_t* d_ring_state_p,
                           uint32_t* d_ring_next_state_p, uint8_t* d_ring_target_p, int32_t* d_ring_action_p,
                           float* d_ring_reward_p, uint8_t* d_ring_done_p, int64_t capacity_n, int64_t* d_pos_n,
                           int64_t* d_size_n, uint32_t* d_ring_state_n, uint32_t* d_ring_next_state_n,
                           uint8_t* d_ring_target_n, int32_t* d_ring_action_n, float* d_ring_reward_n,
                           uint8_t* d_ring_done_n, int32_t* d_work, int64_t* d_counts, void* stream) {
  if (n < 1 || n >= ((int64_t)1 << 31) || capacity_p < n || capacity_n < n || words < 1 || words > 4 || n_branches < 1)
    return pbn::set_error(PBN_EINVAL, "1 <= n < 2^31, both capacities >= n, words 1..4, n_branches >= 1");
  if (!term_mask || !done_mask) return pbn::set_error(PBN_EINVAL, "term_mask and done_mask must be nonzero");
  if (!d_state || !d_next_state || !d_target || !d_action || !d_reward || !d_flags || !d_pos_p || !d_size_p ||
      !d_ring_state_p || !d_ring_next_state_p || !d_ring_target_p || !d_ring_action_p || !d_ring_reward_p ||
      !d_ring_done_p || !d_pos_n || !d_size_n || !d_ring_state_n || !d_ring_next_state_n || !d_ring_target_n ||
      !d_ring_action_n || !d_ring_reward_n || !d_ring_done_n || !d_work || !d_counts)
    return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_pos_p, 8) || !pbn::aligned(d_size_p, 8) || !pbn::aligned(d_pos_n, 8) || !pbn::aligned(d_size_n, 8) ||
      !pbn::aligned(d_counts, 8) || !pbn::aligned(d_work, 4))
    return pbn::set_error(PBN_EINVAL, "the positions, fill levels and d_counts must be 8-byte, d_work 4-byte aligned");
  const int blocks = (int)((n + kSplitThreads - 1) / kSplitThreads);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(split_count_kernel, dim3(blocks), dim3(kSplitThreads), 0, s, n, d_flags, term_mask, d_work);
  int rc = launch_error();
  if (rc) return rc;
  const SplitRing rp = {capacity_p, d_pos_p, d_ring_state_p, d_ring_next_state_p, d_ring_target_p, d_ring_action_p,
                        d_ring_reward_p, d_ring_done_p};
  const SplitRing rn = {capacity_n, d_pos_n, d_ring_state_n, d_ring_next_state_n, d_ring_target_n, d_ring_action_n,
                        d_ring_reward_n, d_ring_done_n};
  hipLaunchKernelGGL(split_store_kernel, dim3(blocks), dim3(kSplitThreads), 0, s, n, (int)words, (int)n_branches, d_state,
                     d_next_state, d_target, d_action, d_reward, d_flags, term_mask, done_mask, rp, rn, d_work);
  if ((rc = launch_error())) return rc;
  hipLaunchKernelGGL(split_tail_kernel, dim3(1), dim3(1), 0, s, n, blocks, d_work, capacity_p, d_pos_p, d_size_p,
                     capacity_n, d_pos_n, d_size_n, d_counts);
  return launch_error();
}
