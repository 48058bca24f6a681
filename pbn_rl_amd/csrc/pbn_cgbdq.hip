// pbn_cgbdq.hip -- the ControlGBDQ agent's tail (control_gbdq_model/network.py:43-78,
// control_gbdq_model/__init__.py:64-86; DESIGN.md "ControlGBDQ").
//
//   pbn_cgbdq_pack      the tail's parameters -> MFMA-fragment-ordered image (csrc/cgbdq_tail.h)
//   pbn_cgbdq_heads     Linear(N N, 256) + ReLU, two Linear(256, 256) + ReLU, the value head and the C
//                       advantage heads as one stacked layer; the raw head outputs to HBM (tests)
//   pbn_cgbdq_flipmask  the same layers, then per env the dueling combination, the argmax over each
//                       head's two outputs, epsilon-greedy and the control flip mask; no heads in HBM
//
// One block takes 32 envs: they are the MFMA columns (two tiles of 16), the layer's outputs the rows
// (weights are the A operand, read as fragments from the image), the activations stay in LDS between
// layers as the B operand.  Layer 1 streams its K = N N inputs in chunks of 64 through a double
// buffer.  Wave w owns row tiles w, w + 4, w + 8, w + 12 (of each group of 16 tiles) for both column
// tiles: eight accumulators that share the two B reads of a k-step.
// v_mfma_f32_16x16x4_f32: exact f32 (an fmaf chain over k, k ascending; layer 1 groups its chain, see
// tail_layers).  Lane l gives A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15] and holds
// D[4 (l >> 4) + r][l & 15] in register r.  No atomics: two runs give the same bits, and both entry
// points run the same layer code, so their heads are bit-equal.
// Every ReLU is dqn_scalar.h's pbn::relu.  Padding (DESIGN.md "Non-finite values", Padding): the k tail
// of layer 1 is zero in the image and written as zero into LDS by index (never loaded), so no
// 0 * NaN arises there; the head rows >= HR are zero in the image and their outputs (0 * h: NaN where
// h is not finite) land in columns HR .. HRp - 1 of the head buffer, which nothing reads: the stores
// and the combination index rows < HR only.  The trunk has no padded rows (256 = 16 tiles).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/pbn_env.h"
#include "cgbdq_tail.h"
#include "dqn_scalar.h"
#include "host_check.h"
#include "net_view.h"
#include "philox.h"
#include "wave_util.h"

namespace {

using pbn::CgLayout;
using pbn::CgTail;
using pbn::kCgChunk;
using pbn::kCgEnvs;
using pbn::kCgHidden;
using pbn::kCgHS;
using pbn::kCgThreads;
using pbn::kCgXS;

// ---- pbn_cgbdq_pack: one launch, grid-stride over every segment of the image
__device__ __forceinline__ void pack_frag(float* __restrict__ dst, int Rp, int Kp, int R, int K, int64_t t0, int64_t dt,
                                          const float* __restrict__ tail, const CgTail T, int layer) {
  const int KG = Kp >> 4;
  for (int64_t idx = t0; idx < (int64_t)Rp * Kp; idx += dt) {
    const int j = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const int64_t t = idx >> 8;
    const int kg = (int)(t % KG), rt = (int)(t / KG);
    const int row = rt * 16 + (lane & 15), k = kg * 16 + 4 * j + (lane >> 4);
    float x = 0.f;
    if (row < R && k < K) {
      if (layer < 3) x = tail[T.w[layer] + (int64_t)row * K + k];
      else if (row == 0) x = tail[T.vw + k];
      else x = tail[T.heads + (int64_t)((row - 1) >> 1) * 514 + ((row - 1) & 1) * kCgHidden + k];
    }
    dst[idx] = x;
  }
}

__global__ void __launch_bounds__(256) cgbdq_pack_kernel(CgLayout L, CgTail T, const float* __restrict__ tail,
                                                         float* __restrict__ image) {
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, dt = (int64_t)gridDim.x * blockDim.x;
  pack_frag(image + L.w1, kCgHidden, L.K1p, kCgHidden, L.K1, t0, dt, tail, T, 0);
  pack_frag(image + L.w2, kCgHidden, kCgHidden, kCgHidden, kCgHidden, t0, dt, tail, T, 1);
  pack_frag(image + L.w3, kCgHidden, kCgHidden, kCgHidden, kCgHidden, t0, dt, tail, T, 2);
  pack_frag(image + L.wh, L.HRp, kCgHidden, L.HR, kCgHidden, t0, dt, tail, T, 3);
  for (int64_t idx = t0; idx < kCgHidden; idx += dt) {
    image[L.b1 + idx] = tail[T.b[0] + idx];
    image[L.b2 + idx] = tail[T.b[1] + idx];
    image[L.b3 + idx] = tail[T.b[2] + idx];
  }
  for (int64_t idx = t0; idx < L.HRp; idx += dt) {
    float x = 0.f;
    if (idx == 0) x = tail[T.vb];
    else if (idx < L.HR) x = tail[T.heads + ((idx - 1) >> 1) * 514 + 2 * kCgHidden + ((idx - 1) & 1)];
    image[L.bh + idx] = x;
  }
}

// ---- the layers
struct Acc {
  f32x4 v[4][2];
};

__device__ __forceinline__ void acc_zero(Acc& a) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t) a.v[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ void acc_add(Acc& a, const Acc& b) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t) a.v[i][t] += b.v[i][t];
}

// kgs k-groups (16 inputs each) from k-group kg0 of a layer with KG of them: row tiles rt0 + 4 i (those
// below RT) times both env tiles.  xs: LDS [32][xstride], its column 0 = input 16 kg0.
__device__ __forceinline__ void mac_groups(Acc& acc, const float* __restrict__ wfrag, int KG, int kg0, int kgs, int RT,
                                           int rt0, const float* xs, int xstride, int lane) {
  const float* xb = xs + (lane & 15) * xstride + (lane >> 4);
  for (int g = 0; g < kgs; ++g) {
    f32x4 a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rt = rt0 + 4 * i;
      a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (rt < RT) a[i] = *reinterpret_cast<const f32x4*>(wfrag + (((int64_t)rt * KG + kg0 + g) * 64 + lane) * 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float b0 = xb[g * 16 + 4 * j], b1 = xb[16 * xstride + g * 16 + 4 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (rt0 + 4 * i < RT) {
          acc.v[i][0] = mfma(a[i][j], b0, acc.v[i][0]);
          acc.v[i][1] = mfma(a[i][j], b1, acc.v[i][1]);
        }
      }
    }
  }
}

// dst[env][row] = acc + bias (then ReLU): lane's four rows of a tile are one float4 of an env's row
template <bool RELU>
__device__ __forceinline__ void store_tiles(const Acc& acc, const float* __restrict__ bias, int RT, int rt0, float* dst,
                                            int dstride, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rt = rt0 + 4 * i;
    if (rt >= RT) continue;
    const int row = rt * 16 + 4 * (lane >> 4);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + row);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc.v[i][t][r] + bv[r];
        o[r] = RELU ? pbn::relu(s) : s;
      }
      *reinterpret_cast<f32x4*>(dst + (t * 16 + (lane & 15)) * dstride + row) = o;
    }
  }
}

// The four layers for the block's 32 envs; on return (after a barrier) lds + L.lds_b holds the head
// outputs [32][L.OS] and lds + L.lds_a is free.
__device__ __forceinline__ void tail_layers(const CgLayout& L, const float* __restrict__ front, int64_t e0,
                                            const float* __restrict__ image, float* lds) {
  float* la = lds + L.lds_a;
  float* lb = lds + L.lds_b;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K1 = L.K1;
  const int KG1 = L.K1p >> 4;
  const int chunks = (L.K1p + kCgChunk - 1) / kCgChunk;
  const float* __restrict__ rows = front + e0 * K1;

  auto stage = [&](int c, float* xs) {
    for (int idx = tid; idx < kCgEnvs * kCgChunk; idx += kCgThreads) {
      const int e = idx >> 6, k = idx & (kCgChunk - 1);
      const int gk = c * kCgChunk + k;
      xs[e * kCgXS + k] = gk < K1 ? rows[(int64_t)e * K1 + gk] : 0.f;
    }
  };

  // Layer 1 sums in three levels, each in ascending order: a chunk's 64 inputs (the MFMA chain), 16
  // chunk sums, then the groups of 16 chunks.  One chain over N N = 16,384 terms has about ten times
  // the rounding error of a blocked GEMM; this grouping has no more than one (DESIGN.md "ControlGBDQ").
  Acc acc, mid, tot;
  acc_zero(acc);
  acc_zero(mid);
  acc_zero(tot);
  stage(0, lb);
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    float* xs = lb + (c & 1) * (kCgEnvs * kCgXS);
    if (c + 1 < chunks) stage(c + 1, lb + ((c + 1) & 1) * (kCgEnvs * kCgXS));
    const int kg0 = c * (kCgChunk / 16);
    const int kgs = KG1 - kg0 < kCgChunk / 16 ? KG1 - kg0 : kCgChunk / 16;
    mac_groups(acc, image + L.w1, KG1, kg0, kgs, 16, wave, xs, kCgXS, lane);
    acc_add(mid, acc);
    acc_zero(acc);
    if ((c & 15) == 15) {
      acc_add(tot, mid);
      acc_zero(mid);
    }
    __syncthreads();
  }
  acc_add(tot, mid);
  store_tiles<true>(tot, image + L.b1, 16, wave, la, kCgHS, lane);
  __syncthreads();

  acc_zero(acc);
  mac_groups(acc, image + L.w2, kCgHidden / 16, 0, kCgHidden / 16, 16, wave, la, kCgHS, lane);
  store_tiles<true>(acc, image + L.b2, 16, wave, lb, kCgHS, lane);
  __syncthreads();

  acc_zero(acc);
  mac_groups(acc, image + L.w3, kCgHidden / 16, 0, kCgHidden / 16, 16, wave, lb, kCgHS, lane);
  store_tiles<true>(acc, image + L.b3, 16, wave, la, kCgHS, lane);
  __syncthreads();

  const int RT = L.HRp >> 4;
  for (int p = 0; p < RT; p += 16) {
    acc_zero(acc);
    mac_groups(acc, image + L.wh, kCgHidden / 16, 0, kCgHidden / 16, RT, p + wave, la, kCgHS, lane);
    store_tiles<false>(acc, image + L.bh, RT, p + wave, lb, L.OS, lane);
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kCgThreads) cgbdq_heads_kernel(CgLayout L, const float* __restrict__ front,
                                                                 const float* __restrict__ image,
                                                                 float* __restrict__ heads) {
  extern __shared__ float lds[];
  const int64_t e0 = (int64_t)blockIdx.x * kCgEnvs;
  tail_layers(L, front, e0, image, lds);
  const float* hd = lds + L.lds_b;
  const int HR = L.HR;
  float* out = heads + e0 * HR;
  for (int idx = threadIdx.x; idx < kCgEnvs * HR; idx += kCgThreads) {
    const int e = idx / HR;
    out[idx] = hd[e * L.OS + (idx - e * HR)];
  }
}

__global__ void __launch_bounds__(kCgThreads) cgbdq_flipmask_kernel(
    CgLayout L, const float* __restrict__ front, const float* __restrict__ image, int W, int64_t n, uint64_t seed,
    uint64_t step, const uint64_t* __restrict__ d_step, uint64_t env_offset, int uniform, uint64_t eps_u,
    const float* __restrict__ d_eps, const int32_t* __restrict__ ctrl, const uint32_t* __restrict__ state,
    uint32_t* __restrict__ flipmask, int32_t* __restrict__ actions) {
  extern __shared__ float lds[];
  const int64_t e0 = (int64_t)blockIdx.x * kCgEnvs;
  tail_layers(L, front, e0, image, lds);
  const float* hd = lds + L.lds_b;
  int* act = reinterpret_cast<int*>(lds + L.lds_a);     // [32][C]
  const int C = L.C;
  const uint64_t st = d_step ? *d_step : step;
  if (d_eps) {   // device epsilon (graph replays): clamped to [0, 1], NaN -> 0
    const float ef = fminf(fmaxf(*d_eps, 0.f), 1.f);
    eps_u = (uint64_t)floor((double)ef * 4294967296.0);
  }
  for (int idx = threadIdx.x; idx < kCgEnvs * C; idx += kCgThreads) {
    const int e = idx & (kCgEnvs - 1), k = idx >> 5;
    const uint64_t ge = env_offset + (uint64_t)(e0 + e);
    const pbn::Word4 r0 = pbn::draw(seed, ge, st, pbn::kStreamExplore, 0);
    int a;
    if ((uint64_t)r0.x < eps_u) {
      // "reference": np.random.randint(0, 1) = 0 for every control node; "uniform": branch k takes
      // EXPLORE word k + 1 (call (k + 1) >> 2), multiply-high onto {0, 1}
      a = 0;
      if (uniform) {
        const int wi = k + 1;
        const pbn::Word4 r = (wi >> 2) == 0 ? r0 : pbn::draw(seed, ge, st, pbn::kStreamExplore, (uint32_t)(wi >> 2));
        const uint32_t rw = (wi & 3) == 0 ? r.x : ((wi & 3) == 1 ? r.y : ((wi & 3) == 2 ? r.z : r.w));
        a = (int)__umulhi(rw, 2u);
      }
    } else {
      const float* h = hd + e * L.OS;
      const float v = h[0], a0 = h[1 + 2 * k], a1 = h[2 + 2 * k];
      const float mean = (a0 + a1) / 2.f;
      const float q0 = (v + a0) - mean, q1 = (v + a1) - mean;
      a = (!isnan(q0) && (isnan(q1) || q1 > q0)) ? 1 : 0;   // torch.argmax: first maximum, NaN is the maximum
    }
    if (actions) actions[(e0 + e) * C + k] = a;
    act[e * C + k] = a;
  }
  __syncthreads();
  if (threadIdx.x < kCgEnvs) {
    const int e = threadIdx.x;
    uint32_t vw[4] = {0u, 0u, 0u, 0u}, cw[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < C; ++k) {
      const int c = ctrl[k];
      if (c < 0 || c >= L.N) continue;   // no such node: the head and its action stay, no bit is set
      const uint32_t bit = 1u << (c & 31), on = act[e * C + k] ? bit : 0u;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (w == (c >> 5)) {
          cw[w] |= bit;
          vw[w] |= on;
        }
    }
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if (w < W) flipmask[(size_t)w * n + e0 + e] = (state[(size_t)w * n + e0 + e] ^ vw[w]) & cw[w];
  }
}

int launch_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PBN_OK : pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
}

int ctrl_error(int32_t n_ctrl) {
  if (n_ctrl < 1 || n_ctrl > pbn::kCgMaxCtrl) return pbn::set_error(PBN_EINVAL, "n_ctrl must be 1..128");
  return PBN_OK;
}

// the checks both layer entry points share; *lds = the block's dynamic LDS bytes, raised for `kernel`
int tail_args(const pbn::NetView& v, int64_t n_envs, const float* d_front, const float* d_image, int32_t n_ctrl,
              const void* kernel, bool* raised, size_t* lds) {
  if (n_envs < 0 || (n_envs & 31)) return pbn::set_error(PBN_EINVAL, "n_envs must be a non-negative multiple of 32");
  if (v.n_nodes > 128) return pbn::set_error(PBN_EINVAL, "the tail kernel takes at most 128 nodes");
  if (n_envs * v.n_nodes * v.n_nodes >= ((int64_t)1 << 31)) return pbn::set_error(PBN_EINVAL, "n_envs too large");
  if (int rc = ctrl_error(n_ctrl)) return rc;
  if (n_envs == 0) return PBN_OK;
  if (!d_front || !d_image) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_front, 4) || !pbn::aligned(d_image, 16))
    return pbn::set_error(PBN_EINVAL, "d_image must be 16-byte, d_front 4-byte aligned");
  *lds = (size_t)pbn::cg_layout(v.n_nodes, n_ctrl).lds_floats * sizeof(float);   // above the default 64 KiB limit
  const int dv = v.device >= 0 && v.device < 64 ? v.device : 0;
  if (!raised[dv]) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, pbn::kCgMaxLds) != hipSuccess)
      return pbn::set_error(PBN_EDEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    raised[dv] = true;
  }
  return PBN_OK;
}

}  // namespace

int pbn_cgbdq_image_floats(const pbn_net* net, int32_t n_ctrl, int64_t* n_floats) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if ((rc = ctrl_error(n_ctrl))) return rc;
  if (!n_floats) return pbn::set_error(PBN_EINVAL, "a non-null n_floats");
  *n_floats = pbn::cg_layout(v.n_nodes, n_ctrl).floats;
  return PBN_OK;
}

int pbn_cgbdq_pack(const pbn_net* net, const float* d_tail, int32_t n_ctrl, float* d_image, void* stream) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if ((rc = pbn::check_device(net))) return rc;
  if ((rc = ctrl_error(n_ctrl))) return rc;
  if (!d_tail || !d_image) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_tail, 4) || !pbn::aligned(d_image, 16))
    return pbn::set_error(PBN_EINVAL, "d_image must be 16-byte, d_tail 4-byte aligned");
  hipLaunchKernelGGL(cgbdq_pack_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, pbn::cg_layout(v.n_nodes, n_ctrl),
                     pbn::cg_tail(v.n_nodes), d_tail, d_image);
  return launch_error();
}

int pbn_cgbdq_heads(const pbn_net* net, int64_t n_envs, const float* d_front, const float* d_image, int32_t n_ctrl,
                    float* d_heads, void* stream) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if ((rc = pbn::check_device(net))) return rc;
  static bool raised[64] = {};   // per device (a pbn_net is bound to one)
  size_t lds = 0;
  if ((rc = tail_args(v, n_envs, d_front, d_image, n_ctrl, reinterpret_cast<const void*>(cgbdq_heads_kernel), raised, &lds)))
    return rc;
  if (n_envs == 0) return PBN_OK;
  if (!d_heads || !pbn::aligned(d_heads, 4)) return pbn::set_error(PBN_EINVAL, "d_heads must be non-null and 4-byte aligned");
  hipLaunchKernelGGL(cgbdq_heads_kernel, dim3((unsigned)(n_envs / kCgEnvs)), dim3(kCgThreads), lds, (hipStream_t)stream,
                     pbn::cg_layout(v.n_nodes, n_ctrl), d_front, d_image, d_heads);
  return launch_error();
}

int pbn_cgbdq_flipmask(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step, uint64_t env_offset,
                       int64_t n_envs, const float* d_front, const float* d_image, int32_t n_ctrl,
                       const int32_t* d_ctrl_nodes, int32_t explore_mode, float epsilon, const float* d_epsilon,
                       const uint32_t* d_state, uint32_t* d_flipmask, int32_t* d_actions, void* stream) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if ((rc = pbn::check_device(net))) return rc;
  if (env_offset & 31) return pbn::set_error(PBN_EINVAL, "env_offset must be a multiple of 32");
  if (explore_mode != 0 && explore_mode != 1) return pbn::set_error(PBN_EINVAL, "explore_mode must be 0 (reference) or 1 (uniform)");
  if (const char* msg = pbn::explore_args_error(epsilon, d_step, d_epsilon)) return pbn::set_error(PBN_EINVAL, msg);
  static bool raised[64] = {};
  size_t lds = 0;
  if ((rc = tail_args(v, n_envs, d_front, d_image, n_ctrl, reinterpret_cast<const void*>(cgbdq_flipmask_kernel), raised, &lds)))
    return rc;
  if (n_envs == 0) return PBN_OK;
  if (!d_ctrl_nodes || !d_state || !d_flipmask) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_ctrl_nodes, 4) || !pbn::aligned(d_state, 4) || !pbn::aligned(d_flipmask, 4) || !pbn::aligned(d_actions, 4))
    return pbn::set_error(PBN_EINVAL, "d_ctrl_nodes, d_state, d_flipmask and d_actions must be 4-byte aligned");
  hipLaunchKernelGGL(cgbdq_flipmask_kernel, dim3((unsigned)(n_envs / kCgEnvs)), dim3(kCgThreads), lds, (hipStream_t)stream,
                     pbn::cg_layout(v.n_nodes, n_ctrl), d_front, d_image, v.W, n_envs, seed, step, d_step, env_offset,
                     (int)explore_mode, pbn::explore_threshold(epsilon), d_epsilon, d_ctrl_nodes, d_state, d_flipmask,
                     d_actions);
  return launch_error();
}
