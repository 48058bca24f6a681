// pbn_env.hip -- MI355X (gfx950) batched PBN environment: kernels + C-ABI.
//
// Replaces the per-env, per-node Python step of the external gym_PBN package
// that the reference calls once per frame (bdq_model/__init__.py:177); the ABI
// is include/pbn_env.h, the semantics DESIGN.md "Step semantics".
//
// Layout: one thread owns 32 consecutive envs ("a group") and works on them
// bit-sliced: after a 32x32 transpose, VGPR/LDS word i of the thread holds
// node i of all 32 envs, so one 32-bit VALU op evaluates one boolean
// operation for 32 envs.  A wave covers 2048 envs.  Per-env scalar work
// (interventions, perturbation, reward, reset) runs on the per-env words.
//
// Per node the S planes (current state, bit-sliced) are read from LDS by
// uniform input index; each function is a 4-level mux tree over its (<= 4)
// input planes with 16 precomputed leaf masks held in SGPRs; the selected
// function is chosen by comparing the prob_bits-bit uniform (bit-sliced digit
// planes straight out of Philox) against the node's cumulative thresholds.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pbn_env.h"
#include "bitslice.h"
#include "host_check.h"
#include "net_image.h"
#include "net_view.h"
#include "philox.h"

#include "step_kernels.h"

namespace pbn {
// pbn_settle.hip: pbn_step_wave<W, B, 3> (lean = 0, pbn_step) or <W, B, 4> (lean = 1,
// pbn_rollout) under the settle law, as an untyped host stub pointer (nullptr: no such W, B)
void* settle_kernel(int W, int B, int lean);
// pbn_settle.hip: pbn_rollout_settle<W, B> (pbn_rollout under the settle law, pipelined)
void* settle_pipe_kernel(int W, int B);
// pbn_settle.hip: pbn_step_wave<W, B, 4, PolicyArgs> (pbn_rollout_dqn under the settle law)
void* settle_dqn_kernel(int W, int B);
}  // namespace pbn

namespace {

// ---------------------------------------------------------------- host side
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_OK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(PBN_EDEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

// a device allocation, freed with its owner
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)hipFree(p_); }
  // allocates count elements (at least one byte) and fills them from src, if given
  template <typename T>
  int upload(const T* src, size_t count) {
    const size_t bytes = count * sizeof(T);
    HIP_OK(hipMalloc(&p_, std::max<size_t>(bytes, 1)));
    if (src && bytes) HIP_OK(hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice));
    return PBN_OK;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p_); }

 private:
  void* p_ = nullptr;
};

// many: some node has more than kNodeRecs functions (the instance that carries those chains)
StepFn pick_pipe(int W, int B, bool many) {
  return for_state_words(W, [&](auto w) {
    constexpr int kW = decltype(w)::value;
    return many ? for_prob_bits(B, [](auto b) -> StepFn { return pbn_rollout_pipe<kW, decltype(b)::value, true>; })
                : for_prob_bits(B, [](auto b) -> StepFn { return pbn_rollout_pipe<kW, decltype(b)::value, false>; });
  });
}

using ResetFn = void (*)(const int32_t*, const uint32_t*, int, int, int, uint32_t, uint64_t, uint64_t, uint64_t,
                         int64_t, uint32_t*, uint8_t*, uint8_t*);
ResetFn pick_reset(int W) {
  switch (W) {
    case 1: return pbn_reset_kernel<1>;
    case 2: return pbn_reset_kernel<2>;
    case 3: return pbn_reset_kernel<3>;
    case 4: return pbn_reset_kernel<4>;
  }
  return nullptr;
}

}  // namespace

struct pbn_net {
  StepArgs base{};   // the launch arguments fixed at create (fill_args adds the key and the env range)
  DevBuf tab, att_start, att_states, att_first, fcompact, nrec, sthr, sthr_pk;
  StepFn kernels[kNumKernels] = {};   // nullptr: no instance for this net
  PolicyFn dqn_kernel = nullptr;      // pbn_rollout_dqn: pbn_step_wave<.., PolicyArgs> under the net's step law
  ResetFn reset = nullptr;
  RouteNet route{};
  int device = 0;
  int n_cus = 256;   // compute units of the device (the pipelined rollout's priority choice)
  int W = 0;
  int slot_words_settle = 0;   // StepArgs::slot_words of pbn_rollout_settle
};

namespace pbn {

int set_error(int code, const char* msg) { return fail(code, msg); }

int net_view(const pbn_net* net, NetView* v) {
  if (!net || !v) return fail(PBN_EINVAL, "null net");
  v->device = net->device;
  v->n_nodes = net->base.n_nodes;
  v->W = net->W;
  v->n_attr = net->base.n_attr;
  v->n_states = net->base.n_states;
  v->att_start = net->base.att_start;
  v->att_states = net->base.att_states;
  v->att_first = net->att_first.as<uint32_t>();
  // the image is cdf [cdf_len] | reward rows [4 (N + 1)] | hash | ..., as the step kernels carve it
  v->att_hash = net->base.tab + net->base.cdf_len + 4 * (net->base.n_nodes + 1);
  v->hash_bits = net->base.hash_bits;
  v->hash_probes = net->base.hash_probes;
  memcpy(v->hash_mult, net->base.hash_mult, sizeof v->hash_mult);
  return PBN_OK;
}

int check_device(const pbn_net* net) {
  if (!net) return fail(PBN_EINVAL, "null net");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != net->device)
    return fail(PBN_EDEVICE, "current device differs from the net's device");
  return PBN_OK;
}

}  // namespace pbn

namespace {

int upload_image(const pbn::NetImage& im, const pbn_net_desc* d, pbn_net* net) {
  const int A = im.n_attr, S = im.n_states;
  int rc;
  if ((rc = net->fcompact.upload(im.fcompact.data(), im.fcompact.size())) ||
      (rc = net->nrec.upload(im.nrec.data(), im.nrec.size())) ||
      (rc = net->sthr.upload(im.sthr.data(), im.sthr.size())) ||
      (rc = net->sthr_pk.upload(im.sthr_pk.data(), im.sthr_pk.size())) ||
      (rc = net->tab.upload(im.tab.data(), im.tab.size())) ||
      (rc = net->att_start.upload(A ? d->attractor_start : nullptr, (size_t)A + 1)) ||
      (rc = net->att_states.upload(S ? d->attractor_states : nullptr, (size_t)S * im.W)) ||
      (rc = net->att_first.upload(A ? im.att_first.data() : nullptr, im.att_first.size())))
    return rc;
  return PBN_OK;
}

void set_base(const pbn::NetImage& im, pbn_net* net) {
  StepArgs& a = net->base;
  a.tab = net->tab.as<uint32_t>();
  a.att_start = net->att_start.as<int32_t>();
  a.att_states = net->att_states.as<uint32_t>();
  a.fcompact = net->fcompact.as<uint4>();
  a.nrec = net->nrec.as<uint4>();
  a.sthr = net->sthr.as<uint32_t>();
  a.sthr_pk = net->sthr_pk.as<uint32_t>();
  a.n_steps = 1;
  a.n_nodes = im.n_nodes;
  a.n_attr = im.n_attr;
  a.horizon = im.horizon;
  a.cdf_len = im.cdf_len;
  a.hash_bits = im.n_attr ? im.hash_bits : 0;
  a.hash_probes = im.hash_probes;
  memcpy(a.hash_mult, im.hash_mult, sizeof a.hash_mult);
  a.tab_words = im.tab_words;
  a.prob_bits = im.prob_bits;
  a.n_funcs = im.n_funcs;
  a.wave_words = im.wave_words;
  a.gap_exact = im.gap_exact;
  a.gap_lut_off = im.gap_lut_off;
  a.gap_shift = im.gap_shift;
  a.gap_nb = im.gap_nb;
  a.inv_log2q = im.inv_log2q;
  a.n_states = im.n_states;
  a.att_off = im.att_off;
  a.sel_off = im.sel_off;
  a.nrec_off = im.nrec_off;
  a.cm_off = im.cm_off;
  a.n_cls = im.n_cls;
  memcpy(a.uthr, im.uthr, sizeof a.uthr);
  a.max_nf = im.max_nf;
  a.lq = im.lq;
  a.slot_words = im.slot_words;
  a.gate_off = im.gate_off;
  a.glayer_off = im.glayer_off;
  a.n_glayers = im.n_glayers;
  a.att_single = im.att_single;
  a.n1_magic = im.n1_magic;
  a.am1_magic = im.am1_magic;
  a.x_mult = im.x_mult;
  a.settle_max = im.settle_max;
  a.settle_pk = im.settle_pk;
}

// the kernel instances of the net's (W, B), and what route_launch chooses among them by
void pick_kernels(const pbn::NetImage& im, pbn_net* net) {
  const int W = im.W, B = im.prob_bits;
  const bool many = im.max_nf > kNodeRecs;
  net->kernels[kWave1] = step_kernel_for(W, B, [](auto w, auto b) -> StepFn {
    return pbn_step_wave<decltype(w)::value, decltype(b)::value, 1>;
  });
  net->kernels[kWaveLean] = step_kernel_for(W, B, [](auto w, auto b) -> StepFn {
    return pbn_step_wave<decltype(w)::value, decltype(b)::value, 2>;
  });
  net->kernels[kWaveSettle] = reinterpret_cast<StepFn>(pbn::settle_kernel(W, B, 0));
  net->kernels[kWaveSettleLean] = reinterpret_cast<StepFn>(pbn::settle_kernel(W, B, 1));
  net->kernels[kPipe] = pick_pipe(W, B, many);
  if (!many) net->kernels[kPipeSettle] = reinterpret_cast<StepFn>(pbn::settle_pipe_kernel(W, B));
  net->dqn_kernel = im.settle_max >= 2
                        ? reinterpret_cast<PolicyFn>(pbn::settle_dqn_kernel(W, B))
                        : step_kernel_for(W, B, [](auto w, auto b) -> PolicyFn {
                            return pbn_step_wave<decltype(w)::value, decltype(b)::value, 2, PolicyArgs>;
                          });
  net->reset = pick_reset(W);
  net->W = W;
  net->slot_words_settle = im.slot_words_settle;
  net->route.settle = im.settle_max >= 2;
  net->route.n_gates = im.n_gates;
  net->route.has_pipe_settle = net->kernels[kPipeSettle] != nullptr;
  net->route.lds_wave = im.lds_wave;
  net->route.lds_pipe = im.lds_pipe;
  net->route.lds_settle = im.lds_settle;
  if (const char* env = getenv("PBN_ROLL")) {
    if (!strcmp(env, "lean")) net->route.force_roll = 2;
    if (!strcmp(env, "pipe")) net->route.force_roll = 3;
  }
}

// lets every kernel the net can run ask for its LDS
int raise_lds_limits(const pbn_net& net) {
  for (int k = 0; k < kNumKernels; ++k) {
    const size_t bytes = kernel_lds_bytes(net.route, (Kernel)k);
    if (!net.kernels[k] || bytes > kLdsDeviceBytes) continue;   // unusable for this net: route_launch never picks it
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(net.kernels[k]),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
      return fail(PBN_EDEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  }
  if (net.dqn_kernel && net.route.lds_wave <= kLdsDeviceBytes &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(net.dqn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)net.route.lds_wave) != hipSuccess)
    return fail(PBN_EDEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  return PBN_OK;
}

}  // namespace

extern "C" {

const char* pbn_last_error(void) { return g_err.c_str(); }

int pbn_state_histogram(const uint32_t* d_states, int64_t n_rows, int64_t n_cols, int64_t row_stride,
                        int32_t n_bits, uint32_t* d_hist, void* stream) {
  if (n_rows < 0 || n_cols < 0 || row_stride < n_cols) return fail(PBN_EINVAL, "bad histogram shape");
  if (n_bits < 1 || n_bits > 32) return fail(PBN_EINVAL, "n_bits must be 1..32");
  if (n_rows == 0 || n_cols == 0) return PBN_OK;
  if (!d_states || !d_hist) return fail(PBN_EINVAL, "null buffer");
  const uint32_t mask = n_bits == 32 ? 0xFFFFFFFFu : ((1u << n_bits) - 1u);
  const int64_t total = n_rows * n_cols;
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(pbn_hist_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_states, n_rows, n_cols,
                     row_stride, mask, d_hist);
  HIP_OK(hipGetLastError());
  return PBN_OK;
}
int pbn_abi_version(void) { return PBN_ABI_VERSION; }

int pbn_host_buffer(int64_t bytes, void** h_ptr, void** d_ptr) {
  if (bytes <= 0 || !h_ptr || !d_ptr) return fail(PBN_EINVAL, "bytes <= 0 or null out pointer");
  *h_ptr = nullptr;
  *d_ptr = nullptr;
  void* h = nullptr;
  if (hipHostMalloc(&h, (size_t)bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || !h)
    return fail(PBN_ENOMEM, "hipHostMalloc failed");
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || !d) {
    (void)hipHostFree(h);
    return fail(PBN_EDEVICE, "hipHostGetDevicePointer failed");
  }
  memset(h, 0, (size_t)bytes);
  *h_ptr = h;
  *d_ptr = d;
  return PBN_OK;
}

int pbn_host_buffer_free(void* h_ptr) {
  if (!h_ptr) return PBN_OK;
  HIP_OK(hipHostFree(h_ptr));
  return PBN_OK;
}

int pbn_stream_sync(void* stream) {
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  return PBN_OK;
}

// pbn_copy_async: a grid-stride copy in 16-byte non-temporal vectors (the records are read once and
// go to the learner: neither side should displace the rollout's table image from L2), four
// independent vectors in flight per thread
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) pbn_copy_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ src,
                                                       int64_t n16) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(src + i + u * stride);
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(v[u], dst + i + u * stride);
  }
  for (; i < n16; i += stride) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

int pbn_copy_async(void* d_dst, const void* d_src, int64_t bytes, void* stream) {
  if (bytes < 0) return fail(PBN_EINVAL, "bytes < 0");
  if (bytes == 0) return PBN_OK;
  if (!d_dst || !d_src) return fail(PBN_EINVAL, "null buffer");
  if ((bytes & 15) || !pbn::aligned(d_dst, 16) || !pbn::aligned(d_src, 16))
    return fail(PBN_EINVAL, "pointers and bytes must be 16-byte aligned");
  const char* d = static_cast<const char*>(d_dst);
  const char* s = static_cast<const char*>(d_src);
  if (d < s + bytes && s < d + bytes) return fail(PBN_EINVAL, "overlapping ranges");
  const int64_t n16 = bytes / 16;
  int dev = 0, n_cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev);
  // 8 blocks per CU at most, each thread moving 4 vectors per trip (the last hand-off of a run, on
  // the launch stream: the most blocks that still stream full 1-KB rows per wave)
  constexpr int64_t kCopyBlocksPerCu = 8;
  const int64_t want = (n16 + 4 * 256 - 1) / (4 * 256);
  const unsigned blocks =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)n_cus * kCopyBlocksPerCu));
  hipLaunchKernelGGL(pbn_copy_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, static_cast<u32x4*>(d_dst),
                     static_cast<const u32x4*>(d_src), n16);
  HIP_OK(hipGetLastError());
  return PBN_OK;
}

int pbn_net_words(const pbn_net* net) { return net ? net->W : PBN_EINVAL; }

int pbn_net_create(const pbn_net_desc* d, pbn_net** out) {
  if (!d || !out) return fail(PBN_EINVAL, "null descriptor/out");
  *out = nullptr;
  pbn::NetImage im;
  std::string err;
  int rc = pbn::compile_net(d, &im, &err);
  if (rc) return fail(rc, err);
  auto net = std::make_unique<pbn_net>();
  if (hipGetDevice(&net->device) != hipSuccess) return fail(PBN_EDEVICE, "no HIP device");
  if (hipDeviceGetAttribute(&net->n_cus, hipDeviceAttributeMultiprocessorCount, net->device) != hipSuccess ||
      net->n_cus <= 0)
    net->n_cus = 256;
  if ((rc = upload_image(im, d, net.get()))) return rc;
  set_base(im, net.get());
  pick_kernels(im, net.get());
  if ((rc = raise_lds_limits(*net))) return rc;
  if (net->route.lds_wave > kLdsDeviceBytes) return fail(PBN_EINVAL, "LDS budget exceeded");
  *out = net.release();
  return PBN_OK;
}

#ifdef PBN_STAMPS
static unsigned long long* g_stamps = nullptr;
int pbn_debug_set_stamps(unsigned long long* d_buf) {
  g_stamps = d_buf;
  return 0;
}
#endif

int pbn_net_destroy(pbn_net* net) {
  delete net;
  return PBN_OK;
}

// ragged: n_envs may be any count (pbn_step: the last 32-env group is partial); env_offset is
// always a multiple of 32 (the groups' RNG keys)
static int check_common(pbn_net* net, uint64_t env_offset, int64_t n_envs, bool ragged = false) {
  if (!net) return fail(PBN_EINVAL, "null net");
  if (n_envs < 0) return fail(PBN_EINVAL, "n_envs < 0");
  if (ragged ? (env_offset & 31) != 0 : ((n_envs & 31) || (env_offset & 31)))
    return fail(PBN_EINVAL, ragged ? "env_offset must be a multiple of 32"
                                   : "n_envs and env_offset must be multiples of 32");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != net->device)
    return fail(PBN_EDEVICE, "current device differs from the net's device");
  return PBN_OK;
}

// The launch arguments every step kernel shares: the net's tables and encodings, the key and
// the env range (the caller adds its buffers, mode and step count)
static void fill_args(const pbn_net* net, StepArgs* a, uint64_t seed, uint64_t step, uint64_t env_offset,
                      int64_t n_envs) {
  *a = net->base;
  a->seed = seed;
  a->step = step;
  a->env_offset = env_offset;
  a->n_envs = n_envs;
  a->n_groups = (n_envs + 31) / 32;
#ifdef PBN_STAMPS
  a->stamps = g_stamps;
#endif
}

// one launch of the kernel r names over a's groups
static int launch(const pbn_net* net, const Route& r, StepArgs a, int threads, void* stream) {
  if (r.kernel == kPipeSettle) a.slot_words = net->slot_words_settle;
  const unsigned blocks = (unsigned)((a.n_groups + r.groups_per_block - 1) / r.groups_per_block);
  hipLaunchKernelGGL(net->kernels[r.kernel], dim3(blocks), dim3(threads), r.lds_bytes, (hipStream_t)stream, a);
  HIP_OK(hipGetLastError());
  return PBN_OK;
}

int pbn_reset(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
              uint32_t* d_state, uint8_t* d_target, uint8_t* d_t, void* stream) {
  int rc = check_common(net, env_offset, n_envs, true);
  if (rc) return rc;
  if (n_envs == 0) return PBN_OK;
  if (!d_state || !d_target || !d_t) return fail(PBN_EINVAL, "null buffer");
  const int threads = 256;
  const unsigned blocks = (unsigned)((n_envs + threads - 1) / threads);
  const StepArgs& b = net->base;
  hipLaunchKernelGGL(net->reset, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, b.att_start, b.att_states,
                     b.n_attr, b.n_states, b.n_nodes, b.am1_magic, seed, step, env_offset, n_envs, d_state, d_target,
                     d_t);
  HIP_OK(hipGetLastError());
  return PBN_OK;
}

static int step_impl(pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step, uint64_t env_offset,
                     int64_t n_envs, uint32_t mode, const uint32_t* d_state, uint32_t* d_flipmask,
                     uint8_t* d_target, uint8_t* d_t, uint32_t* d_state_out, uint32_t* d_final_state,
                     float* d_reward, uint8_t* d_flags, void* stream, const pbn_ring_store* ring = nullptr) {
  int rc = check_common(net, env_offset, n_envs, true);
  if (rc) return rc;
  if (n_envs == 0) return PBN_OK;
  if (mode & ~(PBN_MODE_AUTORESET | PBN_MODE_RANDOM_ACTIONS)) return fail(PBN_EINVAL, "unknown mode bits");
  if (!d_state || !d_flipmask || !d_target || !d_t || !d_state_out || !d_reward || !d_flags)
    return fail(PBN_EINVAL, "null buffer");
  // (the ring form steps in place: the wave kernel's lane reads its env's state once, at entry)
  if (d_state_out == d_state && !ring) return fail(PBN_EINVAL, "d_state_out must not alias d_state");
  for (const void* p : {(const void*)d_state, (const void*)d_flipmask, (const void*)d_target, (const void*)d_t,
                        (const void*)d_state_out, (const void*)d_reward, (const void*)d_flags,
                        (const void*)d_final_state})   // (d_final_state may be null)
    if (!pbn::aligned(p, 16)) return fail(PBN_EINVAL, "device buffers must be 16-byte aligned");
  StepArgs a;
  fill_args(net, &a, seed, step, env_offset, n_envs);
  a.step_ptr = d_step;
  a.state = d_state;
  a.state_out = d_state_out;
  a.flipmask = d_flipmask;
  a.target = d_target;
  a.t = d_t;
  a.final_state = d_final_state;
  a.reward = d_reward;
  a.flags = d_flags;
  a.mode = (int)mode;
  if (ring) {
    const pbn_ring_store& r = *ring;
    if (net->route.settle) return fail(PBN_EINVAL, "pbn_step_dev_store: the one-update law only (settle_max < 2)");
    if (r.capacity < n_envs) return fail(PBN_EINVAL, "pbn_ring_store: capacity < n_envs");
    if (r.n_branches < 1 || r.n_branches > kRingMaxK) return fail(PBN_EINVAL, "pbn_ring_store: n_branches 1..8");
    if (!r.d_pos || !pbn::aligned(r.d_pos, 8) || !r.d_state || !r.d_next_state || !r.d_target || !r.d_reward ||
        !r.d_done || !r.d_action || !r.d_actions_in)
      return fail(PBN_EINVAL, "pbn_ring_store: null or misaligned buffer");
    a.r_state = r.d_state;
    a.r_next = r.d_next_state;
    a.r_target = r.d_target;
    a.r_action = r.d_action;
    a.r_reward = r.d_reward;
    a.r_done = r.d_done;
    a.r_act_in = r.d_actions_in;
    a.r_done_out = r.d_done_out;
    a.r_pos = r.d_pos;
    a.r_cap = r.capacity;
    a.r_k = r.n_branches;
    a.r_done_mask = r.done_mask;
  }
  // the settle law on whole groups: a one-step launch of the pipelined settle kernel
  // (pbn_rollout_settle; its env-major outputs of one step are pbn_step's), where every env runs
  // its own update sequence and an update is one pipeline iteration, against the wave kernel's
  // variant 3, whose wave runs every update of its slowest env as a serial chain (VERDICT r05
  // next 2).  Ragged env counts, gates, PBN_ROLL=lean: the wave kernel.
  const Route r = route_launch(net->route, false, !(n_envs & 31));
  return launch(net, r, a, r.threads, stream);
}

int pbn_step(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs, uint32_t mode,
             const uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target, uint8_t* d_t,
             uint32_t* d_state_out, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
             void* stream) {
  return step_impl(net, seed, step, nullptr, env_offset, n_envs, mode, d_state, d_flipmask, d_target, d_t,
                   d_state_out, d_final_state, d_reward, d_flags, stream);
}

int pbn_step_dev(pbn_net* net, uint64_t seed, const uint64_t* d_step, uint64_t env_offset, int64_t n_envs,
                 uint32_t mode, const uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target, uint8_t* d_t,
                 uint32_t* d_state_out, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                 void* stream) {
  if (const char* msg = pbn::dev_scalars_error(d_step, nullptr, true)) return fail(PBN_EINVAL, msg);
  return step_impl(net, seed, 0, d_step, env_offset, n_envs, mode, d_state, d_flipmask, d_target, d_t,
                   d_state_out, d_final_state, d_reward, d_flags, stream);
}

int pbn_step_dev_store(pbn_net* net, uint64_t seed, const uint64_t* d_step, uint64_t env_offset, int64_t n_envs,
                       uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target, uint8_t* d_t,
                       uint32_t* d_final_state, float* d_reward, uint8_t* d_flags, const pbn_ring_store* ring,
                       void* stream) {
  if (const char* msg = pbn::dev_scalars_error(d_step, nullptr, true)) return fail(PBN_EINVAL, msg);
  if (!ring) return fail(PBN_EINVAL, "null ring");
  return step_impl(net, seed, 0, d_step, env_offset, n_envs, mode, d_state, d_flipmask, d_target, d_t, d_state,
                   d_final_state, d_reward, d_flags, stream, ring);
}

int pbn_rollout(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                int32_t n_steps, uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
                uint8_t* d_t, uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                void* stream) {
  return pbn_rollout_ex(net, seed, step, env_offset, n_envs, n_steps, mode, d_state, d_flipmask, d_target, d_t,
                        d_obs, d_final_state, d_reward, d_flags, nullptr, stream);
}

}  // extern "C"


// pbn_rollout_ex, with (cp_bytes > 0) a copy riding along (pbn_rollout_copy): a fourth wave per
// block of the pipelined one-update kernel, else pbn_copy_async right after the launch on the
// same stream
static int rollout_impl(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                        int32_t n_steps, uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
                        uint8_t* d_t, uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                        uint16_t* d_updates, void* cp_dst, const void* cp_src, int64_t cp_bytes, void* stream) {
  int rc = check_common(net, env_offset, n_envs);
  if (rc) return rc;
  if (n_steps < 0) return fail(PBN_EINVAL, "n_steps < 0");
  // a lane's byte offset into one output row is 32 bits wide (step_debug.h LANE_AT, StepRows)
  if (n_envs >= ((int64_t)1 << 30)) return fail(PBN_EINVAL, "n_envs must be below 2^30");
  bool copy_after = cp_bytes > 0;   // cleared when the copy rides along the launch
  struct After {   // the standalone copy, if it is still owed when the launch has been issued
    bool& owed;
    void *dst, *stream;
    const void* src;
    int64_t bytes;
    int finish(int r) { return (r == PBN_OK && owed) ? pbn_copy_async(dst, src, bytes, stream) : r; }
  } after{copy_after, cp_dst, stream, cp_src, cp_bytes};
  if (n_envs == 0 || n_steps == 0) return after.finish(PBN_OK);
  if (mode & ~(PBN_MODE_AUTORESET | PBN_MODE_RANDOM_ACTIONS)) return fail(PBN_EINVAL, "unknown mode bits");
  if (!d_state || !d_flipmask || !d_target || !d_t || !d_reward || !d_flags) return fail(PBN_EINVAL, "null buffer");
  StepArgs a;
  fill_args(net, &a, seed, step, env_offset, n_envs);
  a.state = d_state;
  a.state_out = d_state;   // in place: every env is read and written by one lane only
  a.flipmask = d_flipmask;
  a.target = d_target;
  a.t = d_t;
  a.final_state = d_final_state;
  a.obs = d_obs;
  a.reward = d_reward;
  a.flags = d_flags;
  a.n_steps = n_steps;
  a.mode = (int)mode;
  a.updates = d_updates;
  // the pipelined kernels for every network they support (they beat the one-wave-per-group
  // rollout at every measured size: profiles/r01_sweep_pbn28_variants_v4.jsonl); networks
  // with gates (lowered wide functions) run the wave kernel.  PBN_ROLL=lean|pipe forces one (pipe:
  // up to the LDS of a CU, route_launch).
  const Route r = route_launch(net->route, true, true);
  int threads = r.threads;
  if (r.kernel == kPipe) {
    // the one-update law applies exactly one synchronous update per env-step
    if (d_updates) HIP_OK(hipMemsetD16Async(d_updates, 1, (size_t)n_steps * (size_t)n_envs, (hipStream_t)stream));
    const int64_t pblocks = (a.n_groups + 1) / 2;
    a.sel_prio = pblocks <= 4 * (int64_t)net->n_cus ? 1 : 0;
    if (cp_bytes > 0) {   // the ride-along copy: a fourth wave per block
      a.cp_src = cp_src;
      a.cp_dst = cp_dst;
      a.cp_n16 = cp_bytes / 16;
      // paced at U vectors per lane and iteration when the grid's barriers cover the copy with
      // U <= 4 (one hand-off of this launch's own records: 12 W + 5 bytes per env-step, 64 envs
      // per block, U = 2 for single-word states), else one burst
      const int64_t slots = (int64_t)(n_steps + 1) * pblocks * 64;
      const int64_t u = (a.cp_n16 + slots - 1) / slots;
      a.cp_u = u <= 1 ? 1 : (u <= 2 ? 2 : (u <= 4 ? 4 : 0));
      // a grid of more blocks than run at once: the burst, whose wave exits early, where the paced
      // wave held a block slot for the whole launch (1M envs: 0.69 -> 0.74x of the bare launches'
      // rate, pbn70 x 1M: 0.65 -> 0.73x; profiles/r05_zj_ab.json)
      if (pblocks > 4 * (int64_t)net->n_cus) a.cp_u = 0;
      copy_after = false;
      threads += 64;
    }
  }
  return after.finish(launch(net, r, a, threads, stream));
}

extern "C" {

int pbn_rollout_ex(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                   int32_t n_steps, uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
                   uint8_t* d_t, uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                   uint16_t* d_updates, void* stream) {
  return rollout_impl(net, seed, step, env_offset, n_envs, n_steps, mode, d_state, d_flipmask, d_target, d_t, d_obs,
                      d_final_state, d_reward, d_flags, d_updates, nullptr, nullptr, 0, stream);
}

int pbn_rollout_dqn(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                    int32_t n_steps, uint32_t mode, uint32_t* d_state, uint8_t* d_target, uint8_t* d_t, int32_t h0,
                    int32_t h1, const float* d_image, float epsilon, uint32_t* d_flipmask, int32_t* d_actions,
                    uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                    uint16_t* d_updates, void* stream) {
  // every argument error before any device call, those that need no net first
  if (mode & ~(PBN_MODE_AUTORESET | PBN_MODE_RANDOM_ACTIONS)) return fail(PBN_EINVAL, "unknown mode bits");
  if (mode & PBN_MODE_RANDOM_ACTIONS)
    return fail(PBN_EINVAL, "pbn_rollout_dqn: the policy chooses the actions (mode takes PBN_MODE_AUTORESET only)");
  if (n_steps < 0) return fail(PBN_EINVAL, "n_steps < 0");
  if (n_envs < 0) return fail(PBN_EINVAL, "n_envs < 0");
  if ((n_envs & 31) || (env_offset & 31)) return fail(PBN_EINVAL, "n_envs and env_offset must be multiples of 32");
  if (n_envs >= ((int64_t)1 << 30)) return fail(PBN_EINVAL, "n_envs must be below 2^30");
  if (const char* msg = shape_error(1, h0, h1)) return fail(PBN_EINVAL, msg);
  if (const char* msg = pbn::explore_args_error(epsilon)) return fail(PBN_EINVAL, msg);
  if (!net) return fail(PBN_EINVAL, "null net");
  if (const char* msg = shape_error(net->base.n_nodes, h0, h1)) return fail(PBN_EINVAL, msg);
  if (!net->dqn_kernel) return fail(PBN_EINVAL, "pbn_rollout_dqn: no kernel instance for this net");
  if (n_envs == 0 || n_steps == 0) return PBN_OK;
  if (!d_state || !d_target || !d_t || !d_image || !d_flipmask || !d_reward || !d_flags)
    return fail(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_image, 16)) return fail(PBN_EINVAL, "d_image must be 16-byte aligned");
  if (((uintptr_t)d_state | (uintptr_t)d_flipmask | (uintptr_t)d_actions | (uintptr_t)d_obs |
       (uintptr_t)d_final_state | (uintptr_t)d_reward) & 3u)
    return fail(PBN_EINVAL, "32-bit device buffers must be 4-byte aligned");
  if (!pbn::aligned(d_updates, 2)) return fail(PBN_EINVAL, "d_updates must be 2-byte aligned");
  if (int rc = pbn::check_device(net)) return rc;
  StepArgs a;
  fill_args(net, &a, seed, step, env_offset, n_envs);
  a.state = d_state;
  a.state_out = d_state;   // in place, as pbn_rollout_ex
  a.flipmask = d_flipmask;
  a.target = d_target;
  a.t = d_t;
  a.final_state = d_final_state;
  a.obs = d_obs;
  a.reward = d_reward;
  a.flags = d_flags;
  a.n_steps = n_steps;
  a.mode = (int)mode;
  a.updates = d_updates;
  PolicyArgs p;
  make_dims(net->base.n_nodes, net->W, net->base.n_attr, h0, h1, &p.d);
  p.img = d_image;
  p.eps_u = explore_threshold(epsilon);
  p.actions = d_actions;
  const unsigned blocks = (unsigned)((a.n_groups + kWavesPerBlock - 1) / kWavesPerBlock);
  hipLaunchKernelGGL(net->dqn_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), net->route.lds_wave,
                     (hipStream_t)stream, a, p);
  HIP_OK(hipGetLastError());
  return PBN_OK;
}

int pbn_rollout_copy(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                     int32_t n_steps, uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
                     uint8_t* d_t, uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                     uint16_t* d_updates, void* d_copy_dst, const void* d_copy_src, int64_t copy_bytes,
                     void* stream) {
  if (copy_bytes < 0) return fail(PBN_EINVAL, "copy_bytes < 0");
  if (copy_bytes > 0) {
    if (!d_copy_dst || !d_copy_src) return fail(PBN_EINVAL, "null copy buffer");
    if ((copy_bytes & 15) || !pbn::aligned(d_copy_dst, 16) || !pbn::aligned(d_copy_src, 16))
      return fail(PBN_EINVAL, "copy pointers and bytes must be 16-byte aligned");
    const char* d = static_cast<const char*>(d_copy_dst);
    const char* s = static_cast<const char*>(d_copy_src);
    if (d < s + copy_bytes && s < d + copy_bytes) return fail(PBN_EINVAL, "overlapping copy ranges");
  }
  return rollout_impl(net, seed, step, env_offset, n_envs, n_steps, mode, d_state, d_flipmask, d_target, d_t, d_obs,
                      d_final_state, d_reward, d_flags, d_updates, d_copy_dst, d_copy_src, copy_bytes, stream);
}

}  // extern "C"
