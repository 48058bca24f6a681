// pbn_table.hip -- counts visited states in a device hash table keyed by the full state (1..4
// words): the sparse accumulation step of the steady-state distribution and of attractor
// discovery, for networks of any width the env runs (pbn_state_histogram's 2^N bins stop at 32
// nodes and are mostly empty long before).
//
// The table, its hash and the probe are state_table.h's; this file adds the launch: a grid-stride
// pass over the input rows in which each wave first merges equal keys (states of steady-state
// chains concentrate on a few attractors), then probes once per distinct key.  The probe never
// waits: see state_table.h for why nothing but the atomics' own results crosses workgroups.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "../../include/pbn_env.h"
#include "net_view.h"
#include "state_table.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4096;
constexpr int kMergeRounds = 4;

// device-scope read-modify-write atomics (relaxed: the values they return are all that is used)
struct DeviceAtomics {
  __device__ __forceinline__ uint64_t cas(uint64_t* p, uint64_t expected, uint64_t desired) const {
    return atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expected,
                     (unsigned long long)desired);
  }
  __device__ __forceinline__ void add(uint64_t* p, uint64_t v) const {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
  }
};

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

template <int W>
__global__ void __launch_bounds__(kThreads) pbn_table_insert_kernel(pbn::TableInput in, int64_t n_rows,
                                                                    const uint64_t* __restrict__ row_counts,
                                                                    pbn::TableArrays tab, uint32_t epoch) {
  const int64_t total = n_rows * in.n_cols;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  // (the loop bounds are uniform over the block: every lane of a wave reaches the ballots)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += stride) {
    const int64_t i = base + threadIdx.x;
    uint32_t k[W] = {};
    uint64_t c = 0;   // the visits this lane will add; 0: nothing to add
    if (i < total) {
      c = row_counts ? row_counts[i] : 1ull;
      if (c != 0) pbn::table_load_key<W>(in, i, k);
    }
    // merge equal keys of the wave: the leader of each round takes the visits of its equals
    bool pending = c != 0;
#pragma unroll
    for (int round = 0; round < kMergeRounds; ++round) {
      const uint64_t act = __ballot(pending);
      if (act == 0) break;
      const int leader = __builtin_ctzll(act);
      uint32_t lk[W];
#pragma unroll
      for (int w = 0; w < W; ++w) lk[w] = __shfl(k[w], leader);
      const bool eq = pending && pbn::table_key_equal<W>(k, lk);
      uint64_t sum;
      if (row_counts) {
        sum = wave_sum64(eq ? c : 0ull);
      } else {
        sum = (uint64_t)__popcll(__ballot(eq));
      }
      if (eq) {
        c = lane == leader ? sum : 0ull;
        pending = false;
      }
    }
    if (c != 0) pbn::table_insert<W>(tab, in, k, (uint32_t)i, c, epoch, DeviceAtomics{});
  }
}

using InsertFn = void (*)(pbn::TableInput, int64_t, const uint64_t*, pbn::TableArrays, uint32_t);
InsertFn pick_insert(int W) {
  switch (W) {
    case 1: return pbn_table_insert_kernel<1>;
    case 2: return pbn_table_insert_kernel<2>;
    case 3: return pbn_table_insert_kernel<3>;
    case 4: return pbn_table_insert_kernel<4>;
  }
  return nullptr;
}

}  // namespace

extern "C" int pbn_table_insert(const uint32_t* d_states, int64_t n_rows, int64_t n_cols, int64_t col_stride,
                                int32_t n_words, int32_t n_bits, const uint64_t* d_row_counts, int64_t capacity,
                                uint64_t* d_owner, uint32_t* d_keys, uint64_t* d_counts, uint64_t* d_used,
                                uint64_t* d_lost, uint32_t epoch, void* stream) {
  if (n_words < 1 || n_words > pbn::kTableMaxWords) return pbn::set_error(PBN_EINVAL, "n_words must be 1..4");
  if (n_bits < 32 * (n_words - 1) + 1 || n_bits > 32 * n_words)
    return pbn::set_error(PBN_EINVAL, "n_bits must be in 32 (n_words - 1) + 1 .. 32 n_words");
  if (capacity < pbn::kTableMinCapacity || (capacity & (capacity - 1)) != 0)
    return pbn::set_error(PBN_EINVAL, "capacity must be a power of two, at least 64");
  if (epoch == 0) return pbn::set_error(PBN_EINVAL, "epoch 0 marks an empty slot: epochs start at 1");
  if (n_rows < 0 || n_cols < 0) return pbn::set_error(PBN_EINVAL, "n_rows < 0 or n_cols < 0");
  if (col_stride < n_cols) return pbn::set_error(PBN_EINVAL, "col_stride < n_cols");
  constexpr int64_t kRowLimit = 0xFFFFFFFFll;   // (both factors below it: the product fits 64 bits)
  if (n_rows != 0 && n_cols != 0 &&
      (n_rows >= kRowLimit || n_cols >= kRowLimit || (uint64_t)n_rows * (uint64_t)n_cols >= (uint64_t)kRowLimit))
    return pbn::set_error(PBN_EINVAL,
                          "n_rows * n_cols must be below 2^32 - 1: a slot's owner names its row in 32 bits");
  if (n_rows == 0 || n_cols == 0) return PBN_OK;
  if (!d_states || !d_owner || !d_keys || !d_counts || !d_used || !d_lost)
    return pbn::set_error(PBN_EINVAL, "null buffer");
  const int64_t total = n_rows * n_cols;
  pbn::TableInput in{d_states, n_cols, col_stride, pbn::table_top_mask(n_words, n_bits)};
  pbn::TableArrays tab{d_owner, d_keys, d_counts, d_used, d_lost, capacity};
  const unsigned blocks = (unsigned)std::min<int64_t>((total + kThreads - 1) / kThreads, kMaxBlocks);
  hipLaunchKernelGGL(pick_insert(n_words), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, in, n_rows,
                     d_row_counts, tab, epoch);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  return PBN_OK;
}
