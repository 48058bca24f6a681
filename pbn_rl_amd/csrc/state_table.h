// state_table.h -- a count of visited states keyed by the full state (1..4 words): an
// open-addressing hash table with linear probing, stated once for the insert kernel
// (pbn_table.hip) and for a single-threaded host insert (tests/state_table_check.cpp).
//
// A table of capacity cap (a power of two) for keys of W words:
//   owner  u64 [cap]     0 = empty, else epoch << 32 | (row + 1): the launch that claimed the slot
//                        and the input row that claimed it
//   keys   u32 [W][cap]  the slot's key, written once by the claiming lane
//   counts u64 [cap]     touched only by atomic adds
//   used   u64 [1]       slots claimed so far
//   lost   u64 [1]       rows that found no slot (the caller keeps the load at or below 1/2, so 0)
//
// The rule the probe keeps to: no lane waits for another lane, and only read-modify-write atomics
// on owner, counts, used and lost carry information between the workgroups of one launch.  A slot
// claimed in the current launch names its input row, and its key is read from there -- the input
// is written by nobody -- while `keys` written in a launch is read only by later launches.  So no
// release/acquire protocol and no fence is needed, whatever the caches between workgroups do.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbn {

constexpr int kTableMaxWords = 4;
constexpr int64_t kTableMinCapacity = 64;

// murmur3's 32-bit finaliser: every input bit reaches every output bit
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// the finaliser chained over the (masked) words of the key
template <int W>
__host__ __device__ __forceinline__ uint32_t table_hash(const uint32_t (&k)[W]) {
  uint32_t h = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) h = fmix32(h ^ k[w]) + 0x9e3779b9u;
  return h;
}

// the mask of the key's top word: bits of the input above n_bits are not part of the key
__host__ __device__ __forceinline__ uint32_t table_top_mask(int n_words, int n_bits) {
  const int bits = n_bits - 32 * (n_words - 1);
  return bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
}

// The launch's read-only input: element (row t, word w, column c) at t * W * col_stride +
// w * col_stride + c, c < n_cols; flattened row id r = t * n_cols + c.
struct TableInput {
  const uint32_t* states;
  int64_t n_cols;
  int64_t col_stride;
  uint32_t top_mask;
};

template <int W>
__host__ __device__ __forceinline__ void table_load_key(const TableInput& in, int64_t r, uint32_t (&k)[W]) {
  const int64_t t = r / in.n_cols, c = r - t * in.n_cols;
  const uint32_t* p = in.states + (t * W) * in.col_stride + c;
#pragma unroll
  for (int w = 0; w < W; ++w) k[w] = p[(int64_t)w * in.col_stride];
  k[W - 1] &= in.top_mask;
}

template <int W>
__host__ __device__ __forceinline__ bool table_key_equal(const uint32_t (&a)[W], const uint32_t (&b)[W]) {
  uint32_t d = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) d |= a[w] ^ b[w];
  return d == 0;
}

struct TableArrays {
  uint64_t* owner;
  uint32_t* keys;
  uint64_t* counts;
  uint64_t* used;
  uint64_t* lost;
  int64_t cap;
};

// Adds `c` visits of key k (input row `row` of launch `epoch`) to the table.  `At` supplies the
// read-modify-write operations: cas(p, expected, desired) -> the old value, add(p, v).  Returns
// false when all cap slots hold other keys (counted in *lost).
template <int W, class At>
__host__ __device__ __forceinline__ bool table_insert(const TableArrays& t, const TableInput& in,
                                                      const uint32_t (&k)[W], uint32_t row, uint64_t c,
                                                      uint32_t epoch, At at) {
  const uint64_t mask = (uint64_t)t.cap - 1;
  const uint64_t tag = ((uint64_t)epoch << 32) | ((uint64_t)row + 1u);
  uint64_t h = table_hash<W>(k) & mask;
  for (int64_t probe = 0; probe < t.cap; ++probe) {
    const uint64_t old = at.cas(&t.owner[h], 0ull, tag);
    bool same;
    if (old == 0) {   // this lane owns the slot
#pragma unroll
      for (int w = 0; w < W; ++w) t.keys[(int64_t)w * t.cap + (int64_t)h] = k[w];
      at.add(t.used, 1ull);
      same = true;
    } else {
      uint32_t o[W];
      if ((uint32_t)(old >> 32) == epoch) {   // claimed in this launch: its key is the claiming input row
        table_load_key<W>(in, (int64_t)(old & 0xFFFFFFFFull) - 1, o);
      } else {                                // claimed by an earlier launch: its key is in `keys`
#pragma unroll
        for (int w = 0; w < W; ++w) o[w] = t.keys[(int64_t)w * t.cap + (int64_t)h];
      }
      same = table_key_equal<W>(k, o);
    }
    if (same) {
      at.add(&t.counts[h], c);
      return true;
    }
    h = (h + 1) & mask;
  }
  at.add(t.lost, 1ull);
  return false;
}

// the atomics of a single thread: the host insert
struct HostAtomics {
  uint64_t cas(uint64_t* p, uint64_t expected, uint64_t desired) const {
    const uint64_t old = *p;
    if (old == expected) *p = desired;
    return old;
  }
  void add(uint64_t* p, uint64_t v) const { *p += v; }
};

// One launch on the host: every input row in order (counts[r] visits each, or one; 0 skips).
template <int W>
inline void table_insert_host(const TableArrays& t, const TableInput& in, int64_t n_rows, const uint64_t* row_counts,
                              uint32_t epoch) {
  const int64_t total = n_rows * in.n_cols;
  for (int64_t r = 0; r < total; ++r) {
    const uint64_t c = row_counts ? row_counts[r] : 1ull;
    if (c == 0) continue;
    uint32_t k[W];
    table_load_key<W>(in, r, k);
    table_insert<W>(t, in, k, (uint32_t)r, c, epoch, HostAtomics{});
  }
}

}  // namespace pbn
