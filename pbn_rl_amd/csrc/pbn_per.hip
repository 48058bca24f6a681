// pbn_per.hip -- proportional prioritised replay on the device (PrioritisedER, bdq_model/memory.py:73-186,
// over the segment trees of bdq_model/data_structures.py), DESIGN.md "Prioritised replay".
//
// Two trees over T = tree_size leaves (T the smallest power of two >= capacity), double[2T]
// each: node 1 is the root, leaf i is node T + i, a sum node is left + right and a min node is
// min(left, right); empty leaves are 0.0 / +inf.  Every ancestor always equals the operation of its
// two children, so the kernels rebuild ancestors from their children level by level instead of
// walking one root path per written leaf as the reference's __setitem__ does: the values are the
// same bits, and the order of the leaf writes does not matter.
//
//   pbn_per_store    n contiguous leaves after the ring position get max_priority ** alpha
//                    (memory.py:114-119).  Launch 1: a block per touched aligned chunk of kChunk
//                    leaves writes the chunk's leaves and rebuilds the chunk's subtree in LDS.
//                    Launch 2: one block rebuilds the levels above the chunk roots.  The second
//                    launch starts after the first has finished (stream order); no block waits for
//                    another.
//   pbn_per_sample   one block: p_total (the prefix sum of leaves [0, size - 2] in the association
//                    of the reference's recursion), a descent and a weight per thread, then beta
//                    and the draw counter advance.
//   pbn_per_update   one block: leaf = p ** alpha for the last occurrence of every index,
//                    max_priority, then the ancestors level by level.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/pbn_env.h"
#include "net_view.h"
#include "philox.h"

namespace {

constexpr int kChunk = 512;          // leaves per block of the store's first launch
constexpr int kChunkThreads = 256;   // one pair of leaves per thread
constexpr int kBlock = 1024;         // the single-block kernels (batch <= 1024)
constexpr int kMaxLevels = 64;

// the reference's operator.add / min(a, b) (Python's min keeps a unless b < a)
__device__ __forceinline__ double tree_min(double a, double b) { return b < a ? b : a; }

// ---- store, launch 1.  The n leaves are (pos + 1 + j) mod cap, j < n: segment A = [s, ea) with
// s = (pos + 1) mod cap, and, when the range wraps, segment B = [0, eb).  Block b takes the b-th
// chunk of A, then the chunks of B that A does not touch (a chunk has exactly one block: nobody
// else reads or writes its subtree in this launch); further blocks exit.
__global__ void __launch_bounds__(kChunkThreads) per_store_chunks_kernel(
    int64_t n, const int64_t* __restrict__ d_pos, int64_t cap, int64_t T, int chunk, double alpha,
    const double* __restrict__ d_maxp, double* sum, double* mn) {
  __shared__ double s_sum[kChunk];
  __shared__ double s_min[kChunk];
  const int64_t pos = ((*d_pos % cap) + cap) % cap;
  const int64_t s = (pos + 1) % cap;
  const int64_t ea = s + n < cap ? s + n : cap;
  const int64_t eb = s + n - cap;                       // > 0: the range wraps
  const int64_t a0 = s / chunk, a1 = (ea - 1) / chunk;  // (n >= 1: A is never empty)
  const int64_t na = a1 - a0 + 1;
  int64_t c = -1;
  if ((int64_t)blockIdx.x < na) {
    c = a0 + blockIdx.x;
  } else if (eb > 0) {
    // B's chunks are 0..b1; those below a0 are not A's (B ends at or before s, so b1 <= a0)
    const int64_t b1 = (eb - 1) / chunk;
    const int64_t nb = (b1 < a0 ? b1 : a0 - 1) + 1;
    const int64_t k = (int64_t)blockIdx.x - na;
    if (k < nb) c = k;
  }
  if (c < 0) return;                                    // (uniform over the block)
  const double v = pow(*d_maxp, alpha);
  const int64_t base = c * chunk;
  for (int i = threadIdx.x; i < chunk; i += kChunkThreads) {
    const int64_t leaf = base + i;
    const bool hit = (leaf >= s && leaf < ea) || leaf < eb;
    double a, m;
    if (hit) {
      a = m = v;
      sum[T + leaf] = v;
      mn[T + leaf] = v;
    } else {
      a = sum[T + leaf];
      m = mn[T + leaf];
    }
    s_sum[i] = a;
    s_min[i] = m;
  }
  __syncthreads();
  // the chunk's subtree bottom-up: level w holds the w nodes (T / chunk * w) + c * w + [0, w),
  // computed in place in the first w LDS slots (slot i from slots 2i and 2i + 1 of the level below:
  // read, barrier, write)
  for (int w = chunk >> 1; w >= 1; w >>= 1) {
    double a[kChunk / 2 / kChunkThreads], m[kChunk / 2 / kChunkThreads];
    int k = 0;
    for (int i = threadIdx.x; i < w; i += kChunkThreads, ++k) {
      a[k] = s_sum[2 * i] + s_sum[2 * i + 1];
      m[k] = tree_min(s_min[2 * i], s_min[2 * i + 1]);
    }
    __syncthreads();
    const int64_t node0 = (T / chunk) * w + c * w;
    k = 0;
    for (int i = threadIdx.x; i < w; i += kChunkThreads, ++k) {
      s_sum[i] = a[k];
      s_min[i] = m[k];
      sum[node0 + i] = a[k];
      mn[node0 + i] = m[k];
    }
    __syncthreads();
  }
}

// ---- store, launch 2 (one block): the levels above the chunk roots, nodes [1, n_roots), level by
// level from the chunk roots' parents to the root.  Each node is written by one thread and read,
// after the barrier, by the thread of its parent.
__global__ void __launch_bounds__(kBlock) per_store_top_kernel(int64_t n_roots, double* sum, double* mn) {
  for (int64_t w = n_roots >> 1; w >= 1; w >>= 1) {
    for (int64_t i = threadIdx.x; i < w; i += kBlock) {
      const int64_t node = w + i;
      sum[node] = sum[2 * node] + sum[2 * node + 1];
      mn[node] = tree_min(mn[2 * node], mn[2 * node + 1]);
    }
    __syncthreads();
  }
}

// ---- sample (one block, thread i = row i of the batch).
__global__ void __launch_bounds__(kBlock) per_sample_kernel(
    int B, int64_t cap, int64_t T, const int64_t* __restrict__ d_size, const double* __restrict__ sum,
    const double* __restrict__ mn, double* __restrict__ d_beta, double max_beta, double beta_step, uint64_t seed,
    int64_t* __restrict__ d_counter, int64_t* __restrict__ idx_out, float* __restrict__ w_out) {
  __shared__ double s_ptotal;
  __shared__ double t[kMaxLevels];
  int64_t N = *d_size;
  N = N < 0 ? 0 : (N > cap ? cap : N);
  const double beta = *d_beta;
  const uint64_t ctr = (uint64_t)*d_counter;
  if (threadIdx.x == 0) {
    // sum(0, N - 1) of memory.py:123 = leaves [0, N - 2] (reduce's end -= 1).  _reduce
    // (data_structures.py:33-60) on a prefix goes left while the prefix fits the left half, and
    // otherwise adds the whole left child to the right child's prefix: t_1 + (t_2 + (... + t_m))
    int m = 0;
    int64_t rem = N - 1, w = T, node = 1;
    if (rem >= 1) {
      for (;;) {
        if (rem == w) {
          t[m++] = sum[node];
          break;
        }
        w >>= 1;
        if (rem <= w) {
          node = 2 * node;
        } else {
          t[m++] = sum[2 * node];
          node = 2 * node + 1;
          rem -= w;
        }
      }
    }
    double p = m > 0 ? t[m - 1] : 0.0;
    for (int k = m - 2; k >= 0; --k) p = __dadd_rn(t[k], p);
    s_ptotal = p;
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < B) {
    const double r = s_ptotal / (double)B;
    const pbn::Word4 x = pbn::draw(seed, (uint64_t)i, ctr, pbn::kStreamReplay, 0);
    const double u = (double)(((uint64_t)x.x << 21) | (uint64_t)(x.y >> 11)) * 0x1.0p-53;
    // random.random() * every_range_len + i * every_range_len (memory.py:126): two rounded
    // products, one rounded sum
    double mass = __dadd_rn(__dmul_rn(u, r), __dmul_rn((double)i, r));
    int64_t node = 1;
    while (node < T) {                                   // find_prefixsum_index (:159-166)
      const double left = sum[2 * node];
      if (left > mass) {
        node = 2 * node;
      } else {
        mass = __dsub_rn(mass, left);
        node = 2 * node + 1;
      }
    }
    int64_t j = node - T;
    j = j > N - 1 ? N - 1 : j;
    j = j < 0 ? 0 : j;
    const double S = sum[1];
    const double nn = (double)N;
    const double wi = pow(nn * (sum[T + j] / S), -beta);
    const double wmax = pow(nn * (mn[1] / S), -beta);
    idx_out[i] = j;
    w_out[i] = (float)(wi / wmax);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double b = beta + beta_step;
    *d_beta = max_beta < b ? max_beta : b;               // min(max_beta, beta + beta_step)
    *d_counter = (int64_t)(ctr + 1);
  }
}

// ---- update (one block, thread b = pair b).
__global__ void __launch_bounds__(kBlock) per_update_kernel(
    int B, int64_t T, int levels, double alpha, const int64_t* __restrict__ d_size, const int64_t* __restrict__ idx,
    const float* __restrict__ prio, double* __restrict__ d_maxp, double* sum, double* mn) {
  __shared__ int64_t s_idx[kBlock];
  __shared__ double s_max[kBlock / 64];
  const int b = threadIdx.x;
  const int64_t size = *d_size;
  int64_t j = -1;
  double p = 0.0;
  if (b < B) {
    j = idx[b];
    if (j < 0 || j >= size || j >= T) j = -1;            // the reference asserts; skipped here
    p = (double)prio[b];
  }
  s_idx[b] = j;
  __syncthreads();
  const bool valid = j >= 0;
  // the reference applies the pairs in order: of equal indices the highest batch position wins
  bool wins = valid;
  for (int o = b + 1; o < B && wins; ++o) wins = s_idx[o] != j;
  if (wins) {
    const double leaf = pow(p, alpha);
    sum[T + j] = leaf;
    mn[T + j] = leaf;
  }
  // max_priority = max(max_priority, every applied p) (the losing duplicates included);
  // Python's max(a, b) keeps a unless b > a
  double m = valid ? p : -INFINITY;
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  if ((b & 63) == 0) s_max[b >> 6] = m;
  __syncthreads();
  if (b == 0) {
    double best = *d_maxp;
    for (int k = 0; k < kBlock / 64; ++k) best = s_max[k] > best ? s_max[k] : best;
    *d_maxp = best;
  }
  // ancestors, one level per barrier: every pair's thread recomputes its ancestor from the two
  // children of the finished level below (pairs under the same ancestor write equal values)
  for (int l = 1; l <= levels; ++l) {
    if (valid) {
      const int64_t node = (T + j) >> l;
      sum[node] = sum[2 * node] + sum[2 * node + 1];
      mn[node] = tree_min(mn[2 * node], mn[2 * node + 1]);
    }
    __syncthreads();
  }
}

bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }
bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

// tree_size must be the trees' T: a power of two >= capacity (the reference takes the smallest)
int check_tree(int64_t capacity, int64_t tree_size) {
  if (capacity < 2) return pbn::set_error(PBN_EINVAL, "capacity must be >= 2");
  if (!pow2(tree_size) || tree_size < capacity || tree_size > ((int64_t)1 << 40))
    return pbn::set_error(PBN_EINVAL, "tree_size must be a power of two >= capacity");
  return PBN_OK;
}

int ilog2(int64_t x) {
  int l = 0;
  while (((int64_t)1 << l) < x) ++l;
  return l;
}

}  // namespace

extern "C" {

int pbn_per_store(int64_t n, const int64_t* d_pos, int64_t capacity, int64_t tree_size, double alpha,
                  const double* d_max_priority, double* d_sum_tree, double* d_min_tree, void* stream) {
  int rc = check_tree(capacity, tree_size);
  if (rc) return rc;
  if (n < 1 || n > capacity) return pbn::set_error(PBN_EINVAL, "n must be in 1..capacity");
  if (!d_pos || !d_max_priority || !d_sum_tree || !d_min_tree) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!aligned8(d_pos) || !aligned8(d_max_priority) || !aligned8(d_sum_tree) || !aligned8(d_min_tree))
    return pbn::set_error(PBN_EINVAL, "buffers must be 8-byte aligned");
  const int chunk = (int)(tree_size < kChunk ? tree_size : kChunk);
  // a segment of L leaves touches at most (L - 2) / chunk + 2 chunks, and there are two segments
  const int64_t blocks = n / chunk + 4;
  if (blocks > 0x7FFFFFFF) return pbn::set_error(PBN_EINVAL, "n too large");
  hipLaunchKernelGGL(per_store_chunks_kernel, dim3((unsigned)blocks), dim3(kChunkThreads), 0, (hipStream_t)stream, n,
                     d_pos, capacity, tree_size, chunk, alpha, d_max_priority, d_sum_tree, d_min_tree);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  const int64_t n_roots = tree_size / chunk;
  if (n_roots > 1) {
    hipLaunchKernelGGL(per_store_top_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, n_roots, d_sum_tree,
                       d_min_tree);
    e = hipGetLastError();
    if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  }
  return PBN_OK;
}

int pbn_per_sample(int32_t batch, int64_t capacity, int64_t tree_size, const int64_t* d_size,
                   const double* d_sum_tree, const double* d_min_tree, double* d_beta, double max_beta,
                   double beta_step, uint64_t seed, int64_t* d_counter, int64_t* d_idx, float* d_weights,
                   void* stream) {
  int rc = check_tree(capacity, tree_size);
  if (rc) return rc;
  if (batch < 1 || batch > kBlock) return pbn::set_error(PBN_EINVAL, "batch must be in 1..1024");
  if (!d_size || !d_sum_tree || !d_min_tree || !d_beta || !d_counter || !d_idx || !d_weights)
    return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!aligned8(d_size) || !aligned8(d_sum_tree) || !aligned8(d_min_tree) || !aligned8(d_beta) ||
      !aligned8(d_counter) || !aligned8(d_idx) || ((uintptr_t)d_weights & 3u) != 0)
    return pbn::set_error(PBN_EINVAL, "buffers must be 8-byte (d_weights 4-byte) aligned");
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (int)batch, capacity,
                     tree_size, d_size, d_sum_tree, d_min_tree, d_beta, max_beta, beta_step, seed, d_counter, d_idx,
                     d_weights);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  return PBN_OK;
}

int pbn_per_update(int32_t batch, int64_t capacity, int64_t tree_size, double alpha, const int64_t* d_size,
                   const int64_t* d_idx, const float* d_priorities, double* d_max_priority, double* d_sum_tree,
                   double* d_min_tree, void* stream) {
  int rc = check_tree(capacity, tree_size);
  if (rc) return rc;
  if (batch < 1 || batch > kBlock) return pbn::set_error(PBN_EINVAL, "batch must be in 1..1024");
  if (!d_size || !d_idx || !d_priorities || !d_max_priority || !d_sum_tree || !d_min_tree)
    return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!aligned8(d_size) || !aligned8(d_idx) || ((uintptr_t)d_priorities & 3u) != 0 || !aligned8(d_max_priority) ||
      !aligned8(d_sum_tree) || !aligned8(d_min_tree))
    return pbn::set_error(PBN_EINVAL, "buffers must be 8-byte (d_priorities 4-byte) aligned");
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (int)batch, tree_size,
                     ilog2(tree_size), alpha, d_size, d_idx, d_priorities, d_max_priority, d_sum_tree, d_min_tree);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  return PBN_OK;
}

}  // extern "C"
