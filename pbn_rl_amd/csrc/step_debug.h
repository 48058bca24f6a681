// step_debug.h -- what differs between the product and the diagnostic builds of the step
// kernels: the phase clocks (PBN_STAMP*, -DPBN_STAMPS), the listing marks (PBN_ISA_*,
// -DPBN_ISA_MARKS) and the bounds-checked indexing (CK, LANE_*, StepRows; -DPBN_CHECKS).  In
// the product the marks are empty and the stores are unguarded streaming stores.
#pragma once
#include "step_args.h"

namespace {

// In-kernel phase clocks (cdna_hip_programming.md section 7, "In-kernel stamps"):
// compiled only into the diagnostic library (-DPBN_STAMPS), never the product.
#ifdef PBN_STAMPS
#define PBN_STAMP(k)                                                                          \
  do {                                                                                        \
    unsigned long long t_;                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    if (a.stamps && (threadIdx.x & 63) == 0)                                                  \
      a.stamps[(size_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 32 + (k)] = t_; \
  } while (0)
// pipelined rollout: per role, clocks at the start of iteration 10, after its work, after the barrier;
// rows of 32 per block (tools/stamps.py): role r at 4r + {0, 1, 2}, HW_ID at 14 / 7 / 11, the
// segment clocks of the single-word fast paths at 15, 3, 12, 13 (state), 16, 17 (env), 18 (selection)
#define PBN_PSTAMP(k, slot_)                                                                  \
  do {                                                                                        \
    if ((k) == 10) {                                                                          \
      unsigned long long t_;                                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                      \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");             \
      __builtin_amdgcn_sched_barrier(0);                                                      \
      if (a.stamps && (threadIdx.x & 63) == 0)                                                \
        a.stamps[(size_t)blockIdx.x * 32 + (threadIdx.x >> 6) * 4 + (slot_)] = t_;            \
    }                                                                                         \
  } while (0)
#define PBN_PSTAMP_AT(k, idx_)                                                                \
  do {                                                                                        \
    if ((k) == 10) {                                                                          \
      unsigned long long t_;                                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                      \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");             \
      __builtin_amdgcn_sched_barrier(0);                                                      \
      if (a.stamps && (threadIdx.x & 63) == 0) a.stamps[(size_t)blockIdx.x * 32 + (idx_)] = t_; \
    }                                                                                         \
  } while (0)
// pipelined rollout: how many lanes of the env-draw wave take the fourth-flip tail in the stamped
// iteration, at column 19 of the block's row (tools/stamps.py splits the blocks by it)
#define PBN_PTAIL(k, cond_)                                                                   \
  do {                                                                                        \
    if ((k) == 10) {                                                                          \
      const unsigned long long n_ = __builtin_popcountll(__builtin_amdgcn_ballot_w64(cond_)); \
      if (a.stamps && (threadIdx.x & 63) == 0) a.stamps[(size_t)blockIdx.x * 32 + 19] = n_;   \
    }                                                                                         \
  } while (0)
// pipelined rollout, launch anatomy: the state wave's s_memrealtime (100 MHz, one clock for the
// whole chip) at kernel entry, after the table image, at the loop start, after iterations 0 and
// 1, after the loop and after its final stores have landed; row gridDim.x + block
#define PBN_RSTAMP(idx_)                                                                      \
  do {                                                                                        \
    unsigned long long t_;                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)(gridDim.x + blockIdx.x) * 32 + (idx_)] = t_; \
  } while (0)
#elif defined(PBN_ISA_MARKS)
// assembly listings only (tools/isa_budget.py compiles one instance with -S): each stamp site
// becomes a comment line in the listing, fenced so that no instruction crosses it; no code
#define PBN_ISA_MARK(txt)                                                                     \
  do {                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    asm volatile(";@mark " txt);                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                        \
  } while (0)
#define PBN_STAMP(k) do {} while (0)
#define PBN_PSTAMP(k, slot_) PBN_ISA_MARK("P" #slot_)
#define PBN_PSTAMP_AT(k, idx_) PBN_ISA_MARK("A" #idx_)
#define PBN_PTAIL(k, cond_) do {} while (0)
#define PBN_RSTAMP(idx_) PBN_ISA_MARK("R" #idx_)
// names the side of a runtime uniform branch it opens (tools/isa_budget.py --arms picks the live ones)
#define PBN_ISA_ARM(name_)                                                                    \
  do {                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    asm volatile(";@arm " name_);                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                        \
  } while (0)
// names the loop body it opens (role and compile-time variant) in the listing
#define PBN_ISA_LOOP(name_, v_)                                                               \
  do {                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    asm volatile(";@loop " name_ " %0" ::"i"(v_));                                            \
    __builtin_amdgcn_sched_barrier(0);                                                        \
  } while (0)
#else
#define PBN_STAMP(k) do {} while (0)
#define PBN_PSTAMP(k, slot_) do {} while (0)
#define PBN_PSTAMP_AT(k, idx_) do {} while (0)
#define PBN_PTAIL(k, cond_) do {} while (0)
#define PBN_RSTAMP(idx_) do {} while (0)
#endif
#ifndef PBN_ISA_LOOP
#define PBN_ISA_LOOP(name_, v_) do {} while (0)
#define PBN_ISA_ARM(name_) do {} while (0)
#endif

// Bounds-checked global indexing for the diagnostic library (-DPBN_CHECKS): an
// out-of-range index is printed and redirected to element 0 instead of faulting.
#ifdef PBN_CHECKS
__device__ __noinline__ size_t pbn_ck(size_t i, size_t len, int site) {
  if (i < len) return i;
  printf("pbn OOB site %d idx %llu len %llu block %u thread %u\n", site, (unsigned long long)i,
         (unsigned long long)len, blockIdx.x, threadIdx.x);
  return 0;
}
#define CK(i, len, site) pbn_ck((size_t)(i), (size_t)(len), (site))
#else
#define CK(i, len, site) (i)
#endif

// ---------------------------------------------------------------- helpers
// Element (uniform base + lane element) of an output array addressed as a wave-uniform 64-bit
// base (SGPRs, advanced per step on the SALU) plus the lane's 32-bit byte offset: the
// global_store / global_load "saddr" form, with no 64-bit VGPR address pair and no per-step
// VALU address arithmetic (lane_elem * sizeof(T) < 2^32: n_envs < 2^30).  Checked builds keep
// the bounds-checked index.
template <typename T>
__device__ __forceinline__ T& lane_at(T* base, size_t uniform_elems, uint32_t lane_bytes) {
  // laundered so that loop strength reduction cannot turn the sum into a 64-bit VGPR
  // induction variable
  asm volatile("" : "+s"(uniform_elems));
  asm volatile("" : "+v"(lane_bytes));
  return *reinterpret_cast<T*>(reinterpret_cast<char*>(base + uniform_elems) + lane_bytes);
}
#ifdef PBN_CHECKS
#define LANE_AT(base, ubase, le_, len, site) (base)[CK((ubase) + (size_t)(le_), (len), (site))]
#else
#define LANE_AT(base, ubase, le_, len, site) lane_at((base), (ubase), (uint32_t)(le_) * (uint32_t)sizeof(*(base)))
#endif
// Streaming store of a rollout output (pbn_rollout_pipe): non-temporal, so that the per-step
// obs / flip-mask / reward / flags stream does not evict the table image from L2 between
// launches (every launch re-reads it)
#ifndef PBN_CHECKS
#define LANE_ST(base, ubase, le_, len, site, v) __builtin_nontemporal_store((v), &LANE_AT(base, ubase, le_, len, site))
#else
#define LANE_ST(base, ubase, le_, len, site, v) (LANE_AT(base, ubase, le_, len, site) = (v))
#endif
// One per-step output of pbn_rollout_pipe ([n_steps][W][n] elements of T), stored through a
// buffer descriptor that covers ONE row of n elements: the row of step t, word 0.  The
// descriptor lives in four SGPRs, is built once before the step loop and moves on by one step
// with a 64-bit add to its base (so n_steps * W * n * sizeof(T) may pass 4 GB), where
// global_store's saddr form took a 64-bit multiply, shift and add per store and step.  The
// hardware's range check (raw buffer, stride 0: the lane's byte offset + sizeof(T) must not pass
// num_records; soffset stays 0) replaces the guards:
//   - a null output has num_records = 0, so every store to it is dropped;
//   - a lane of an invalid group (env le >= n) has offset le * sizeof(T) >= n * sizeof(T) =
//     num_records, so its store is dropped: no EXEC mask, and no lane can reach the next word's
//     row, the next step's row or another array.
// Word w > 0 of a multi-word state is a copy of the descriptor moved on by w rows.  Non-temporal
// as LANE_ST.  The stores are inline assembly because the compiler rebuilds a
// __builtin_amdgcn_make_buffer_rsrc descriptor from its pointer on every step (four SALU
// instructions each); the kernel never reads these arrays back, so the statements need no
// memory clobber and LDS traffic may move across them.  Checked builds (PBN_CHECKS) keep the
// guarded, bounds-checked index.
typedef uint32_t pbn_u32x4 __attribute__((ext_vector_type(4)));
template <typename T>
struct StepRows {
#ifndef PBN_CHECKS
  pbn_u32x4 d;      // base[31:0] | base[47:32], stride 0 | num_records (bytes) | format word
#else
  T* base;
  size_t at, len;   // first element of the current step's row; elements in all
#endif
};
template <typename T>
__device__ __forceinline__ StepRows<T> rows_open(T* base, int64_t n, size_t len) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 1, "dword and byte stores only");
  StepRows<T> r;
#ifndef PBN_CHECKS
  const uint64_t p = (uint64_t)reinterpret_cast<uintptr_t>(base);
  r.d.x = (uint32_t)p;
  r.d.y = (uint32_t)(p >> 32) & 0xFFFFu;
  r.d.z = base ? (uint32_t)n * (uint32_t)sizeof(T) : 0u;   // n < 2^30 (the host checks it)
  r.d.w = 0x00020000u;                                       // untyped 32-bit data, no swizzle
#else
  r.base = base;
  r.at = 0;
  r.len = len;
#endif
  return r;
}
// moves the descriptor on by `elems` elements (one step: W * n)
template <typename T>
__device__ __forceinline__ void rows_advance(StepRows<T>& r, size_t elems) {
#ifndef PBN_CHECKS
  const uint64_t b = (((uint64_t)r.d.y << 32) | r.d.x) + (uint64_t)elems * sizeof(T);
  r.d.x = (uint32_t)b;
  r.d.y = (uint32_t)(b >> 32);   // (a 48-bit address: no carry into the stride field)
#else
  r.at += elems;
#endif
}
// element le of the current step's row of word w (word_elems = w * n)
// (bits: the element's bit pattern; a byte store writes the low byte)
template <typename T>
__device__ __forceinline__ void rows_store(const StepRows<T>& r, int w, size_t word_elems, int64_t le, bool valid,
                                           int site, uint32_t bits) {
#ifndef PBN_CHECKS
  StepRows<T> q = r;
  if (w > 0) rows_advance(q, word_elems);
  const uint32_t off = (uint32_t)le * (uint32_t)sizeof(T);
  if constexpr (sizeof(T) == 4)
    asm volatile("buffer_store_dword %0, %1, %2, 0 offen nt" ::"v"(bits), "v"(off), "s"(q.d));
  else
    asm volatile("buffer_store_byte %0, %1, %2, 0 offen nt" ::"v"(bits), "v"(off), "s"(q.d));
#else
  if (valid && r.base) {
    T v;
    __builtin_memcpy(&v, &bits, sizeof(T));   // (little-endian: the low byte)
    r.base[CK(r.at + word_elems + (size_t)le, r.len, site)] = v;
  }
#endif
}

// LANE_ST with a per-lane element index (pbn_rollout_settle: every env is at its own step, so
// the step's base is not wave-uniform).  Write-back stores, not streaming ones: the few lanes
// that end a step in an iteration each write one element of a different output row, and a
// non-temporal partial-line write went to HBM as a whole write each time (WRITE_SIZE 21x the
// outputs' bytes, r05_t); through the L2 the lines fill up over the iterations before they are
// written back
// (r05_u: 495 -> 49 MB written per 20-step launch at config 2, +1 % on the settle line)
#define LANE_STV(base, idx, len, site, v) ((base)[CK((idx), (len), (site))] = (v))

}  // namespace
