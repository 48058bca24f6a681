// bdq_layout.h -- what the fused BDQ update's kernels (learn_fwd.h, learn_bwd.h, learn_apply.h,
// bdq_pack.h), their launcher (pbn_learn.hip) and the acting kernel (pbn_qnet.hip) must agree on:
// BranchingQNetwork's shape, the flat parameter layout, the network image, the workspace, the
// apply launch's tasks and the LDS carvings of learn_fwd and learn_bwd.  Each is stated once: the
// host's sizes and the kernels' pointers come from the same functions, and tests/
// bdq_layout_check.cpp prints them for tests/test_bdq_layout_host.py, their second statement.
// Plain C++17, free of HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef PBN_HD
#if defined(__HIPCC__)
#define PBN_HD __host__ __device__
#else
#define PBN_HD
#endif
#endif
// what the hand-scheduled kernels call: inlined before any optimisation, as if written in place
#define PBN_HDI PBN_HD __attribute__((always_inline)) inline

namespace bdq {

PBN_HDI constexpr int imax(int a, int b) { return a > b ? a : b; }

constexpr int kD0 = 256, kD1 = 128, kD2 = 64, kD3 = 32, kDH = 64;   // bdq_model/network.py:29-36,46
constexpr int kRows = 16;         // transitions per tile: the MFMA's 16 columns
constexpr int kLearnWaves = 8;    // waves per forward / backward block
constexpr int kApplyWaves = 4;    // waves (= tasks) per apply block
constexpr int kMaxNT = 8;         // 16-column tiles of the bilinear layer's j (N <= 127)
constexpr size_t kLdsBytes = 160 * 1024;   // LDS of one CU: no block may ask for more

PBN_HD constexpr int64_t up16(int64_t x) { return (x + 15) & ~int64_t(15); }
// a head's A = N + 1 outputs, padded to whole 16-row tiles
PBN_HD constexpr int apad(int N) { return 16 * ((N + 16) / 16); }
PBN_HD constexpr int state_words(int N) { return (N + 31) / 32; }
// 16-column tiles of the bilinear layer's j: learn_apply_kernel<NT>
PBN_HD constexpr int bil_col_tiles(int N) { return (N + 15) / 16; }

// ---- the network.  Segments of the flat parameter buffer (pbn_bdq_layout; Adam's moments and
// the gradient share it), each starting on a 16-float boundary: the bilinear layer, then the
// dense layers, the H first head layers stacked as [64 H][32], the second ones as [H A][64]
enum Seg { BIL_W, BIL_B, L2_W, L2_B, L3_W, L3_B, L4_W, L4_B, H1_W, H1_B, H2_W, H2_B, TOTAL };
enum Lay { LY2, LY3, LY4, LYH1, LYH2, NLAY };   // the dense layers: also their slot in the image

// Dense layer l as a rows x cols matrix (outputs x inputs) and its parameter segments.  The
// second head layers are H stacked heads of head_rows rows: A in the parameters, Apad in the
// image (zero past each head's A).
struct Layer {
  int rows, cols;
  Seg w, b;
};
PBN_HDI constexpr int layer_rows(int l, int H = 0, int head_rows = 0) {   // (the trunk's need neither)
  return l == LY2 ? kD1 : l == LY3 ? kD2 : l == LY4 ? kD3 : l == LYH1 ? H * kDH : H * head_rows;
}
// (Macros where pack_tiles_kernel, bdq_pack.h, needs the chain expanded in place.)
#define PBN_LAYER_COLS(l) ((l) == LY2 ? kD0 : (l) == LY3 ? kD1 : (l) == LY4 ? kD2 : (l) == LYH1 ? kD3 : kDH)
PBN_HDI constexpr int layer_cols(int l) { return PBN_LAYER_COLS(l); }
PBN_HDI constexpr Layer layer(int l, int H = 0, int head_rows = 0) {
  return Layer{layer_rows(l, H, head_rows), layer_cols(l), Seg(L2_W + 2 * l), Seg(L2_B + 2 * l)};
}

// the weights of layer l < LYH2 in the flat buffer (off: its segment offsets), without indexing off
// by a variable
#define PBN_LAYER_W_OFF(off, l) \
  ((l) == LY2 ? (off)[L2_W] : (l) == LY3 ? (off)[L3_W] : (l) == LY4 ? (off)[L4_W] : (off)[H1_W])

inline void make_layout(int N, int H, int64_t* off) {
  int64_t sz[TOTAL];
  sz[BIL_W] = (int64_t)kD0 * N * N;
  sz[BIL_B] = kD0;
  for (int l = 0; l < NLAY; ++l) {
    const Layer y = layer(l, H, N + 1);
    sz[y.w] = (int64_t)y.rows * y.cols;
    sz[y.b] = y.rows;
  }
  int64_t o = 0;
  for (int s = 0; s < TOTAL; ++s) {
    off[s] = o;
    o += up16(sz[s]);
  }
  off[TOTAL] = o;
}

// ---- the network image (pbn_bdq_pack; the online one rewritten by learn_apply): the bilinear
// target table [n_attr][N][256] (the acting kernels' operand), then the dense layers' weights as
// 16 x 16 tiles in MFMA-fragment order, so that a wave's fragment of a tile is one 1 KB contiguous
// load (as 16-row x 64-byte fragment loads of the row-major weights they cost learn_fwd 3.7 of its
// 22.8 us, profiles/r06_l_learn_fwd_probes.json).  Layer matrix M (layer(l, H, Apad)), tile
// (ot, kt) at float (ot * cols/16 + kt) * 256, twice:
//   fwd: lane g*16 + r holds M[16 ot + r][16 kt + 4g + v], v = 0..3 (learn_fwd's A operand)
//   bwd: lane g*16 + r holds M[16 ot + 4g + v][16 kt + r]            (learn_bwd's transposed one)
struct ImageLayout {
  int64_t fwd[NLAY], bwd[NLAY], total;   // float offsets from the image's start
};

inline void make_image(int N, int H, int n_attr, ImageLayout* im) {
  int64_t o = (int64_t)n_attr * N * kD0;
  for (int l = 0; l < NLAY; ++l) {
    const Layer y = layer(l, H, apad(N));
    im->fwd[l] = o;
    o += (int64_t)y.rows * y.cols;
    im->bwd[l] = o;
    o += (int64_t)y.rows * y.cols;
  }
  im->total = o;
}

// ---- the workspace, [feature][B] planes unless noted: X(element type, name, elements), in order,
// with H, Ap = apad(N), W = state_words(N) and the batch B in scope.  Work's offsets, LearnArgs'
// pointers (learn_args.h) and their fill are all made from this list.
#define PBN_BDQ_WORK(X)                                                                                  \
  X(float, heads, 3LL * H * Ap * B)          /* [3][H][B][Apad]: a row's outputs contiguous (the TD  */ \
                                             /* pass reads them by rows)                             */ \
  X(float, y1, (int64_t)kD0 * B)             /* online s rows, after the activation                  */ \
  X(float, h2, (int64_t)kD1 * B)                                                                         \
  X(float, h3, (int64_t)kD2 * B)                                                                         \
  X(float, h4, (int64_t)kD3 * B)                                                                         \
  X(float, hh, (int64_t)H * kDH * B)                                                                     \
  X(float, dheads, (int64_t)H * Ap * B)      /* [H][Apad][B]                                         */ \
  X(float, dhh, (int64_t)H * kDH * B)                                                                    \
  X(float, dh4, (int64_t)kD3 * B)                                                                        \
  X(float, dh3, (int64_t)kD2 * B)                                                                        \
  X(float, dh2, (int64_t)kD1 * B)                                                                        \
  X(float, g1, (int64_t)kD0 * B)                                                                         \
  X(uint32_t, srow, (int64_t)W * B)          /* state words of the sampled rows                      */ \
  X(uint32_t, trow, (int64_t)W * B)          /* their target attractors' first-state words           */ \
  X(float, partial, B / kRows)               /* the backward blocks' loss sums                       */

struct Work {   // float offsets, each a multiple of 16
#define PBN_X(type, name, n) int64_t name;
  PBN_BDQ_WORK(PBN_X)
#undef PBN_X
  int64_t total;
};

inline Work make_work(int N, int H, int64_t B) {
  const int Ap = apad(N), W = state_words(N);
  Work w{};
  int64_t o = 0;
#define PBN_X(type, name, n) \
  w.name = o;                \
  o += up16(n);
  PBN_BDQ_WORK(PBN_X)
#undef PBN_X
  w.total = o;
  return w;
}

// ---- learn_apply's tasks, one wave each: the bilinear layer's 16 N (output tile, input i)
// tiles, then every 16 x 16 tile of the dense layers in Lay's order, the second head layers'
// head by head (at16 = Apad / 16 output tiles each); within a layer, (ot, kt) row-major
PBN_HDI constexpr int apply_bil_tasks(int N) { return kD0 / 16 * N; }
PBN_HDI constexpr int apply_tiles(int l, int H = 0, int at16 = 0) {   // (the trunk's need neither)
  const Layer y = layer(l, H, 16 * at16);
  return l == LYH2 ? H * at16 * (y.cols / 16) : (y.rows / 16) * (y.cols / 16);
}
PBN_HD constexpr int apply_tasks(int N, int H, int at16) {
  int n = apply_bil_tasks(N);
  for (int l = 0; l < NLAY; ++l) n += apply_tiles(l, H, at16);
  return n;
}
PBN_HD constexpr int apply_blocks(int N, int H, int at16) {
  return (apply_tasks(N, H, at16) + kApplyWaves - 1) / kApplyWaves;
}

// ---- learn_fwd's dynamic LDS, in 4-byte words.  The activations are blocked [K/16][16 rows][16]
// planes; the biases are staged in the order [bilinear 256 | 128 | 64 | 32 | H x 64 | H x A]
// (the layer epilogues read them there: a global load of the bias put its round trip on every
// layer's path), plus one spare word that the lanes past the biases store to.
PBN_HDI constexpr int fwd_bias_at(int l, int H) {   // layer l's biases; the bilinear layer's at 0
  return l == LY2    ? kD0
         : l == LY3  ? kD0 + kD1
         : l == LY4  ? kD0 + kD1 + kD2
         : l == LYH1 ? kD0 + kD1 + kD2 + kD3
                     : kD0 + kD1 + kD2 + kD3 + kDH * H;
}
PBN_HDI constexpr int fwd_bias_floats(int H, int A) { return fwd_bias_at(LYH2, H) + H * A; }
// the parameter (an index into the flat buffer, off = its segment offsets) staged at bias word idx
PBN_HDI constexpr int64_t fwd_bias_src(const int64_t* off, int H, int idx) {
  if (idx < kD0) return off[BIL_B] + idx;
  idx -= kD0;
  if (idx < kD1) return off[L2_B] + idx;
  idx -= kD1;
  if (idx < kD2) return off[L3_B] + idx;
  idx -= kD2;
  if (idx < kD3) return off[L4_B] + idx;
  idx -= kD3;
  if (idx < kDH * H) return off[H1_B] + idx;
  return off[H2_B] + idx - kDH * H;
}

// (Offsets as functions of the shape: a kernel pays for an offset's arithmetic where it asks for it.)
struct FwdLds {
  int H, A;
  PBN_HDI constexpr FwdLds(int H_, int A_) : H(H_), A(A_) {}
  static constexpr int y1 = 0;                    // [256/16][16][16]
  static constexpr int x2 = y1 + kD0 * kRows;     // [128/16][16][16]
  static constexpr int x3 = x2 + kD1 * kRows;
  static constexpr int x4 = x3 + kD2 * kRows;
  static constexpr int xh = x4 + kD3 * kRows;     // [64 H / 16][16][16]
  // what follows the H planes, from tail(): constant offsets
  PBN_HDI constexpr int tail() const { return xh + kDH * H * kRows; }
  static constexpr int sw = 0;                          // uint32 [4][16]: the rows' state words
  static constexpr int stg = sw + 4 * kRows;            // int [16]: their targets
  static constexpr int scnt = stg + kRows;              // int [16]: set bits per row
  static constexpr int slist = scnt + kRows;            // uint8 [16][128]: their indices, ascending
  static constexpr int sbias = slist + kRows * 128 / 4;   // fwd_bias_floats + 1
  PBN_HDI constexpr int end() const { return tail() + sbias + fwd_bias_floats(H, A) + 1; }
  PBN_HDI constexpr size_t bytes() const { return (size_t)end() * 4; }
};

// ---- learn_bwd's dynamic LDS, in 4-byte words: the delta planes and the split first-head-layer
// tiles; over the same space, before them, the TD pass's staged head rows (the row pitch Apad + 4
// puts the 16 rows' lanes on distinct banks); past both, the per-(row, branch) TD values
struct BwdLds {
  int H, Apad, K;
  PBN_HDI constexpr BwdLds(int H_, int Apad_, int K_) : H(H_), Apad(Apad_), K(K_) {}
  static constexpr int dh = 0;                                               // per head [Apad/16][16][16]
  PBN_HDI constexpr int dhh() const { return H * Apad * kRows; }              // [64 H / 16][16][16]
  PBN_HDI constexpr int dhh_words() const { return H * kDH * kRows; }
  // what follows the H planes, from trunk() = dhh() + dhh_words(): constant offsets
  PBN_HDI constexpr int trunk() const { return dhh() + dhh_words(); }
  static constexpr int dh4 = 0;
  static constexpr int dh3 = dh4 + kD3 * kRows;
  static constexpr int dh2 = dh3 + kD2 * kRows;
  static constexpr int part = dh2 + kD1 * kRows;                             // [8 waves][64 lanes][4]: the split tiles
  static constexpr int trunk_end = part + kLearnWaves * 64 * 4;
  // the planes' end, trunk() + trunk_end (in this form: learn_bwd's listing, tools/listing_diff.py)
  PBN_HDI constexpr int planes() const { return (H * Apad + H * kDH) * kRows + trunk_end; }
  static constexpr int sh = 0;                                               // [set][h][16][pitch]
  PBN_HDI constexpr int pitch() const { return Apad + 4; }
  PBN_HDI constexpr int staged() const { return 3 * H * kRows * pitch(); }    // the staged rows' end
  // past both: the TD values sg, sd (float) and sact (int), [16][K] each, one after the other
  PBN_HDI constexpr int td() const { return imax(planes(), staged()); }
  PBN_HDI constexpr int td_words() const { return kRows * K; }
  PBN_HDI constexpr int end() const { return td() + 3 * td_words(); }
  PBN_HDI constexpr size_t bytes() const { return (size_t)end() * 4; }
};

}  // namespace bdq
