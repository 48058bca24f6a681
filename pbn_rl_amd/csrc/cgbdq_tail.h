// cgbdq_tail.h -- the one statement of the ControlGBDQ tail's parameter order, image layout and LDS
// carving (pbn_cgbdq.hip; host and device read the same structs).  N = the net's nodes (1..128), C = the
// control nodes (1..128), K1 = N N, HR = 1 + 2 C head rows.
//
// d_tail (floats, flat, torch's (out, in) layout):
//   model.0.weight [256][K1], model.0.bias [256]; model.2.weight [256][256], model.2.bias [256];
//   model.4.weight [256][256], model.4.bias [256]; value_head.weight [1][256], value_head.bias [1];
//   then for head k = 0 .. C - 1: weight [2][256], bias [2]
//
// Image (floats; every segment starts at a multiple of 16 floats).  A dense layer with R rows (outputs)
// and K inputs, Rp and Kp their next multiples of 16, is stored as MFMA fragments: tile rt (16 rows),
// k-group kg (16 inputs = four v_mfma_f32_16x16x4_f32 steps) is 256 contiguous floats,
//   element ((rt (Kp / 16) + kg) 64 + lane) 4 + j  =  W[rt 16 + (lane & 15)][kg 16 + 4 j + (lane >> 4)],
// zero where the row is >= R or the input >= K: a wave reads a tile's four A operands of one k-group
// with one contiguous 1 KiB load (a float4 per lane; operand j is its element j).
//   w1 [256][K1p] frag, b1 [256]; w2 [256][256] frag, b2 [256]; w3 [256][256] frag, b3 [256];
//   wh [HRp][256] frag, bh [HRp]: the head rows stacked, row 0 = the value head, row 1 + 2 k + a =
//   output a of advantage head k; rows >= HR zero
//
// LDS of one block (floats), 32 envs (two MFMA column tiles):
//   a    [32][260]         activations after layers 1 and 3 (row = env, 256 hidden + 4: an MFMA B read
//                          takes 16 envs x 4 consecutive k, row stride 4 mod 32 spreads them over the
//                          banks); after the heads, int [32][C]: the chosen actions
//   b    [32][max(260, OS)] layer 1's input chunks, double buffered (2 x [32][68]: 64 inputs + 4), then
//                          the activations after layer 2, then the head outputs [32][OS], OS = HRp + 4
#pragma once
#include <stdint.h>

namespace pbn {

constexpr int kCgHidden = 256;       // the tail's width
constexpr int kCgEnvs = 32;          // envs of one block
constexpr int kCgThreads = 256;      // four waves
constexpr int kCgChunk = 64;         // layer 1's inputs per staged chunk
constexpr int kCgXS = kCgChunk + 4;  // a chunk's row stride
constexpr int kCgHS = kCgHidden + 4; // the activations' row stride
constexpr int kCgMaxCtrl = 128;
constexpr int kCgMaxLds = 160 * 1024;

__host__ __device__ inline int64_t cg_al16(int64_t x) { return (x + 15) & ~int64_t(15); }

struct CgLayout {
  int N, C, K1, K1p, HR, HRp, OS;
  int64_t w1, b1, w2, b2, w3, b3, wh, bh, floats;   // float offsets into the image, and its size
  int64_t lds_a, lds_b, lds_floats;                 // float offsets into LDS
};

__host__ __device__ inline CgLayout cg_layout(int N, int C) {
  CgLayout L;
  L.N = N;
  L.C = C;
  L.K1 = N * N;
  L.K1p = (int)cg_al16(L.K1);
  L.HR = 1 + 2 * C;
  L.HRp = (int)cg_al16(L.HR);
  L.OS = L.HRp + 4;
  int64_t o = 0;
  L.w1 = o, o += (int64_t)kCgHidden * L.K1p;
  L.b1 = o, o += kCgHidden;
  L.w2 = o, o += (int64_t)kCgHidden * kCgHidden;
  L.b2 = o, o += kCgHidden;
  L.w3 = o, o += (int64_t)kCgHidden * kCgHidden;
  L.b3 = o, o += kCgHidden;
  L.wh = o, o += (int64_t)L.HRp * kCgHidden;
  L.bh = o, o += L.HRp;
  L.floats = o;
  int64_t s = 0;
  L.lds_a = s, s += (int64_t)kCgEnvs * kCgHS;
  L.lds_b = s, s += (int64_t)kCgEnvs * (L.OS > kCgHS ? L.OS : kCgHS);
  L.lds_floats = s;
  return L;
}

// float offsets of d_tail's segments
struct CgTail {
  int64_t w[3], b[3], vw, vb, heads;   // head k: weight at heads + 514 k, bias 512 floats behind it
};

__host__ __device__ inline CgTail cg_tail(int N) {
  CgTail T;
  int64_t o = 0;
  for (int l = 0; l < 3; ++l) {
    T.w[l] = o, o += (int64_t)kCgHidden * (l == 0 ? N * N : kCgHidden);
    T.b[l] = o, o += kCgHidden;
  }
  T.vw = o, o += kCgHidden;
  T.vb = o, o += 1;
  T.heads = o;
  return T;
}

}  // namespace pbn
