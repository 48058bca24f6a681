// net_image.h -- the descriptor compiler: pbn_net_desc -> the table image the step kernels copy
// into LDS, the record and threshold arrays they read from global memory, and the scalars of
// their launch arguments.  Plain C++17, free of HIP (tests/test_net_image.py runs it on the CPU);
// pbn_net_create uploads the result.  Every step below appends its section to NetImage::tab and
// records the section's offset; the kernels' view of the sections is StepArgs (step_args.h).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/pbn_env.h"
#include "net_layout.h"

namespace pbn {

struct NetImage {
  std::vector<uint32_t> tab;        // the LDS image
  std::vector<uint32_t> fcompact;   // uint4 [n_funcs] {inputs as plane bytes, 16-bit table, threshold, 0}
  std::vector<uint32_t> nrec;       // uint4 [N][kNodeRecs]: a node's first records, .y = threshold class,
                                    // records 0 and 1 carry {nf, f0} in .w
  std::vector<uint32_t> sthr;       // settle law: thresholds scaled to 16 bits [lq][32W]
  std::vector<uint32_t> sthr_pk;    // the same, packed biased node pairs [lq][W][16]
  std::vector<uint32_t> att_first;  // [n_attr][W]: each attractor's first state
  int n_nodes = 0, W = 0, prob_bits = 0, horizon = 0, n_funcs = 0, n_gates = 0, settle_max = 0;
  int n_attr = 0, n_states = 0, att_single = 0;
  int cdf_len = 0, hash_bits = 0, hash_probes = 0;
  uint32_t hash_mult[4] = {0, 0, 0, 0};
  int att_off = 0, sel_off = 0, nrec_off = 0, gate_off = 0, glayer_off = 0, n_glayers = 0;
  int gap_lut_off = 0, gap_shift = 0, gap_nb = 0, gap_exact = 1, cm_off = 0, tab_words = 0;
  float inv_log2q = 0.f;
  int n_cls = 0;
  uint32_t uthr[kNodeRecs] = {0, 0, 0, 0};
  int max_nf = 0, lq = 1, settle_pk = 0;
  int wave_words = 0, slot_words = 0, slot_words_settle = 0;
  uint32_t n1_magic = 0, am1_magic = 0;   // ceil(2^32 / (N + 1)), ceil(2^32 / (A - 1))
  uint64_t x_mult = 0;
  size_t lds_wave = 0, lds_pipe = 0, lds_settle = 0;   // bytes
};

namespace image {

inline void align_tab(std::vector<uint32_t>* tab, size_t words) {
  while (tab->size() & (words - 1)) tab->push_back(0u);
}

// LDS plane of an input reference: nodes first, then the gates' outputs
inline uint32_t plane_of(int ref, int N, int W) { return (uint32_t)(ref < N ? ref : 32 * W + (ref - N)); }

// a k-input truth table (k <= 4) over four inputs: the unused inputs do not matter
inline uint32_t table16(uint32_t T, int k) {
  const uint32_t kmask = (1u << k) - 1u;
  uint32_t T16 = 0;
  for (uint32_t m = 0; m < 16; ++m) T16 |= ((T >> (m & kmask)) & 1u) << m;
  return T16;
}

inline bool table_fits(uint32_t T, int k) { return (1u << k) >= 32 || (T >> (1u << k)) == 0u; }

inline int func_count(const pbn_net_desc& d, int i) { return d.node_func_start[i + 1] - d.node_func_start[i]; }

inline bool check_header(const pbn_net_desc& d, std::string* err) {
  const int N = d.n_nodes;
  if (N < 1 || N > PBN_MAX_NODES) return *err = "n_nodes out of range 1..128", false;
  if (!(d.prob_bits == 4 || d.prob_bits == 8 || d.prob_bits == 12 || d.prob_bits == 16))
    return *err = "prob_bits must be 4, 8, 12 or 16", false;
  if (d.horizon < 0 || d.horizon > 255) return *err = "horizon out of range 0..255", false;
  if (d.settle_max < 0 || d.settle_max > PBN_MAX_SETTLE) return *err = "settle_max out of range 0..4096", false;
  if (d.n_attractors < 0 || d.n_attractors > PBN_MAX_ATTRACTORS)
    return *err = "n_attractors out of range 0..254", false;
  if (!d.node_func_start || !d.func_arity || !d.func_inputs || !d.func_table || !d.func_threshold ||
      !d.perturb_cdf || !d.reward_table)
    return *err = "null table in descriptor", false;
  const int W = (N + 31) / 32;
  if (d.n_gates < 0 || d.n_gates > PBN_MAX_GATES || 32 * W + d.n_gates > 256)
    return *err = "n_gates out of range (32 * W + n_gates must be <= 256)", false;
  if (d.n_gates && (!d.gate_arity || !d.gate_inputs || !d.gate_table)) return *err = "null gate table", false;
  return true;
}

// glevel[g]: 1 + the deepest gate input (nodes are level 0)
inline bool check_gates(const pbn_net_desc& d, std::vector<int>* glevel, std::string* err) {
  const int N = d.n_nodes;
  glevel->assign(d.n_gates, 1);
  for (int g = 0; g < d.n_gates; ++g) {
    const int k = d.gate_arity[g];
    if (k < 0 || k > PBN_MAX_ARITY) return *err = "gate arity must be 0..4", false;
    if (!table_fits(d.gate_table[g], k)) return *err = "gate truth table has bits beyond 2^arity", false;
    for (int j = 0; j < k; ++j) {
      const int r = d.gate_inputs[4 * g + j];
      if (r < 0 || r >= N + g) return *err = "gate input must be a node or an earlier gate", false;
      if (r >= N) (*glevel)[g] = std::max((*glevel)[g], (*glevel)[r - N] + 1);
    }
  }
  return true;
}

inline bool check_funcs(const pbn_net_desc& d, std::string* err) {
  const int N = d.n_nodes;
  const uint32_t one = 1u << d.prob_bits;
  if (d.node_func_start[0] != 0 || d.node_func_start[N] != d.n_funcs)
    return *err = "node_func_start must span 0..n_funcs", false;
  for (int i = 0; i < N; ++i) {
    const int f0 = d.node_func_start[i], f1 = d.node_func_start[i + 1];
    if (f1 <= f0 || f1 - f0 > PBN_MAX_FUNCS_PER_NODE)
      return *err = "node " + std::to_string(i) + " needs 1..16 functions", false;
    uint32_t prev = 0;
    for (int f = f0; f < f1; ++f) {
      const int k = d.func_arity[f];
      if (k < 0 || k > PBN_MAX_ARITY) return *err = "function arity must be 0..4", false;
      const uint32_t c = d.func_threshold[f];
      if (c < prev || c > one) return *err = "thresholds must be non-decreasing and <= 2^prob_bits", false;
      if (f == f1 - 1 && c != one) return *err = "last threshold of a node must be 2^prob_bits", false;
      prev = c;
      for (int j = 0; j < k; ++j) {
        const int g = d.func_inputs[4 * f + j];
        if (g < 0 || g >= N + d.n_gates) return *err = "function input reference out of range", false;
      }
      if (!table_fits(d.func_table[f], k)) return *err = "truth table has bits beyond 2^arity", false;
    }
  }
  return true;
}

// ids[k]: the attractor of state k
inline bool check_attractors(const pbn_net_desc& d, std::vector<uint32_t>* ids, std::string* err) {
  const int A = d.n_attractors;
  if (!A) return true;
  if (!d.attractor_start || !d.attractor_states) return *err = "null attractor tables", false;
  if (d.attractor_start[0] != 0 || d.attractor_start[A] != d.n_attractor_states)
    return *err = "bad attractor_start", false;
  for (int at = 0; at < A; ++at) {
    if (d.attractor_start[at + 1] <= d.attractor_start[at]) return *err = "empty attractor", false;
    ids->insert(ids->end(), d.attractor_start[at + 1] - d.attractor_start[at], (uint32_t)at);
  }
  return true;
}

// open-addressing hash of the attractor states [S][W], slot-major [1 << bits][hash_stride(W)];
// deterministic multiplier search
inline bool build_hash(const uint32_t* states, const std::vector<uint32_t>& ids, int W, NetImage* im,
                       std::vector<uint32_t>* image) {
  const size_t S = ids.size();
  int bits = 1;
  while ((size_t(1) << bits) < 2 * S) ++bits;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&rng]() {
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return (uint32_t)(rng >> 11) | 1u;
  };
  // places every state with the multipliers mult; the longest probe sequence, or (out given)
  // the table
  auto place = [&](const uint32_t mult[4], int nbits, std::vector<uint32_t>* out) {
    const uint32_t size = 1u << nbits, mask = size - 1;
    const int HS = hash_stride(W);
    std::vector<int> used(size, 0);
    int probes = 1;
    for (size_t k = 0; k < S; ++k) {
      uint32_t h = 0;
      for (int w = 0; w < W; ++w) h += states[k * W + w] * mult[w];
      h >>= (32 - nbits);
      int p = 0;
      while (used[(h + p) & mask]) ++p;
      const uint32_t slot = (h + p) & mask;
      used[slot] = 1;
      probes = std::max(probes, p + 1);
      if (out) {
        for (int w = 0; w < W; ++w) (*out)[(size_t)slot * HS + w] = states[k * W + w];
        (*out)[(size_t)slot * HS + W] = ids[k];
      }
    }
    return probes;
  };
  // prefer a collision-free table (one probe per lookup) up to 16x the minimal size
  const int min_bits = bits;
  for (; bits <= kMaxHashBits; ++bits) {
    int best_probes = 1 << 30;
    uint32_t best_mult[4] = {0, 0, 0, 0};
    for (int trial = 0; trial < 64 && best_probes != 1; ++trial) {
      uint32_t mult[4];
      for (int w = 0; w < 4; ++w) mult[w] = next();
      const int probes = place(mult, bits, nullptr);
      if (probes < best_probes) {
        best_probes = probes;
        std::copy(mult, mult + 4, best_mult);
      }
    }
    const bool accept = best_probes == 1 || (best_probes <= 4 && bits >= std::min(min_bits + 4, kMaxHashBits));
    if (accept || bits == kMaxHashBits) {
      const size_t size = size_t(1) << bits, HS = hash_stride(W);
      image->assign(HS * size, 0u);
      for (size_t s = 0; s < size; ++s) (*image)[s * HS + W] = 0xFFFFFFFFu;   // empty
      place(best_mult, bits, image);
      im->hash_bits = bits;
      im->hash_probes = best_probes;
      std::copy(best_mult, best_mult + 4, im->hash_mult);
      return true;
    }
  }
  return false;
}

// cdf[cdf_len], padded with 0xFFFFFFFF to a power of two
inline bool put_cdf(const pbn_net_desc& d, NetImage* im, std::string* err) {
  const int N = d.n_nodes;
  im->cdf_len = 32;
  while (im->cdf_len < N) im->cdf_len <<= 1;
  im->tab.assign(im->cdf_len, 0xFFFFFFFFu);
  for (int m = 0; m < N; ++m) im->tab[m] = d.perturb_cdf[m];
  for (int m = 1; m < N; ++m)
    if (im->tab[m] < im->tab[m - 1]) return *err = "perturb_cdf must be non-decreasing", false;
  return true;
}

// reward rows by popcount(flipmask): {none, wrong attractor, target, 0} (one 16-byte read)
inline void put_reward_rows(const pbn_net_desc& d, NetImage* im) {
  const int N = d.n_nodes;
  for (int pc = 0; pc <= N; ++pc)
    for (int c = 0; c < 4; ++c) {
      uint32_t u = 0;
      if (c < 3) memcpy(&u, &d.reward_table[c * (N + 1) + pc], 4);
      im->tab.push_back(u);
    }
}

// the hash, then attractor start[A+1] | states[S][W], read by autoreset in the wave kernel
inline void put_attractors(const pbn_net_desc& d, const std::vector<uint32_t>& hash_img, NetImage* im) {
  const int A = im->n_attr, S = im->n_states, W = im->W;
  im->tab.insert(im->tab.end(), hash_img.begin(), hash_img.end());
  im->att_off = (int)im->tab.size();
  if (A) {
    for (int k = 0; k <= A; ++k) im->tab.push_back((uint32_t)d.attractor_start[k]);
    im->tab.insert(im->tab.end(), d.attractor_states, d.attractor_states + (size_t)S * W);
  }
  im->att_first.resize((size_t)A * W);
  for (int t = 0; t < A; ++t)
    for (int w = 0; w < W; ++w)
      im->att_first[(size_t)t * W + w] = d.attractor_states[(size_t)d.attractor_start[t] * W + w];
}

// records per node in the LDS image: no kernel reads record q >= max_nf (the chains stop at a
// node's function count, the padded ones at max_nf), so the image holds min(max_nf, kNodeRecs)
// of them at the [kNodeRecs]-layout's strides
inline int image_recs(const NetImage& im) { return std::min(std::max(im.max_nf, 1), kNodeRecs); }

// leaf selectors of the first Q functions of every node, uint4 [Q][2][32W] (lane-consecutive
// 16-byte reads); see eval_sel.  Records beyond a node's last function repeat the last one: the
// pipelined kernel's chain then needs no per-lane function count
inline void put_selectors(const pbn_net_desc& d, NetImage* im) {
  const int N = d.n_nodes, W = im->W, Q = image_recs(*im);
  align_tab(&im->tab, 4);
  im->sel_off = (int)im->tab.size();
  std::vector<uint32_t> sel((size_t)Q * 2 * 32 * W * 4, 0x0C0C0C0Cu);
  for (int i = 0; i < N; ++i) {
    const int f0 = d.node_func_start[i], nf = func_count(d, i);
    for (int q = 0; q < Q; ++q) {
      const int f = f0 + std::min(q, nf - 1);
      const uint32_t T16 = table16(d.func_table[f], d.func_arity[f]);
      for (int mm = 0; mm < 8; ++mm) {
        const uint32_t l0 = (T16 >> (2 * mm)) & 1u, l1 = (T16 >> (2 * mm + 1)) & 1u;   // x0 = 0, x0 = 1
        uint32_t word = 0;
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t b = (!l0 && !l1) ? 12u : (l0 && l1) ? 13u : (l1 ? j : 4u + j);
          word |= b << (8 * j);
        }
        sel[(((size_t)q * 2 + (mm >> 2)) * 32 * W + i) * 4 + (mm & 3)] = word;
      }
    }
  }
  im->tab.insert(im->tab.end(), sel.begin(), sel.end());
}

// threshold classes: the distinct values among the first kNodeRecs thresholds of all nodes; with
// at most kNodeRecs of them the kernels compare against wave-uniform digits (n_cls, uthr)
inline std::vector<uint32_t> classify_thresholds(const pbn_net_desc& d, NetImage* im) {
  std::vector<uint32_t> cls_of((size_t)d.n_funcs, 0u), vals;
  bool ok = true;
  for (int i = 0; i < d.n_nodes && ok; ++i) {
    const int f0 = d.node_func_start[i], nf = func_count(d, i);
    for (int q = 0; q < kNodeRecs && q < nf - 1; ++q) {
      auto it = std::find(vals.begin(), vals.end(), d.func_threshold[f0 + q]);
      if (it == vals.end()) {
        if ((int)vals.size() == kNodeRecs) { ok = false; break; }
        vals.push_back(d.func_threshold[f0 + q]);
        it = vals.end() - 1;
      }
      cls_of[f0 + q] = (uint32_t)(it - vals.begin());
    }
  }
  im->n_cls = ok ? (int)vals.size() : 0;
  for (int q = 0; q < kNodeRecs; ++q) im->uthr[q] = (ok && q < (int)vals.size()) ? vals[q] : 0u;
  return cls_of;
}

// fcompact and nrec (global memory), and the records in the LDS image, record-major uint4
// [Q][32W]: lane = node, so consecutive lanes read consecutive 16-byte records (no bank conflicts)
inline void put_node_records(const pbn_net_desc& d, const std::vector<uint32_t>& cls_of, NetImage* im) {
  const int N = d.n_nodes, W = im->W, Q = image_recs(*im);
  im->fcompact.assign((size_t)d.n_funcs * 4, 0u);
  for (int f = 0; f < d.n_funcs; ++f) {
    uint32_t ins = 0;   // missing inputs read plane 0
    for (int j = 0; j < d.func_arity[f]; ++j) ins |= plane_of(d.func_inputs[4 * f + j], N, W) << (8 * j);
    const uint32_t rec[4] = {ins, table16(d.func_table[f], d.func_arity[f]), d.func_threshold[f], 0u};
    std::copy(rec, rec + 4, &im->fcompact[(size_t)f * 4]);
  }
  im->nrec.assign((size_t)N * kNodeRecs * 4, 0u);
  auto rec_at = [&](int i, int q) { return &im->nrec[((size_t)i * kNodeRecs + q) * 4]; };
  for (int i = 0; i < N; ++i) {
    const int f0 = d.node_func_start[i], nf = func_count(d, i);
    for (int q = 0; q < kNodeRecs && q < nf; ++q) {
      std::copy(&im->fcompact[(size_t)(f0 + q) * 4], &im->fcompact[(size_t)(f0 + q) * 4] + 4, rec_at(i, q));
      rec_at(i, q)[1] = cls_of[f0 + q];   // threshold class (the table lives in the selectors)
    }
    rec_at(i, 0)[3] = (uint32_t)nf;
    rec_at(i, 1)[3] = (uint32_t)f0;
  }
  im->nrec_off = (int)im->tab.size();
  for (int q = 0; q < Q; ++q)
    for (int i = 0; i < 32 * W; ++i) {
      uint32_t r4[4] = {0, 0, 0, 0};
      if (i < N) {
        std::copy(rec_at(i, q), rec_at(i, q) + 4, r4);
        const int nf = func_count(d, i);
        if (q >= nf) r4[0] = rec_at(i, nf - 1)[0];   // padded inputs as the selectors (the .w metadata stays)
      }
      if (W <= 2) r4[0] *= 4u;   // plane byte offsets (every index < 64: no carry between bytes)
      im->tab.insert(im->tab.end(), r4, r4 + 4);
    }
}

// gate records by level: {input planes as bytes, 16-bit table, output plane 32W + g, 0}, then
// the level starts [n_glayers + 1]
inline void put_gates(const pbn_net_desc& d, const std::vector<int>& glevel, NetImage* im) {
  const int N = d.n_nodes, W = im->W, n_gates = d.n_gates;
  if (!n_gates) return;
  const int n_lv = *std::max_element(glevel.begin(), glevel.end());
  std::vector<int> order(n_gates);
  for (int g = 0; g < n_gates; ++g) order[g] = g;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return glevel[x] < glevel[y]; });
  im->gate_off = (int)im->tab.size();
  std::vector<int> starts(n_lv + 1, 0);
  for (int idx = 0; idx < n_gates; ++idx) {
    const int g = order[idx], k = d.gate_arity[g];
    uint32_t ins = 0;
    for (int j = 0; j < k; ++j) ins |= plane_of(d.gate_inputs[4 * g + j], N, W) << (8 * j);
    const uint32_t rec[4] = {ins, table16(d.gate_table[g], k), (uint32_t)(32 * W + g), 0u};
    im->tab.insert(im->tab.end(), rec, rec + 4);
    starts[glevel[g]] = idx + 1;   // running end of each level (levels are contiguous)
  }
  im->glayer_off = (int)im->tab.size();
  im->tab.push_back(0u);
  for (int lv = 1; lv <= n_lv; ++lv) {
    if (starts[lv] == 0) starts[lv] = starts[lv - 1];
    im->tab.push_back((uint32_t)starts[lv]);
  }
  im->n_glayers = n_lv;
}

// gap bucket table, uint2 [gap_nb + 1] {threshold, gap}: the smallest bucket width 2^shift,
// shift = 32 - k with k = 6..10, under which every bucket below C[N-1] holds at most one CDF
// threshold; none found (p tiny) -> the estimate / binary search paths (gap_exact)
inline void put_gap_table(const pbn_net_desc& d, NetImage* im) {
  const int N = d.n_nodes;
  const double p = (double)d.perturb_cdf[0] / 4294967296.0;
  const bool exact = p < 1e-6 || p > 0.5;
  auto gap_at = [&](uint64_t u) {   // min{m : u < C[m-1]}, N+1 if none
    int m = 1;
    while (m <= N && (uint64_t)d.perturb_cdf[m - 1] <= u) ++m;
    return m;
  };
  for (int k = 6; k <= 10 && !exact && !im->gap_nb; ++k) {
    const int shift = 32 - k;
    const uint64_t w = 1ull << shift;
    const uint32_t nb = (uint32_t)(((uint64_t)d.perturb_cdf[N - 1]) >> shift) + 1u;   // buckets that can see a flip
    bool ok = true;
    std::vector<uint32_t> lut;
    for (uint32_t b = 0; b < nb && ok; ++b) {
      const int lo = gap_at((uint64_t)b * w), hi = gap_at((uint64_t)b * w + w - 1);
      ok = hi - lo <= 1;
      lut.push_back(lo <= N ? d.perturb_cdf[lo - 1] : 0xFFFFFFFFu);
      lut.push_back((uint32_t)lo);
    }
    if (!ok) continue;
    lut.push_back(0xFFFFFFFFu);   // sentinel: u >= C[N-1] -> gap N+1 (u = 2^32-1 gives N+2, also no flip)
    lut.push_back((uint32_t)(N + 1));
    align_tab(&im->tab, 2);
    im->gap_lut_off = (int)im->tab.size();
    im->tab.insert(im->tab.end(), lut.begin(), lut.end());
    im->gap_shift = shift;
    im->gap_nb = (int)nb;
  }
  im->gap_exact = exact ? 1 : (im->gap_nb ? 2 : 0);
  im->inv_log2q = im->gap_exact ? 0.f : (float)(1.0 / log2(1.0 - p));
}

// the pipelined one-update kernel's threshold digit masks (single-word states), lane-major
// [32][sel_mask_stride(B)]: mask (i, q, d) = ~0 if bit B-1-d of node i's threshold q is set.  In
// the image they arrive with the table copy; built by each block from the LDS records, they
// cost a second prologue barrier (DESIGN.md "Launch anatomy")
inline void put_digit_masks(const pbn_net_desc& d, NetImage* im) {
  if (im->W != 1) return;
  align_tab(&im->tab, 4);
  im->cm_off = (int)im->tab.size();
  const int B = d.prob_bits, S = sel_mask_stride(B);
  std::vector<uint32_t> cmv((size_t)32 * S, 0u);
  for (int i = 0; i < d.n_nodes; ++i) {
    const int f0 = d.node_func_start[i], nf = func_count(d, i);
    for (int q = 0; q < kNodeRecs - 1 && q < nf - 1; ++q) {
      const uint32_t c = d.func_threshold[f0 + q];
      for (int dd = 0; dd < B; ++dd) cmv[(size_t)i * S + q * B + dd] = ((c >> (B - 1 - dd)) & 1u) ? ~0u : 0u;
    }
  }
  im->tab.insert(im->tab.end(), cmv.begin(), cmv.end());
}

// the settle law's per-env selection thresholds (settle_lt_word): node i, threshold q < nf_i - 1
// as c << (16 - B), 65536 (always) past a node's last function and past the network; and the
// packed biased node pairs for settle_lt_word_pk, exact when no compared threshold is 65536
inline void build_settle_thresholds(const pbn_net_desc& d, NetImage* im) {
  const int N = d.n_nodes, W = im->W, lq = im->lq;
  im->sthr.assign((size_t)lq * 32 * W, 65536u);
  for (int i = 0; i < N; ++i) {
    const int f0 = d.node_func_start[i], nf = func_count(d, i);
    for (int q = 0; q < nf - 1 && q < lq; ++q)
      im->sthr[(size_t)q * 32 * W + i] = d.func_threshold[f0 + q] << (16 - d.prob_bits);
  }
  im->sthr_pk.assign((size_t)lq * W * 16, 0u);
  im->settle_pk = 1;
  for (int q = 0; q < lq; ++q)
    for (int i = 0; i < 32 * W; i += 2) {
      uint32_t c[2];
      for (int h = 0; h < 2; ++h) {
        const int ii = i + h;
        const bool real = ii < N && q < func_count(d, ii) - 1;
        const uint32_t v = im->sthr[(size_t)q * 32 * W + ii];
        if (real && v > 65535u) im->settle_pk = 0;
        c[h] = std::min(v, 65535u) ^ 0x8000u;
      }
      im->sthr_pk[((size_t)q * W + i / 32) * 16 + (i % 32) / 2] = c[0] | (c[1] << 16);
    }
}

// multiply-high divisors (exact for the operand ranges used: see actions_from_draw, autoreset),
// and the kernels' LDS needs
inline void finish_scalars(NetImage* im) {
  const int N = im->n_nodes, A = im->n_attr, W = im->W;
  im->n1_magic = (uint32_t)(((1ull << 32) + (uint64_t)N) / (uint64_t)(N + 1));
  im->att_single = A >= 1 && im->n_states == A ? 1 : 0;
  im->am1_magic = A >= 3 ? (uint32_t)(((1ull << 32) + (uint64_t)(A - 2)) / (uint64_t)(A - 1)) : 0u;   // 0: A - 1 == 1
  im->x_mult = (uint64_t)(N + 1) * (uint64_t)(N + 1) * (uint64_t)(N + 1) * (A >= 2 ? (uint64_t)A * (uint64_t)(A - 1) : 1ull);
  im->wave_words = wave_plane_words(W, im->n_gates);
  im->slot_words = pipe_slot_words(W, im->lq);
  im->slot_words_settle = settle_slot_words(W, im->lq);
  im->lds_wave = wave_lds_words(im->tab_words, im->wave_words) * 4;
  im->lds_pipe = pipe_lds_words(im->tab_words, W, im->lq) * 4;
  im->lds_settle = settle_lds_words(im->tab_words, W, im->lq) * 4;
}

}  // namespace image

// PBN_OK, or PBN_EINVAL with the reason in *err
inline int compile_net(const pbn_net_desc* d, NetImage* im, std::string* err) {
  using namespace image;
  std::vector<int> glevel;
  std::vector<uint32_t> ids, hash_img;
  if (!check_header(*d, err) || !check_gates(*d, &glevel, err) || !check_funcs(*d, err) ||
      !check_attractors(*d, &ids, err))
    return PBN_EINVAL;
  *im = NetImage();
  im->n_nodes = d->n_nodes;
  im->W = (d->n_nodes + 31) / 32;
  im->prob_bits = d->prob_bits;
  im->horizon = d->horizon;
  im->n_funcs = d->n_funcs;
  im->n_gates = d->n_gates;
  im->settle_max = d->settle_max;
  im->n_attr = d->n_attractors;
  im->n_states = d->n_attractors ? d->n_attractor_states : 0;
  for (int i = 0; i < d->n_nodes; ++i) im->max_nf = std::max(im->max_nf, func_count(*d, i));
  im->lq = std::max(im->max_nf - 1, 1);
  if (im->n_attr && !build_hash(d->attractor_states, ids, im->W, im, &hash_img))
    return *err = "too many attractor states for the LDS hash", PBN_EINVAL;
  if (!put_cdf(*d, im, err)) return PBN_EINVAL;
  put_reward_rows(*d, im);
  put_attractors(*d, hash_img, im);
  put_selectors(*d, im);
  put_node_records(*d, classify_thresholds(*d, im), im);
  put_gates(*d, glevel, im);
  put_gap_table(*d, im);
  put_digit_masks(*d, im);
  align_tab(&im->tab, 4);   // the kernels copy the image as uint4
  im->tab_words = (int)im->tab.size();
  build_settle_thresholds(*d, im);
  finish_scalars(im);
  return PBN_OK;
}

}  // namespace pbn
