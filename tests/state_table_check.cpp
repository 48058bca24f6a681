// Stand-alone host check of csrc/state_table.h (no GPU, no Python): the hash, the masked key load,
// the key compare and the probe loop as the insert kernel runs them, with a single thread's
// atomics.  Driven by commands on stdin, one result line per command;
// tests/test_state_table_host.py compiles it (host side only) and compares with numpy.
//   table W n_bits cap                     a fresh, empty table
//   insert epoch T n_cols stride has_counts <T * W * stride words> [T * n_cols counts]
//                                          one launch over the rows -> used lost
//   rehash cap                             the table's entries into a fresh table of cap slots, as a
//                                          launch over its keys with its counts -> used lost
//   drain                                  S, then per used slot (in slot order) W words and the count
//   disp                                   sum over the used slots of the probe displacement, and S
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "state_table.h"

namespace {

struct Table {
  int W = 1, n_bits = 32;
  int64_t cap = 0;
  std::vector<uint64_t> owner, counts;
  std::vector<uint32_t> keys;
  uint64_t used = 0, lost = 0;
  void reset(int W_, int n_bits_, int64_t cap_) {
    W = W_, n_bits = n_bits_, cap = cap_;
    owner.assign(cap, 0);
    counts.assign(cap, 0);
    keys.assign((size_t)W * cap, 0);
    used = lost = 0;
  }
  pbn::TableArrays arrays() { return {owner.data(), keys.data(), counts.data(), &used, &lost, cap}; }
};

Table g_tab;

void launch(Table& t, const uint32_t* states, int64_t T, int64_t n_cols, int64_t stride, const uint64_t* row_counts,
            uint32_t epoch) {
  const pbn::TableInput in{states, n_cols, stride, pbn::table_top_mask(t.W, t.n_bits)};
  switch (t.W) {
    case 1: pbn::table_insert_host<1>(t.arrays(), in, T, row_counts, epoch); break;
    case 2: pbn::table_insert_host<2>(t.arrays(), in, T, row_counts, epoch); break;
    case 3: pbn::table_insert_host<3>(t.arrays(), in, T, row_counts, epoch); break;
    default: pbn::table_insert_host<4>(t.arrays(), in, T, row_counts, epoch); break;
  }
}

template <int W>
uint32_t hash_w(const Table& t, int64_t slot) {
  uint32_t k[W];
  for (int w = 0; w < W; ++w) k[w] = t.keys[(size_t)w * t.cap + slot];
  return pbn::table_hash<W>(k);
}

uint32_t hash_of(const Table& t, int64_t slot) {
  switch (t.W) {
    case 1: return hash_w<1>(t, slot);
    case 2: return hash_w<2>(t, slot);
    case 3: return hash_w<3>(t, slot);
    default: return hash_w<4>(t, slot);
  }
}

}  // namespace

int main() {
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "table")) {
      int W, n_bits;
      long long cap;
      if (scanf("%d %d %lld", &W, &n_bits, &cap) != 3 || W < 1 || W > 4 || cap < 1 || (cap & (cap - 1))) return 2;
      g_tab.reset(W, n_bits, cap);
      printf("table 0\n");
    } else if (!strcmp(cmd, "insert")) {
      unsigned epoch;
      long long T, n_cols, stride;
      int has_counts;
      if (scanf("%u %lld %lld %lld %d", &epoch, &T, &n_cols, &stride, &has_counts) != 5 || n_cols > stride) return 2;
      std::vector<uint32_t> st((size_t)(T * g_tab.W * stride));
      for (auto& v : st)
        if (scanf("%" SCNu32, &v) != 1) return 2;
      std::vector<uint64_t> rc(has_counts ? (size_t)(T * n_cols) : 0);
      for (auto& v : rc)
        if (scanf("%" SCNu64, &v) != 1) return 2;
      launch(g_tab, st.data(), T, n_cols, stride, has_counts ? rc.data() : nullptr, epoch);
      printf("insert %" PRIu64 " %" PRIu64 "\n", g_tab.used, g_tab.lost);
    } else if (!strcmp(cmd, "rehash")) {
      long long cap;
      if (scanf("%lld", &cap) != 1 || cap < 1 || (cap & (cap - 1))) return 2;
      Table next;
      next.reset(g_tab.W, g_tab.n_bits, cap);
      launch(next, g_tab.keys.data(), 1, g_tab.cap, g_tab.cap, g_tab.counts.data(), 1);
      g_tab = next;
      printf("rehash %" PRIu64 " %" PRIu64 "\n", g_tab.used, g_tab.lost);
    } else if (!strcmp(cmd, "drain")) {
      printf("drain %" PRIu64, g_tab.used);
      for (int64_t s = 0; s < g_tab.cap; ++s) {
        if (g_tab.owner[s] == 0) continue;
        for (int w = 0; w < g_tab.W; ++w) printf(" %" PRIu32, g_tab.keys[(size_t)w * g_tab.cap + s]);
        printf(" %" PRIu64, g_tab.counts[s]);
      }
      printf("\n");
    } else if (!strcmp(cmd, "disp")) {
      uint64_t sum = 0, n = 0;
      for (int64_t s = 0; s < g_tab.cap; ++s) {
        if (g_tab.owner[s] == 0) continue;
        const int64_t home = (int64_t)(hash_of(g_tab, s) & (uint64_t)(g_tab.cap - 1));
        sum += (uint64_t)((s - home) & (g_tab.cap - 1));
        ++n;
      }
      printf("disp %" PRIu64 " %" PRIu64 "\n", sum, n);
    } else {
      return 2;
    }
  }
  return 0;
}
