// Stand-alone host check of csrc/curriculum_law.h (no GPU, no Python): the table build and the draw
// as pbn_curriculum.hip's kernels call them, driven by commands on stdin, one result line per
// command.  tests/test_curriculum_host.py compiles it (host side only) and compares the lines with
// tests/curriculum_reference.py.
//   tab A H n (s t E L)*n     the table of a pairs matrix that is zero but for the n listed entries:
//                             total, bytes, then rowcdf[0..A) and cdf[0..A*A)
//   first a[0..A]             the attractor-state table's att_start of the draws below
//   draw x0 x1 x2 x3          s t row of the restart drawn from the four words
//   phx seed id step          the four words of the CURRICULUM call (draw(seed, id, step, 8, 0))
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "curriculum_law.h"

namespace {

int g_A = 0;
uint64_t g_total = 0;
std::vector<uint64_t> g_rowcdf;
std::vector<uint32_t> g_cdf;
std::vector<int32_t> g_first;

bool next_u64(char*& p, uint64_t* out) {
  char* end;
  *out = strtoull(p, &end, 10);
  if (end == p) return false;
  p = end;
  return true;
}

}  // namespace

int main() {
  std::vector<char> line(1 << 24);
  while (fgets(line.data(), (int)line.size(), stdin)) {
    char* p = line.data();
    char cmd[8] = {0};
    int used = 0;
    if (sscanf(p, "%7s%n", cmd, &used) != 1) continue;
    p += used;
    uint64_t v[4];
    if (!strcmp(cmd, "tab")) {
      uint64_t A, H, n;
      if (!next_u64(p, &A) || !next_u64(p, &H) || !next_u64(p, &n) || A < 2 || A > 254) return 2;
      std::vector<int64_t> pairs(A * A * pbn::kStatPairFields, 0);
      for (uint64_t j = 0; j < n; ++j) {
        if (!next_u64(p, &v[0]) || !next_u64(p, &v[1]) || !next_u64(p, &v[2]) || !next_u64(p, &v[3])) return 2;
        if (v[0] >= A || v[1] >= A) return 2;
        int64_t* e = &pairs[(v[0] * A + v[1]) * pbn::kStatPairFields];
        e[0] = (int64_t)v[2];
        e[2] = (int64_t)v[3];
      }
      g_A = (int)A;
      g_rowcdf.assign(A, 0);
      g_cdf.assign(A * A, 0);
      g_total = pbn::curriculum_build(g_A, (uint32_t)H, pairs.data(), g_rowcdf.data(), g_cdf.data());
      printf("tab %" PRIu64 " %lld", g_total, (long long)pbn::curriculum_table_bytes(g_A));
      for (uint64_t r : g_rowcdf) printf(" %" PRIu64, r);
      for (uint32_t c : g_cdf) printf(" %u", c);
      printf("\n");
    } else if (!strcmp(cmd, "first")) {
      g_first.clear();
      while (next_u64(p, &v[0])) g_first.push_back((int32_t)v[0]);
      printf("first %zu\n", g_first.size());
    } else if (!strcmp(cmd, "draw")) {
      if (!next_u64(p, &v[0]) || !next_u64(p, &v[1]) || !next_u64(p, &v[2]) || !next_u64(p, &v[3])) return 2;
      if ((int)g_first.size() != g_A + 1) return 3;
      const pbn::Word4 x{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]};
      const pbn::CurriculumDraw d = pbn::curriculum_draw(
          x, g_A, g_total, [](int s) { return g_rowcdf[s]; }, [](int s, int t) { return g_cdf[(size_t)s * g_A + t]; },
          [](int a) { return g_first[a]; });
      printf("draw %u %u %u\n", d.s, d.t, d.row);
    } else if (!strcmp(cmd, "phx")) {
      if (!next_u64(p, &v[0]) || !next_u64(p, &v[1]) || !next_u64(p, &v[2])) return 2;
      const pbn::Word4 x = pbn::draw(v[0], v[1], v[2], pbn::kStreamCurriculum, 0u);
      printf("phx %u %u %u %u\n", x.x, x.y, x.z, x.w);
    } else {
      return 4;
    }
  }
  return 0;
}
