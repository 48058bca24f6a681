// Stand-alone dump of csrc/bdq_layout.h (no GPU, no Python, no HIP): for every shape of the sweep,
// one JSON object per line with the flat parameter layout, the network image, the workspace, the
// two LDS carvings and the apply launch's tasks, for tests/test_bdq_layout_host.py to hold against
// its own statement of them.  Built there with -fsanitize=address,undefined: the host sanitizer
// run of the layout code.
#include <stdio.h>

#include "bdq_layout.h"

using namespace bdq;

namespace {

// What the header spells out for the sake of the kernels' listings (fwd_bias_at, fwd_bias_src,
// PBN_LAYER_W_OFF, BwdLds::planes), held to layer() and to the carving's own sums.
constexpr bool spellings_ok(int H, int A, int Apad, int K) {
  int64_t id[TOTAL + 1] = {};   // a segment's "offset" names it
  for (int s = 0; s <= TOTAL; ++s) id[s] = 1000000LL * s;
  if (fwd_bias_src(id, H, 0) != id[BIL_B] || fwd_bias_src(id, H, kD0 - 1) != id[BIL_B] + kD0 - 1) return false;
  int o = kD0;
  for (int l = 0; l < NLAY; ++l) {
    const Layer y = layer(l, H, A);
    if (fwd_bias_at(l, H) != o) return false;
    if (fwd_bias_src(id, H, o) != id[y.b] || fwd_bias_src(id, H, o + y.rows - 1) != id[y.b] + y.rows - 1) return false;
    if (l < LYH2 && PBN_LAYER_W_OFF(id, l) != id[y.w]) return false;
    o += y.rows;
  }
  const BwdLds b(H, Apad, K);
  return fwd_bias_floats(H, A) == o && b.planes() == b.trunk() + b.trunk_end;
}
static_assert(spellings_ok(2, 2, 16, 1) && spellings_ok(8, 128, 128, 7), "bdq_layout.h: a spelled-out copy has drifted");

void ints(const char* key, const int64_t* v, int n, const char* end = ",") {
  printf("\"%s\":[", key);
  for (int i = 0; i < n; ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
  printf("]%s", end);
}

struct Region {
  const char* name;
  int at;   // 4-byte words from the start of the block's LDS
};
void regions(const char* key, const Region* r, int n, int end_words, size_t bytes) {
  printf("\"%s\":{\"regions\":[", key);
  for (int i = 0; i < n; ++i) printf("%s[\"%s\",%d]", i ? "," : "", r[i].name, r[i].at);
  printf("],\"end\":%d,\"bytes\":%zu},", end_words, bytes);
}

// learn_apply_kernel's decode of a task, restated over the header's counts (the kernel keeps its
// chain in line): lay -1 is the bilinear layer (ot, i); ot counts the layer's tiles in the image
struct Task {
  int lay, ot, kt;
};
Task decode(int task, int N, int H, int at16) {
  if (task < apply_bil_tasks(N)) return {-1, task / N, task % N};
  task -= apply_bil_tasks(N);
  for (int l = 0; l < NLAY; ++l) {
    const int n = apply_tiles(l, H, at16);
    if (task < n) {
      int ot0 = 0;
      if (l == LYH2) {
        const int per = apply_tiles(LYH2, 1, at16), h = task / per;
        task -= h * per;
        ot0 = h * at16;
      }
      const int kts = layer(l).cols / 16;
      return {l, ot0 + task / kts, task % kts};
    }
    task -= n;
  }
  return {NLAY, 0, 0};
}

void dump(int N, int K, int64_t B, int n_attr) {
  const int H = K + 1, A = N + 1, Ap = apad(N);
  printf("{\"N\":%d,\"K\":%d,\"B\":%lld,\"n_attr\":%d,\"Apad\":%d,\"W\":%d,\"NT\":%d,", N, K, (long long)B, n_attr, Ap,
         state_words(N), bil_col_tiles(N));

  int64_t off[TOTAL + 1];
  make_layout(N, H, off);
  ints("layout", off, TOTAL + 1);

  ImageLayout im;
  make_image(N, H, n_attr, &im);
  int64_t rc[2 * NLAY];
  for (int l = 0; l < NLAY; ++l) {
    rc[2 * l] = layer(l, H, Ap).rows;
    rc[2 * l + 1] = layer(l, H, Ap).cols;
  }
  ints("image_fwd", im.fwd, NLAY);
  ints("image_bwd", im.bwd, NLAY);
  ints("image_rows_cols", rc, 2 * NLAY);
  printf("\"image_total\":%lld,", (long long)im.total);

  const Work w = make_work(N, H, B);
  printf("\"work\":[");
  const char* sep = "";
#define PBN_X(type, name, n)                                              \
  printf("%s[\"%s\",%lld,%zu]", sep, #name, (long long)w.name, sizeof(type)); \
  sep = ",";
  PBN_BDQ_WORK(PBN_X)
#undef PBN_X
  printf("],\"work_total\":%lld,", (long long)w.total);

  const FwdLds f(H, A);
  const int ft = f.tail();
  const Region fr[] = {{"y1", f.y1},         {"x2", f.x2},           {"x3", f.x3},
                       {"x4", f.x4},         {"xh", f.xh},           {"sw", ft + f.sw},
                       {"stg", ft + f.stg},  {"scnt", ft + f.scnt},  {"slist", ft + f.slist},
                       {"sbias", ft + f.sbias}};
  regions("fwd_lds", fr, sizeof fr / sizeof fr[0], f.end(), f.bytes());
  printf("\"fwd_bias_floats\":%d,", fwd_bias_floats(H, A));
  int64_t bias_src[4096];
  const int nb = fwd_bias_floats(H, A);
  for (int i = 0; i < nb; ++i) bias_src[i] = fwd_bias_src(off, H, i);
  ints("fwd_bias_src", bias_src, nb);

  const BwdLds b(H, Ap, K);
  const int bt = b.trunk();
  const Region br[] = {{"dh", b.dh},           {"dhh", b.dhh()},        {"dh4", bt + b.dh4}, {"dh3", bt + b.dh3},
                       {"dh2", bt + b.dh2},    {"part", bt + b.part},   {"planes_end", b.planes()},
                       {"sg", b.td()},         {"sd", b.td() + b.td_words()},
                       {"sact", b.td() + 2 * b.td_words()}};
  regions("bwd_lds", br, sizeof br / sizeof br[0], b.end(), b.bytes());
  printf("\"bwd_staged\":[%d,%d,%d],", b.sh, b.pitch(), b.staged());
  printf("\"bwd_refused\":%d,", b.bytes() > kLdsBytes ? 1 : 0);

  int64_t tiles[NLAY];
  for (int l = 0; l < NLAY; ++l) tiles[l] = apply_tiles(l, H, Ap / 16);
  ints("apply_tiles", tiles, NLAY);
  const int ntasks = apply_tasks(N, H, Ap / 16);
  printf("\"apply_bil\":%d,\"apply_tasks\":%d,\"apply_blocks\":%d,\"apply_waves\":%d", apply_bil_tasks(N), ntasks,
         apply_blocks(N, H, Ap / 16), kApplyWaves);
  if (B == 16 && n_attr == 0) {   // (the decode depends on neither)
    printf(",\"decode\":[");
    for (int t = 0; t < ntasks; ++t) {
      const Task d = decode(t, N, H, Ap / 16);
      printf("%s[%d,%d,%d]", t ? "," : "", d.lay, d.ot, d.kt);
    }
    printf("],\"decode_past\":%d", decode(ntasks, N, H, Ap / 16).lay);
  }
  printf("}\n");
}

}  // namespace

int main() {
  const int shapes[][2] = {{1, 1}, {15, 3}, {16, 3}, {28, 3}, {31, 7}, {95, 7}, {96, 6}, {96, 7}, {127, 1}, {127, 7}};
  const int64_t batches[] = {16, 256};
  const int n_attrs[] = {0, 14};
  for (const auto& s : shapes)
    for (int64_t B : batches)
      for (int n_attr : n_attrs) dump(s[0], s[1], B, n_attr);
  return 0;
}
