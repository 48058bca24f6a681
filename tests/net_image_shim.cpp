// C entry points around csrc/net_image.h for tests/test_net_image.py (ctypes): compile a
// descriptor on the CPU and read the image's vectors and scalars by name.
#include <stdio.h>
#include <string.h>

#include <string>

#include "net_image.h"

extern "C" {

// the compiled image (ni_free it), or null with the return code in *rc and the reason in err
void* ni_compile(const pbn_net_desc* d, int* rc, char* err, int err_len) {
  auto* im = new pbn::NetImage();
  std::string why;
  *rc = pbn::compile_net(d, im, &why);
  snprintf(err, (size_t)err_len, "%s", why.c_str());
  if (*rc == PBN_OK) return im;
  delete im;
  return nullptr;
}

void ni_free(void* h) { delete static_cast<pbn::NetImage*>(h); }

const uint32_t* ni_vector(void* h, const char* name, int64_t* n) {
  const pbn::NetImage& im = *static_cast<pbn::NetImage*>(h);
  const std::string s = name;
  const std::vector<uint32_t>* v = s == "tab" ? &im.tab : s == "fcompact" ? &im.fcompact : s == "nrec" ? &im.nrec
                                 : s == "sthr" ? &im.sthr : s == "sthr_pk" ? &im.sthr_pk
                                 : s == "att_first" ? &im.att_first : nullptr;
  if (s == "uthr") return *n = kNodeRecs, im.uthr;
  if (s == "hash_mult") return *n = 4, im.hash_mult;
  if (!v) return *n = -1, nullptr;
  return *n = (int64_t)v->size(), v->data();
}

// 1 and *out, or 0 for an unknown name
int ni_scalar(void* h, const char* name, uint64_t* out) {
  const pbn::NetImage& im = *static_cast<pbn::NetImage*>(h);
  const std::string s = name;
  uint32_t inv_log2q_bits;
  memcpy(&inv_log2q_bits, &im.inv_log2q, 4);
#define NI_FIELD(f) if (s == #f) return *out = (uint64_t)im.f, 1;
  NI_FIELD(n_nodes) NI_FIELD(W) NI_FIELD(n_attr) NI_FIELD(horizon) NI_FIELD(cdf_len) NI_FIELD(hash_bits)
  NI_FIELD(hash_probes) NI_FIELD(tab_words) NI_FIELD(prob_bits) NI_FIELD(n_funcs) NI_FIELD(wave_words)
  NI_FIELD(gap_exact) NI_FIELD(gap_lut_off) NI_FIELD(gap_shift) NI_FIELD(gap_nb) NI_FIELD(n_states)
  NI_FIELD(att_off) NI_FIELD(sel_off) NI_FIELD(nrec_off) NI_FIELD(cm_off) NI_FIELD(n_cls) NI_FIELD(max_nf)
  NI_FIELD(lq) NI_FIELD(slot_words) NI_FIELD(gate_off) NI_FIELD(glayer_off) NI_FIELD(n_glayers)
  NI_FIELD(att_single) NI_FIELD(n1_magic) NI_FIELD(am1_magic) NI_FIELD(x_mult) NI_FIELD(settle_max)
  NI_FIELD(settle_pk) NI_FIELD(n_gates) NI_FIELD(slot_words_settle) NI_FIELD(lds_wave) NI_FIELD(lds_pipe)
  NI_FIELD(lds_settle)
#undef NI_FIELD
  if (s == "inv_log2q_bits") return *out = inv_log2q_bits, 1;
  return 0;
}

}  // extern "C"
