// Stand-alone check of csrc/net_image.h and net_layout.h (no GPU, no Python): three hand-written
// descriptors through compile_net, and route_launch against the two conditions of the launcher
// it replaced, over every combination of its inputs.  Built plain by tests/test_net_image.py;
// built with -fsanitize=address,undefined it is the host sanitizer run of the compiler.
#include <stdio.h>

#include <string>
#include <vector>

#include "net_image.h"

namespace {

int g_failed = 0;
#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                  \
    }                                                              \
  } while (0)

// a network of identity functions (node i <- node i), one function per node, and the tables
// the descriptor points into
struct Desc {
  std::vector<int32_t> func_start, arity, inputs, att_start, gate_arity, gate_inputs;
  std::vector<uint32_t> table, threshold, cdf, att_states, gate_table;
  std::vector<float> reward;
  pbn_net_desc d{};
  explicit Desc(int N) {
    for (int i = 0; i < N; ++i) {
      func_start.push_back(i);
      arity.push_back(1);
      const int in[4] = {i, 0, 0, 0};
      inputs.insert(inputs.end(), in, in + 4);
      table.push_back(0x2u);
      threshold.push_back(1u << 16);
      cdf.push_back((uint32_t)(((uint64_t)(i + 1) << 32) / (uint64_t)(N + 1)));
    }
    func_start.push_back(N);
    reward.assign(4 * (size_t)(N + 1), -1.f);
    d.n_nodes = N;
    d.n_funcs = N;
    d.prob_bits = 16;
    d.horizon = 20;
  }
  const pbn_net_desc* get() {
    d.node_func_start = func_start.data();
    d.func_arity = arity.data();
    d.func_inputs = inputs.data();
    d.func_table = table.data();
    d.func_threshold = threshold.data();
    d.perturb_cdf = cdf.data();
    d.reward_table = reward.data();
    d.n_attractors = att_start.empty() ? 0 : (int)att_start.size() - 1;
    d.n_attractor_states = att_start.empty() ? 0 : att_start.back();
    d.attractor_start = att_start.empty() ? nullptr : att_start.data();
    d.attractor_states = att_states.empty() ? nullptr : att_states.data();
    d.n_gates = (int)gate_arity.size();
    d.gate_arity = gate_arity.data();
    d.gate_inputs = gate_inputs.data();
    d.gate_table = gate_table.data();
    return &d;
  }
};

void check_image(const pbn::NetImage& im) {
  EXPECT(im.tab_words == (int)im.tab.size() && im.tab_words % 4 == 0);
  EXPECT(im.sel_off % 4 == 0 && im.att_off <= im.sel_off && im.sel_off < im.nrec_off && im.nrec_off < im.tab_words);
  EXPECT(im.fcompact.size() == 4 * (size_t)im.n_funcs);
  EXPECT(im.nrec.size() == 4 * (size_t)im.n_nodes * kNodeRecs);
  EXPECT(im.sthr.size() == (size_t)im.lq * 32 * im.W && im.sthr_pk.size() == (size_t)im.lq * im.W * 16);
  EXPECT(im.att_first.size() == (size_t)im.n_attr * im.W);
  EXPECT(im.lds_wave == ((size_t)im.tab_words + 4 * (size_t)im.wave_words) * 4);
}

void one_node_no_attractors() {
  Desc n(1);
  n.arity[0] = 0;   // a constant function
  n.table[0] = 1u;
  pbn::NetImage im;
  std::string err;
  EXPECT(pbn::compile_net(n.get(), &im, &err) == PBN_OK);
  check_image(im);
  EXPECT(im.W == 1 && im.n_attr == 0 && im.hash_bits == 0 && im.att_off == im.cdf_len + 8);
  EXPECT(im.max_nf == 1 && im.lq == 1 && im.cm_off > 0 && im.n_gates == 0 && im.n_glayers == 0);
  EXPECT(im.fcompact[1] == 0xFFFFu);   // the constant 1 over four inputs
}

Desc gated33() {
  Desc n(33);
  n.gate_arity = {2};
  n.gate_inputs = {1, 2, 0, 0};
  n.gate_table = {0x8u};   // AND
  n.inputs[0] = 33;        // node 0 <- the gate
  n.att_start = {0, 2};
  n.att_states = {0x0u, 0x0u, 0xFFFFFFFFu, 0x1u};
  return n;
}

void gate_and_two_state_attractor() {
  Desc n = gated33();
  pbn::NetImage im;
  std::string err;
  EXPECT(pbn::compile_net(n.get(), &im, &err) == PBN_OK);
  check_image(im);
  EXPECT(im.W == 2 && im.n_attr == 1 && im.n_states == 2 && im.att_single == 0 && im.hash_bits >= 2);
  EXPECT(im.n_gates == 1 && im.n_glayers == 1 && im.cm_off == 0);
  EXPECT(im.wave_words == 68);                       // 64 node planes + 1 gate plane, rounded to 4
  EXPECT((im.fcompact[0] & 0xFFu) == 64u);           // node 0 reads the gate's plane
  EXPECT(im.tab[im.gate_off] == (1u | (2u << 8)) && im.tab[im.gate_off + 1] == 0x8888u &&
         im.tab[im.gate_off + 2] == 64u);
  EXPECT(im.tab[im.glayer_off] == 0u && im.tab[im.glayer_off + 1] == 1u);
  EXPECT(im.att_first[0] == 0u && im.att_first[1] == 0u);
  int found = 0;   // both states sit in the hash with the attractor's id
  for (int s = 0; s < (1 << im.hash_bits); ++s) {
    const uint32_t* e = &im.tab[im.cdf_len + 4 * 34 + (size_t)s * hash_stride(2)];
    if (e[2] == 0u) ++found;
  }
  EXPECT(found == 2);
}

void rejected_after_the_hash() {
  Desc n = gated33();
  n.cdf[5] = n.cdf[4] - 1;
  pbn::NetImage im;
  std::string err;
  EXPECT(pbn::compile_net(n.get(), &im, &err) == PBN_EINVAL);
  EXPECT(err == "perturb_cdf must be non-decreasing");
}

// the launcher before route_launch: step_impl's and rollout_impl's conditions, as they stood
bool old_step_pipes(int settle_max, bool whole, bool pipe_settle, int n_gates, size_t lds_settle, int force_roll) {
  return settle_max >= 2 && whole && pipe_settle && !n_gates && lds_settle <= 64 * 1024 && force_roll != 2;
}
bool old_rollout_pipes(int settle_max, bool pipe_settle, int n_gates, size_t lds_pipe, size_t lds_settle,
                       int force_roll) {
  const bool settle = settle_max >= 2;
  bool pipe = (settle ? lds_settle : lds_pipe) <= 64 * 1024 && !n_gates && (!settle || pipe_settle);
  if (force_roll) pipe = force_roll == 3 && !n_gates && (!settle || pipe_settle);
  return pipe;
}

void routing() {
  const size_t sizes[2] = {64 * 1024, 64 * 1024 + 4};
  const int settles[3] = {0, 1, 64}, forces[3] = {0, 2, 3};
  for (int settle_max : settles)
    for (int force : forces)
      for (int bits = 0; bits < 32; ++bits) {
        const bool whole = bits & 1, has_ps = bits & 2;
        const int n_gates = (bits & 4) ? 3 : 0;
        const RouteNet n{settle_max >= 2, n_gates, has_ps, force, 100000, sizes[(bits >> 3) & 1], sizes[(bits >> 4) & 1]};
        const Route s = route_launch(n, false, whole), r = route_launch(n, true, true);
        const bool settle = settle_max >= 2;
        if (old_step_pipes(settle_max, whole, has_ps, n_gates, n.lds_settle, force)) {
          EXPECT(s.kernel == kPipeSettle && s.lds_bytes == n.lds_settle && s.threads == 192 && s.groups_per_block == 2);
        } else {
          EXPECT(s.kernel == (settle ? kWaveSettle : kWave1) && s.lds_bytes == n.lds_wave && s.threads == 256 &&
                 s.groups_per_block == 4);
        }
        if (old_rollout_pipes(settle_max, has_ps, n_gates, n.lds_pipe, n.lds_settle, force)) {
          EXPECT(r.kernel == (settle ? kPipeSettle : kPipe) && r.threads == 192 && r.groups_per_block == 2);
          EXPECT(r.lds_bytes == (settle ? n.lds_settle : n.lds_pipe));
        } else {
          EXPECT(r.kernel == (settle ? kWaveSettleLean : kWaveLean) && r.lds_bytes == n.lds_wave &&
                 r.threads == 256 && r.groups_per_block == 4);
        }
      }
}

// a pipelined kernel that needs more LDS than a CU has is never launched, forced or not: the
// wave kernel runs, with the wave kernel's LDS, and no route asks for more than kLdsDeviceBytes
void routing_at_the_device_limit() {
  const size_t at = kLdsDeviceBytes, over = kLdsDeviceBytes + 4;
  const size_t sizes[3] = {64 * 1024 + 4, at, over};
  const int forces[3] = {0, 2, 3};
  for (int settle = 0; settle < 2; ++settle)
    for (int force : forces)
      for (size_t pipe_bytes : sizes)
        for (size_t settle_bytes : sizes)
          for (int whole = 0; whole < 2; ++whole) {
            const RouteNet n{(bool)settle, 0, true, force, 150000, pipe_bytes, settle_bytes};
            const Route s = route_launch(n, false, (bool)whole), r = route_launch(n, true, true);
            const size_t own = settle ? settle_bytes : pipe_bytes;
            EXPECT(s.lds_bytes <= kLdsDeviceBytes && r.lds_bytes <= kLdsDeviceBytes);
            EXPECT(s.kernel == (settle ? kWaveSettle : kWave1) && s.lds_bytes == n.lds_wave);   // all above 64 KB
            if (force == 3 && own <= at) {
              EXPECT(r.kernel == (settle ? kPipeSettle : kPipe) && r.lds_bytes == own && r.threads == 192 &&
                     r.groups_per_block == 2);
            } else {
              EXPECT(r.kernel == (settle ? kWaveSettleLean : kWaveLean) && r.lds_bytes == n.lds_wave &&
                     r.threads == 256 && r.groups_per_block == 4);
            }
          }
  // the case that showed it: 100 nodes, 254 attractors (lds_pipe 157,728, lds_settle 174,176 bytes)
  const RouteNet one{false, 0, true, 3, 150048, 157728, 174176}, law{true, 0, true, 3, 150048, 157728, 174176};
  EXPECT(route_launch(one, true, true).kernel == kPipe && route_launch(one, true, true).lds_bytes == 157728);
  EXPECT(route_launch(law, true, true).kernel == kWaveSettleLean && route_launch(law, true, true).lds_bytes == 150048);
}

}  // namespace

int main() {
  one_node_no_attractors();
  gate_and_two_state_attractor();
  rejected_after_the_hash();
  routing();
  routing_at_the_device_limit();
  if (g_failed) return printf("net_image_check: %d failed\n", g_failed), 1;
  printf("net_image_check: ok\n");
  return 0;
}
