// osg_vpnet_learn_plan.h on the CPU: prints the plan of `obs width depth actions batch limit` (tests/test_vpnet_learn_host.py).
#include <cstdio>
#include <cstdlib>

#include "osg_vpnet_learn_plan.h"

int main(int argc, char** argv) {
  using namespace osg_vpnet;
  if (argc != 7) return 2;
  VpShape s;
  s.obs = std::atoi(argv[1]); s.width = std::atoi(argv[2]); s.depth = std::atoi(argv[3]); s.actions = std::atoi(argv[4]);
  const VpLearnPlan L = plan_vpnet_learn(s, std::atoi(argv[5]), static_cast<size_t>(std::atol(argv[6])));
  if (!L.ok) { std::printf("refused %s\n", L.why); return 0; }
  const VpPlan& p = L.f;
  std::printf("ok %zu %d %d %d %d %d %d %d %d %d %zu\n", p.lds_bytes, p.rows, L.group, p.kc, L.kb, L.bstride, p.param_count, L.partial_stride,
              L.slice, L.slots, L.scratch_bytes);
  const int panel = p.panel_rows * p.kc > L.kb * L.bstride ? p.panel_rows * p.kc : L.kb * L.bstride;
  std::printf("buf %d %d\nbuf %d %d\n", p.act, p.rows * p.act_stride, p.logits, p.rows * p.logits_stride);   // buf: offset, floats
  for (int b = 0; b < 2; ++b) std::printf("buf %d %d\n", p.panel[b], panel);
  std::printf("buf %d %d\nbuf %d %d\nbuf %d %d\nbuf %d %d\n", p.vpart, kVpWaveCols * p.rows, p.vals, p.rows, L.row_words, kVlRowWords * p.rows, L.red, 16);
  std::printf("scratch %zu %zu %d\n", L.scratch_partial, L.scratch_saved, L.slot_floats);
  // the banks the 64 lanes (16 g + i) of an operand read name: dY as dX's A operand (row i, column g), a backward panel
  // as its B operand (row g, column i), dY as dW's A operand (row 4 g, column i)
  unsigned long long a = 0, b = 0, c = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const int i = lane & 15, g = lane >> 4;
    a |= 1ull << ((i * p.act_stride + g) % 64);
    b |= 1ull << ((g * L.bstride + i) % 64);
    c |= 1ull << ((4 * g * p.act_stride + i) % 64);
  }
  std::printf("banks %d %d %d\n", __builtin_popcountll(a), __builtin_popcountll(b), __builtin_popcountll(c));
  return 0;
}
