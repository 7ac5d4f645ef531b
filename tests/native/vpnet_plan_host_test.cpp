// osg_vpnet_plan.h on the CPU: prints the plan of `obs width depth actions limit` (tests/test_vpnet_host.py).
#include <cstdio>
#include <cstdlib>

#include "osg_vpnet_plan.h"

int main(int argc, char** argv) {
  using namespace osg_vpnet;
  if (argc != 6) return 2;
  VpShape s;
  s.obs = std::atoi(argv[1]); s.width = std::atoi(argv[2]); s.depth = std::atoi(argv[3]); s.actions = std::atoi(argv[4]);
  const VpPlan p = plan_vpnet(s, static_cast<size_t>(std::atol(argv[5])));
  if (!p.ok) { std::printf("refused %s\n", p.why); return 0; }
  std::printf("ok %zu %d %d %d %d %d %d %d\n", p.lds_bytes, p.rows, p.mr, p.nc, p.kc, p.panel_stride, p.panel_rows, p.param_count);
  std::printf("stride %d\nstride %d\n", p.act_stride, p.logits_stride);
  std::printf("buf %d %d\nbuf %d %d\n", p.act, p.rows * p.act_stride, p.logits, p.rows * p.logits_stride);   // buf: offset, floats
  for (int b = 0; b < 2; ++b) std::printf("buf %d %d\n", p.panel[b], p.panel_rows * p.panel_stride);
  std::printf("buf %d %d\nbuf %d %d\n", p.vpart, kVpWaveCols * p.rows, p.vals, p.rows);
  for (int b = 0; b < 2; ++b) std::printf("alias %d %d\n", p.xstage[b], p.rows * p.kc);   // the observation stages, inside act
  std::printf("params");
  for (int l = 0; l <= p.depth; ++l) std::printf(" %d", p.torso[l]);
  std::printf(" %d %d %d %d\n", p.v1, p.v2, p.p1, p.p2);
  // the banks the 64 lanes of an operand read name in a panel or stage row block (lane 16 g + i: row i, column g), and in act
  for (int kk = 0; kk < p.kc; kk += 4) {
    unsigned long long seen = 0, seen_act = 0;
    for (int lane = 0; lane < 64; ++lane) {
      const int i = lane & 15, g = lane >> 4;
      seen |= 1ull << ((i * p.kc + ((kk + g) ^ vp_swizzle(p.kc, i))) % 64);
      seen_act |= 1ull << ((i * p.act_stride + kk + g) % 64);
    }
    std::printf("banks %d %d\n", __builtin_popcountll(seen), __builtin_popcountll(seen_act));
  }
  return 0;
}
