// osg_adam_wide_plan.h on the CPU: prints the plan of `n_linear widths... batch limit` (tests/test_deep_cfr_learn_wide_host.py).
#include <cstdio>
#include <cstdlib>

#include "osg_adam_wide_plan.h"

int main(int argc, char** argv) {
  using namespace osg_adam_wide;
  if (argc < 5) return 2;
  WideShape s;
  s.n_linear = std::atoi(argv[1]);
  if (s.n_linear < 1 || s.n_linear > kWideMaxLinear || argc != s.n_linear + 5) return 2;
  for (int l = 0; l <= s.n_linear; ++l) s.widths[l] = std::atoi(argv[2 + l]);
  s.batch = std::atoi(argv[3 + s.n_linear]);
  const WideLayout p = plan_adam_wide(s, static_cast<size_t>(std::atol(argv[4 + s.n_linear])));
  if (!p.ok) { std::printf("refused %s\n", p.why); return 0; }
  std::printf("ok %zu %d %d %zu %d %d %d\n", p.lds_bytes, p.rows, p.group, p.scratch_bytes, p.param_count, p.partial_stride, p.slice);
  for (int l = 0; l < p.n_linear; ++l) std::printf("stride %d\nbuf %d %d\n", p.act_stride[l], p.act[l], p.rows * p.act_stride[l]);   // buf: offset, floats
  std::printf("stride %d\nstride %d\nstride %d\n", p.n_stride, p.z_stride, p.panel_stride);
  std::printf("buf %d %d\nbuf %d %d\n", p.gamma, p.ln_pad, p.beta, p.ln_pad);
  for (int b = 0; b < 2; ++b) std::printf("buf %d %d\n", p.panel[b], kWideTile * p.panel_stride);
  std::printf("buf %d %d\nbuf %d %d\n", p.n, p.rows * p.n_stride, p.z, p.rows * p.z_stride);
  std::printf("buf %d %d\nbuf %d %d\n", p.row_words, kWideRowWords * p.rows, p.flags, kWideFlagWords);
  return 0;
}
