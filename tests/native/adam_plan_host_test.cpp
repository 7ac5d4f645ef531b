// osg_adam_plan.h on the CPU: prints the layout of `n_linear widths... batch limit` (tests/test_deep_cfr_learn_host.py).
#include <cstdio>
#include <cstdlib>

#include "osg_adam_plan.h"

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  osg_adam::AdamShape s;
  s.n_linear = std::atoi(argv[1]);
  if (s.n_linear < 1 || s.n_linear > osg_adam::kAdamMaxLinear || argc != s.n_linear + 5) return 2;
  for (int l = 0; l <= s.n_linear; ++l) s.widths[l] = std::atoi(argv[2 + l]);
  s.batch = std::atoi(argv[3 + s.n_linear]);
  const osg_adam::AdamLayout p = osg_adam::plan_adam(s, static_cast<size_t>(std::atol(argv[4 + s.n_linear])));
  if (!p.ok) { std::printf("refused %s\n", p.why); return 0; }
  std::printf("ok %zu %d %d %d %d %d %d\n", p.lds_bytes, p.tile, p.n_tiles, int(p.wt_resident), int(p.moments_resident), p.param_count,
              p.tile_off[p.n_linear]);
  const int last = p.n_linear - 1;
  for (int l = 0; l < p.n_linear; ++l) {   // buf: offset, floats
    std::printf("stride %d\nstride %d\n", p.w_stride[l], p.act_stride[l]);
    std::printf("buf %d %d\nbuf %d %d\n", p.w[l], p.out_pad[l] * p.w_stride[l], p.b[l], p.out_pad[l]);
    std::printf("buf %d %d\n", p.act[l], p.tile * p.act_stride[l]);
    if (l && p.wt_resident) std::printf("stride %d\nbuf %d %d\n", p.wt_stride[l], p.wt[l], p.in_pad[l] * p.wt_stride[l]);
  }
  std::printf("stride %d\nstride %d\n", p.n_stride, p.z_stride);
  std::printf("buf %d %d\nbuf %d %d\n", p.gamma, p.ln_pad, p.beta, p.ln_pad);
  std::printf("buf %d %d\nbuf %d %d\n", p.n, p.tile * p.act_stride[last], p.z, p.tile * p.z_stride);
  if (p.moments_resident) std::printf("buf %d %d\nbuf %d %d\n", p.mom_m, p.param_count, p.mom_v, p.param_count);
  std::printf("buf %d %d\nbuf %d %d\n", p.rows, osg_adam::kAdamRowWords * p.tile, p.reduce, osg_adam::kAdamReduceWords);
  return 0;
}
