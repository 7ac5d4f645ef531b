// osg_mlp_plan.h on the CPU: prints the layout of `n_linear widths... batch dqn limit` (tests/test_nfsp_learn_host.py).
#include <cstdio>
#include <cstdlib>

#include "osg_mlp_plan.h"

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  osg_mlp::MlpShape s;
  s.n_linear = std::atoi(argv[1]);
  if (s.n_linear < 1 || s.n_linear > osg_mlp::kMlpMaxLinear || argc != s.n_linear + 6) return 2;
  for (int l = 0; l <= s.n_linear; ++l) s.widths[l] = std::atoi(argv[2 + l]);
  s.batch = std::atoi(argv[3 + s.n_linear]);
  s.dqn = std::atoi(argv[4 + s.n_linear]) != 0;
  const osg_mlp::MlpLayout p = osg_mlp::plan_mlp(s, static_cast<size_t>(std::atol(argv[5 + s.n_linear])));
  if (!p.ok) { std::printf("refused %s\n", p.why); return 0; }
  std::printf("ok %zu %d %d\n", p.lds_bytes, p.batch_pad, p.param_count);
  for (int l = 0; l < p.n_linear; ++l) std::printf("w %d %d %d %d\n", p.in_pad[l], p.out_pad[l], p.w_stride[l], p.wt_stride[l]);
  for (int l = 0; l <= p.n_linear; ++l) std::printf("act %d\n", p.act_stride[l]);
  return 0;
}
