// The arithmetic of extensive-form fictitious play's averaging pass (open_spiel_amd/csrc/osg_xfp.h: xfp_reach,
// xfp_update_row, xfp_alpha — the functions the kernels of osg_cfr_xfp.hip run) driven on the CPU over the trajectories
// of tests/golden/xfp_vectors.npz.  tests/test_xfp_native.py writes one binary file per game:
//   int32 I, A, P, T; int32 nact[I], player[I], pred_info[I], pred_action[I];
//   then per iteration t = 1 .. T: int32 best[I]; double avg_reach[I], br_reach[I], policy[I * A]
// Starting from the uniform policy, every iteration feeds the recorded best response through the header's functions;
// both reaches and the policy afterwards must equal the recorded ones bit for bit.  The root paths are built here from
// the predecessor chain in the tabular solvers' code format, with a chance entry and another player's entry between the
// owner's entries, which the reach product must skip.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "osg_xfp.h"

namespace {

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: xfp_host_test <cases.bin>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  int32_t head[4];
  if (fread(head, sizeof(int32_t), 4, f) != 4) { printf("short header\n"); return 2; }
  const int I = head[0], A = head[1], P = head[2], T = head[3];
  std::vector<int32_t> nact, player, pred_info, pred_action, best;
  if (!read_vec(f, nact, I) || !read_vec(f, player, I) || !read_vec(f, pred_info, I) || !read_vec(f, pred_action, I)) {
    printf("short layout\n");
    return 2;
  }
  std::vector<int32_t> path_off{0}, path;
  for (int i = 0; i < I; ++i) {
    std::vector<int32_t> rev;
    for (int j = i; pred_info[j] >= 0; j = pred_info[j]) {
      rev.push_back((player[i] << 24) | (pred_info[j] * A + pred_action[j]));
      rev.push_back((((player[i] + 1) % P) << 24) | 0);   // another player's decision
      rev.push_back((P << 24) | (1 << 23) | 5);           // a chance outcome
    }
    path.insert(path.end(), rev.rbegin(), rev.rend());
    path_off.push_back(static_cast<int32_t>(path.size()));
  }
  std::vector<double> pol(static_cast<size_t>(I) * A, 0.0), want_avg, want_br, want_pol;
  for (int i = 0; i < I; ++i)
    for (int a = 0; a < nact[i]; ++a) pol[i * A + a] = 1.0 / nact[i];
  std::vector<osg::XfpReach> reach(I);
  long checked = 0;
  for (int t = 1; t <= T; ++t) {
    if (!read_vec(f, best, I) || !read_vec(f, want_avg, I) || !read_vec(f, want_br, I) ||
        !read_vec(f, want_pol, static_cast<size_t>(I) * A)) {
      printf("short iteration %d\n", t);
      return 2;
    }
    for (int i = 0; i < I; ++i) {   // every reach from the old table before the first row is stored
      reach[i] = osg::xfp_reach(path.data(), path_off[i], path_off[i + 1], player[i], A, pol.data(), best.data());
      if (!same_bits(reach[i].avg, want_avg[i]) || !same_bits(reach[i].br, want_br[i])) {
        printf("iteration %d infostate %d: reaches %a %a, recorded %a %a\n", t, i, reach[i].avg, reach[i].br, want_avg[i], want_br[i]);
        return 1;
      }
    }
    const double alpha = osg::xfp_alpha(t);
    for (int i = 0; i < I; ++i) osg::xfp_update_row(&pol[i * A], nact[i], best[i], alpha, reach[i]);
    for (int i = 0; i < I; ++i)
      for (int a = 0; a < nact[i]; ++a) {
        if (!same_bits(pol[i * A + a], want_pol[i * A + a])) {
          printf("iteration %d infostate %d action %d: %a, recorded %a\n", t, i, a, pol[i * A + a], want_pol[i * A + a]);
          return 1;
        }
        ++checked;
      }
  }
  fclose(f);
  printf("ok: %d iterations, %d infostates, %ld cells\n", T, I, checked);
  return 0;
}
