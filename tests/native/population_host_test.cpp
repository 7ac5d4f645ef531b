// The payoff-tensor cells and the aggregated policies of a population as the kernels compute them
// (open_spiel_amd/csrc/osg_population.h, host + device) driven on the CPU over every case of
// tests/golden/population_vectors.npz: what the reference's own expected_game_score.py and policy_aggregator.py
// computed.  Built by tests/test_population_native.py with hipcc --cuda-host-only -ffp-contract=off, like the library.
//
//   population_host_test <cases.bin> <tolerance>
//
// cases.bin is written by tests/population_cases.py write_cases().  The program forms every table's realization plan,
// every terminal's plan indices and chance product, every recorded profile's returns in the kernel's order (chunks of
// kPopChunk terminals, pop_wave_sum per 64, pop_chunk_sum, the chunks ascending) and every aggregated row by
// pop_aggregate_row, and prints the largest deviation from the recorded values.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "osg_population.h"

using namespace osg;

namespace {

struct Reader {
  FILE* f;
  template <class T>
  std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
  }
};

double deviation(const std::vector<double>& got, const std::vector<double>& want) {
  double d = 0.0;
  for (size_t k = 0; k < got.size(); ++k) {
    const double e = std::fabs(got[k] - want[k]);
    if (!(e <= d)) d = e;   // (a NaN sticks)
  }
  return d;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s cases.bin tolerance\n", argv[0]); return 2; }
  Reader in{fopen(argv[1], "rb")};
  if (!in.f) { perror(argv[1]); return 2; }
  const double tol = atof(argv[2]);
  const std::vector<int32_t> hdr = in.take<int32_t>(8);
  const int H = hdr[0], I = hdr[1], A = hdr[2], P = hdr[3], M = hdr[4], K = hdr[5], NP = hdr[6], NW = hdr[7];
  const size_t IA = static_cast<size_t>(I) * A;
  const std::vector<int32_t> parent = in.take<int32_t>(H), kind = in.take<int32_t>(H), actor = in.take<int32_t>(H),
                             info = in.take<int32_t>(H), nact = in.take<int32_t>(I), player = in.take<int32_t>(I),
                             mem_off = in.take<int32_t>(I + 1), mem = in.take<int32_t>(M);
  const std::vector<double> edge_prob = in.take<double>(H), term_ret = in.take<double>(static_cast<size_t>(H) * P);
  const double epsilon = in.take<double>(1)[0];
  const std::vector<double> tables = in.take<double>(K * IA);
  const std::vector<int32_t> profiles = in.take<int32_t>(static_cast<size_t>(NP) * P);
  const std::vector<double> want_returns = in.take<double>(static_cast<size_t>(NP) * P);
  // the links and root paths the solver keeps (osg_cfr.hip build_tree)
  std::vector<int32_t> first_child(H, 0);
  for (int h = H - 1; h > 0; --h) first_child[parent[h]] = h;
  std::vector<int32_t> path_off{0}, path;
  for (int m = 0; m < M; ++m) {
    std::vector<int32_t> rev;
    for (int32_t v = mem[m]; parent[v] >= 0; v = parent[v]) {
      const int32_t par = parent[v];
      const bool chance = kind[par] == 0;
      const int slot = chance ? P : actor[par];
      const int32_t idx = chance ? v : info[par] * A + (v - first_child[par]);
      rev.push_back((slot << 24) | ((chance ? 1 : 0) << 23) | idx);
    }
    path.insert(path.end(), rev.rbegin(), rev.rend());
    path_off.push_back(static_cast<int32_t>(path.size()));
  }
  // the terminals' plan indices, chance products and returns (osg_cfr_population.hip build_population_plan)
  std::vector<int32_t> last(static_cast<size_t>(H) * P, -1), seq;
  std::vector<double> chance(H, 1.0), tchance, tret;
  for (int h = 1; h < H; ++h) {
    const int par = parent[h];
    for (int p = 0; p < P; ++p) last[static_cast<size_t>(h) * P + p] = last[static_cast<size_t>(par) * P + p];
    chance[h] = chance[par];
    if (kind[par] == 0) chance[h] = chance[par] * edge_prob[h];
    else last[static_cast<size_t>(h) * P + actor[par]] = info[par] * A + (h - first_child[par]);
  }
  for (int h = 0; h < H; ++h) {
    if (kind[h] != 2) continue;
    for (int p = 0; p < P; ++p) { seq.push_back(last[static_cast<size_t>(h) * P + p]); tret.push_back(term_ret[static_cast<size_t>(h) * P + p]); }
    tchance.push_back(chance[h]);
  }
  const int T = static_cast<int>(tchance.size());
  // every table's realization plan
  std::vector<double> plans(K * IA);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < I; ++i) {
      const double* pol = &tables[k * IA];
      const int m0 = mem_off[i];
      const double own = mem_off[i + 1] > m0 ? pop_own_reach(path.data(), path_off[m0], path_off[m0 + 1], player[i], pol, 1.0) : 0.0;
      pop_plan_row(own, pol + static_cast<size_t>(i) * A, nact[i], A, &plans[k * IA + static_cast<size_t>(i) * A]);
    }
  // the recorded profiles
  std::vector<double> returns(static_cast<size_t>(NP) * P, 0.0);
  for (int m = 0; m < NP; ++m)
    for (int t0 = 0; t0 < T; t0 += kPopChunk) {
      const int here = T - t0 < kPopChunk ? T - t0 : kPopChunk;
      double w[kPopChunk];
      for (int j = 0; j < here; ++j)
        w[j] = pop_terminal_weight(tchance[t0 + j], &seq[static_cast<size_t>(t0 + j) * P], P,
                                   [&](int p) { return &plans[profiles[static_cast<size_t>(m) * P + p] * IA]; });
      for (int q = 0; q < P; ++q) {
        double term[kPopChunk], wave[kPopChunk / 64];
        for (int j = 0; j < kPopChunk; ++j) term[j] = j < here ? pop_return_term(tret[static_cast<size_t>(t0 + j) * P + q], w[j]) : 0.0;
        for (int v = 0; v < kPopChunk / 64; ++v) wave[v] = pop_wave_sum(term + 64 * v);
        returns[static_cast<size_t>(m) * P + q] += pop_chunk_sum(wave[0], wave[1], wave[2], wave[3]);
      }
    }
  bool failed = false;
  double d = deviation(returns, want_returns);
  printf("%d profiles of %d tables, %d terminals: largest deviation of the returns %.3g\n", NP, K, T, d);
  if (!(d <= tol)) { printf("returns FAILED\n"); failed = true; }
  // the recorded weight matrices
  for (int c = 0; c < NW; ++c) {
    const std::vector<double> weights = in.take<double>(static_cast<size_t>(P) * K), want = in.take<double>(IA);
    std::vector<double> got(IA);
    for (int i = 0; i < I; ++i)
      pop_aggregate_row(i, player[i], nact[i], A, mem_off[i], mem_off[i + 1], path_off.data(), path.data(), tables.data(), K, IA,
                        &weights[static_cast<size_t>(player[i]) * K], epsilon, &got[static_cast<size_t>(i) * A]);
    d = deviation(got, want);
    printf("weight matrix %d: largest deviation of the aggregate %.3g\n", c, d);
    if (!(d <= tol)) { printf("aggregate %d FAILED\n", c); failed = true; }
  }
  fclose(in.f);
  if (failed) return 1;
  printf("ok: %d profiles, %d aggregates\n", NP, NW);
  return 0;
}
