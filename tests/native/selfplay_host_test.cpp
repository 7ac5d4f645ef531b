// The self-play arithmetic of open_spiel_amd/csrc/osg_selfplay.h on the CPU: the functions the kernels of
// osg_selfplay.hip run, driven over files tests/selfplay_cases.py writes and compares.  Stand-alone (own main), built
// plain and with the address / undefined-behaviour sanitizers by tests/test_selfplay_host.py.
//
//   select <in> <out>   policy targets (f64 and f32) and moves of synthetic visit rows
//   ring   <in> <out>   the ring slot of every row of a sequence of flushes
//   noise  <in> <out>   dirichlet_row over N priors; mode 0 as the kernel, 1 without the alpha < 1 step (the defect a
//                       statistical test must reject), 2 / 3 with every logarithm one ulp up / down
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "osg_selfplay.h"

using namespace osg;

static int g_log_ulps = 0;
struct PerturbedLog {   // libm's logarithm moved by g_log_ulps last bits
  static double of(double x) {
    const double y = std::log(x);
    if (g_log_ulps == 0) return y;
    return std::nextafter(y, g_log_ulps > 0 ? INFINITY : -INFINITY);
  }
};

namespace {

struct Reader {
  FILE* f;
  template <class T> T one() { T v{}; if (fread(&v, sizeof(T), 1, f) != 1) fail(); return v; }
  template <class T> std::vector<T> many(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) fail();
    return v;
  }
  [[noreturn]] static void fail() { fprintf(stderr, "FAILED: short input\n"); exit(2); }
};
template <class T> void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int run_select(FILE* in, FILE* out) {
  Reader r{in};
  const int cases = r.one<int32_t>();
  for (int c = 0; c < cases; ++c) {
    const int A = r.one<int32_t>(), rows = r.one<int32_t>(), drop = r.one<int32_t>();
    (void)r.one<int32_t>();
    const double temperature = r.one<double>();
    const uint64_t seed = r.one<uint64_t>();
    const int64_t offset = r.one<int64_t>();
    const auto visits = r.many<int32_t>(static_cast<size_t>(rows) * A);
    const auto best = r.many<int32_t>(rows);
    const auto move = r.many<int32_t>(rows);
    const auto plyc = r.many<int64_t>(rows);
    std::vector<double> p64(static_cast<size_t>(rows) * A, 0.0);
    std::vector<float> p32(static_cast<size_t>(rows) * A, 0.0f);
    std::vector<int32_t> action(rows, -1);
    std::vector<uint8_t> ok(rows, 0);
    for (int i = 0; i < rows; ++i) {
      const int32_t* v = visits.data() + static_cast<size_t>(i) * A;
      double* p = p64.data() + static_cast<size_t>(i) * A;
      if (!policy_from_visits(v, A, temperature, p)) continue;   // a zero-visit row: reported, not recorded
      ok[i] = 1;
      for (int a = 0; a < A; ++a) p32[static_cast<size_t>(i) * A + a] = static_cast<float>(p[a]);
      action[i] = draw_action(v, A, temperature, move[i] >= drop, best[i], seed, static_cast<uint64_t>(offset + i),
                              static_cast<uint64_t>(plyc[i]));
    }
    put(out, p64); put(out, p32); put(out, action); put(out, ok);
  }
  printf("ok: %d select cases\n", cases);
  return 0;
}

int run_ring(FILE* in, FILE* out) {
  Reader r{in};
  const int cases = r.one<int32_t>();
  for (int c = 0; c < cases; ++c) {
    const int64_t capacity = r.one<int64_t>();
    const int flushes = r.one<int32_t>(), n = r.one<int32_t>();
    int64_t total_seen = 0;
    for (int f = 0; f < flushes; ++f) {
      const auto flen = r.many<int32_t>(n);   // 0: the environment did not finish
      std::vector<int64_t> prefix(n);
      int64_t rows = 0;
      for (int i = 0; i < n; ++i) { prefix[i] = rows; rows += flen[i]; }
      std::vector<int64_t> slots;
      for (int i = 0; i < n; ++i)
        for (int t = 0; t < flen[i]; ++t) {
          const int64_t g = prefix[i] + t;
          slots.push_back(ring_written(rows, g, capacity) ? ring_slot(total_seen, g, capacity) : -1);
        }
      total_seen += rows;
      const std::vector<int64_t> tail{total_seen, ring_size(total_seen, capacity)};
      put(out, slots); put(out, tail);
    }
  }
  printf("ok: %d ring cases\n", cases);
  return 0;
}

int run_noise(FILE* in, FILE* out) {
  Reader r{in};
  const int64_t N = r.one<int64_t>();
  const int A = r.one<int32_t>(), words = r.one<int32_t>(), mode = r.one<int32_t>();
  (void)r.one<int32_t>();
  const double alpha = r.one<double>(), epsilon = r.one<double>();
  const uint64_t seed = r.one<uint64_t>();
  const int64_t offset = r.one<int64_t>();
  const uint64_t sub = r.one<uint64_t>();
  auto prior = r.many<double>(static_cast<size_t>(N) * A);
  const auto mask = r.many<uint32_t>(static_cast<size_t>(N) * words);
  g_log_ulps = mode == 2 ? 1 : (mode == 3 ? -1 : 0);
  std::vector<double> noise(A);
  for (int64_t i = 0; i < N; ++i) {
    Rng rng(seed, static_cast<uint64_t>(offset + i), sub);
    double* p = prior.data() + static_cast<size_t>(i) * A;
    const uint32_t* m = mask.data() + static_cast<size_t>(i) * words;
    if (mode == 1) dirichlet_row_t<false>(p, m, A, alpha, epsilon, rng, noise.data(), 1);
    else if (mode >= 2) dirichlet_row_t<true, PerturbedLog>(p, m, A, alpha, epsilon, rng, noise.data(), 1);
    else dirichlet_row(p, m, A, alpha, epsilon, rng, noise.data(), 1);
  }
  put(out, prior);
  printf("ok: %lld noise rows\n", static_cast<long long>(N));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: selfplay_host_test select|ring|noise <in> <out>\n"); return 2; }
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) { fprintf(stderr, "FAILED: cannot open files\n"); return 2; }
  const std::string what = argv[1];
  int rc = 2;
  if (what == "select") rc = run_select(in, out);
  else if (what == "ring") rc = run_ring(in, out);
  else if (what == "noise") rc = run_noise(in, out);
  fclose(in);
  fclose(out);
  return rc;
}
