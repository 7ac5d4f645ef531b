// Alpha-rank as the kernels compute it (open_spiel_amd/csrc/osg_alpharank.h, host + device) driven on the CPU in the
// kernels' order over every case of tests/alpharank_cases.py.  Built by tests/test_alpharank_native.py with
// hipcc --cuda-host-only -ffp-contract=off, like the library.
//
//   alpharank_host_test <cases.bin> [<outputs.bin>]
//
// cases.bin is written by tests/alpharank_cases.py write_cases().  Per case the program runs what k_alpharank_solve and
// k_alpharank_stop run — the off-diagonal entries by ar_entry, the elimination and back-substitution by ar_stationary,
// the sweep's epsilons by ar_eps_at and its stop rule by ar_close, the marginals by ar_marginal — twice: with the rows
// of the matrix n doubles apart (the LDS form) and padded to a multiple of 16 (the global form).  The two must agree bit
// for bit.  With infinite alpha and for the sweep the entries, pi, the marginals, eps_used, iterations and status must be
// the NumPy restatement's bit for bit; with finite alpha (libm's exp and NumPy's may differ in the last place) pi lies
// within the case's entrywise relative bound of the exact pi, which every case must meet.  outputs.bin receives per
// case status, iterations (int32), eps_used, pi [n], marginals [SK].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "osg_alpharank.h"

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

bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}
// The largest entrywise relative deviation (a NaN sticks; 0 against 0 counts as 0).
double relative(const std::vector<double>& got, const std::vector<double>& want) {
  double d = 0.0;
  for (size_t k = 0; k < got.size(); ++k) {
    const double e = got[k] == want[k] ? 0.0 : std::fabs(got[k] - want[k]) / std::fabs(want[k]);
    if (!(e <= d)) d = e;
  }
  return d;
}

struct Problem {
  ArShape sh;
  int mode, m, min_iters, max_iters;
  double alpha, eps;
  std::vector<double> tensors;
};
struct Answer {
  int status = 0, iterations = 0;
  double eps_used = 0.0;
  std::vector<double> entries, pi, marginals;   // entries: [n, moves] at eps_used
};

// One solve: k_alpharank_solve on one (problem, eps).
int solve_at(const Problem& c, int64_t lda, double eps, std::vector<double>* entries, std::vector<double>* pi) {
  const int n = c.sh.n;
  std::vector<double> a(static_cast<size_t>(n) * lda, 0.0), x(n);
  entries->assign(static_cast<size_t>(n) * c.sh.moves, 0.0);
  for (int row = 0; row < n; ++row)
    for (int mv = 0; mv < c.sh.moves; ++mv) {
      int col = -1;
      const double value = ar_entry(c.sh, c.tensors.data(), row, mv, c.mode, eps, c.alpha, c.m, &col);
      if (col < 0 || col >= n || col == row) { fprintf(stderr, "bad neighbour\n"); exit(2); }
      a[row * lda + col] = value;
      (*entries)[static_cast<size_t>(row) * c.sh.moves + mv] = value;
    }
  pi->assign(n, 0.0);
  return ar_stationary(a.data(), n, lda, x.data(), pi->data());
}

// The whole problem: the host's loop over chunks and k_alpharank_stop.
Answer solve(const Problem& c, int64_t lda) {
  Answer r;
  const int n = c.sh.n;
  if (c.mode != kArSweep) {
    r.status = solve_at(c, lda, c.eps, &r.entries, &r.pi);
    r.eps_used = c.mode == kArInfinite ? c.eps : 0.0;
  } else {
    const double eps0 = ar_sweep_start(c.eps);
    std::vector<double> prev;
    for (int t = 0;; ++t) {
      r.iterations = t;
      r.eps_used = ar_eps_at(eps0, t);
      const int status = solve_at(c, lda, r.eps_used, &r.entries, &r.pi);
      if (status != kArOk) { r.status = kArReducible; break; }
      if (t > c.min_iters) {
        bool close = true;
        for (int i = 0; i < n; ++i) close = close && ar_close(r.pi[i], prev[i]);
        if (close) { r.status = kArOk; break; }
      }
      if (t + 1 >= c.max_iters) { r.status = kArNoStop; break; }
      prev = r.pi;
    }
  }
  if (r.status != kArOk) r.pi.assign(n, ar_nan());
  r.marginals.resize(c.sh.SK);
  for (int x = 0; x < c.sh.SK; ++x) r.marginals[x] = r.status == kArOk ? ar_marginal(c.sh, r.pi.data(), x) : ar_nan();
  return r;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin [outputs.bin]\n", argv[0]); return 2; }
  Reader in{fopen(argv[1], "rb")};
  if (!in.f) { perror(argv[1]); return 2; }
  FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
  if (argc > 2 && !out) { perror(argv[2]); return 2; }
  const int n_cases = in.take<int32_t>(1)[0];
  bool failed = false;
  double worst[2] = {0.0, 0.0}, worst_of_bound = 0.0;   // relative to the exact pi: infinite alpha and sweeps, finite alpha
  for (int k = 0; k < n_cases; ++k) {
    const std::vector<int32_t> hdr = in.take<int32_t>(13);
    const std::vector<double> par = in.take<double>(4);
    Problem c;
    const int P = hdr[0];
    if (P < 1 || P > kArMaxPlayers) { fprintf(stderr, "case %d: %d players\n", k, P); return 2; }
    int32_t shape[kArMaxPlayers];
    int64_t n = 1;
    for (int p = 0; p < kArMaxPlayers; ++p) shape[p] = hdr[1 + p];
    for (int p = 0; p < (P == 1 ? 2 : P); ++p) {
      if (shape[p] < 1) { fprintf(stderr, "case %d: a size below 1\n", k); return 2; }
      n *= shape[p];
    }
    if (P == 1 ? shape[0] != shape[1] || shape[0] > kArMaxProfiles : n > kArMaxProfiles) { fprintf(stderr, "case %d: not served\n", k); return 2; }
    c.sh = ar_shape(P, shape);
    c.mode = hdr[6]; c.m = hdr[7]; c.min_iters = hdr[8]; c.max_iters = hdr[9];
    const bool exact_only = hdr[10] != 0;
    const int want_status = hdr[11], want_iterations = hdr[12];
    c.alpha = par[0]; c.eps = par[1];
    const double bound = par[2], want_eps = par[3];
    c.tensors = in.take<double>(static_cast<size_t>(c.sh.cells));
    const std::vector<double> want_entries = in.take<double>(static_cast<size_t>(c.sh.n) * c.sh.moves), want_pi = in.take<double>(c.sh.n),
                              want_marginals = in.take<double>(c.sh.SK), exact = in.take<double>(c.sh.n);
    const Answer r = solve(c, c.sh.n), padded = solve(c, (static_cast<int64_t>(c.sh.n) + 15) & ~int64_t{15});
    if (!same_bits(r.pi, padded.pi) || !same_bits(r.marginals, padded.marginals) || r.status != padded.status || r.iterations != padded.iterations) {
      printf("case %d: the two layouts differ FAILED\n", k);
      failed = true;
    }
    if (r.status != want_status || r.iterations != want_iterations || r.eps_used != want_eps) {
      printf("case %d: status %d after %d iterations at %.17g, not the restatement's %d, %d, %.17g FAILED\n", k, r.status, r.iterations,
             r.eps_used, want_status, want_iterations, want_eps);
      failed = true;
    }
    const double off = relative(r.pi, want_pi), err = relative(r.pi, exact);
    if (c.mode != kArFinite && (!same_bits(r.entries, want_entries) || !same_bits(r.pi, want_pi) || !same_bits(r.marginals, want_marginals))) {
      printf("case %d: not the restatement's bits (pi off by %.3g relative) FAILED\n", k, off);
      failed = true;
    }
    if (c.mode == kArFinite && !(off <= bound)) { printf("case %d: %.3g (relative) from the restatement FAILED\n", k, off); failed = true; }
    if (!(err <= bound)) { printf("case %d: %.3g (relative) from the exact pi, the bound is %.3g FAILED\n", k, err, bound); failed = true; }
    double total = 0.0;
    for (double v : r.pi) {
      if (!(v >= 0.0) || !std::isfinite(v)) { printf("case %d: a mass of %.3g FAILED\n", k, v); failed = true; }
      total += v;
    }
    if (exact_only && !(std::fabs(total - 1.0) <= 4 * 2.220446049250313e-16)) { printf("case %d: pi sums to 1 %+.3g FAILED\n", k, total - 1.0); failed = true; }
    const int kind = c.mode == kArFinite ? 1 : 0;
    if (!(err <= worst[kind])) worst[kind] = err;
    if (c.sh.n > 1 && !(err / bound <= worst_of_bound)) worst_of_bound = err / bound;
    if (out) {
      const int32_t ints[2] = {r.status, r.iterations};
      fwrite(ints, sizeof(int32_t), 2, out);
      fwrite(&r.eps_used, sizeof(double), 1, out);
      fwrite(r.pi.data(), sizeof(double), r.pi.size(), out);
      fwrite(r.marginals.data(), sizeof(double), r.marginals.size(), out);
    }
  }
  fclose(in.f);
  if (out) fclose(out);
  printf("largest relative deviation from the exact pi: infinite alpha %.3g, finite alpha %.3g; at most %.3g of the bound\n", worst[0], worst[1],
         worst_of_bound);
  if (failed) return 1;
  printf("ok: %d cases, both layouts, bit-equal to the restatement\n", n_cases);
  return 0;
}
