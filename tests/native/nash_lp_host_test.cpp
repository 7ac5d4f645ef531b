// The exact Nash meta-solver as the kernel computes it (open_spiel_amd/csrc/osg_nash_lp.h, host + device) driven on the
// CPU over every case of tests/nash_lp_cases.py.  Built by tests/test_nash_lp_native.py with hipcc --cuda-host-only
// -ffp-contract=off, like the library.
//
//   nash_lp_host_test <cases.bin>
//
// cases.bin is written by tests/nash_lp_cases.py write_cases().  Per case the program runs k_nash_lp's steps in the
// kernel's arrangement — the selection as a wavefront makes it (the candidates as a 64-bit set, the smallest label bit
// by bit from the top, the minimum ratio over the set), the pivot row and column copied out before the first write,
// the rows rewritten wavefront by wavefront (rows w, w + 4, ..) — and once more through the header's serial nl_solve.
// Both must give the NumPy restatement's x, y, v, pivot count and status bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "osg_nash_lp.h"

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
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0;
}

struct Answer {
  std::vector<double> x, y, v;
  int pivots, status;
};

// lowest_label of osg_nash_lp.hip: labels are distinct and below 128.
int lowest_label(uint64_t members, const int* label) {
  for (int bit = 6; bit >= 0; --bit) {
    uint64_t clear = 0;
    for (int l = 0; l < 64; ++l)
      if (((members >> l) & 1) && !((label[l] >> bit) & 1)) clear |= uint64_t{1} << l;
    if (clear) members = clear;
  }
  return __builtin_ffsll(static_cast<long long>(members)) - 1;
}

// k_nash_lp on one matrix.
Answer as_the_kernel(const std::vector<double>& a, int m, int n) {
  const int ld = nl_stride(n), waves = 4;
  std::vector<double> t(static_cast<size_t>(m + 1) * ld, 0.0);
  int col_label[64] = {0}, row_label[64] = {0};
  Answer out{std::vector<double>(m, nl_nan()), std::vector<double>(n, nl_nan()), {nl_nan()}, 0, kNlOk};
  double lo = a[0], hi = a[0];
  for (int e = 0; e < m * n; ++e) {
    if (!nl_is_finite(a[e])) out.status = kNlNotFinite;
    lo = a[e] < lo ? a[e] : lo;
    hi = a[e] > hi ? a[e] : hi;
  }
  if (out.status != kNlOk) return out;
  double pre, base, span;
  nl_range(lo, hi, &pre, &base, &span);
  for (int e = 0; e < m * n; ++e) t[(e / n) * ld + e % n] = nl_normalise(a[e] * pre, base, span);
  for (int i = 0; i < m; ++i) { t[i * ld + n] = 1.0; row_label[i] = n + i; }
  for (int j = 0; j < n; ++j) { t[m * ld + j] = -1.0; col_label[j] = j; }
  for (;;) {
    uint64_t entering = 0;
    for (int j = 0; j < n; ++j)
      if (nl_enters(t[m * ld + j])) entering |= uint64_t{1} << j;
    if (!entering) break;
    if (out.pivots == kNlMaxPivots) { out.status = kNlNoOptimum; break; }
    const int pc = lowest_label(entering, col_label);
    double column[64], ratio[64], best = 0.0;
    uint64_t candidates = 0, ties = 0;
    for (int i = 0; i < m; ++i) {
      column[i] = t[i * ld + pc];
      if (!nl_pivotable(column[i])) continue;
      ratio[i] = nl_ratio(t[i * ld + n], column[i]);
      best = !candidates || ratio[i] < best ? ratio[i] : best;
      candidates |= uint64_t{1} << i;
    }
    for (int i = 0; i < m; ++i)
      if (((candidates >> i) & 1) && nl_ties(ratio[i], best)) ties |= uint64_t{1} << i;
    if (!ties) { out.status = kNlNoOptimum; break; }
    const int pr = lowest_label(ties, row_label);
    const double p = column[pr], bottom = t[m * ld + pc];
    double scaled[65];
    for (int j = 0; j <= n; ++j) scaled[j] = nl_scaled(t[pr * ld + j], p);
    for (int w = 0; w < waves; ++w)
      for (int i = w; i <= m; i += waves) {
        double* row = &t[i * ld];
        const double ci = i < m ? column[i] : bottom;
        for (int j = 0; j <= n; ++j) {
          if (i == pr) row[j] = j == pc ? nl_inverse(p) : scaled[j];
          else row[j] = j == pc ? nl_column(ci, p) : nl_update(row[j], ci, scaled[j]);
        }
      }
    const int label = col_label[pc];
    col_label[pc] = row_label[pr];
    row_label[pr] = label;
    ++out.pivots;
  }
  if (out.status != kNlOk) return out;
  std::vector<double> yv(64, 0.0), xv(64, 0.0);
  for (int i = 0; i < m; ++i)
    if (row_label[i] < n) yv[row_label[i]] = nl_clamp(t[i * ld + n]);
  for (int j = 0; j < n; ++j)
    if (col_label[j] >= n) xv[col_label[j] - n] = nl_clamp(t[m * ld + j]);
  const double sy = nl_sum(yv.data(), n), sx = nl_sum(xv.data(), m);
  for (int i = 0; i < m; ++i) out.x[i] = xv[i] / sx;
  for (int j = 0; j < n; ++j) out.y[j] = yv[j] / sy;
  out.v[0] = nl_value(sy, span, base) / pre;
  return out;
}

Answer serially(const std::vector<double>& a, int m, int n) {
  std::vector<double> t(static_cast<size_t>(m + 1) * nl_stride(n));
  std::vector<int> row_label(m), col_label(n);
  Answer out{std::vector<double>(m), std::vector<double>(n), {0.0}, 0, 0};
  out.status = nl_solve(a.data(), m, n, t.data(), row_label.data(), col_label.data(), out.x.data(), out.y.data(), out.v.data(), &out.pivots);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  Reader in{fopen(argv[1], "rb")};
  if (!in.f) { perror(argv[1]); return 2; }
  const int n_cases = in.take<int32_t>(1)[0];
  bool failed = false;
  int most = 0;
  for (int k = 0; k < n_cases; ++k) {
    const std::vector<int32_t> hdr = in.take<int32_t>(4);
    const int m = hdr[0], n = hdr[1];
    if (m < 1 || m > kNlMaxSide || n < 1 || n > kNlMaxSide) { fprintf(stderr, "case %d: %d x %d\n", k, m, n); return 2; }
    const std::vector<double> a = in.take<double>(static_cast<size_t>(m) * n);
    const Answer want{in.take<double>(m), in.take<double>(n), in.take<double>(1), hdr[2], hdr[3]};
    const Answer got[2] = {as_the_kernel(a, m, n), serially(a, m, n)};
    for (int form = 0; form < 2; ++form) {
      const Answer& g = got[form];
      if (g.status != want.status || g.pivots != want.pivots || !same_bits(g.x, want.x) || !same_bits(g.y, want.y) || !same_bits(g.v, want.v)) {
        printf("case %d (%d x %d), %s: status %d pivots %d v %.17g, the restatement has %d %d %.17g FAILED\n", k, m, n,
               form == 0 ? "in the kernel's arrangement" : "nl_solve", g.status, g.pivots, g.v[0], want.status, want.pivots, want.v[0]);
        failed = true;
      }
    }
    most = want.pivots > most ? want.pivots : most;
  }
  fclose(in.f);
  printf("most pivots: %d\n", most);
  if (failed) return 1;
  printf("ok: %d cases, both arrangements, bit-equal to the restatement\n", n_cases);
  return 0;
}
