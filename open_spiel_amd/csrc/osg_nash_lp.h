// The exact Nash equilibrium of a two-player zero-sum matrix game by linear programming (psro_v2's "nash":
// meta_strategies.nash_strategy -> lp_solver.solve_zero_sum_matrix_game): every formula and the ONE order of every
// operation, host + device.  The kernel of osg_nash_lp.hip runs these functions, and so does
// tests/native/nash_lp_host_test.cpp on the CPU; tests/nash_lp_cases.py restates them in NumPy.
//
// The game.  A [m, n], row-major: the row player's payoffs; the row player maximises.  x [m], y [n]: the two
// equilibrium strategies, v the value (the column player's is -v).
//
// Normalise.  lo = min A, span = max A - lo, A' = (A - lo) / span + 1 in [1, 2] (span = 0, a constant matrix: A' = 1).
//   Equilibria do not change and the value of A' is at least 1 > 0.  An entry that is not finite: status 1, NaN outputs.
//   A finite matrix whose max A - lo overflows is normalised from its halved entries (nl_range: every entry, lo and the
//   span times 0.5, the value times 2 at the end); every other matrix keeps factors of 1, which change no bit.
// LP.  maximise 1^T y' subject to A' y' <= 1, y' >= 0: y = y' / sum y', the value of A' is 1 / sum y', and the duals
//   x' of the rows give x the same way.  y' = 0 is feasible and A' >= 1 bounds the LP: no phase 1.
// Tableau.  t [m + 1, n + 1] at t[i * ld + j]: rows 0 .. m-1 are the constraints (the slacks are the first basis),
//   column n is the right-hand side (1), row m the reduced costs (-1; t[m][n] = 0 is the objective).  The tableau is
//   CONDENSED: only the non-basic columns are kept, and a pivot swaps the label of its column with the label of its
//   row.  Labels: 0 .. n-1 the variables y', n .. n+m-1 the slacks.
// Entering column (Bland): of the columns j < n with t[m][j] < -kNlEps the one with the smallest label; none: optimal.
// Leaving row: of the rows i < m with t[i][c] > kNlPivotEps those with the smallest ratio t[i][n] / t[i][c]; of these the
//   one with the smallest label.  No such row (impossible for a bounded LP in exact arithmetic): status 2.
// Pivot on p = t[r][c], every element from the values BEFORE the pivot:
//     t[r][j] = t[r][j] / p            j != c         (nl_scaled)
//     t[i][j] = t[i][j] - t[i][c] * t[r][j]'          i != r, j != c, t[r][j]' the scaled pivot row (nl_update)
//     t[i][c] = -(t[i][c] / p)         i != r         (nl_column)
//     t[r][c] = 1 / p
//   THE MULTIPLY-SUBTRACT IS NOT FUSED: the product is rounded, then subtracted.  The library, the host test and NumPy
//   all do that; everything here is compiled with -ffp-contract=off.  No floating-point atomics.
// Read-out.  y'[label] = max(t[i][n], 0) of the rows with a label < n, 0 elsewhere; x'[label - n] = max(t[m][j], 0) of
//   the columns with a label >= n, 0 elsewhere (the clamps: a degenerate right-hand side or a reduced cost may end a
//   rounding error below 0, and a strategy has no negative weight).  S = nl_sum(y'), y = y' / S, x = x' / nl_sum(x'),
//   v = (1 / S - 1) * span + lo.  nl_sum: ascending, with every addition's rounding error collected in a second
//   double and added at the end, so that a strategy's weights sum to 1 within an ulp or two for any length.
// Pivot cap: kNlMaxPivots; beyond it status 2 and NaN outputs.
#ifndef OSG_NASH_LP_H_
#define OSG_NASH_LP_H_

#include "osg_common.h"

#include <math.h>

namespace osg {

constexpr int kNlMaxSide = 64;          // rows, cols: a wavefront holds a row or a column of labels, one per lane
// A reduced cost above -kNlEps does not enter.  The normalised entries lie in [1, 2] and a few hundred rank-1 updates
// leave rounding noise on an entry that is 0 in exact arithmetic: mostly 1e-17 .. 1e-13, up to 3e-11 where Bland's rule
// has divided by small true entries (1e-6, 1e-5) on the way.  A reduced cost of that size that is chased costs a pivot
// or two; one that is ignored costs the duality gap at most kNlEps * sum y' <= 1e-12, below the certificate's bound.
constexpr double kNlEps = 1e-12;
// An entry at or below kNlPivotEps is no pivot.  Dividing by noise is the one mistake the tableau does not recover from,
// so this is not the reduced costs' threshold, as it once was: at a degenerate vertex of a 63 x 64 table over
// {-1, 0, 1} an exact zero that had become 1.04e-12 was pivoted on, which put a linearly dependent column into the
// basis, and the solve ended "optimal" 570 pivots later with a duality gap of 0.087.  1e-9 lies between the noise
// (3e-11 at the most over the tested matrices) and the smallest true entries met in a pivot column (1e-6).  A true
// entry e below it that is passed over lets its row's right-hand side end at -e * ratio at the worst, which the
// read-out clamps.
constexpr double kNlPivotEps = 1e-9;
// Ratios tie only when they are EQUAL.  A degenerate vertex has right-hand sides that are exactly 0 (0 - c * 0), so its
// ties are exact and Bland's smallest-label rule sees them all; a tolerance would make "tie" intransitive, and the
// choice among near-ties would no longer be a minimum-ratio choice, which Bland's termination argument needs.
constexpr double kNlRatioTie = 0.0;
// A safety cap against cycling on rounding noise, not a tuning figure: the tested matrices need fewer than 700 pivots.
constexpr int kNlMaxPivots = 20000;
enum NlStatus { kNlOk = 0, kNlNotFinite = 1, kNlNoOptimum = 2 };

OSG_HD double nl_nan() { return __builtin_nan(""); }
OSG_HD bool nl_is_finite(double x) { return x - x == 0.0; }
// The row stride of the tableau, in doubles: odd, so that the pivot column's rows i = 0 .. 31 start in 32 different
// pairs of LDS banks (2 * ld * i mod 64 takes every even value once) while a row's elements are consecutive anyway.
OSG_HD int nl_stride(int cols) { return (cols + 1) | 1; }

// What a matrix with the minimum lo and the maximum hi is normalised with: entry * pre, then (.. - base) / span + 1.
// pre is 1 unless hi - lo overflows (then 0.5: the halves' difference is finite), and nl_value's result is divided by it.
OSG_HD void nl_range(double lo, double hi, double* pre, double* base, double* span) {
  *pre = nl_is_finite(hi - lo) ? 1.0 : 0.5;
  *base = lo * *pre;
  *span = hi * *pre - *base;
}
OSG_HD double nl_normalise(double a, double lo, double span) { return span > 0.0 ? (a - lo) / span + 1.0 : 1.0; }
OSG_HD bool nl_enters(double cost) { return cost < -kNlEps; }
OSG_HD bool nl_pivotable(double entry) { return entry > kNlPivotEps; }
OSG_HD double nl_ratio(double rhs, double entry) { return rhs / entry; }
OSG_HD bool nl_ties(double ratio, double best) { return ratio - best <= kNlRatioTie; }   // (best is the minimum)
OSG_HD double nl_scaled(double t, double p) { return t / p; }
OSG_HD double nl_update(double t, double column, double scaled) {
  const double product = column * scaled;   // rounded: NOT a fused multiply-add
  return t - product;
}
OSG_HD double nl_column(double column, double p) { return -(column / p); }
OSG_HD double nl_inverse(double p) { return 1.0 / p; }
OSG_HD double nl_clamp(double x) { return x > 0.0 ? x : 0.0; }
// One step of nl_sum: (*sum, *err) += v.
OSG_HD void nl_sum_step(double* sum, double* err, double v) {
  const double s = *sum, t = s + v;
  const double lost = fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
  *err = *err + lost;
  *sum = t;
}
OSG_HD double nl_sum(const double* v, int count) {
  double sum = 0.0, err = 0.0;
  for (int k = 0; k < count; ++k) nl_sum_step(&sum, &err, v[k]);
  return sum + err;
}
OSG_HD double nl_value(double total, double span, double lo) {
  const double scaled = (1.0 / total - 1.0) * span;   // rounded, then added
  return scaled + lo;
}

// The whole solve on one matrix, serially (every element's operations are those of the kernel, which spreads the
// selection over a wavefront's lanes and the update over the workgroup).  t: (m + 1) * nl_stride(n) doubles of
// scratch; row_label [m], col_label [n], x [m], y [n].  Returns the status.
inline int nl_solve(const double* a, int m, int n, double* t, int* row_label, int* col_label, double* x, double* y, double* value,
                    int* pivots) {
  const int ld = nl_stride(n);
  int status = kNlOk, done = 0;
  double lo = a[0], hi = a[0];
  for (int e = 0; e < m * n; ++e) {
    if (!nl_is_finite(a[e])) status = kNlNotFinite;
    lo = a[e] < lo ? a[e] : lo;
    hi = a[e] > hi ? a[e] : hi;
  }
  double pre, base, span;
  nl_range(lo, hi, &pre, &base, &span);
  if (status == kNlOk) {
    for (int i = 0; i <= m; ++i)
      for (int j = 0; j <= n; ++j) t[i * ld + j] = i < m ? (j < n ? nl_normalise(a[i * n + j] * pre, base, span) : 1.0) : (j < n ? -1.0 : 0.0);
    for (int j = 0; j < n; ++j) col_label[j] = j;
    for (int i = 0; i < m; ++i) row_label[i] = n + i;
  }
  while (status == kNlOk) {
    int c = -1, r = -1;
    for (int j = 0; j < n; ++j)
      if (nl_enters(t[m * ld + j]) && (c < 0 || col_label[j] < col_label[c])) c = j;
    if (c < 0) break;
    if (done == kNlMaxPivots) { status = kNlNoOptimum; break; }
    double best = 0.0;
    for (int i = 0; i < m; ++i)
      if (nl_pivotable(t[i * ld + c])) {
        const double ratio = nl_ratio(t[i * ld + n], t[i * ld + c]);
        if (r < 0 || ratio < best) { best = ratio; r = i; }
      }
    if (r < 0 || !nl_ties(best, best)) { status = kNlNoOptimum; break; }   // (a ratio that overflowed: inf - inf is no tie)
    for (int i = 0; i < m; ++i)
      if (nl_pivotable(t[i * ld + c]) && nl_ties(nl_ratio(t[i * ld + n], t[i * ld + c]), best) && row_label[i] < row_label[r]) r = i;
    const double p = t[r * ld + c];
    for (int j = 0; j <= n; ++j)
      if (j != c) t[r * ld + j] = nl_scaled(t[r * ld + j], p);
    for (int i = 0; i <= m; ++i) {
      if (i == r) continue;
      const double column = t[i * ld + c];
      for (int j = 0; j <= n; ++j)
        if (j != c) t[i * ld + j] = nl_update(t[i * ld + j], column, t[r * ld + j]);
      t[i * ld + c] = nl_column(column, p);
    }
    t[r * ld + c] = nl_inverse(p);
    const int label = col_label[c];
    col_label[c] = row_label[r];
    row_label[r] = label;
    ++done;
  }
  *pivots = done;
  if (status != kNlOk) {
    for (int i = 0; i < m; ++i) x[i] = nl_nan();
    for (int j = 0; j < n; ++j) y[j] = nl_nan();
    *value = nl_nan();
    return status;
  }
  for (int i = 0; i < m; ++i) x[i] = 0.0;
  for (int j = 0; j < n; ++j) y[j] = 0.0;
  for (int i = 0; i < m; ++i)
    if (row_label[i] < n) y[row_label[i]] = nl_clamp(t[i * ld + n]);
  for (int j = 0; j < n; ++j)
    if (col_label[j] >= n) x[col_label[j] - n] = nl_clamp(t[m * ld + j]);
  const double sy = nl_sum(y, n), sx = nl_sum(x, m);
  for (int i = 0; i < m; ++i) x[i] = x[i] / sx;
  for (int j = 0; j < n; ++j) y[j] = y[j] / sy;
  *value = nl_value(sy, span, base) / pre;
  return status;
}

}  // namespace osg

#endif  // OSG_NASH_LP_H_
