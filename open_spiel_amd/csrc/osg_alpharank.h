// Alpha-rank (Omidshafiei et al., "alpha-Rank"; open_spiel/python/egt/alpharank.py, "ar" below) on a normal-form
// meta-game: the Markov chain over pure profiles, its stationary distribution, the sweep over the infinite-alpha noise
// epsilon and the per-player marginals (psro_v2/utils.py get_alpharank_marginals): every formula and the ONE order of
// every sum, host + device.  The kernels of osg_alpharank.hip run these functions, and so does
// tests/native/alpharank_host_test.cpp on the CPU; tests/alpharank_cases.py restates them in NumPy.
//
// Profiles.  A problem is P payoff tensors T_p [K_0 .. K_{P-1}], row-major.  A profile's id is its row-major index
// (get_id_from_strat_profile = tensor.reshape(-1)); the chain's states are the n = prod K_p profiles, a profile's
// neighbours differ from it in exactly one player's strategy, eta = 1 / sum (K_p - 1).  A row's neighbours are numbered
// ("moves") player after player, and within a player its other strategies ascending (ar_neighbour).  P = 1 is the
// single-population chain with the local selection model over a [K, K] table: n = K states, eta = 1 / (K - 1), the move
// from s to r compares pc = T[r, s] with pr = T[s, r] (ar:294-319).
//
// Off-diagonal entries.  pc / pr: the deviating player's payoff at the column / row profile.
//   infinite alpha (ar:354-374): |pc - pr| <= 1e-14 + 1e-5 * |pr| (np.isclose with its default rtol, relative to the
//     SECOND argument): eta * 0.5; else pc > pr: eta * (1 - eps); else eta * eps.  One multiplication each.
//   finite alpha (_get_rho_sr_multipop with use_fast_compute, ar:237-243): u = alpha * (pc - pr); |u| <= 1e-14: rho = 1 / m;
//     else rho = (1 - e^-u) / (1 - e^-mu), evaluated WITHOUT the reference's cancellation and overflow:
//       u > 0: expm1(-u) / expm1(-m u);   u < 0: (exp((m - 1) u) * expm1(u)) / expm1(m u)   (every exponent <= 0);
//     where the true rho underflows the result is 0.  The entry is eta * rho.
//   A payoff that is not finite makes the entry NaN (the reference would compare it and go on).
//
// Stationary distribution: Grassmann-Taksar-Heyman elimination (no eigen-solve).  a[i][j] at a[i * lda + j]; the
// diagonal is never read.  For k = n - 1 down to 1:
//     s = ar_lane_sum(a[k][0 .. k-1]);  s == 0 or not finite: status 1 (the chain is not irreducible in floating point)
//     for i < k: q = a[i][k] / s; a[i][k] = q; for j < k: a[i][j] = a[i][j] + q * a[k][j]
//   then x[0] = 1 and, for i = 0 .. n-2 in turn, x[k] = x[k] + x[i] * a[i][k] for every k > i (x[k] starts at 0.0: a plain
//   sum over i ascending); total = ar_lane_sum(x); pi = x / total (a total that is not finite: status 1).
//   ar_lane_sum(v[0 .. c-1]): 64 partial sums, partial l = v[l] + v[l + 64] + .. from 0.0 ascending, combined by a pairwise
//   tree over neighbours ((p0 + p1) + (p2 + p3)) + ..: a wavefront's lanes and six exchange steps.
//   Nothing is subtracted, so nothing turns negative and small masses keep their relative accuracy.
//   THE MULTIPLY-ADD IS NOT FUSED: q * a[k][j] is rounded, then added (ar_madd).  The library, the host test and NumPy
//   all do that; everything here is compiled with -ffp-contract=off.  No floating-point atomics.
//
// The sweep (the error-free path of sweep_pi_vs_epsilon, ar:506-528): eps_0 = the warm start or 0.5, eps_{t+1} = 0.5 *
// eps_t; stop at the first t > min_iters with |pi_t - pi_{t-1}| <= 1e-8 + 1e-5 * |pi_{t-1}| in every entry (np.allclose);
// a solve at t that does not stop with t + 1 >= max_iters: status 2.  A status 1 ends the sweep (GTH does not fail where
// the reference's eig does, so its except-branch that raises epsilon again has no counterpart).
//
// Marginals: player p's strategy k gets the sum of pi over the profiles with idx_p = k, from 0.0, ids ascending.
#ifndef OSG_ALPHARANK_H_
#define OSG_ALPHARANK_H_

#include "osg_common.h"

#include <math.h>

namespace osg {

constexpr int kArMaxPlayers = 5;
constexpr int kArMaxProfiles = 4096;
constexpr int kArLanes = 64;
enum ArMode { kArFinite = 0, kArInfinite = 1, kArSweep = 2 };
enum ArStatus { kArOk = 0, kArReducible = 1, kArNoStop = 2 };

struct ArShape {
  int P;                      // populations: 1 = the single-population chain over a [K, K] table
  int K[kArMaxPlayers];       // P = 1: K[0] = K
  int stride[kArMaxPlayers];  // of a profile's id; P = 1: the table's row stride K at [0]
  int n;                      // states
  int SK;                     // sum K_p (P = 1: K): the length of the marginals
  int moves;                  // neighbours of a state: sum (K_p - 1)
  int64_t cells;              // doubles of one problem's tensors: P * n, or K * K
  double eta;
};

// shape: [P] sizes, or for P = 1 the table's [K, K] (the caller has checked it square).
OSG_HD ArShape ar_shape(int P, const int32_t* shape) {
  ArShape sh{};
  sh.P = P;
  sh.n = 1;
  for (int p = P - 1; p >= 0; --p) {
    sh.K[p] = shape[p];
    sh.stride[p] = sh.n;
    sh.n *= shape[p];
  }
  for (int p = 0; p < P; ++p) { sh.SK += sh.K[p]; sh.moves += sh.K[p] - 1; }
  if (P == 1) sh.stride[0] = sh.K[0];
  sh.cells = P == 1 ? static_cast<int64_t>(sh.K[0]) * sh.K[0] : static_cast<int64_t>(P) * sh.n;
  sh.eta = 1.0 / static_cast<double>(sh.moves);   // (moves = 0: one state, no entry)
  return sh;
}

OSG_HD double ar_nan() { return __builtin_nan(""); }
OSG_HD bool ar_is_finite(double x) { return x - x == 0.0; }
OSG_HD int ar_index(const ArShape& sh, int id, int p) { return (id / sh.stride[p]) % sh.K[p]; }

// Move `mv` of state `row`: the column state and where the two payoffs lie in the problem's tensors.
OSG_HD void ar_neighbour(const ArShape& sh, int row, int mv, int* col, int64_t* at_col, int64_t* at_row) {
  if (sh.P == 1) {
    const int r = mv + (mv >= row ? 1 : 0);
    *col = r;
    *at_col = static_cast<int64_t>(r) * sh.K[0] + row;   // T[r, s]
    *at_row = static_cast<int64_t>(row) * sh.K[0] + r;   // T[s, r]
    return;
  }
  int p = 0;
#pragma unroll
  for (int q = 0; q < kArMaxPlayers - 1; ++q)
    if (q + 1 < sh.P && p == q && mv >= sh.K[q] - 1) { mv -= sh.K[q] - 1; p = q + 1; }
  int stride = 0, own = 0;
#pragma unroll
  for (int q = 0; q < kArMaxPlayers; ++q)
    if (q == p) { stride = sh.stride[q]; own = (row / sh.stride[q]) % sh.K[q]; }
  const int alt = mv + (mv >= own ? 1 : 0);
  *col = row + (alt - own) * stride;
  *at_col = static_cast<int64_t>(p) * sh.n + *col;
  *at_row = static_cast<int64_t>(p) * sh.n + row;
}

OSG_HD bool ar_tie(double pc, double pr) { return fabs(pc - pr) <= 1e-14 + 1e-5 * fabs(pr); }
OSG_HD double ar_entry_infinite(double eta, double pc, double pr, double eps) {
  if (!ar_is_finite(pc) || !ar_is_finite(pr)) return ar_nan();
  if (ar_tie(pc, pr)) return eta * 0.5;
  if (pc > pr) return eta * (1.0 - eps);
  return eta * eps;
}
OSG_HD double ar_rho(double pc, double pr, double alpha, int m) {
  if (!ar_is_finite(pc) || !ar_is_finite(pr)) return ar_nan();
  const double u = alpha * (pc - pr), md = static_cast<double>(m);
  if (fabs(u) <= 1e-14) return 1.0 / md;
  if (u > 0.0) return expm1(-u) / expm1(-(md * u));
  return (exp((md - 1.0) * u) * expm1(u)) / expm1(md * u);
}
OSG_HD double ar_entry_finite(double eta, double pc, double pr, double alpha, int m) { return eta * ar_rho(pc, pr, alpha, m); }
OSG_HD double ar_entry(const ArShape& sh, const double* tensors, int row, int mv, int mode, double eps, double alpha, int m, int* col) {
  int64_t at_col, at_row;
  ar_neighbour(sh, row, mv, col, &at_col, &at_row);
  const double pc = tensors[at_col], pr = tensors[at_row];
  return mode == kArFinite ? ar_entry_finite(sh.eta, pc, pr, alpha, m) : ar_entry_infinite(sh.eta, pc, pr, eps);
}

OSG_HD double ar_madd(double acc, double q, double r) {
  const double product = q * r;   // rounded: NOT a fused multiply-add
  return acc + product;
}
OSG_HD bool ar_pivot_ok(double s) { return s > 0.0 && ar_is_finite(s); }

// The tree over the 64 partial sums (destroys them).
OSG_HD double ar_tree(double* part) {
  for (int width = kArLanes; width > 1; width >>= 1)
    for (int l = 0; l < (width >> 1); ++l) part[l] = part[2 * l] + part[2 * l + 1];
  return part[0];
}
OSG_HD double ar_lane_sum(const double* v, int count) {
  double part[kArLanes];
  for (int l = 0; l < kArLanes; ++l) {
    double sum = 0.0;
    for (int j = l; j < count; j += kArLanes) sum = sum + v[j];
    part[l] = sum;
  }
  return ar_tree(part);
}

// The whole solve on one matrix, serially (every element's operations are those of the kernel, which spreads the
// trailing block over its lanes): a [n, lda] with the off-diagonals, x [n] scratch, pi [n].  Returns the status.
inline int ar_stationary(double* a, int n, int64_t lda, double* x, double* pi) {
  int status = kArOk;
  for (int k = n - 1; k >= 1 && status == kArOk; --k) {
    const double* rk = a + k * lda;
    const double s = ar_lane_sum(rk, k);
    if (!ar_pivot_ok(s)) { status = kArReducible; break; }
    for (int i = 0; i < k; ++i) {
      double* ri = a + i * lda;
      const double q = ri[k] / s;
      ri[k] = q;
      for (int j = 0; j < k; ++j) ri[j] = ar_madd(ri[j], q, rk[j]);
    }
  }
  if (status == kArOk) {
    for (int i = 0; i < n; ++i) x[i] = i == 0 ? 1.0 : 0.0;
    for (int i = 0; i + 1 < n; ++i)
      for (int k = i + 1; k < n; ++k) x[k] = ar_madd(x[k], x[i], a[i * lda + k]);
    const double total = ar_lane_sum(x, n);
    if (!ar_is_finite(total)) status = kArReducible;
    else for (int i = 0; i < n; ++i) pi[i] = x[i] / total;
  }
  if (status != kArOk)
    for (int i = 0; i < n; ++i) pi[i] = ar_nan();
  return status;
}

// ---- the sweep ----
OSG_HD double ar_sweep_start(double warm_start) { return warm_start == 0.0 ? 0.5 : warm_start; }
OSG_HD double ar_eps_at(double eps0, int t) {
  double eps = eps0;
  for (int k = 0; k < t; ++k) eps = eps * 0.5;
  return eps;
}
OSG_HD bool ar_close(double now, double prev) { return fabs(now - prev) <= 1e-8 + 1e-5 * fabs(prev); }

// ---- marginals ----  entry x of [SK]: which player and strategy
OSG_HD double ar_marginal(const ArShape& sh, const double* pi, int x) {
  if (sh.P == 1) return pi[x];
  int p = 0;
#pragma unroll
  for (int q = 0; q < kArMaxPlayers - 1; ++q)
    if (q + 1 < sh.P && p == q && x >= sh.K[q]) { x -= sh.K[q]; p = q + 1; }
  int stride = 0, Kp = 1;
#pragma unroll
  for (int q = 0; q < kArMaxPlayers; ++q)
    if (q == p) { stride = sh.stride[q]; Kp = sh.K[q]; }
  double sum = 0.0;
  for (int id = 0; id < sh.n; ++id)
    if ((id / stride) % Kp == x) sum = sum + pi[id];
  return sum;
}

}  // namespace osg

#endif  // OSG_ALPHARANK_H_
