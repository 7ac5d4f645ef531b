// Meta-strategy solvers of PSRO on a normal-form meta-game: projected replicator dynamics
// (open_spiel/python/algorithms/projected_replicator_dynamics.py, "prd" below) and regret matching (regret_matching.py,
// "rm"), with nfg_utils.StrategyAverager's average (nfg_utils.py): the arithmetic of ONE step of ONE player, host + device.
// The kernel of osg_meta_solver.hip runs these functions (one wavefront per player, lane a = own action a), and so does
// tests/native/meta_solver_host_test.cpp on the CPU against what the reference's own files left in
// tests/golden/meta_solver_vectors.npz.
//
// A problem is P payoff tensors T_p [K_0 .. K_{P-1}] and P strategies s_p [K_p].  All players step simultaneously from
// the previous step's strategies (prd:139-153, rm:73-95).  ONE order for every sum:
//
//   values (_partial_multi_dot, prd:45-52 = rm:48-55): the other players q_0 < q_1 < .. are contracted from the last to
//     the first, each contraction a full intermediate,
//       v[a] = sum_{j_0} ( .. ( sum_{j_last} T_p[a; j_0 .. j_last] * s_last[j_last] ) .. ) * s_{q_0}[j_0]
//     every sum from 0.0 over its index ascending, each term one product added to the running sum (meta_value).  NumPy
//     hands these sums to BLAS in an order nobody controls: the reference is matched within a tolerance, not bit for bit.
//   average_return = sum_a v[a] * s[a] from 0.0, a ascending (prd:145 = rm:79; meta_average_return)
//   prd: delta = s * (v - avg), u = s + dt * delta (prd:146-148; meta_prd_update), then the projection
//     exact (_simplex_projection, prd:114-119): u sorted descending (equal values in index order: meta_rank_desc);
//       cumsum[0] = u_(0), cumsum[i] = cumsum[i-1] + u_(i); u_tmp[i] = (1 - cumsum[i] - (n - (i+1)) * gamma) / (i+1)
//       (meta_u_tmp); b[i] = u_(i) + u_tmp[i] <= gamma (meta_rho_test); rho = numpy's LEFT BISECTION for True over b,
//       which need not be sorted (meta_bisect_left: lo = 0, hi = n; mid = lo + (hi - lo) / 2; b[mid] false: lo = mid + 1,
//       else hi = mid); shift = u_tmp[rho - 1], and rho = 0 reads u_tmp[n - 1] as Python's index -1 does (meta_rho_index);
//       s' = max(u + shift, gamma) (meta_project).
//     approximate (_approx_simplex_projection, prd:88-90): c = u < gamma ? gamma : u (meta_clamp); s' = c / sum_a c[a],
//       the sum from 0.0 ascending.
//   rm: regrets start at 1 / 1e6 (rm:26,131-134); R += v - avg (rm:80; meta_rm_regret); R+ = R < 0 ? 0 : R (rm:82-83);
//     sum = sum_a R+[a] from 0.0 ascending (rm:84); sum > 0: s' = gamma * (1 / n) + (1 - gamma) * (R+ / sum), else
//     s' = 1 / n (rm:85-92; meta_rm_strategy).
//   average (StrategyAverager, nfg_utils.py:46-82; prd:194-202 = rm:136-144): the initial strategies are entry 0, every
//     iteration appends one; with `window` = 0 all iterations + 1 entries count, otherwise the last
//     min(window, iterations + 1) (meta_average_count).  Their sum starts at 0.0 at the oldest counted entry and adds
//     oldest to newest; it is divided by the count.  No ring buffer: accumulation starts at entry iterations + 1 - count.
//
// Nothing here may be contracted into a fused multiply-add: the library and the host test are compiled with
// -ffp-contract=off.  No floating-point atomics.  The tensors are expected finite (a NaN has no place in a sort).
#ifndef OSG_META_SOLVER_H_
#define OSG_META_SOLVER_H_

#include "osg_common.h"

namespace osg {

constexpr int kMetaMinPlayers = 2;
constexpr int kMetaMaxPlayers = 5;
constexpr int kMetaMaxActions = 64;                       // one wavefront's lanes
constexpr int64_t kMetaMaxCells = int64_t{1} << 22;       // K_0 * .. * K_{P-1} per problem
constexpr double kMetaInitialRegret = 1.0 / 1e6;          // rm:26,131-134
enum MetaMethod { kMetaPrd = 0, kMetaRm = 1 };

// How player p's values read its tensor: the other players in ascending order, for each its size, the distance between
// two of its indices in the tensor as stored, and where its strategy starts in the flat strategy vector [sum K].
struct MetaView {
  int others;                            // P - 1
  int n[kMetaMaxPlayers - 1];
  int64_t stride[kMetaMaxPlayers - 1];
  int s_off[kMetaMaxPlayers - 1];
  int64_t own_stride;
};

// Player p's view of a tensor [K_0 .. K_{P-1}] (off[q]: where player q's strategy starts): row-major as the caller keeps
// it, or `staged` with p's OWN index fastest and the others row-major above it (what the kernel keeps in LDS: lane a
// then reads word a of a row).  The same cells either way, so meta_value adds the same terms in the same order.
OSG_HD MetaView meta_view(int P, const int* K, const int* off, int p, bool staged) {
  MetaView w{};
  w.others = P - 1;
  int64_t natural[kMetaMaxPlayers] = {0, 0, 0, 0, 0};
  int64_t run = 1;
  for (int q = P - 1; q >= 0; --q) { natural[q] = run; run *= K[q]; }
  w.own_stride = staged ? 1 : natural[p];
  run = K[p];
  for (int d = P - 2; d >= 0; --d) {
    const int q = d + (d >= p ? 1 : 0);
    w.n[d] = K[q];
    w.s_off[d] = off[q];
    w.stride[d] = staged ? run : natural[q];
    run *= K[q];
  }
  return w;
}
// Where the cell idx[0 .. P-1] of player p's tensor lies under p's view w.
OSG_HD int64_t meta_cell_at(const MetaView& w, int p, const int* idx) {
  int64_t at = idx[p] * w.own_stride;
#pragma unroll
  for (int d = 0; d < kMetaMaxPlayers - 1; ++d)
    if (d < w.others) at += idx[d + (d >= p ? 1 : 0)] * w.stride[d];
  return at;
}

// The contraction below level D (levels D .. M - 1 remain), `cells` at the indices chosen so far.
template <int M, int D>
OSG_HD double meta_contract(const MetaView& w, const double* cells, const double* s) {
  double acc = 0.0;
  const double* sq = s + w.s_off[D];
  for (int j = 0; j < w.n[D]; ++j) {
    double x;
    if constexpr (D == M - 1) x = cells[j * w.stride[D]];
    else x = meta_contract<M, D + 1>(w, cells + j * w.stride[D], s);
    acc = acc + x * sq[j];
  }
  return acc;
}
// v[a] of the player whose view is w: `tensor` its payoff tensor, `s` the flat strategies of the previous step.
OSG_HD double meta_value(const MetaView& w, const double* tensor, const double* s, int a) {
  const double* cells = tensor + a * w.own_stride;
  switch (w.others) {
    case 1: return meta_contract<1, 0>(w, cells, s);
    case 2: return meta_contract<2, 0>(w, cells, s);
    case 3: return meta_contract<3, 0>(w, cells, s);
    default: return meta_contract<4, 0>(w, cells, s);
  }
}

OSG_HD double meta_sum_step(double sum, double x) { return sum + x; }   // every ascending sum: from 0.0, one of these per index
OSG_HD double meta_return_term(double v, double s) { return v * s; }
OSG_HD double meta_average_return(const double* v, const double* s, int n) {
  double avg = 0.0;
  for (int a = 0; a < n; ++a) avg = meta_sum_step(avg, meta_return_term(v[a], s[a]));
  return avg;
}

// ---- projected replicator dynamics ----
OSG_HD double meta_prd_update(double s, double v, double avg, double dt) {
  const double delta = s * (v - avg);
  return s + dt * delta;
}
// Whether u_j stands before u_a in the descending order (equal values: the lower index first).
OSG_HD bool meta_before(double uj, int j, double ua, int a) { return uj > ua || (uj == ua && j < a); }
OSG_HD int meta_rank_desc(const double* u, int n, int a) {
  int rank = 0;
  for (int j = 0; j < n; ++j) rank += meta_before(u[j], j, u[a], a) ? 1 : 0;
  return rank;
}
OSG_HD double meta_u_tmp(double cumsum, int n, int i /* 0-based position in the sorted order */, double gamma) {
  const int idx = i + 1;
  return (1.0 - cumsum - static_cast<double>(n - idx) * gamma) / static_cast<double>(idx);
}
OSG_HD bool meta_rho_test(double u_sorted, double u_tmp, double gamma) { return u_sorted + u_tmp <= gamma; }
// np.searchsorted(b, True) (side="left") over b[i] = bit i of `mask`, i < n.
OSG_HD int meta_bisect_left(uint64_t mask, int n) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (!((mask >> mid) & 1u)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
OSG_HD int meta_rho_index(int rho, int n) { return rho > 0 ? rho - 1 : n - 1; }
OSG_HD double meta_project(double u, double shift, double gamma) {
  const double x = u + shift;
  return (x >= gamma || x != x) ? x : gamma;   // np.maximum
}
OSG_HD double meta_clamp(double u, double gamma) { return u < gamma ? gamma : u; }

// One player's exact-projection step over arrays: u [n] in, s_new [n] out.
OSG_HD void meta_simplex_projection(const double* u, int n, double gamma, double* s_new) {
  double sorted[kMetaMaxActions], u_tmp[kMetaMaxActions];
  for (int a = 0; a < n; ++a) sorted[meta_rank_desc(u, n, a)] = u[a];
  uint64_t mask = 0;
  double cumsum = 0.0;
  for (int i = 0; i < n; ++i) {
    cumsum = i == 0 ? sorted[0] : meta_sum_step(cumsum, sorted[i]);
    u_tmp[i] = meta_u_tmp(cumsum, n, i, gamma);
    if (meta_rho_test(sorted[i], u_tmp[i], gamma)) mask |= uint64_t{1} << i;
  }
  const double shift = u_tmp[meta_rho_index(meta_bisect_left(mask, n), n)];
  for (int a = 0; a < n; ++a) s_new[a] = meta_project(u[a], shift, gamma);
}
OSG_HD void meta_approx_projection(const double* u, int n, double gamma, double* s_new) {
  double sum = 0.0;
  for (int a = 0; a < n; ++a) sum = meta_sum_step(sum, meta_clamp(u[a], gamma));
  for (int a = 0; a < n; ++a) s_new[a] = meta_clamp(u[a], gamma) / sum;
}
// One player's PRD step: v [n] its values, s [n] its strategy of the previous step.
OSG_HD void meta_prd_step(const double* v, const double* s, int n, double dt, double gamma, bool use_approx, double* s_new) {
  const double avg = meta_average_return(v, s, n);
  double u[kMetaMaxActions];
  for (int a = 0; a < n; ++a) u[a] = meta_prd_update(s[a], v[a], avg, dt);
  if (use_approx) meta_approx_projection(u, n, gamma, s_new);
  else meta_simplex_projection(u, n, gamma, s_new);
}

// ---- regret matching ----
OSG_HD double meta_rm_regret(double regret, double v, double avg) { return regret + (v - avg); }
OSG_HD double meta_rm_positive(double regret) { return regret < 0.0 ? 0.0 : regret; }
OSG_HD double meta_rm_strategy(double positive, double sum, int n, double gamma) {
  const double uniform = 1.0 / static_cast<double>(n);
  if (!(sum > 0.0)) return uniform;
  const double x = positive / sum;
  return gamma * uniform + (1.0 - gamma) * x;
}
// One player's step: regrets [n] updated in place.
OSG_HD void meta_rm_step(const double* v, const double* s, int n, double gamma, double* regrets, double* s_new) {
  const double avg = meta_average_return(v, s, n);
  double sum = 0.0;
  for (int a = 0; a < n; ++a) {
    regrets[a] = meta_rm_regret(regrets[a], v[a], avg);
    sum = meta_sum_step(sum, meta_rm_positive(regrets[a]));
  }
  for (int a = 0; a < n; ++a) s_new[a] = meta_rm_strategy(meta_rm_positive(regrets[a]), sum, n, gamma);
}

// ---- the average ----
OSG_HD int64_t meta_average_count(int iterations, int window) {
  const int64_t all = static_cast<int64_t>(iterations) + 1;
  return window > 0 && window < all ? window : all;
}
OSG_HD double meta_average(double sum, int64_t count) { return sum / static_cast<double>(count); }

}  // namespace osg

#endif  // OSG_META_SOLVER_H_
