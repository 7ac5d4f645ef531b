// Payoff-tensor cells and policy aggregation for a population of policy tables (policy_value in
// open_spiel/python/algorithms/expected_game_score.py:35-58; PolicyAggregator.aggregate in policy_aggregator.py:130-265):
// the arithmetic of ONE own-reach product, ONE row of a table's realization plan, ONE terminal history, ONE chunk of
// terminals and ONE aggregated row, host + device.  The kernels of osg_cfr_population.hip run exactly these functions,
// and so does tests/native/population_host_test.cpp on the CPU against what the reference's own files left in
// tests/golden/population_vectors.npz.
//
// A population is a stack [K, I, A] of policy tables in the legal-index layout; "policy k of player p" is table k's rows
// at p's infostates.  The games have perfect recall: every member history of an infostate i of player p is reached by
// the same own actions in the same order, so p's own reach there is one number per table,
//   own_k(i)        the product of table k's cells on the root path of i's FIRST member, p's own entries only, started at
//                   `start` and multiplied root to leaf
// Profile returns (start = 1.0).  The realization plan of table k, plan_k[i, a] = own_k(i) * pi_k(a | i), is the own
// reach of whoever acts at i after taking a.  A terminal history z keeps, per player p, the plan index seq_p(z) of p's
// last action on its root path (-1: p never acted) and c(z), the product of the chance probabilities root to leaf from
// 1.0.  For the profile (k_0 .. k_{P-1}):
//   w(z)         = (((c(z) * plan_{k_0}[seq_0(z)]) * plan_{k_1}[seq_1(z)]) ...)       a player who never acted: no factor
//   returns[q]   = sum_z u_q(z) * w(z)
// summed in ONE order: the terminals in history order in chunks of kPopChunk = 256; inside a chunk the 64 terms of each
// wavefront by the halving tree of pop_wave_sum (x[l] += x[l + 32], then 16, ... 1), the four wavefronts' sums left to
// right, and the chunks' sums added to 0.0 in ascending order.  A term past the last terminal is 0.0.  The bits of a
// profile's returns depend on the game and its P tables alone.  The reference adds the same products along the tree
// instead (bottom-up, skipping actions of probability 0): the difference is rounding, bounded by the tests' tolerance.
//
// Aggregation (start = the weight).  For infostate i of player p and legal action a, over i's member histories h in the
// reference's visiting order and per history k ascending (policy_aggregator.py:250-260):
//   acc[a] += own_k(h; start = weights[p, k]) * pi_k(a | i)                                       (:255-260)
//   out[a] = (acc[a] + epsilon) / sum_a' (acc[a'] + epsilon), the sum from 0 left to right        (:171-178)
// A table of weight 0 adds +0.0 terms: nothing.  Nothing here may be contracted into a fused multiply-add: the library
// and the host test are compiled with -ffp-contract=off.
//
// A root path is the list of codes the tabular solvers keep per decision history (osg_action_values.h).
#ifndef OSG_POPULATION_H_
#define OSG_POPULATION_H_

#include "osg_common.h"

namespace osg {

constexpr int kPopChunk = 256;      // terminals per chunk: four wavefronts
constexpr int kPopMaxActions = 8;   // widest row aggregated in registers

// Player p's own reach at the history whose root path is path[begin, end) under the table `pol` [I, A].
OSG_HD double pop_own_reach(const int32_t* path, int begin, int end, int p, const double* pol, double start) {
  double x = start;
  for (int e = begin; e < end; ++e) {
    const int code = path[e];
    if (((code >> 23) & 1) || ((code >> 24) & 0xF) != p) continue;
    x = x * pol[code & 0x7FFFFF];
  }
  return x;
}

// One row of a realization plan: own * pi(a), padding cells 0.
OSG_HD void pop_plan_row(double own, const double* pol_row, int n, int A, double* plan_row) {
  for (int a = 0; a < A; ++a) plan_row[a] = a < n ? own * pol_row[a] : 0.0;
}

// w(z): seq [P] are z's plan indices, plan_of(p) the realization plan of the table player p follows.
template <class PlanOf>
OSG_HD double pop_terminal_weight(double chance, const int32_t* seq, int P, PlanOf plan_of) {
  double w = chance;
  for (int p = 0; p < P; ++p)
    if (seq[p] >= 0) w = w * plan_of(p)[seq[p]];
  return w;
}
OSG_HD double pop_return_term(double utility, double weight) { return utility * weight; }

// The sum of a wavefront's 64 terms, in place: what six shuffle-down steps leave in lane 0.
OSG_HD double pop_wave_sum(double* x) {
  for (int off = 32; off >= 1; off >>= 1)
    for (int l = 0; l < off; ++l) x[l] = x[l] + x[l + off];
  return x[0];
}
OSG_HD double pop_chunk_sum(double w0, double w1, double w2, double w3) { return ((w0 + w1) + w2) + w3; }

// One aggregated row by ONE thread: infostate i of player p with n legal actions and the members m0 .. m1 - 1 (positions
// in path_off).  tables [K, I, A], weights_p [K] player p's row of the weights.
OSG_HD void pop_aggregate_row(int i, int p, int n, int A, int m0, int m1, const int32_t* path_off, const int32_t* path,
                              const double* tables, int K, size_t table_stride, const double* weights_p, double epsilon,
                              double* out_row) {
  double acc[kPopMaxActions];
  for (int a = 0; a < n; ++a) acc[a] = 0.0;
  for (int m = m0; m < m1; ++m)
    for (int k = 0; k < K; ++k) {
      const double* pol = tables + static_cast<size_t>(k) * table_stride;
      const double reach = pop_own_reach(path, path_off[m], path_off[m + 1], p, pol, weights_p[k]);
      for (int a = 0; a < n; ++a) acc[a] += reach * pol[static_cast<size_t>(i) * A + a];
    }
  double denom = 0.0;
  for (int a = 0; a < n; ++a) denom += acc[a] + epsilon;
  for (int a = 0; a < A; ++a) out_row[a] = a < n ? (acc[a] + epsilon) / denom : 0.0;
}

}  // namespace osg

#endif  // OSG_POPULATION_H_
