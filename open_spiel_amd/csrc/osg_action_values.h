// Per-infostate action values and reaches of a policy profile (TreeWalkCalculator in
// open_spiel/python/algorithms/action_value.py:87-216; Calculator in action_value_vs_best_response.py:63-156): the
// arithmetic of ONE policy row, ONE member history, ONE tree node and ONE infostate, host + device.  The kernels of
// osg_cfr_qvalues.hip run exactly these functions, and so does tests/native/action_values_host_test.cpp on the CPU
// against what the reference's own files left in tests/golden/action_value_vectors.npz.
//
// The profile sigma: every player plays the evaluated policy, except a best responder b (if any), whose rows are the
// indicator of its TabularBestResponse action.  For a decision history h of player p with infostate i
// (action_value.py:117-132, 139-152):
//   r_q(h)     the product of sigma_q's probabilities on the root path, c(h) the same for chance: started at 1.0 and
//              multiplied root to leaf (:141-142)
//   reach(h)   np.prod([r_0 .. r_{P-1}, c]) left to right (:119)
//   opp(h)     np.prod(r[:p]) * np.prod(r[p+1:-1]), an empty product 1.0 (:122-124)
//   v(h)[q]    the returns at a terminal, else sum_a sigma(a) * v(child(h, a))[q] over the legal actions ascending,
//              started at 0.0, no term skipped (:134, 152)
// and per infostate, over its member histories in the DFS order the reference visits them:
//   reach[i] += reach(h)   cf_reach[i] += c(h) * opp(h)   chance_reach[i] += c(h)   player_reach[i] = r_p(h)   (:125-132)
//   weighted[i, a, q] += v(child(h, a))[q] * reach(h)                                                        (:148)
//   cf_q[i, a] += (v(child(h, a))[p] * opp(h)) * c(h)                                                        (:149-151)
//   q[i, a] = weighted[i, a, p] / reach[i] where reach[i] > 0, else 0                                        (:202-204)
// Every member of an infostate holds the same r_p bits under perfect recall (the same own cells in the same order): the
// first member's is taken.  Every sum has this one order in every kernel form, so two runs and any two forms give the
// same bits.  Nothing here may be contracted into a fused multiply-add: the library and the host test are compiled with
// -ffp-contract=off.
//
// A root path is the list of codes the tabular solvers keep per decision history (osg_cfr.hip build_tree), root to
// leaf: slot << 24 | is_chance << 23 | index, where slot is the acting player of the ancestor (P for chance) and
// index is the child history for a chance ancestor, (its infostate) * A + (the action's index among its legal actions)
// for a decision ancestor.
#ifndef OSG_ACTION_VALUES_H_
#define OSG_ACTION_VALUES_H_

#include "osg_common.h"

namespace osg {

// One row of sigma.  mode 0: `src` is a row of the cumulative-policy table and the evaluated policy its normalisation
// (CFRAveragePolicy, cfr.cc:104-125, as k_policy_eval forms it); mode 1: `src` is the policy row itself.  best >= 0:
// the row belongs to the best responder and becomes the indicator of that action index.  dst may be src.
OSG_HD void qv_sigma_row(const double* src, double* dst, int n, int A, int mode, int best) {
  double sum = 0.0;
  if (mode == 0)
    for (int a = 0; a < n; ++a) sum += src[a];
  for (int a = 0; a < A; ++a) {
    double p = a >= n ? 0.0 : (mode == 0 ? (sum == 0.0 ? 1. / n : src[a] / sum) : src[a]);
    if (best >= 0) p = a == best ? 1.0 : 0.0;
    dst[a] = p;
  }
}

// The P + 1 reach products of the member history whose root path is path[begin, end): r[q] for player q, r[P] for chance.
OSG_HD void qv_member_reach(const int32_t* path, int begin, int end, int P, const double* sigma, const double* edge_prob,
                            double* r) {
  for (int q = 0; q <= P; ++q) {   // slot by slot: every product still takes its factors root to leaf
    double x = 1.0;
    for (int e = begin; e < end; ++e) {
      const int code = path[e];
      if (((code >> 24) & 0xF) != q) continue;
      const int idx = code & 0x7FFFFF;
      x = x * (((code >> 23) & 1) ? edge_prob[idx] : sigma[idx]);
    }
    r[q] = x;
  }
}

struct QvMember { double reach, opp, chance, own; };

// What a member history of player p adds to its infostate, from its P + 1 reach products.
OSG_HD QvMember qv_member(const double* r, int P, int p) {
  QvMember m;
  m.reach = r[0];
  for (int q = 1; q <= P; ++q) m.reach = m.reach * r[q];
  double before = 1.0, after = 1.0;
  for (int q = 0; q < p; ++q) before = q == 0 ? r[0] : before * r[q];
  for (int q = p + 1; q < P; ++q) after = q == p + 1 ? r[q] : after * r[q];
  m.opp = before * after;
  m.chance = r[P];
  m.own = r[p];
  return m;
}
OSG_HD double qv_cf_reach_term(const QvMember& m) { return m.chance * m.opp; }
OSG_HD double qv_weighted_term(double child_value, const QvMember& m) { return child_value * m.reach; }
OSG_HD double qv_cf_value_term(double child_value, const QvMember& m) { return (child_value * m.opp) * m.chance; }
OSG_HD double qv_action_value(double weighted, double reach) { return reach > 0 ? weighted / reach : 0.0; }

// v(h)[q] of an inner node with nc children from first_child on: prob[a] is sigma's row or the chance probabilities of
// the children; value is [H, P].
OSG_HD double qv_node_value(const double* prob, const double* value, int first_child, int nc, int P, int q) {
  double v = 0.0;
  for (int a = 0; a < nc; ++a) v += value[static_cast<size_t>(first_child + a) * P + q] * prob[a];
  return v;
}

struct QvTables {   // the per-infostate outputs; padding cells are written 0
  double* reach;         // [I]
  double* cf_reach;      // [I]
  double* chance_reach;  // [I]
  double* player_reach;  // [I]
  double* q;             // [I, A]
  double* cf_q;          // [I, A]
  double* weighted;      // [I, A, P]
};

// Every output of infostate i (player p, n legal actions) by ONE thread: the members mem[m0, m1) in order.  rm is
// [M, P + 1] (qv_member_reach per member position), value [H, P].
OSG_HD void qv_infostate(int i, int p, int n, int A, int P, int m0, int m1, const int32_t* mem, const int32_t* first_child,
                         const double* rm, const double* value, const QvTables& o) {
  double reach = 0.0, cf = 0.0, chance = 0.0;
  for (int m = m0; m < m1; ++m) {
    const QvMember x = qv_member(rm + static_cast<size_t>(m) * (P + 1), P, p);
    cf += qv_cf_reach_term(x);
    reach += x.reach;
    chance += x.chance;
  }
  o.reach[i] = reach;
  o.cf_reach[i] = cf;
  o.chance_reach[i] = chance;
  // the reference assigns ("=", action_value.py:132) at every member: the LAST member's own reach stays.  The members agree
  // under perfect recall; leduc_poker(action_mapping=True) reaches an infostate by fold and by call, and they do not.
  o.player_reach[i] = m1 > m0 ? rm[static_cast<size_t>(m1 - 1) * (P + 1) + p] : 0.0;
  for (int a = 0; a < A; ++a) {
    double cfq = 0.0, own = 0.0;
    for (int q = 0; q < P; ++q) {
      double w = 0.0;
      if (a < n)
        for (int m = m0; m < m1; ++m) {
          const QvMember x = qv_member(rm + static_cast<size_t>(m) * (P + 1), P, p);
          const double v = value[static_cast<size_t>(first_child[mem[m]] + a) * P + q];
          w += qv_weighted_term(v, x);
          if (q == p) cfq += qv_cf_value_term(v, x);
        }
      o.weighted[(static_cast<size_t>(i) * A + a) * P + q] = w;
      if (q == p) own = w;
    }
    o.q[static_cast<size_t>(i) * A + a] = a < n ? qv_action_value(own, reach) : 0.0;
    o.cf_q[static_cast<size_t>(i) * A + a] = cfq;
  }
}

}  // namespace osg

#endif  // OSG_ACTION_VALUES_H_
