// Magnetic mirror descent over the sequence form with dilated entropy (Sokota et al. 2023, arXiv 2206.05825;
// MMDDilatedEnt in open_spiel/python/algorithms/mmd_dilated.py:132-176, 232-323, 325-366, with
// sequence_form_utils.py:120-228, 325-389): the arithmetic of ONE cell, ONE row and ONE infostate, host + device.  The
// kernels of osg_cfr_mmd.hip run exactly these functions, and so does tests/native/mmd_host_test.cpp on the CPU against
// the trajectories the reference's own file left in tests/golden/mmd_vectors.npz.
//
// Two players, zero-sum.  Player p's sequence (I, a) is the cell I * A + a of an [I, A] table; its value is
// x(I, a) = x(parent I) * pi(I, a) (sequence_form_utils.py:382-383), x of the empty sequence 1.  One update_sequences()
// (mmd_dilated.py:261-281) at stepsize eta and regularisation alpha:
//   psi(I, a)  = (log(x(I, a) / x(parent I)) + 1) - c(I, a)   where x(parent I) > 0, else 0            (:246-258)
//   loss(I, a) = sum over the terminals z whose last p-sequence is (I, a) of -(chance(z) u_p(z)) * x_opp(z)   (:267-270)
//   g(I, a)    = (eta * loss - psi) / (1 + eta * alpha)                                                 (:266-271)
//   deepest infostates first: g(I, a) += dot(g(K, .), pi'(K, .)); g(I, a) += neg_entropy(pi'(K, .)) for every child
//   infostate K of (I, a); then pi'(I, .) = softmax(-g(I, .))                                            (:283-323)
//   x from pi'; k += 1; avg_x = (avg_x * (k - 1) + x) / k                                               (:278-281, 361-366)
// The reference sums its payoff products through BLAS in no fixed order; here every sum has one order (a cell's
// terminals in history-index order, a cell's child infostates in infostate-index order, a row left to right), so two
// runs and any two kernel forms give the same bits.  Nothing here may be contracted into a fused multiply-add: the
// library and the host test are compiled with -ffp-contract=off.
#ifndef OSG_MMD_H_
#define OSG_MMD_H_

#include <math.h>

#include "osg_common.h"

namespace osg {

constexpr int kMmdMaxRow = 8;   // widest policy row one lane holds (kuhn 2, leduc 3)

// What an iteration reads of the tree, built once per solver (device pointers in the kernels, host ones in the test).
struct MmdTree {
  int I, A, L;                // infostates, table width, infostate levels
  const int32_t* nact;        // [I]
  const int32_t* lvl_off;     // [L + 1] the infostates of a level: lvl_info[lvl_off[l] ...), DEEPEST level first
  const int32_t* lvl_info;    // [I]
  const int32_t* own_off;     // [I + 1] the cells of the owner's earlier decisions on the way to I, root to leaf; the last
  const int32_t* own;         //         one is parent(I)
  const int32_t* child_off;   // [I * A + 1] the owner's infostates whose parent is the cell, ascending
  const int32_t* child;
  const int32_t* term_off;    // [I * A + 3] the terminals whose last own sequence is the cell, ascending history index;
  const int32_t* term_opp;    //   the opponent's last sequence on the way (a cell, -1 = none), and
  const double* term_cu;      //   chance(z) * u_owner(z).  Buckets I * A and I * A + 1: the terminals before which
                              //   player 0 / player 1 never acted (they enter the bilinear value of the gap only)
};

// x(parent I): the product of the owner's probabilities root to leaf, started at 1 (sequence_form_utils.py:345,382-386).
OSG_HD double mmd_parent_seq(const MmdTree& t, int i, const double* pol) {
  double r = 1.0;
  for (int e = t.own_off[i]; e < t.own_off[i + 1]; ++e) r = r * pol[t.own[e]];
  return r;
}

// mmd_dilated.py:246-258
OSG_HD double mmd_psi(double x, double x_parent, int children) {
  if (!(x_parent > 0)) return 0.0;
  return (log(x / x_parent) + 1.0) - static_cast<double>(children);
}

// One cell of payoff_mat @ sequences[opponent] (mmd_dilated.py:164,267,269): x = the [I, A] table of sequence values.
OSG_HD double mmd_loss(const MmdTree& t, int bucket, const double* x) {
  double sum = 0.0;
  for (int e = t.term_off[bucket]; e < t.term_off[bucket + 1]; ++e) {
    const int o = t.term_opp[e];
    sum = sum + (-t.term_cu[e]) * (o < 0 ? 1.0 : x[o]);
  }
  return sum;
}

OSG_HD double mmd_grad(double loss, double psi, double eta, double alpha) { return (eta * loss - psi) / (1.0 + eta * alpha); }

// neg_entropy (mmd_dilated.py:42-43) = -scipy.stats.entropy(p): p is divided by its sum first, a zero cell counts 0.
OSG_HD double mmd_neg_entropy(const double* p, int n) {
  double sum = 0.0;
  for (int a = 0; a < n; ++a) sum = sum + p[a];
  double s = 0.0;
  for (int a = 0; a < n; ++a) {
    const double q = p[a] / sum;
    s = s + (q > 0 ? -(q * log(q)) : 0.0);
  }
  return -s;
}

// softmax(-g) (mmd_dilated.py:46-48,321) into pi[0, n); *dot = dot(g, pi), *neg_ent = neg_entropy(pi) (:311-312).
OSG_HD void mmd_row(const double* g, int n, double* pi, double* dot, double* neg_ent) {
  double top = -g[0];
  for (int a = 1; a < n; ++a) top = -g[a] > top ? -g[a] : top;
  double e[kMmdMaxRow];
  double sum = 0.0;
  for (int a = 0; a < n; ++a) {
    e[a] = exp(-g[a] - top);
    sum = sum + e[a];
  }
  double d = 0.0;
  for (int a = 0; a < n; ++a) {
    pi[a] = e[a] / sum;
    d = d + g[a] * pi[a];
  }
  *dot = d;
  *neg_ent = mmd_neg_entropy(pi, n);
}

// Steps 1-4 for infostate i by one lane, once every deeper infostate has its dot[] and neg_ent[]: reads the OLD sequence
// values x, writes the new row pi[i, .], dot[i] and neg_ent[i].  regularised_br: the sweep of get_gap()
// (mmd_dilated.py:334-341): g = loss / alpha, no psi.
OSG_HD void mmd_infostate(const MmdTree& t, int i, const double* x, double eta, double alpha, bool regularised_br, double* pi,
                          double* dot, double* neg_ent) {
  const int n = t.nact[i];
  const int pb = t.own_off[i], pe = t.own_off[i + 1];
  const double x_parent = pe > pb ? x[t.own[pe - 1]] : 1.0;
  double g[kMmdMaxRow];
  for (int a = 0; a < n; ++a) {
    const int cell = i * t.A + a;
    const double loss = mmd_loss(t, cell, x);
    double v = regularised_br ? loss / alpha
                              : mmd_grad(loss, mmd_psi(x[cell], x_parent, t.child_off[cell + 1] - t.child_off[cell]), eta, alpha);
    for (int c = t.child_off[cell]; c < t.child_off[cell + 1]; ++c) {
      v = v + dot[t.child[c]];
      v = v + neg_ent[t.child[c]];
    }
    g[a] = v;
  }
  mmd_row(g, n, pi + i * t.A, dot + i, neg_ent + i);
}

// policy_to_sequence for the row of infostate i (sequence_form_utils.py:382-383): x[i, .] from the finished table pi.
OSG_HD void mmd_sequence_row(const MmdTree& t, int i, const double* pi, double* x) {
  const double x_parent = mmd_parent_seq(t, i, pi);
  for (int a = 0; a < t.nact[i]; ++a) x[i * t.A + a] = x_parent * pi[i * t.A + a];
}

// update_avg_sequences (mmd_dilated.py:361-366) for one cell; k = iteration_count after its increment.
OSG_HD double mmd_average(double avg, double x, double k) { return (avg * (k - 1.0) + x) / k; }

// dgf_eval's term of infostate i (mmd_dilated.py:224-228): parent_seq * neg_entropy(children_seq / parent_seq).
OSG_HD double mmd_dgf_term(const MmdTree& t, int i, const double* x) {
  const int pb = t.own_off[i], pe = t.own_off[i + 1];
  const double x_parent = pe > pb ? x[t.own[pe - 1]] : 1.0;
  if (!(x_parent > 0)) return 0.0;
  double q[kMmdMaxRow];
  for (int a = 0; a < t.nact[i]; ++a) q[a] = x[i * t.A + a] / x_parent;
  return x_parent * mmd_neg_entropy(q, t.nact[i]);
}

// One cell's share of own^T payoff_mat opp (mmd_dilated.py:355,358): x_own(cell) * (payoff_mat @ x_opp)(cell).  The
// payoff matrix is the minimising player 0's, so the caller passes player 0's cells (and bucket I * A with x_own 1).
OSG_HD double mmd_bilinear_cell(const MmdTree& t, int bucket, double x_own, const double* x_opp) { return x_own * mmd_loss(t, bucket, x_opp); }

// get_gap() from its six pieces (mmd_dilated.py:354-359), in the reference's order.
OSG_HD double mmd_gap(double x_a_ybr, double xbr_a_y, const double d[2], const double d_br[2], double alpha) {
  double gap = 0.0;
  gap = gap + x_a_ybr;
  gap = gap + alpha * (d[1] - d_br[1]);
  gap = gap + alpha * (d[0] - d_br[0]);
  gap = gap + -xbr_a_y;
  return gap;
}

// The default stepsize (mmd_dilated.py:169): alpha / max|payoff_mat| ** 2.
inline double mmd_default_stepsize(double alpha, double max_abs_payoff) { return alpha / (max_abs_payoff * max_abs_payoff); }

}  // namespace osg

#endif  // OSG_MMD_H_
