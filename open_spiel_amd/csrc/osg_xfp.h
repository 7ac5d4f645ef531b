// Extensive-form fictitious play (Heinrich, Lanctot and Silver 2015, Algorithm 1; XFPSolver in
// open_spiel/python/algorithms/fictitious_play.py:115-240): the arithmetic of update_average_policies for ONE
// infostate, host + device.  The kernels of osg_cfr_xfp.hip run exactly these functions, and so does
// tests/native/xfp_host_test.cpp on the CPU against the trajectories the reference's own file left in
// tests/golden/xfp_vectors.npz.
//
// At infostate I of player p the reference holds (fictitious_play.py:196-240)
//   avg_reach   the product of the average policy's probabilities of p's own actions on the way to I,
//   br_reach    the same product under p's best response (every factor 1.0 or 0.0),
// both started at 1.0 and multiplied root to leaf (:220-223), taken at the first history of I it visits, and with
// alpha = 1 / (iterations + 1) sets, for every legal action a (:232-236),
//   new[a] = avg[a] + (alpha * br_reach * (br[a] - avg[a])) / ((1.0 - alpha) * avg_reach + alpha * br_reach)
// evaluated in that order.  Nothing here may be contracted into a fused multiply-add: the library and the host test
// are compiled with -ffp-contract=off.  A row whose denominator is 0 (an uploaded policy with zero probabilities)
// gets the reference's IEEE result, 0 / 0.
//
// A root path is the list of codes the tabular solvers keep per decision history (osg_cfr.hip build_tree), root to
// leaf: slot << 24 | is_chance << 23 | index, where slot is the acting player of the ancestor and index, for a
// decision ancestor, is (its infostate) * A + (the action's index among its legal actions).
#ifndef OSG_XFP_H_
#define OSG_XFP_H_

#include "osg_common.h"

namespace osg {

struct XfpReach { double avg, br; };

// The two reach products of the infostate whose first member history has the root path path[begin, end): the entries
// of `owner` (the infostate's player) only.  pol: [I, A] average policy; best: [I] best-response action index.
OSG_HD XfpReach xfp_reach(const int32_t* path, int begin, int end, int owner, int A, const double* pol, const int32_t* best) {
  XfpReach r{1.0, 1.0};
  for (int e = begin; e < end; ++e) {
    const int code = path[e];
    if (((code >> 23) & 1) || ((code >> 24) & 0xF) != owner) continue;
    const int idx = code & 0x7FFFFF;
    r.avg = r.avg * pol[idx];
    r.br = r.br * (best[idx / A] == idx % A ? 1.0 : 0.0);
  }
  return r;
}

// One cell of the row: avg = the average policy's probability of the action, br = 1.0 at the best-response action.
OSG_HD double xfp_mix(double avg, double br, double alpha, XfpReach r) {
  return avg + (alpha * r.br * (br - avg)) / ((1.0 - alpha) * r.avg + alpha * r.br);
}

// The row of an infostate with n legal actions, in place (every cell reads its own old value only).
OSG_HD void xfp_update_row(double* row, int n, int best, double alpha, XfpReach r) {
  for (int a = 0; a < n; ++a) row[a] = xfp_mix(row[a], a == best ? 1.0 : 0.0, alpha, r);
}

// alpha of the iteration that raises the counter to `iterations` (fictitious_play.py:166,228): Python's int / int.
inline double xfp_alpha(int iterations) { return 1.0 / static_cast<double>(iterations + 1); }

}  // namespace osg

#endif  // OSG_XFP_H_
