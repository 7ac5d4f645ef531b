// AlphaZero self-play arithmetic (open_spiel/algorithms/alpha_zero_torch/alpha_zero.cc PlayGame, python/algorithms/
// alpha_zero/alpha_zero.py _play_game, algorithms/mcts.cc dirichlet_noise): the policy target of a search, the move drawn
// from it, Dirichlet noise for a root's prior and the slots of a circular replay buffer.  Host + device: the kernels of
// osg_selfplay.hip run these functions, and so does tests/native/selfplay_host_test.cpp on the CPU against the NumPy
// restatement in tests/selfplay_cases.py.
//
//   policy target (alpha_zero.cc:127-134, alpha_zero.py:234-239): w[a] = visits[a] ^ (1 / temperature) for the root's
//     children, 0 elsewhere; S = sum_a w[a] from 0.0, a ascending; p[a] = w[a] / S.  temperature == 1 takes no pow:
//     w[a] = visits[a] exactly, S is an integer below 2^53 and exact in any order, p[a] = visits[a] / S.
//   move (alpha_zero.cc:135-139): with fewer than temperature_drop moves played in this game the action is drawn from p by
//     SampleAction's rule (spiel.cc:372-409, sample_action_w in osg_sample.h): z = rng.unit(), the first a in ascending
//     order with acc <= z < acc + p[a], acc accumulated in fp64; the last a with p[a] > 0 otherwise.  From
//     temperature_drop on no draw is made and the action is the search's best_action.
//   Dirichlet noise (mcts.cc:188-203, 284-292): one Gamma(alpha, 1) draw per legal action in ascending order, normalised
//     by their (compensated) sum; prior[a] = (1 - eps) * prior[a] + eps * noise[a].  Gamma: Marsaglia-Tsang for
//     alpha >= 1, gamma(alpha + 1) * u ^ (1 / alpha) below; normals by Box-Muller over rng.unit(); a unit draw of 0 that
//     would reach a logarithm is replaced by 2^-53.
//   ring (replay_buffer.py append, sequential over the finished games in ascending environment order, each in ply order):
//     row t of finished environment i goes to slot (total_seen + prefix[i] + t) % capacity, prefix = exclusive sum of the
//     finished lengths; of a flush of more than `capacity` rows only the last `capacity` are written.
//
// Nothing here may be contracted into a fused multiply-add (-ffp-contract=off, library and host test alike).
#ifndef OSG_SELFPLAY_H_
#define OSG_SELFPLAY_H_

#include <math.h>

#include "osg_common.h"

namespace osg {

// The logarithm of the gamma draws as a type: the host test hands in one that is a last bit off, to show what such a
// difference between two math libraries can flip.
struct SpLog {
  OSG_HD static double of(double x) { return log(x); }
};

constexpr int kSpGammaTries = 64;   // Marsaglia-Tsang accepts > 95 % of its proposals: 64 rejections in a row do not happen

// ---- policy target and move -------------------------------------------------------------------------------------------
OSG_HD double sp_weight(int32_t visits, double inv_t, bool unit_t) {
  if (visits <= 0) return 0.0;
  const double v = static_cast<double>(visits);
  return unit_t ? v : pow(v, inv_t);
}
OSG_HD double sp_policy_sum(const int32_t* visits, int A, double inv_t, bool unit_t) {
  double sum = 0.0;
  for (int a = 0; a < A; ++a) sum = sum + sp_weight(visits[a], inv_t, unit_t);
  return sum;
}
// p[a] for every a (handed to emit(a, p)) and, with `draw`, the action SampleAction's rule picks for z; -1 without.
template <class Emit>
OSG_HD int sp_policy_and_draw(const int32_t* visits, int A, double inv_t, bool unit_t, double sum, bool draw, double z,
                              Emit emit) {
  double acc = 0.0;
  int chosen = -1, last = -1;
  for (int a = 0; a < A; ++a) {
    const double p = sp_weight(visits[a], inv_t, unit_t) / sum;
    emit(a, p);
    if (!draw || p <= 0.0) continue;
    if (chosen < 0 && acc <= z && z < acc + p) chosen = a;
    acc = acc + p;
    last = a;
  }
  if (!draw) return -1;
  return chosen >= 0 ? chosen : last;
}
// The policy target as an array (temperature finite and > 0; a row whose visits sum to 0 has none: returns false).
OSG_HD bool policy_from_visits(const int32_t* visits, int A, double temperature, double* p) {
  const bool unit_t = temperature == 1.0;
  const double inv_t = 1.0 / temperature;
  const double sum = sp_policy_sum(visits, A, inv_t, unit_t);
  if (!(sum > 0.0)) return false;
  sp_policy_and_draw(visits, A, inv_t, unit_t, sum, false, 0.0, [&](int a, double x) { p[a] = x; });
  return true;
}
// The move of one environment: stream Rng(seed, index_offset + env, ply_counter); greedy rows consume no draw.
OSG_HD int draw_action(const int32_t* visits, int A, double temperature, bool greedy, int best_action, uint64_t seed,
                       uint64_t stream, uint64_t ply_counter) {
  if (greedy) return best_action;
  const bool unit_t = temperature == 1.0;
  const double inv_t = 1.0 / temperature;
  const double sum = sp_policy_sum(visits, A, inv_t, unit_t);
  Rng rng(seed, stream, ply_counter);
  return sp_policy_and_draw(visits, A, inv_t, unit_t, sum, true, rng.unit(), [](int, double) {});
}

// ---- Dirichlet noise ------------------------------------------------------------------------------------------------------
OSG_HD double sp_unit_open(Rng& rng) {
  const double u = rng.unit();
  return u > 0.0 ? u : 1.0 / 9007199254740992.0;
}
template <class L = SpLog>
OSG_HD double sp_normal(Rng& rng) {   // Box-Muller, the cosine branch
  const double u1 = sp_unit_open(rng);
  const double u2 = rng.unit();
  return sqrt(-2.0 * L::of(u1)) * cos(6.283185307179586476925 * u2);
}
template <bool kBoost = true, class L = SpLog>
OSG_HD double gamma_draw_t(double alpha, Rng& rng) {
  const bool boost = alpha < 1.0;
  const double a = boost ? alpha + 1.0 : alpha;
  const double d = a - 1.0 / 3.0;
  const double c = 1.0 / sqrt(9.0 * d);
  double g = d;
  for (int tries = 0; tries < kSpGammaTries; ++tries) {
    const double x = sp_normal<L>(rng);
    double v = 1.0 + c * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    const double u = sp_unit_open(rng);
    const double x2 = x * x;
    if (u < 1.0 - 0.0331 * x2 * x2 || L::of(u) < 0.5 * x2 + d * (1.0 - v + L::of(v))) {
      g = d * v;
      break;
    }
  }
  if (boost && kBoost) g = g * pow(sp_unit_open(rng), 1.0 / alpha);
  return g;
}
OSG_HD double gamma_draw(double alpha, Rng& rng) { return gamma_draw_t<true>(alpha, rng); }

OSG_HD bool sp_mask_bit(const uint32_t* mask, int a) { return (mask[a >> 5] >> (a & 31)) & 1u; }

// One root: `prior` [A] mixed in place at the legal actions (bit a of mask), the draws kept in noise[k * stride] for the
// k-th legal action.  kBoost = false leaves the alpha < 1 step out (the defect the statistical test must reject).
template <bool kBoost = true, class L = SpLog>
OSG_HD void dirichlet_row_t(double* prior, const uint32_t* mask, int A, double alpha, double epsilon, Rng& rng,
                            double* noise, int64_t stride) {
  double sum = 0.0, comp = 0.0;   // Kahan: the noise sums to 1 within an ulp whatever the number of actions
  int count = 0;
  for (int a = 0; a < A; ++a) {
    if (!sp_mask_bit(mask, a)) continue;
    const double g = gamma_draw_t<kBoost, L>(alpha, rng);
    noise[count * stride] = g;
    const double y = g - comp;
    const double t = sum + y;
    comp = (t - sum) - y;
    sum = t;
    ++count;
  }
  int k = 0;
  for (int a = 0; a < A; ++a) {
    if (!sp_mask_bit(mask, a)) continue;
    const double nz = sum > 0.0 ? noise[k * stride] / sum : 1.0 / static_cast<double>(count);
    prior[a] = (1.0 - epsilon) * prior[a] + epsilon * nz;
    ++k;
  }
}
OSG_HD void dirichlet_row(double* prior, const uint32_t* mask, int A, double alpha, double epsilon, Rng& rng, double* noise,
                          int64_t stride) {
  dirichlet_row_t<true>(prior, mask, A, alpha, epsilon, rng, noise, stride);
}

// ---- ring ---------------------------------------------------------------------------------------------------------------
// Row g (0-based, in append order) of a flush of `rows` rows into a ring that has seen total_seen rows before it.
OSG_HD bool ring_written(int64_t rows, int64_t g, int64_t capacity) { return g >= rows - capacity; }
OSG_HD int64_t ring_slot(int64_t total_seen, int64_t g, int64_t capacity) { return (total_seen + g) % capacity; }
OSG_HD int64_t ring_size(int64_t total_seen, int64_t capacity) { return total_seen < capacity ? total_seen : capacity; }

// ---- end of a game ------------------------------------------------------------------------------------------------------
// |root_value| > cutoff_value ends the game with returns +-root_value for the mover (alpha_zero.cc:154-158): player 0's.
OSG_HD bool sp_cut_off(double root_value, double cutoff_value) { return fabs(root_value) > cutoff_value; }
OSG_HD double sp_cutoff_return0(double root_value, int mover) { return mover == 0 ? root_value : -root_value; }

}  // namespace osg

#endif  // OSG_SELFPLAY_H_
