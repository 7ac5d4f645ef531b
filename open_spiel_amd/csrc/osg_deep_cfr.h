// Deep CFR arithmetic (open_spiel/python/pytorch/deep_cfr.py): the strategy of an infostate from its advantage-network
// outputs, the opponent / chance draw, the traverser's sampled advantages, the reservoir rule and the row bounds of a
// trajectory.  Host + device: the kernels of osg_deep_cfr.hip run these functions, and so does
// tests/native/deep_cfr_host_test.cpp on the CPU against the NumPy restatement in tests/deep_cfr_cases.py.
//
//   strategy (_sample_action_from_advantage, deep_cfr.py:484-512): raw float32 outputs by action id, legal ids
//     ascending.  The reference's dtypes follow the values (`max(0., x)` keeps the float32 scalar when x > 0 and gives a
//     Python float otherwise; np.sum of a list of float32 scalars adds in float32, of a mixed list in float64):
//       every legal output > 0:   S = float32 sum in legal order; p[a] = double(float32(adv[a] / S))
//       some legal output > 0:    S = fp64 sum of the clipped values in legal order; p[a] = double(clip(adv[a])) / S
//       none:                     p = 1 at the legal id with the largest raw output, the first one on a tie
//     illegal ids are 0.
//   draw (:466-468, :432-433; NumPy's RandomState.choice(p=)): cdf_k = the sequential fp64 running sum, cdf_k /= cdf_last,
//     the pick is the number of k with cdf_k <= u.  At an opponent node p is first renormalised, p / sum(p), over all ids.
//   traverser node (:436-461): cfv = sum_a p[a] * payoff[a] in fp64, legal order, from 0; row[a] = float32(payoff[a] - cfv).
//   reservoir (ReservoirBuffer.append, :150-182): the row with add index n goes to slot n while n < capacity, else to
//     idx = mulhi64(Rng(seed, n, stream).next(), n + 1) when idx < capacity, else nowhere.
//   sample: `m` distinct filled slots = the m smallest of the keys Rng(seed, slot, stream).next(), ascending by
//     (key, slot) — a uniformly random m-subset in uniformly random order.
//
// Nothing here may be contracted into a fused multiply-add (-ffp-contract=off, library and host test alike).
#ifndef OSG_DEEP_CFR_H_
#define OSG_DEEP_CFR_H_

#include "osg_common.h"

namespace osg {

constexpr int kDcfrMaxA = 4;   // the widest row served (osg_cfr_impl::kMaxA: kuhn 2, leduc 3)

// ---- strategy from advantages -------------------------------------------------------------------------------------------
// adv [NA] by action id, legal [n] ascending ids (each < NA), p [NA] out.  Returns the branch taken: 0 every legal
// output positive, 1 some, 2 none.
OSG_HD int dcfr_strategy(const float* adv, const int32_t* legal, int n, int NA, double* p) {
  for (int a = 0; a < NA; ++a) p[a] = 0.0;
  bool all_pos = true, any_pos = false;
  for (int k = 0; k < n; ++k) {
    if (adv[legal[k]] > 0.0f) any_pos = true;
    else all_pos = false;
  }
  if (!any_pos) {
    int best = legal[0];
    for (int k = 1; k < n; ++k)
      if (adv[legal[k]] > adv[best]) best = legal[k];
    p[best] = 1.0;
    return 2;
  }
  if (all_pos) {
    float sum = 0.0f;
    for (int k = 0; k < n; ++k) sum = sum + adv[legal[k]];
    for (int k = 0; k < n; ++k) {
      const float q = adv[legal[k]] / sum;
      p[legal[k]] = static_cast<double>(q);
    }
    return 0;
  }
  double sum = 0.0;
  for (int k = 0; k < n; ++k) {
    const float x = adv[legal[k]];
    sum = sum + (x > 0.0f ? static_cast<double>(x) : 0.0);
  }
  for (int k = 0; k < n; ++k) {
    const float x = adv[legal[k]];
    p[legal[k]] = (x > 0.0f ? static_cast<double>(x) : 0.0) / sum;
  }
  return 1;
}

// ---- draws ----------------------------------------------------------------------------------------------------------------
// RandomState.choice(n, p=p) for the uniform u in [0, 1): p is read through at(k).
template <class At>
OSG_HD int dcfr_choice(int n, double u, At at) {
  double last = 0.0;
  for (int k = 0; k < n; ++k) last = last + at(k);
  double acc = 0.0;
  int pick = 0;
  for (int k = 0; k < n; ++k) {
    acc = acc + at(k);
    if (acc / last <= u) ++pick;
  }
  return pick < n ? pick : n - 1;
}
// The opponent's action id: probs = p / p.sum() over all NA ids, then choice.
OSG_HD int dcfr_opponent_draw(const double* p, int NA, double u) {
  double sum = 0.0;
  for (int a = 0; a < NA; ++a) sum = sum + p[a];
  return dcfr_choice(NA, u, [&](int a) { return p[a] / sum; });
}

// ---- traverser node -------------------------------------------------------------------------------------------------------
// payoff [n] by legal index; row [NA] by action id; returns cfv.
OSG_HD double dcfr_advantage_row(const double* p, const double* payoff, const int32_t* legal, int n, int NA, float* row) {
  double cfv = 0.0;
  for (int k = 0; k < n; ++k) cfv = cfv + p[legal[k]] * payoff[k];
  for (int a = 0; a < NA; ++a) row[a] = 0.0f;
  for (int k = 0; k < n; ++k) row[legal[k]] = static_cast<float>(payoff[k] - cfv);
  return cfv;
}

// ---- reservoir ------------------------------------------------------------------------------------------------------------
OSG_HD uint64_t dcfr_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * static_cast<unsigned __int128>(b)) >> 64);
#endif
}
// The slot of the row with add index n (0-based), -1: dropped.
OSG_HD int64_t dcfr_reservoir_slot(uint64_t seed, uint64_t stream, int64_t n, int64_t capacity) {
  if (n < capacity) return n;
  Rng rng(seed, static_cast<uint64_t>(n), stream);
  const uint64_t idx = dcfr_mulhi64(rng.next(), static_cast<uint64_t>(n) + 1u);
  return idx < static_cast<uint64_t>(capacity) ? static_cast<int64_t>(idx) : -1;
}
OSG_HD uint64_t dcfr_sample_key(uint64_t seed, uint64_t stream, int64_t slot) {
  Rng rng(seed, static_cast<uint64_t>(slot), stream);
  return rng.next();
}

// ---- rows and frames of one trajectory (host) -----------------------------------------------------------------------------
// Children are numbered above their parent (level order and depth-first order both do), so one descending pass folds
// every subtree; child(h, c) names child c of h.  kind: 0 chance, 1 decision, 2 terminal.  adv: at the traverser's node
// 1 + sum over the children, else the max; strat: at an opponent's node 1 + max, at the traverser's the sum, at a chance
// node the max; frames: traverser nodes on one path.
struct DcfrBounds { int64_t adv, strat, frames; };
template <class Kind, class Count, class Actor, class Child>
inline DcfrBounds dcfr_row_bounds(int H, const Kind* kind, const Count* nchild, const Actor* actor, int player, Child child,
                                  int64_t* work /* [3 H] */) {
  int64_t* adv = work; int64_t* strat = work + H; int64_t* frames = work + 2 * static_cast<int64_t>(H);
  for (int h = H - 1; h >= 0; --h) {
    int64_t a_sum = 0, a_max = 0, s_sum = 0, s_max = 0, f_max = 0;
    if (kind[h] != 2)
      for (int k = 0; k < static_cast<int>(nchild[h]); ++k) {
        const int c = child(h, k);
        a_sum += adv[c]; s_sum += strat[c];
        if (adv[c] > a_max) a_max = adv[c];
        if (strat[c] > s_max) s_max = strat[c];
        if (frames[c] > f_max) f_max = frames[c];
      }
    const bool own = kind[h] == 1 && actor[h] == player, opp = kind[h] == 1 && !own;
    adv[h] = own ? 1 + a_sum : a_max;
    strat[h] = own ? s_sum : (opp ? 1 + s_max : s_max);
    frames[h] = own ? 1 + f_max : f_max;
  }
  return DcfrBounds{adv[0], strat[0], frames[0]};
}

}  // namespace osg

#endif  // OSG_DEEP_CFR_H_
