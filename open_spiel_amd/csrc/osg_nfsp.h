// Neural Fictitious Self-Play arithmetic (open_spiel/python/pytorch/nfsp.py with dqn.py inside it, driven by the loop of
// examples/kuhn_nfsp.py): one self-play episode against an [I, A] table of Q-network outputs and an [I, A] table of
// average-policy probabilities that are frozen for the call, the DQN transitions and supervised rows it appends, the
// row bound of an episode and the ring rule.  Host + device: the kernels of osg_nfsp.hip run these functions, and so
// does tests/native/nfsp_host_test.cpp on the CPU against the NumPy restatement in tests/nfsp_cases.py.
//
//   stream: episode g (a global index) owns Rng(seed, g, 0).  Its draws, in order:
//     modes (_sample_episode_policy, nfsp.py:241-245): P uniforms in player order, player p plays BEST_RESPONSE for the
//       whole episode iff u < anticipatory[p], else AVERAGE_POLICY;
//     then the walk from the root.  Chance node (rl_environment.ChanceEventSampler): one uniform, NumPy's choice(p=) rule
//       over the outcome probabilities (dcfr_choice).
//     BEST_RESPONSE decision (_act_epsilon_greedy, dqn.py:468-499): u = unit(); u < eps[p]: the action is
//       legal[below(n)] on the next draw and probs[legal] = (1 / n) / sum(probs); else the legal id with the largest Q,
//       the first one on a tie, probs one-hot.  The supervised row (infostate, float32(probs) [A]) goes to player p's
//       reservoir (NFSP.add_transition, nfsp.py:330-362).
//     AVERAGE_POLICY decision (_act, nfsp.py:247-259): one uniform, choice(p=) over all A ids with p the double of the
//       float32 row of the average-policy table (zero at illegal ids).  No supervised row.
//   transitions (DQN.add_transition, dqn.py:427-466): in both modes every own decision after the first, and the terminal,
//     closes one for that player: (info, action, reward f32 — 0 before the end, float32(return) at it —, next_info, -1 at
//     the end, final).  A player who never acted gets none.
//   counters: NFSP._iteration of player p grows by its decisions + 1 per episode (every agent steps on the last time
//     step), DQN._iteration by the same in its BEST_RESPONSE episodes only.
//   ring (dqn.ReplayBuffer): the row with entry index n goes to slot n % capacity; of m rows appended in one call, row r
//     stays iff r + capacity >= m (no later row of the call has its slot).  sample: the m smallest keys
//     Rng(seed, slot, stream).next() over the filled slots, as the reservoir's sample rule.
//
// Nothing here may be contracted into a fused multiply-add (-ffp-contract=off, library and host test alike).
#ifndef OSG_NFSP_H_
#define OSG_NFSP_H_

#include "osg_deep_cfr.h"

namespace osg {

constexpr int kNfspMaxA = kDcfrMaxA;
constexpr int kNfspMaxP = 8;   // served: kuhn_poker with 2 to 5 players, leduc_poker with 2 or 3

struct NfspParams { double eps[kNfspMaxP]; double anticipatory[kNfspMaxP]; };

// ---- decisions ----------------------------------------------------------------------------------------------------------
// q [NA] by action id, legal [n] ascending ids: the index into legal of the greedy action (torch.argmax: the first
// maximum).
OSG_HD int nfsp_greedy(const float* q, const int32_t* legal, int n) {
  int best = 0;
  for (int k = 1; k < n; ++k)
    if (q[legal[k]] > q[legal[best]]) best = k;
  return best;
}
// probs [NA] of the supervised row: uniform over the legal ids (pick < 0) or one-hot at legal[pick]; probs / probs.sum()
// in fp64, then float32.
OSG_HD void nfsp_probs_row(const int32_t* legal, int n, int NA, int pick, float* row) {
  double p[kNfspMaxA];
  for (int a = 0; a < NA; ++a) p[a] = 0.0;
  if (pick < 0) {
    for (int k = 0; k < n; ++k) p[legal[k]] = 1.0 / static_cast<double>(n);
  } else {
    p[legal[pick]] = 1.0;
  }
  double sum = 0.0;
  for (int a = 0; a < NA; ++a) sum = sum + p[a];
  for (int a = 0; a < NA; ++a) row[a] = static_cast<float>(p[a] / sum);
}

// ---- one episode ----------------------------------------------------------------------------------------------------------
// What an episode reports besides its rows: bit p of modes is set iff player p played BEST_RESPONSE; nibble p of
// transitions / supervised is the number of rows player p got (a player's transitions are its decisions).
constexpr int kNfspMaxRows = 15;
struct NfspEpisode { int32_t draws; uint32_t modes, transitions, supervised; };
OSG_HD int nfsp_rows_of(uint32_t packed, int p) { return static_cast<int>((packed >> (4 * p)) & 15u); }

// tree: P, A, kind(h) (0 chance, 1 decision, 2 terminal), nchild(h), child(h, c), prob(node) (of the edge into a chance
//   node's child), info(h), actor(h), ret(h, p).  legal [I, A] action ids, -1 padded; q and avg [I, A] float32.
// sink: a transition is opened at the decision it starts from, open(p, n, info, action), and closed at the player's next
//   decision or at the end, close(p, n, reward, next_info, final): n is its position among the player's transitions of
//   the episode, the order in which the reference's loop appends them (no per-player state is carried in between: the
//   open row is the state).  supervised(p, n, info, row [A]) likewise.  A sink refuses n at or beyond its bound; the
//   counts keep growing (to at most kNfspMaxRows, which the host checks against the tree beforehand).
template <class TreeView, class Sink>
OSG_HD NfspEpisode nfsp_episode(const TreeView& t, const int32_t* legal, const float* q, const float* avg, const NfspParams& prm,
                                uint64_t seed, uint64_t g, Sink& sink) {
  const int P = t.P, A = t.A;
  Rng rng(seed, g, 0);
  NfspEpisode ep{0, 0u, 0u, 0u};
  for (int p = 0; p < P; ++p) {
    const double u = rng.unit();
    ++ep.draws;
    if (u < prm.anticipatory[p]) ep.modes |= 1u << p;
  }
  int node = 0;
  for (;;) {
    const int k = t.kind(node);
    if (k == 2) break;
    const int nc = t.nchild(node);
    if (k == 0) {
      const double u = rng.unit();
      ++ep.draws;
      node = t.child(node, dcfr_choice(nc, u, [&](int c) { return t.prob(t.child(node, c)); }));
      continue;
    }
    const int p = t.actor(node), i = t.info(node);
    int32_t ids[kNfspMaxA];
    for (int a = 0; a < A; ++a) ids[a] = legal[i * A + a];
    const int n = nfsp_rows_of(ep.transitions, p);
    if (n > 0) sink.close(p, n - 1, 0.0f, i, 0);
    int pick;
    if ((ep.modes >> p) & 1u) {
      const double u = rng.unit();
      ++ep.draws;
      float row[kNfspMaxA];
      if (u < prm.eps[p]) {
        pick = static_cast<int>(rng.below(static_cast<uint32_t>(nc)));
        ++ep.draws;
        nfsp_probs_row(ids, nc, A, -1, row);
      } else {
        float qs[kNfspMaxA];
        for (int a = 0; a < A; ++a) qs[a] = q[i * A + a];
        pick = nfsp_greedy(qs, ids, nc);
        nfsp_probs_row(ids, nc, A, pick, row);
      }
      sink.supervised(p, nfsp_rows_of(ep.supervised, p), i, row);
      if (nfsp_rows_of(ep.supervised, p) < kNfspMaxRows) ep.supervised += 1u << (4 * p);
    } else {
      const double u = rng.unit();
      ++ep.draws;
      const int id = dcfr_choice(A, u, [&](int a) { return static_cast<double>(avg[i * A + a]); });
      pick = 0;
      for (int c = 0; c < nc; ++c)
        if (ids[c] == id) pick = c;
    }
    sink.open(p, n, i, ids[pick]);
    if (n < kNfspMaxRows) ep.transitions += 1u << (4 * p);
    node = t.child(node, pick);
  }
  for (int p = 0; p < P; ++p) {
    const int n = nfsp_rows_of(ep.transitions, p);
    if (n > 0) sink.close(p, n - 1, static_cast<float>(t.ret(node, p)), -1, 1);
  }
  return ep;
}

// ---- rows of one episode (host) -------------------------------------------------------------------------------------------
// The most decisions `player` takes on one path: an episode appends at most that many transitions and that many
// supervised rows for the player.  Children are numbered above their parent; work [H].
template <class Kind, class Count, class Actor, class Child>
inline int64_t nfsp_row_bound(int H, const Kind* kind, const Count* nchild, const Actor* actor, int player, Child child, int64_t* work) {
  for (int h = H - 1; h >= 0; --h) {
    int64_t deepest = 0;
    if (kind[h] != 2)
      for (int k = 0; k < static_cast<int>(nchild[h]); ++k)
        if (work[child(h, k)] > deepest) deepest = work[child(h, k)];
    work[h] = deepest + (kind[h] == 1 && actor[h] == player ? 1 : 0);
  }
  return work[0];
}

// ---- ring -----------------------------------------------------------------------------------------------------------------
OSG_HD int64_t nfsp_ring_slot(int64_t entry_index, int64_t capacity) { return entry_index % capacity; }
// Row r of the m rows of one append call is still there after the call.
OSG_HD bool nfsp_ring_row_stays(int64_t r, int64_t m, int64_t capacity) { return r + capacity >= m; }

}  // namespace osg

#endif  // OSG_NFSP_H_
