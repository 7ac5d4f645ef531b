// The steps of MCTSBot::MCTSearch (mcts.cc:353-467) that the lane-per-root kernels share: k_mcts (osg_mcts.hip: whole
// searches in one launch) and k_mcts_advance / k_mcts_tree_results (osg_mcts_step.hip: trees that persist between
// launches).  Each step is written once, over a per-lane view of the lane's own tree: an object with meta(i), first(i),
// parent(i), count(i), total(i), remap(i) — and prior(i) where kHasPrior — that yield something a field's value can be
// read from and assigned to.  LaneNodes below yields plain references into the pool; k_mcts_advance's view
// (StepNodes, osg_mcts_step.hip) yields NodeRef proxies that pick LDS or the pool by index.
//
// Not here, on purpose: each kernel's descent and UCT / PUCT arg-max (chunked scan with carried headers, LDS shuffle
// stage, fp32 filter in lockstep), k_mcts_advance's lane-parallel expansion, and everything of k_mcts_wave.
#ifndef OSG_MCTS_LANE_H_
#define OSG_MCTS_LANE_H_

#include "osg_mcts_internal.h"

namespace osg {

// NodePool::at for one root with its stride and offset formed once per lane, so the address arithmetic of a node access
// is one multiply-add.
struct LaneSpan {
  int64_t stride, offset;
  OSG_D LaneSpan(const NodePool& pool, int64_t r) : stride(pool.stride()), offset(pool.offset(r)) {}
  OSG_D int64_t at(uint32_t i) const { return static_cast<int64_t>(i) * stride + offset; }
};

// One lane's tree in the pool, as plain references.  (P: a NodePool that says whether it adds a `prior` plane.)
template <class P>
struct LaneNodes {
  static constexpr bool kHasPrior = P::kHasPrior;
  const P& pool;
  LaneSpan span;
  OSG_D LaneNodes(const P& pool_, int64_t r) : pool(pool_), span(pool_, r) {}
  OSG_D uint32_t& meta(uint32_t i) const { return pool.meta[span.at(i)]; }
  OSG_D uint32_t& first(uint32_t i) const { return pool.first[span.at(i)]; }
  OSG_D uint32_t& parent(uint32_t i) const { return pool.parent[span.at(i)]; }
  OSG_D uint32_t& count(uint32_t i) const { return pool.count[span.at(i)]; }
  OSG_D double& total(uint32_t i) const { return pool.total[span.at(i)]; }
  OSG_D uint32_t& remap(uint32_t i) const { return pool.remap[span.at(i)]; }
  OSG_D double& prior(uint32_t i) const { return pool.prior[span.at(i)]; }   // (instantiated only where kHasPrior)
};

// A finished game reached by the descent (mcts.cc:372-376): has-outcome and terminal, and for the win / draw / loss
// games player 0's return as the outcome code.
template <bool kBoard, class N>
OSG_D void mark_terminal_leaf(const N& nodes, uint32_t node, const double* returns) {
  uint32_t meta = nodes.meta(node) | (1u << 20) | (1u << 23);
  if (kBoard) meta = (meta & ~(3u << 21)) | (static_cast<uint32_t>(static_cast<int>(returns[0]) + 1) << 21);
  nodes.meta(node) = meta;
}

// The children of `node` in slots first ... first + c - 1, in the order of the legal actions, then shuffled on the pool
// (mcts.cc:281-299; Fisher-Yates on the tree-policy stream == std::shuffle's role: order only).  prior_of(action) is
// asked where the pool keeps priors.
struct NoPrior { OSG_D double operator()(int) const { return 0.0; } };
template <bool kWide, class N, class LegalMask, class PriorOf = NoPrior>
OSG_D void expand_on_pool(const N& nodes, const LegalMask& legal, int c, int cur, uint32_t node, uint32_t first, Rng& trng,
                          PriorOf prior_of = {}) {
  for (int k = 0; k < c; ++k) {
    const int a = select_action(legal, k);
    nodes.meta(first + k) = mw_make<kWide>(a, cur, 0);
    nodes.first(first + k) = 0; nodes.parent(first + k) = node; nodes.count(first + k) = 0; nodes.total(first + k) = 0.0;
    if constexpr (N::kHasPrior) nodes.prior(first + k) = prior_of(a);
  }
  for (int i = c - 1; i >= 1; --i) {
    const int j = static_cast<int>(trng.below(static_cast<uint32_t>(i + 1)));
    const uint32_t mi = nodes.meta(first + i), mj = nodes.meta(first + j);
    nodes.meta(first + i) = mj;
    nodes.meta(first + j) = mi;
    if constexpr (N::kHasPrior) {
      const double pi = nodes.prior(first + i), pj = nodes.prior(first + j);
      nodes.prior(first + i) = pj;
      nodes.prior(first + j) = pi;
    }
  }
}

// Backup (mcts.cc:383-435) from `node` to the root: every node on the way gains a visit and the return of the player
// who moved into it (a chance node: the nearest decision player above it), and, while `solved`, MCTS-Solver folds the
// children's proven outcomes max^n into the node's.  counted: the visits and returns were already added (k_mcts_advance's
// path lanes); the walk then only solves, and ends where solving does.
template <bool kBoard, bool kWide, class N>
OSG_D void backup_and_solve(const N& nodes, uint32_t node, const double* returns, int num_players, double max_utility,
                            bool solved, bool counted) {
  for (uint32_t v = node; v != kNoNode && !(counted && !solved); v = nodes.parent(v)) {
    uint32_t meta = nodes.meta(v);
    int pl = m_player(meta);
    for (uint32_t up = v; pl == kChancePlayer;) {  // chance node: use the parent decision player
      up = nodes.parent(up);
      if (up == kNoNode) { pl = 0; break; }
      pl = m_player(nodes.meta(up));
    }
    if (!counted) {
      nodes.total(v) += returns[(pl < 0 || pl >= num_players) ? 0 : pl];  // (a terminal root has no player)
      nodes.count(v) += 1;
    }
    if (kBoard && solved && mw_nchild<kWide>(meta) > 0) {  // MCTS-Solver, max^n over proven children
      const uint32_t first = nodes.first(v);
      const int c = mw_nchild<kWide>(meta);
      const int mover = m_player(nodes.meta(first));
      bool all_solved = true, have = false;
      double best = 0.0;
      int best_code = 0;
      for (int k = 0; k < c; ++k) {
        const uint32_t cm = nodes.meta(first + k);
        if (!m_has_outcome(cm)) { all_solved = false; continue; }
        const double val = outcome_value<true>(cm, 1, 0.0, mover);
        if (!have || val > best) { have = true; best = val; best_code = m_code(cm); }
      }
      if (have && (all_solved || best == max_utility)) {
        nodes.meta(v) = (meta & ~(3u << 21)) | (1u << 20) | (static_cast<uint32_t>(best_code) << 21);
      } else {
        solved = false;
      }
    } else if (!kBoard) {
      solved = false;
    }
  }
}

// The early exit of the simulation loop (mcts.cc:437-440): the root is proven or has a single child — or is a
// finished game, where there is nothing to search.
template <bool kWide>
OSG_D bool search_is_over(uint32_t root_meta) {
  return (m_has_outcome(root_meta) && !m_terminal(root_meta)) || mw_nchild<kWide>(root_meta) == 1 || m_terminal(root_meta);
}

// GarbageCollect (mcts.cc:441-482): when nodes_ >= max_nodes_, every node with explore_count < gc_limit_ loses its
// children.  Visit counts never grow from parent to child, so a node survives exactly when its parent's count
// reaches the limit; the survivors are compacted in index order (children blocks stay contiguous, parents stay
// below their children).
template <bool kWide, class N>
OSG_D void garbage_collect(const N& nodes, int gc_nodes, uint32_t& used, int& gc_limit) {
  if (!(gc_nodes > 1 && used >= static_cast<uint32_t>(gc_nodes))) return;
  const uint32_t limit = static_cast<uint32_t>(gc_limit);
  uint32_t w = 1;
  nodes.remap(0) = 0;
  for (uint32_t i = 1; i < used; ++i) {
    const bool alive = nodes.count(nodes.parent(i)) >= limit;
    nodes.remap(i) = alive ? w : kNoNode;
    w += alive ? 1u : 0u;
  }
  for (uint32_t i = 0; i < used; ++i) {
    const uint32_t to = nodes.remap(i);
    if (to == kNoNode) continue;
    uint32_t meta = nodes.meta(i), first = nodes.first(i);
    const uint32_t cnt = nodes.count(i), par = nodes.parent(i);
    const double tot = nodes.total(i);
    [[maybe_unused]] double pri = 0.0;
    if constexpr (N::kHasPrior) pri = nodes.prior(i);
    if (mw_nchild<kWide>(meta) > 0) {
      if (cnt < limit) { meta = mw_clear_children<kWide>(meta); first = 0; }   // children.clear(); the outcome stays
      else first = nodes.remap(first);
    }
    nodes.meta(to) = meta; nodes.first(to) = first; nodes.count(to) = cnt; nodes.total(to) = tot;
    if constexpr (N::kHasPrior) nodes.prior(to) = pri;
    nodes.parent(to) = i == 0 ? kNoNode : nodes.remap(par);
  }
  used = w;
  gc_limit = next_gc_limit(gc_limit, used, gc_nodes);
}

// Results of root r: BestChild by CompareFinal (mcts.cc:114-143), the per-action statistics (child_prior where the pool
// keeps priors) and root_stats = {root visits, nodes in use, proven root outcome or NaN, simulations}.
template <bool kBoard, bool kWide, class N>
OSG_D void write_root_results(const N& nodes, int64_t r, int num_actions, int root_player, uint32_t used, int sims_done,
                              const MctsOut& out, double* child_prior) {
  const uint32_t rm = nodes.meta(0);
  const int c = mw_nchild<kWide>(rm);
  const uint32_t first = nodes.first(0);
  for (int a = 0; a < num_actions; ++a) {
    if (out.child_visits) out.child_visits[r * num_actions + a] = 0;
    if (out.child_reward) out.child_reward[r * num_actions + a] = 0.0;
    if (out.child_outcome) out.child_outcome[r * num_actions + a] = 3;
    if (child_prior) child_prior[r * num_actions + a] = 0.0;
  }
  int best = -1;
  double b_out = 0.0, b_tot = 0.0;
  uint32_t b_cnt = 0;
  for (int k = 0; k < c; ++k) {
    const uint32_t cm = nodes.meta(first + k);
    const uint32_t cc = nodes.count(first + k);
    const double ct = nodes.total(first + k);
    const int a = static_cast<int>(mw_action<kWide>(cm));
    const bool has = m_has_outcome(cm);
    const int pl = m_player(cm);
    const double val = (has && pl >= 0 && cc > 0) ? outcome_value<kBoard>(cm, cc, ct, pl)
                                                  : ((has && kBoard && pl >= 0) ? outcome_value<true>(cm, 1, 0.0, pl) : 0.0);
    // strict "a < b" ordering, first maximum kept (std::max_element)
    const bool better = best < 0 || (b_out != val ? b_out < val : (b_cnt != cc ? b_cnt < cc : b_tot < ct));
    if (better) { best = a; b_out = val; b_cnt = cc; b_tot = ct; }
    if (a < num_actions) {
      if (out.child_visits) out.child_visits[r * num_actions + a] = static_cast<int32_t>(cc);
      if (out.child_reward) out.child_reward[r * num_actions + a] = ct;
      if constexpr (N::kHasPrior) {
        if (child_prior) child_prior[r * num_actions + a] = nodes.prior(first + k);
      }
      if (out.child_outcome) {
        int8_t code = 2;
        if (has && kBoard && root_player >= 0) code = static_cast<int8_t>(outcome_value<true>(cm, 1, 0.0, root_player));
        out.child_outcome[r * num_actions + a] = code;
      }
    }
  }
  if (out.best_action) out.best_action[r] = best;
  if (out.root_stats) {
    out.root_stats[r * 4 + 0] = static_cast<double>(nodes.count(0));
    out.root_stats[r * 4 + 1] = static_cast<double>(used);
    out.root_stats[r * 4 + 2] = (kBoard && m_has_outcome(rm) && root_player >= 0) ? outcome_value<true>(rm, 1, 0.0, root_player)
                                                                                : NAN;
    out.root_stats[r * 4 + 3] = static_cast<double>(sims_done);
  }
}

}  // namespace osg
#endif  // OSG_MCTS_LANE_H_
