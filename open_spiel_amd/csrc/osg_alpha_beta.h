// algorithms::AlphaBetaSearch (open_spiel/algorithms/minimax.cc:49-137, 222-256; python/algorithms/minimax.py:26-149)
// for ONE root, as a loop without recursion: host + device.
//
// The reference's _alpha_beta is a recursion whose frames hold (state, the legal actions not yet tried, alpha, beta,
// value).  Here the open frame of the current ply lives in registers and its ancestors on an explicit stack reached
// through an accessor, so the same loop body serves a lane of k_alpha_beta (osg_minimax.hip: stack in HBM, one lane
// per root, lanes of a wavefront in different phases — k_rollout's form) and a plain host call (tests/native/
// alpha_beta_host_test.cpp: array models of the rules, stack in a std::vector).  One step() is one of
//   descend   take the lowest untried action of the open frame, apply it, count the child (the reference's
//             _alpha_beta invocation), and — where the child is neither terminal nor at the depth limit —
//             push the frame and open the child's;
//   evaluate  a terminal child returns PlayerReturn(maximizing_player) (minimax.cc:53-55), a child at depth 0 the
//             leaf constant (minimax.cc:63-65) or status 1 (minimax.cc:57-61); the value is folded into the open frame
//             without a push;
//   return    an open frame with nothing left to try (all children done, or alpha >= beta: minimax.cc:95-98,
//             129-132) hands its value to its parent, popped from the stack.
// Children in ascending action order (LegalActions() order of the three board games); the maximiser replaces on
// child > value, the minimiser on child < value (minimax.cc:88,122); best_action is recorded at the root only
// (minimax.cc:90-92: the recursive calls pass nullptr).  Values are only copied and compared: doubles throughout.
//
// Rules model R (an object: it carries the game's parameters):
//   typename R::State, typename R::Todo (a set of actions)
//   bool terminal(const State&)            IsTerminal()
//   int mover(const State&)                the player to move by the position's own count (also of a terminal state)
//   double player_return(const State&, int player)
//   Todo legal(const State&)               LegalActions() of a state that is not terminal
//   void apply(State&, int action)
//   bool todo_any(const Todo&), int todo_pop(Todo&)   (lowest action first), void todo_clear(Todo&)
// Stack accessor S: void store(int ply, const AbFrame<R>&), void load(int ply, AbFrame<R>&); plies
// 0 .. min(depth_limit, max_game_length) - 2 are used (the deepest open frame is never pushed).
#ifndef OSG_ALPHA_BETA_H_
#define OSG_ALPHA_BETA_H_

#include <math.h>

#include "osg_common.h"

namespace osg {

enum AbStatus { kAbDone = 0, kAbDepthLimit = 1, kAbBudget = 2 };
enum AbLeafMode { kAbLeafNone = 0, kAbLeafConstant = 1 };   // OSG_AB_LEAF_* of include/osg_abi.h

struct AbConfig {
  int depth_limit;        // < 0: unlimited
  int maximizing_player;  // -1: the mover of the root (kInvalidPlayer, minimax.cc:244-246)
  int leaf_mode;
  double leaf_value;
  int64_t max_nodes;      // > 0
};

template <class R>
struct AbFrame {
  typename R::State s;
  typename R::Todo todo;   // legal actions not tried yet; emptied by a cut-off
  uint32_t is_max;         // CurrentPlayer() == maximizing_player
  double alpha, beta, value;
};

template <class R, class S>
struct AbSearch {
  AbFrame<R> f;   // the open frame of ply `ply`
  int ply, maxp, root_action;
  int64_t nodes;
  // results, valid once done
  double value;
  int best_action;
  int status;
  bool done;

  OSG_HD void finish(int st, double v) {
    status = st;
    value = st == kAbDone ? v : NAN;
    if (st != kAbDone) best_action = -1;
    done = true;
  }
  OSG_HD void open(const R& r, const typename R::State& s, double alpha, double beta) {
    f.s = s;
    f.todo = r.legal(s);
    f.is_max = r.mover(s) == maxp ? 1u : 0u;
    f.alpha = alpha;
    f.beta = beta;
    f.value = f.is_max ? -INFINITY : INFINITY;
  }
  // minimax.cc:88-98 / 122-132 for the open frame and the child reached by `action`
  OSG_HD void fold(double child, int action) {
    const bool better = f.is_max ? child > f.value : child < f.value;
    if (better) {
      f.value = child;
      if (ply == 0) best_action = action;
    }
    if (f.is_max) f.alpha = f.alpha > f.value ? f.alpha : f.value;   // std::max(alpha, value)
    else f.beta = f.beta < f.value ? f.beta : f.value;               // std::min(beta, value)
    if (f.alpha >= f.beta) R::todo_clear(f.todo);
  }
  // The root's own _alpha_beta invocation (minimax.cc:250-253: window (-inf, +inf)).
  OSG_HD void start(const R& r, const typename R::State& root, const AbConfig& cfg) {
    ply = 0;
    nodes = 1;
    best_action = -1;
    root_action = -1;
    status = kAbDone;
    value = 0.0;
    done = false;
    maxp = cfg.maximizing_player < 0 ? r.mover(root) : cfg.maximizing_player;
    if (r.terminal(root)) { finish(kAbDone, r.player_return(root, maxp)); return; }
    if (cfg.depth_limit == 0) {
      if (cfg.leaf_mode == kAbLeafNone) finish(kAbDepthLimit, 0.0); else finish(kAbDone, cfg.leaf_value);
      return;
    }
    open(r, root, -INFINITY, INFINITY);
  }
  OSG_HD void step(const R& r, S& stack, const AbConfig& cfg) {
    if (!R::todo_any(f.todo)) {   // return
      if (ply == 0) { finish(kAbDone, f.value); return; }
      const double v = f.value;
      --ply;
      stack.load(ply, f);
      fold(v, root_action);
      return;
    }
    const int a = R::todo_pop(f.todo);
    if (ply == 0) root_action = a;
    typename R::State child = f.s;
    r.apply(child, a);
    if (++nodes > cfg.max_nodes) { finish(kAbBudget, 0.0); return; }
    if (r.terminal(child)) { fold(r.player_return(child, maxp), a); return; }
    if (cfg.depth_limit >= 0 && ply + 1 == cfg.depth_limit) {   // the child's depth is 0
      if (cfg.leaf_mode == kAbLeafNone) { finish(kAbDepthLimit, 0.0); return; }
      fold(cfg.leaf_value, a);
      return;
    }
    stack.store(ply, f);   // descend
    ++ply;
    const double alpha = f.alpha, beta = f.beta;
    open(r, child, alpha, beta);
  }
};

// The whole search of one root (the host's form; a kernel interleaves step() with taking the next root).
template <class R, class S>
OSG_HD void alpha_beta_search(const R& r, S& stack, const typename R::State& root, const AbConfig& cfg, double* value,
                              int* best_action, int64_t* nodes, int* status) {
  AbSearch<R, S> search;
  search.start(r, root, cfg);
  while (!search.done) search.step(r, stack, cfg);
  *value = search.value;
  *best_action = search.best_action;
  *nodes = search.nodes;
  *status = search.status;
}

}  // namespace osg
#endif  // OSG_ALPHA_BETA_H_
