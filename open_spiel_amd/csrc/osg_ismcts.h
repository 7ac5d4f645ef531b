// Information-set MCTS (python/algorithms/ismcts.py ISMCTSBot with mcts.RandomRolloutEvaluator; its C++ twin is
// algorithms/is_mcts.{h,cc}) for ONE root of kuhn_poker or leduc_poker: host + device.
//
// One tree per search, its nodes keyed by (player to act, what that player knows); the root state is resampled from
// the searcher's information state before every simulation.  The whole search of a root is ismcts_search() below, so
// a lane of k_ismcts (osg_ismcts.hip: node table in HBM) and a plain host call (tests/native/ismcts_host_test.cpp: node
// table in a std::vector) run the same code.  The Python file is the one followed where the two differ: it draws
// randint(len(candidates)) even for a single candidate.
//
// Every draw of a root comes from ONE stream Rng(seed, index_offset + root index, 0), in the reference's order:
//   per simulation   the root sample: a resample (below), or — once max_world_samples samples are kept —
//                    below(max_world_samples) to pick one of them (ismcts.py:206-217)
//   resample         kuhn_poker.cc:351-373 / leduc_poker.cc:746-769: from the initial state, for p = 0 .. P-1 the
//                    searcher's own card is replayed and every other player's card is drawn by the chance CDF scan
//                    with unit() over the clone's current outcomes, again while it equals the searcher's card (leduc:
//                    or the public card); then the betting (leduc: round 1, the public card, round 2) is replayed
//   descent          chance node: one unit() CDF draw.  Decision node: look up or create the node of (player, key).
//                    A node just created is marked expanded with 0 visits and the evaluator's value is returned.
//                    Otherwise, while it has fewer children than legal actions: Fisher-Yates over the ascending legal
//                    actions (for i = n-1 .. 1: j = below(i+1); swap) and the first action without a child becomes
//                    one (ismcts.py:336-345); else the UCT / PUCT values, the candidates with value > max - 1e-5 in
//                    child insertion order, and candidates[below(count)] (ismcts.py:299-334)
//   evaluator        n_rollouts playouts: chance by the CDF draw, decisions by legal[below(count)]; the returns are
//                    added in playout order and divided by n_rollouts (mcts.py:56-76)
//   the end          one unit() for step_with_policy's draw from the final policy (ismcts.py:155-159), a CDF scan over
//                    the root's children in insertion order followed by the legal actions never expanded
// A root with a single legal action gets policy {a: 1}, no simulation, no draw and 0 nodes (ismcts.py:117-119).
//
// Node table T (an accessor: the caller chooses where the words live): nodes of kIsNodeHead + IsRules<G>::kWords 8-byte
// words, a hash of `hash_slots` (a power of two, > max_nodes) 32-bit slots holding node index + 1, and the kept root
// samples.  T offers
//   uint64_t node(int i, int w), void set_node(int i, int w, uint64_t v)
//   uint32_t slot(uint32_t h), void set_slot(uint32_t h, uint32_t v)
//   uint64_t sample(int i, int w), void set_sample(int i, int w, uint64_t v)
// Node words: 0 the key; 1 total_visits (low half, -1 = not evaluated yet) and the children (high half: count in bits
// 0-1, the action of the k-th child created in bits 2+2k .. 3+2k); 2 visits of actions 0 and 1; 3 visits of action 2
// (low half) and the player (high half); 4-6 return_sum of actions 0-2; then the state the node was created from.
#ifndef OSG_ISMCTS_H_
#define OSG_ISMCTS_H_

#include <math.h>

#include "osg_common.h"
#include "osg_game_poker.h"

namespace osg {

enum IsStatus { kIsDone = 0, kIsNoVisits = 1, kIsTableFull = 2, kIsBadRoot = 3 };
constexpr int kIsActions = 3;      // leduc_poker's fold / call / raise; kuhn_poker uses two
constexpr int kIsPlayers = 3;      // the games are searched with 2 or 3 players
constexpr int kIsNodeHead = 7;     // node words before the creating state
constexpr int kIsMaxDepth = 16;    // decision nodes on one path: kuhn 2P-1 <= 5, leduc 2 (3P-2) <= 14
constexpr int kIsMaxPlayoutPlies = 64;
constexpr int kIsMaxRejections = 4096;   // a consistent deal rejects with probability <= 1/2 per draw
constexpr double kIsTieTolerance = 1e-5;   // TIE_TOLERANCE, ismcts.py:28

struct IsConfig {
  double uct_c;
  int max_simulations, n_rollouts;
  int max_world_samples;        // <= 0: unlimited (UNLIMITED_NUM_WORLD_SAMPLES)
  int final_policy_type;        // 1 NORMALIZED_VISITED_COUNT, 2 MAX_VISIT_COUNT, 3 MAX_VALUE
  int child_selection_policy;   // 1 UCT, 2 PUCT
  int max_nodes;
  uint32_t hash_slots;          // a power of two above max_nodes
};

// The root's stream with a count of what was drawn.
struct IsRng {
  Rng r;
  uint32_t draws;
  OSG_HD IsRng(uint64_t seed, uint64_t stream) : r(seed, stream, 0), draws(0) {}
  OSG_HD double unit() { ++draws; return r.unit(); }
  OSG_HD uint32_t below(uint32_t n) { ++draws; return r.below(n); }
};

// SampleAction's CDF scan over ChanceOutcomes() (spiel.cc:372-409) with z = unit(): sample_action_w's chance branch,
// for host and device.
template <class G>
OSG_HD int is_chance_draw(const typename G::Params& p, const typename G::State& s, IsRng& rng) {
  const Mask m = G::legal(p, s);
  const int cnt = m.count();
  const double z = rng.unit();
  double acc = 0.0;
  int last = -1;
  for (int k = 0; k < cnt; ++k) {
    const int o = select_action(m, k);
    const double pr = G::chance_prob(p, s, o);
    if (acc <= z && z < acc + pr) return o;
    acc += pr;
    last = o;
  }
  return last;
}

// Per game: the record of a state in 8-byte words, the key of what `player` knows at a state where it acts (equal keys
// <=> equal InformationStateString of the same player), and ResampleFromInfostate.
template <class G> struct IsRules;

template <> struct IsRules<Kuhn> {
  using G = Kuhn;
  static constexpr int kWords = 1;
  OSG_HD static void to_words(const G::State& s, uint64_t* w) { w[0] = s.h; }
  OSG_HD static G::State from_words(const uint64_t* w) { return {w[0]}; }
  // the private card and the betting (kuhn_poker.cc:148-163); the player is the betting's length mod P
  OSG_HD static uint64_t key(const G::Params& p, const G::State& s, int player) {
    return static_cast<uint64_t>(player) | (static_cast<uint64_t>(G::card(s, player)) << 2) |
           (static_cast<uint64_t>(G::nact(p, s)) << 6) | (static_cast<uint64_t>(G::bets(s)) << 11);
  }
  OSG_HD static bool resample(const G::Params& p, const G::State& root, int me, IsRng& rng, G::State& out) {
    G::State c = G::initial(p);
    const int mine = G::card(root, me);
    int tries = 0;
    for (int q = 0; q < p.players; ++q) {
      int a = mine;
      if (q != me) {
        do {
          if (++tries > kIsMaxRejections) return false;
          a = is_chance_draw<G>(p, c, rng);
        } while (a == mine);
      }
      G::apply(p, c, a);
    }
    const int n = G::nact(p, root);
    const uint32_t b = G::bets(root);
    for (int j = 0; j < n; ++j) G::apply(p, c, static_cast<int>((b >> j) & 1u));
    out = c;
    return true;
  }
};

template <> struct IsRules<Leduc> {
  using G = Leduc;
  static constexpr int kWords = 2;
  OSG_HD static void to_words(const G::State& s, uint64_t* w) { G::pack(s, w[0], w[1]); }
  OSG_HD static G::State from_words(const uint64_t* w) { return G::unpack(w[0], w[1]); }
  // player, private card, public card and both rounds' moves (leduc_poker.cc:194-239: round, pot and money follow)
  OSG_HD static uint64_t key(const G::Params&, const G::State& s, int player) {
    return static_cast<uint64_t>(player) | (static_cast<uint64_t>(G::priv(s, player) + 1) << 2) |
           (static_cast<uint64_t>(s.pub + 1) << 6) | (static_cast<uint64_t>(s.len0) << 10) |
           (static_cast<uint64_t>(s.seq0) << 13) | (static_cast<uint64_t>(s.len1) << 27) |
           (static_cast<uint64_t>(s.seq1) << 30);
  }
  OSG_HD static bool resample(const G::Params& p, const G::State& root, int me, IsRng& rng, G::State& out) {
    G::State c = G::initial(p);
    const int mine = G::priv(root, me), pub = root.pub;
    int tries = 0;
    for (int q = 0; q < p.players; ++q) {
      int a = mine;
      if (q != me) {
        do {
          if (++tries > kIsMaxRejections) return false;
          a = is_chance_draw<G>(p, c, rng);
        } while (a == mine || a == pub);
      }
      G::apply(p, c, a);
    }
    for (int i = 0; i < root.len0; ++i) G::apply(p, c, static_cast<int>((root.seq0 >> (2 * i)) & 3u));
    if (pub >= 0) {
      G::apply(p, c, pub);
      for (int i = 0; i < root.len1; ++i) G::apply(p, c, static_cast<int>((root.seq1 >> (2 * i)) & 3u));
    }
    out = c;
    return true;
  }
};

// The children of a node as the high half of node word 1.
OSG_HD int is_child_count(uint32_t order) { return static_cast<int>(order & 3u); }
OSG_HD int is_child_action(uint32_t order, int k) { return static_cast<int>((order >> (2 + 2 * k)) & 3u); }
// insertion rank of `action` among the children, or -1
OSG_HD int is_child_rank(uint32_t order, int action) {
  int rank = -1;
  for (int k = 0; k < is_child_count(order); ++k) rank = is_child_action(order, k) == action ? k : rank;
  return rank;
}

// What a root hands back (arrays by action; kIsActions entries are written).
struct IsResult {
  double policy[kIsActions];
  double return_sum[kIsActions];
  int visits[kIsActions];
  int rank[kIsActions];
  int sampled_action, nodes, status;
  uint32_t draws;
};

template <class G, class T>
struct IsSearch {
  using R = IsRules<G>;
  using State = typename G::State;
  const typename G::Params& p;
  const IsConfig& cfg;
  T& table;
  IsRng rng;
  int nodes;

  OSG_HD IsSearch(const typename G::Params& p_, const IsConfig& cfg_, T& table_, uint64_t seed, uint64_t stream)
      : p(p_), cfg(cfg_), table(table_), rng(seed, stream), nodes(0) {}

  OSG_HD static uint32_t lo(uint64_t w) { return static_cast<uint32_t>(w); }
  OSG_HD static uint32_t hi(uint64_t w) { return static_cast<uint32_t>(w >> 32); }
  OSG_HD static uint64_t join(uint32_t l, uint32_t h) { return static_cast<uint64_t>(l) | (static_cast<uint64_t>(h) << 32); }
  OSG_HD int visits_of(int node, int a) const {
    const uint64_t w = table.node(node, a < 2 ? 2 : 3);
    return static_cast<int>(a == 1 ? hi(w) : lo(w));
  }
  OSG_HD void bump_visits(int node, int a) {
    const int w = a < 2 ? 2 : 3;
    table.set_node(node, w, table.node(node, w) + (a == 1 ? (1ull << 32) : 1ull));   // (counts stay below 2^31: no carry)
  }
  OSG_HD static double as_double(uint64_t w) { double d; __builtin_memcpy(&d, &w, 8); return d; }
  OSG_HD static uint64_t as_word(double d) { uint64_t w; __builtin_memcpy(&w, &d, 8); return w; }

  // lookup_node (ismcts.py:237-240): the node's index or -1
  OSG_HD int find(uint64_t key) const {
    const uint32_t mask = cfg.hash_slots - 1u;
    for (uint32_t h = static_cast<uint32_t>(mix64(key)) & mask;; h = (h + 1u) & mask) {
      const uint32_t v = table.slot(h);
      if (v == 0u) return -1;
      if (table.node(static_cast<int>(v - 1u), 0) == key) return static_cast<int>(v - 1u);
    }
  }
  // create_new_node (ismcts.py:226-232); the caller has checked that the table has room
  OSG_HD int create(uint64_t key, const State& s, int player) {
    const int i = nodes++;
    table.set_node(i, 0, key);
    table.set_node(i, 1, join(0xFFFFFFFFu, 0u));   // UNEXPANDED_VISIT_COUNT, no children
    table.set_node(i, 2, 0ull);
    table.set_node(i, 3, join(0u, static_cast<uint32_t>(player)));
    for (int a = 0; a < kIsActions; ++a) table.set_node(i, 4 + a, as_word(0.0));
    uint64_t w[R::kWords];
    R::to_words(s, w);
    for (int k = 0; k < R::kWords; ++k) table.set_node(i, kIsNodeHead + k, w[k]);
    const uint32_t mask = cfg.hash_slots - 1u;
    uint32_t h = static_cast<uint32_t>(mix64(key)) & mask;
    while (table.slot(h) != 0u) h = (h + 1u) & mask;
    table.set_slot(h, static_cast<uint32_t>(i) + 1u);
    return i;
  }

  // RandomRolloutEvaluator.evaluate (mcts.py:56-76)
  OSG_HD void evaluate(const State& s, double* ret) {
    double sum[kIsPlayers] = {0.0, 0.0, 0.0};
    for (int r = 0; r < cfg.n_rollouts; ++r) {
      State w = s;
      for (int ply = 0; ply < kIsMaxPlayoutPlies && !G::terminal(p, w); ++ply) {
        int a;
        if (G::current_player(p, w) == kChancePlayer) {
          a = is_chance_draw<G>(p, w, rng);
        } else {
          const Mask m = G::legal(p, w);
          a = select_action(m, static_cast<int>(rng.below(static_cast<uint32_t>(m.count()))));
        }
        G::apply(p, w, a);
      }
      double one[kMaxPlayers];
      G::returns(p, w, one);
      for (int q = 0; q < kIsPlayers; ++q) sum[q] = r == 0 ? (q < p.players ? one[q] : 0.0) : sum[q] + (q < p.players ? one[q] : 0.0);
    }
    for (int q = 0; q < kIsPlayers; ++q) ret[q] = sum[q] / cfg.n_rollouts;
  }

  // check_expand (ismcts.py:336-345) for a node with fewer children than legal actions: the action of the new child
  OSG_HD int expand_action(uint32_t legal, int n_legal, uint32_t order) {
    uint32_t perm = 0u;   // the ascending legal actions, 2 bits each
    for (int k = 0; k < n_legal; ++k) perm |= static_cast<uint32_t>(select32(legal, k)) << (2 * k);
    for (int i = n_legal - 1; i >= 1; --i) {
      const int j = static_cast<int>(rng.below(static_cast<uint32_t>(i + 1)));
      const uint32_t xi = (perm >> (2 * i)) & 3u, xj = (perm >> (2 * j)) & 3u;
      perm = (perm & ~((3u << (2 * i)) | (3u << (2 * j)))) | (xj << (2 * i));
      perm = (perm & ~(3u << (2 * j))) | (xi << (2 * j));
    }
    for (int k = 0; k < n_legal; ++k) {
      const int a = static_cast<int>((perm >> (2 * k)) & 3u);
      if (is_child_rank(order, a) < 0) return a;
    }
    return -1;   // (not reached: the node has fewer children than legal actions)
  }

  // _action_value (ismcts.py:299-315) of child `a` of `node` with `total` visits
  OSG_HD double action_value(int node, int a, int total, int n_legal) const {
    const double visits = static_cast<double>(visits_of(node, a));
    double v = as_double(table.node(node, 4 + a)) / visits;
    if (cfg.child_selection_policy == 1) v += cfg.uct_c * sqrt(log(static_cast<double>(total)) / visits);
    else v += cfg.uct_c * (1.0 / n_legal) * sqrt(static_cast<double>(total)) / (1.0 + visits);
    return v;
  }
  // select_action (ismcts.py:317-334)
  OSG_HD int select(int node, uint32_t order, int total, int n_legal) {
    const int n = is_child_count(order);
    double val[kIsActions];   // by insertion rank (n <= 3: unrolled selects, no runtime index)
    double best = -INFINITY;
#pragma unroll
    for (int k = 0; k < kIsActions; ++k) {
      val[k] = k < n ? action_value(node, is_child_action(order, k), total, n_legal) : -INFINITY;
      best = val[k] > best ? val[k] : best;
    }
    int count = 0;
#pragma unroll
    for (int k = 0; k < kIsActions; ++k) count += (k < n && val[k] > best - kIsTieTolerance) ? 1 : 0;
    int pick = static_cast<int>(rng.below(static_cast<uint32_t>(count)));
    int action = -1;
#pragma unroll
    for (int k = 0; k < kIsActions; ++k) {
      const bool cand = k < n && val[k] > best - kIsTieTolerance;
      if (cand && pick == 0 && action < 0) action = is_child_action(order, k);
      pick -= cand ? 1 : 0;
    }
    return action;
  }

  // run_simulation (ismcts.py:347-384) from a sampled root; false when the table is full or the record is inconsistent
  OSG_HD bool simulate(State s, int* status) {
    uint32_t path[kIsMaxDepth];   // node | action << 24 | player << 28
    int depth = 0;
    double ret[kIsPlayers];
    for (;;) {
      if (G::terminal(p, s)) {
        double one[kMaxPlayers];
        G::returns(p, s, one);
        for (int q = 0; q < kIsPlayers; ++q) ret[q] = q < p.players ? one[q] : 0.0;
        break;
      }
      const int cur = G::current_player(p, s);
      if (cur == kChancePlayer) {
        G::apply(p, s, is_chance_draw<G>(p, s, rng));
        continue;
      }
      const uint32_t legal = G::legal(p, s).w[0];
      const int n_legal = __builtin_popcount(legal);
      const uint64_t key = R::key(p, s, cur);
      int node = find(key);
      if (node < 0) {
        if (nodes >= cfg.max_nodes) { *status = kIsTableFull; return false; }
        node = create(key, s, cur);
      }
      const uint64_t w1 = table.node(node, 1);
      const int total = static_cast<int>(lo(w1));
      uint32_t order = hi(w1);
      if (total < 0) {   // first visit: expanded with 0 visits, the evaluator's value goes back up
        table.set_node(node, 1, join(0u, order));
        evaluate(s, ret);
        break;
      }
      if (depth == kIsMaxDepth) { *status = kIsBadRoot; return false; }
      int a;
      if (is_child_count(order) < n_legal) {
        a = expand_action(legal, n_legal, order);
        order = (order + 1u) | (static_cast<uint32_t>(a) << (2 + 2 * is_child_count(order)));
      } else {
        a = select(node, order, total, n_legal);
      }
      table.set_node(node, 1, join(static_cast<uint32_t>(total + 1), order));
      bump_visits(node, a);
      path[depth++] = static_cast<uint32_t>(node) | (static_cast<uint32_t>(a) << 24) | (static_cast<uint32_t>(cur) << 28);
      G::apply(p, s, a);
    }
    for (int d = 0; d < depth; ++d) {   // each child takes one addend per simulation: the order among nodes is free
      const int node = static_cast<int>(path[d] & 0xFFFFFFu), a = static_cast<int>((path[d] >> 24) & 3u);
      const int player = static_cast<int>(path[d] >> 28);
      const double r = player == 0 ? ret[0] : (player == 1 ? ret[1] : ret[2]);
      table.set_node(node, 4 + a, as_word(as_double(table.node(node, 4 + a)) + r));
    }
    return true;
  }

  // get_final_policy (ismcts.py:161-204) and step_with_policy's draw (ismcts.py:155-159)
  OSG_HD void finish(uint32_t legal, IsResult* out) {
    const uint64_t w1 = table.node(0, 1);
    const int total = static_cast<int>(lo(w1));
    const uint32_t order = hi(w1);
    const int n = is_child_count(order);
    for (int a = 0; a < kIsActions; ++a) {
      out->visits[a] = visits_of(0, a);
      out->return_sum[a] = as_double(table.node(0, 4 + a));
      out->rank[a] = is_child_rank(order, a);
    }
    if (total <= 0) {   // the reference's `assert node.total_visits > 0`
      out->status = kIsNoVisits;
      return;
    }
    int max_visits = -1, ties = 0;
    double max_value = -INFINITY;
    for (int k = 0; k < n; ++k) {
      const int a = is_child_action(order, k);
      if (cfg.final_policy_type == 2) {
        const int v = out->visits[a];
        if (v == max_visits) ++ties;
        else if (v > max_visits) { max_visits = v; ties = 1; }
      } else if (cfg.final_policy_type == 3) {
        const double v = out->return_sum[a] / static_cast<double>(out->visits[a]);
        if (v == max_value) ++ties;
        else if (v > max_value) { max_value = v; ties = 1; }
      }
    }
    for (int a = 0; a < kIsActions; ++a) {
      double pr = 0.0;   // a legal action never expanded is appended with 0
      if (out->rank[a] >= 0) {
        const double v = static_cast<double>(out->visits[a]);
        if (cfg.final_policy_type == 1) pr = v / total;
        else if (cfg.final_policy_type == 2) pr = out->visits[a] == max_visits ? 1.0 / ties : 0.0;
        else pr = out->return_sum[a] / v == max_value ? 1.0 / ties : 0.0;
      }
      out->policy[a] = pr;
    }
    // the policy list: children in insertion order, then the other legal actions ascending
    const double z = rng.unit();
    double acc = 0.0;
    int last = -1, chosen = -1;
    const int n_legal = __builtin_popcount(legal);
    for (int k = 0; k < n + n_legal && chosen < 0; ++k) {
      int a;
      if (k < n) {
        a = is_child_action(order, k);
      } else {
        a = select32(legal, k - n);
        if (out->rank[a] >= 0) continue;
      }
      const double pr = a == 0 ? out->policy[0] : (a == 1 ? out->policy[1] : out->policy[2]);
      if (acc <= z && z < acc + pr) chosen = a;
      acc += pr;
      last = a;
    }
    out->sampled_action = chosen >= 0 ? chosen : last;
  }

  // run_search + step_with_policy (ismcts.py:110-159) of a root that is a decision node
  OSG_HD void run(const State& root, IsResult* out) {
    for (int a = 0; a < kIsActions; ++a) {
      out->policy[a] = NAN;
      out->return_sum[a] = 0.0;
      out->visits[a] = 0;
      out->rank[a] = -1;
    }
    out->sampled_action = -1;
    out->status = kIsDone;
    const int me = G::current_player(p, root);
    const uint32_t legal = G::legal(p, root).w[0];
    if (__builtin_popcount(legal) == 1) {
      const int a = __builtin_ctz(legal);
      for (int b = 0; b < kIsActions; ++b) out->policy[b] = b == a ? 1.0 : 0.0;
      out->sampled_action = a;
      out->nodes = 0;
      out->draws = 0;
      return;
    }
    for (uint32_t h = 0; h < cfg.hash_slots; ++h) table.set_slot(h, 0u);
    if (cfg.max_nodes < 1) {
      out->status = kIsTableFull;
    } else {
      create(R::key(p, root, me), root, me);
      const int keep = cfg.max_world_samples > 0 ? cfg.max_world_samples : 0;
      for (int sim = 0; sim < cfg.max_simulations && out->status == kIsDone; ++sim) {
        State s;
        if (keep > 0 && sim >= keep) {   // sample_root_state, ismcts.py:206-217
          const int i = static_cast<int>(rng.below(static_cast<uint32_t>(keep)));
          uint64_t w[R::kWords];
          for (int k = 0; k < R::kWords; ++k) w[k] = table.sample(i, k);
          s = R::from_words(w);
        } else {
          if (!R::resample(p, root, me, rng, s)) { out->status = kIsBadRoot; break; }
          if (keep > 0) {
            uint64_t w[R::kWords];
            R::to_words(s, w);
            for (int k = 0; k < R::kWords; ++k) table.set_sample(sim, k, w[k]);
          }
        }
        simulate(s, &out->status);
      }
    }
    if (out->status == kIsDone) finish(legal, out);
    else if (nodes > 0) {
      const uint32_t order = hi(table.node(0, 1));
      for (int a = 0; a < kIsActions; ++a) {
        out->visits[a] = visits_of(0, a);
        out->return_sum[a] = as_double(table.node(0, 4 + a));
        out->rank[a] = is_child_rank(order, a);
      }
    }
    if (out->status != kIsDone) {
      for (int a = 0; a < kIsActions; ++a) out->policy[a] = NAN;
      out->sampled_action = -1;
    }
    out->nodes = nodes;
    out->draws = rng.draws;
  }
};

// The hash of a table of max_nodes nodes: at most half full.
OSG_HD uint32_t is_hash_slots(int max_nodes) {
  uint32_t h = 2u;
  while (h < 2u * static_cast<uint32_t>(max_nodes > 0 ? max_nodes : 0)) h <<= 1;
  return h;
}
// The sample slots a search keeps: the first max_world_samples simulations each keep theirs.
OSG_HD int is_sample_slots(const IsConfig& cfg) {
  if (cfg.max_world_samples <= 0) return 0;
  return cfg.max_world_samples < cfg.max_simulations ? cfg.max_world_samples : cfg.max_simulations;
}

// The whole search of one root.
template <class G, class T>
OSG_HD void ismcts_search(const typename G::Params& p, const typename G::State& root, const IsConfig& cfg, uint64_t seed,
                          uint64_t stream, T& table, IsResult* out) {
  IsSearch<G, T> search(p, cfg, table, seed, stream);
  search.run(root, out);
}

}  // namespace osg
#endif  // OSG_ISMCTS_H_
