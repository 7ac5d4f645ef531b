// algorithms::MCTSBot (open_spiel/algorithms/mcts.{h,cc}) for a batch of roots.
//
// Mapping: ONE LANE PER ROOT.  A search is a strictly sequential chain
// (simulation s+1 reads the statistics simulation s wrote), and with
// RandomRolloutEvaluator the chain is dominated by the random playout, which is
// itself sequential.  The SIMT-efficient unit of parallelism is therefore the
// root: 64 independent searches per wavefront, every lane running the same
// select / expand / rollout / backup code on its own tree.  (A wave-per-root
// layout spreads a node's children over the lanes and leaves 63 of 64 lanes idle
// in a move-by-move playout; where the playout itself is lane-parallel — hex
// without the swap rule: one random fill of the board — it is the faster one and
// layout = 0 picks it, osg_mcts_wave.hip)
//
// Tree storage in HBM: a node pool of `cap` nodes per root, struct-of-arrays and — since round 6 — root-major
// (field[root * cap + node]): a lane scans and writes runs of its own tree (rounds 1-5: root-minor, which coalesces
// across lanes only near the root; see k_mcts).
//   meta   u32  action | (player+1)<<8 | nchild<<12 | has_outcome<<20 | code<<21 | terminal<<23
//   first  u32  index of the first child (children are contiguous)
//   parent u32
//   count  u32  explore_count
//   total  f64  total_reward
#include <algorithm>
#include <cmath>
#include <vector>

#include "osg_mcts_lane.h"

using namespace osg;

namespace {

template <class G, bool kBoard>
__global__ void __launch_bounds__(kBlockM)
k_mcts(typename G::Params p, const typename G::word_t* base, int64_t n, int num_players, int num_actions,
       osg_mcts_cfg cfg, double max_utility, const double* __restrict__ log_table, Pool pool, int32_t* best_action,
       int32_t* child_visits, double* child_reward, int8_t* child_outcome, double* root_stats) {
  // (games with more than 255 actions — hex above 15 x 15 — use the nine-bit action / child-count fields)
  constexpr bool kWide = G::kMaskW > kMaskWords;
  using LegalMask = MaskT<G::kMaskW>;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlockM + threadIdx.x;
  if (r >= n) return;
  // the lane's column of the shuffle stage: entry k at sh[k * kBlockM] (dynamic LDS: widest node x kBlockM entries)
  using act_t = uint8_t;   // (boards of up to six plane words: at most 193 actions)
  extern __shared__ unsigned char s_shuffle[];
  act_t* sh = reinterpret_cast<act_t*>(s_shuffle) + threadIdx.x;
  (void)sh;
  const uint64_t gr = static_cast<uint64_t>(cfg.index_offset + r);
  // This lane's tree.  Round 6: ROOT-MAJOR (field[root * cap + node], the wave layout's form) — a root's nodes are
  // contiguous, so a lane's scan of a node's children and the stores of an expansion walk ONE run of memory (32 children's
  // counts per 128-byte line) instead of one line per child and field; root-minor (field[node * n + root]; rounds 1-5)
  // coalesces across lanes only while the lanes stand on the same node index, i.e. near the root.  2^16 roots
  // (profiles/r06zf_*, r06zi_*): hex(9) x 512 simulations 4.5e8 -> 7.2e8, 11 x 11 2.2e8 -> 4.4e8, 13 x 13 1.2e8 -> 2.9e8,
  // tic_tac_toe x 1000 8.2e8 -> 9.9e8, connect_four x 256 1.35e9 -> 1.42e9 simulations/s; SHORT searches of narrow games
  // stay near the root and keep root-minor (connect_four x 32: 2.78e9 against 2.27e9, tic_tac_toe x 100: 2.09e9 against
  // 1.89e9): the host picks (pool.root_major; OSG_MCTS_ROOT_MAJOR=0/1 forces one).
  const LaneNodes<Pool> nodes(pool, r);

  const typename G::State root_state = G::load(p, base, n, r);
  const int root_player = G::current_player(p, root_state);
  nodes.meta(0) = mw_make<kWide>(0xFF, root_player, 0);  // mcts.cc:356-357: root = (kInvalidAction, CurrentPlayer(), 1)
  nodes.first(0) = 0; nodes.parent(0) = kNoNode; nodes.count(0) = 0; nodes.total(0) = 0.0;
  uint32_t used = 1;       // = the reference's nodes_: 1 + the children blocks allocated (mcts.cc:299,354)
  int gc_limit = kMinGcLimit;
  int sims_done = 0;

  for (int sim = 0; sim < cfg.max_simulations; ++sim) {
    Rng trng(cfg.seed ^ kTreeSalt, gr, static_cast<uint64_t>(sim));
    // ---- ApplyTreePolicy (mcts.cc:273-351) ----
    typename G::State s = root_state;
    uint32_t node = 0;
    bool term;
    for (;;) {
      term = G::terminal(p, s);
      const uint32_t cnt = nodes.count(node);
      if (term || cnt == 0) break;
      uint32_t meta = nodes.meta(node);
      const int cur = G::current_player(p, s);
      if (mw_nchild<kWide>(meta) == 0) {  // expand: children = Prior(state), shuffled (mcts.cc:281-299)
        const LegalMask legal = G::legal(p, s);
        const int c = legal.count();
        // slots exhausted (unreachable unless the caller's HBM could not hold max_nodes + slack), or a record that is
        // not terminal and has no legal action (only an uploaded inconsistent one): evaluate as a leaf
        if (c == 0 || used + static_cast<uint32_t>(c) > static_cast<uint32_t>(pool.cap)) break;
        const uint32_t first = used;
        used += c;
        if constexpr (G::kMaskW < 8) {
        // Round 6: the children's order is formed in LDS and every header written ONCE.  The shuffle used to run on
        // the pool — per child two loads and two stores of the lane's own, scattered node words on top of the five
        // initialising stores — which is most of what an expansion of a wide node (hex: ~100 children) costs.
        // Same draws, same swaps, same order.
        {
          int k = 0;
#pragma unroll
          for (int w = 0; w < G::kMaskW; ++w)
            for (uint32_t bits = legal.w[w]; bits != 0u; bits &= bits - 1u)
              sh[(k++) * kBlockM] = static_cast<act_t>(32 * w + __builtin_ctz(bits));
        }
        for (int i = c - 1; i >= 1; --i) {  // Fisher-Yates == std::shuffle's role (order only)
          const int j = static_cast<int>(trng.below(static_cast<uint32_t>(i + 1)));
          const act_t ai = sh[i * kBlockM], aj = sh[j * kBlockM];
          sh[i * kBlockM] = aj;
          sh[j * kBlockM] = ai;
        }
        for (int k = 0; k < c; ++k) {
          nodes.meta(first + k) = mw_make<kWide>(static_cast<int>(sh[k * kBlockM]), cur, 0);
          nodes.first(first + k) = 0; nodes.parent(first + k) = node; nodes.count(first + k) = 0; nodes.total(first + k) = 0.0;
        }
        } else {   // (boards from 16 x 16 on: two-byte entries x 362 children x 64 lanes would cost the kernel a wavefront per CU — 19 x 19: 2.9e8 -> 1.5e8)
        expand_on_pool<kWide>(nodes, legal, c, cur, node, first, trng);
        }
        meta = mw_make<kWide>(static_cast<int>(mw_action<kWide>(meta)), m_player(meta), c) | (meta & kMetaOutcomeBits);
        nodes.meta(node) = meta;
        nodes.first(node) = first;
      }
      const uint32_t first = nodes.first(node);
      const int c = mw_nchild<kWide>(meta);
      uint32_t chosen = first, chosen_meta = 0;
      bool have_meta = false;
      if (cur == kChancePlayer) {  // mcts.cc:311-322
        const LegalMask legal = G::legal(p, s);
        const int a = sample_action_chance<G>(p, s, legal, trng);
        for (int k = 0; k < c; ++k)
          if (static_cast<int>(mw_action<kWide>(nodes.meta(first + k))) == a) { chosen = first + k; break; }
      } else {  // arg-max of UCTValue, first maximum wins (mcts.cc:324-341, 90-101)
        double best = -INFINITY;
        const double logn = log_table[cnt];
        const bool puct = cfg.child_selection_policy == 1;
        const double prior = 1.0 / c;                              // Prior(): uniform over the legal actions
        const double sqrt_n = sqrt(static_cast<double>(cnt));
        // a search is ONE chain of dependent, scattered loads: the children's statistics are requested eight children at a
        // time with clamped indices (24 independent loads, one round trip) instead of child by child behind the
        // branches of the value formula (see k_mcts_advance, osg_mcts_step.hip)
        constexpr int kChunk = 8;
        // Round 6.  Under UCT a child that was never visited scores +infinity (mcts.cc:95) and the FIRST such child wins:
        // nothing behind it can score higher, nothing before it needs its value formed.  While a node still has
        // unvisited children — most visits of a wide node (hex: ~100 children, visited in order) — the scan therefore
        // only looks for the first one: counts and headers, no totals, none of the ~60 fp64 instructions per child.
        // Whether that is the case is read off the LAST child (the children are first visited in order, so it is the
        // last to go); if it was visited the full scan below runs, which is exact whatever the order was.
        bool scan_only = false;
        if (!puct) {
          const uint32_t at = first + static_cast<uint32_t>(c - 1);
          scan_only = nodes.count(at) == 0 && !m_has_outcome(nodes.meta(at));
        }
        bool settled = false;   // an unvisited child was found: the arg-max is decided
        for (int k0 = 0; k0 < c && !settled; k0 += kChunk) {
          uint32_t cm[kChunk], cc[kChunk];
          double ct[kChunk];
#pragma unroll
          for (int j = 0; j < kChunk; ++j) {
            const uint32_t at = first + static_cast<uint32_t>(k0 + j < c ? k0 + j : c - 1);
            cm[j] = nodes.meta(at);
            cc[j] = nodes.count(at);
            ct[j] = scan_only ? 0.0 : nodes.total(at);
          }
#pragma unroll
          for (int j = 0; j < kChunk; ++j) {
            if (k0 + j >= c || settled) continue;
            const bool unvisited = !puct && cc[j] == 0 && !m_has_outcome(cm[j]);
            if (scan_only && !unvisited) continue;
            double v;
            if (m_has_outcome(cm[j])) v = outcome_value<kBoard>(cm[j], cc[j], ct[j], m_player(cm[j]));
            else if (puct) v = (cc[j] != 0 ? ct[j] / cc[j] : 0.0) + cfg.uct_c * prior * sqrt_n / (cc[j] + 1);  // mcts.cc:103-112
            else if (cc[j] == 0) v = INFINITY;
            else v = ct[j] / cc[j] + cfg.uct_c * sqrt(logn / cc[j]);
            if (v > best) { best = v; chosen = first + static_cast<uint32_t>(k0 + j); chosen_meta = cm[j]; have_meta = true; }
            settled = unvisited;
          }
        }
      }
      G::apply(p, s, static_cast<int>(mw_action<kWide>(have_meta ? chosen_meta : nodes.meta(chosen))));
      node = chosen;
    }
    // ---- evaluate (mcts.cc:372-381) ----
    double returns[kMaxPlayers];
    bool solved = false;
    if (term) {
      G::returns(p, s, returns);
      mark_terminal_leaf<kBoard>(nodes, node, returns);
      solved = cfg.solve != 0;
    } else {  // RandomRolloutEvaluator::Evaluate (mcts.cc:43-72)
      for (int q = 0; q < num_players; ++q) returns[q] = 0.0;
      for (int ro = 0; ro < cfg.n_rollouts; ++ro) {
        Rng rng(cfg.seed, gr, static_cast<uint64_t>(sim) * cfg.n_rollouts + ro);
        double rr[kMaxPlayers];
        playout_returns<G>(p, s, rng, rr);
        for (int q = 0; q < num_players; ++q) returns[q] += rr[q];
      }
      for (int q = 0; q < num_players; ++q) returns[q] /= cfg.n_rollouts;
    }
    // ---- backup (mcts.cc:383-435) ----
    backup_and_solve<kBoard, kWide>(nodes, node, returns, num_players, max_utility, solved, /*counted=*/false);
    ++sims_done;
    if (search_is_over<kWide>(nodes.meta(0))) break;  // mcts.cc:437-440
    garbage_collect<kWide>(nodes, pool.gc_nodes, used, gc_limit);
  }

  write_root_results<kBoard, kWide>(nodes, r, num_actions, root_player, used, sims_done,
                                    MctsOut{best_action, child_visits, child_reward, child_outcome, root_stats}, nullptr);
}

}  // namespace

extern "C" int osg_mcts_search(const osg_batch* roots, const osg_mcts_cfg* cfg_in, int32_t* best_action,
                               int32_t* child_visits, double* child_reward, int8_t* child_outcome,
                               double* root_stats, int on_host) {
  if (!roots || !cfg_in) return set_error(OSG_ERR_INVALID, "osg_mcts_search: null argument");
  osg_ctx* ctx = roots->ctx;
  osg_mcts_cfg cfg = *cfg_in;
  const osg_game_desc& d = roots->spec.desc;
  const bool board = d.game_kind <= kHex;
  if (cfg.max_simulations < 1 || cfg.n_rollouts < 1) return set_error(OSG_ERR_INVALID, "max_simulations and n_rollouts must be >= 1");
  if (int rc = refuse_endless_playouts(roots->spec, "osg_mcts_search")) return rc;
  if (roots->spec.desc.num_distinct_actions > kMaxSearchActions)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_mcts_search: a node holds up to 511 actions");
  // the games beyond the 4-word mask / the two-word records (hex above 11 x 11 with the swap rule, connect_four above 64
  // board bits, leduc_poker with 4+ players) are searched by the lane-per-root kernel; the wave-per-root kernel keeps a hex
  // position in scalar registers (two 64-cell sets per colour up to 128 cells, three / four / six on the boards above)
  const bool wide_game = roots->spec.desc.num_distinct_actions > 32 * kMaskWords || roots->spec.c4_wide || roots->spec.leduc_big;
  if (cfg.solve && !board)
    return set_error(OSG_ERR_UNSUPPORTED, "solve=true needs win/draw/loss outcomes (tic_tac_toe, connect_four, hex)");
  int layout = cfg.layout;
  if (layout != 0 && layout != 1 && layout != 2) return set_error(OSG_ERR_INVALID, "osg_mcts_cfg.layout must be 0, 1 or 2");
  // (round 6: the hex boards above 128 cells too — kS = 3 / 4 / 6 cell sets per colour in scalar registers and as many
  // child slots per lane — in the random-fill form only: no swap rule, and at most 64 columns so that a cell's neighbours
  // lie in the adjacent cell sets)
  bool wide_hex_fill = false;
  if (wide_game && d.game_kind == kHex && d.num_distinct_actions == d.obs_shape[1] * d.obs_shape[2]) {
    int rows = 0, cols = 0, cells = 0;
    hex_dims(roots->spec, &rows, &cols, &cells);
    wide_hex_fill = rows >= 2 && cols >= 2 && cols <= 64;
  }
  if (layout == 0)  // auto: the wave layout where its parallel playout applies (hex without the swap rule; measured on the
                    // boards above 128 cells too: 2.1-2.6 x the lane layout on 12 x 12 ... 16 x 16, profiles/r06zn_*)
    layout = ((!wide_game || wide_hex_fill) && d.game_kind == kHex && d.num_distinct_actions == d.obs_shape[1] * d.obs_shape[2]) ? 2 : 1;
  if (layout == 2 && wide_game && !wide_hex_fill)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_mcts_search: layout 2 (a wavefront per root) serves games of up to 128 actions and "
                                          "the larger hex boards without the swap rule (2 ... 64 columns); "
                                          "this game is searched with layout 1 (or 0 = automatic)");
  if (cfg.child_selection_policy != 0 && cfg.child_selection_policy != 1)
    return set_error(OSG_ERR_INVALID, "osg_mcts_cfg.child_selection_policy must be 0 (UCT) or 1 (PUCT)");
  const int64_t n = roots->n;
  const int A = d.num_distinct_actions;
  const int widest = A > d.max_chance_outcomes ? A : d.max_chance_outcomes;
  // Node pool: `cap` slots per root.  A simulation expands at most one node (<= widest children), so
  // 1 + max_simulations * widest slots can never run out.  cfg.max_nodes > 0 is the reference's max_nodes_
  // (mcts.cc:214: (max_memory_mb << 20) / sizeof(SearchNode) + 1): the search garbage-collects when
  // nodes_ >= max_nodes_ (mcts.cc:441-482), and the pool gets the slots one search can hold between two
  // collections (a collection that frees nothing is followed by ever stricter ones: gc_limit_ grows by a
  // quarter each time, so at most ~log_1.25(max_simulations / 5) consecutive collections fail).
  // cfg.max_nodes <= 0: no limit from the caller: the pool gets the slots that can never run out when they fit
  // in 60 % of the free HBM (288 GB: 2^16 hex(9) roots x 1024 simulations need 130 GB of address space and
  // touch a twentieth of it), otherwise what fits, and a tree that outgrows it is collected like the
  // reference collects at that size.
  // (node indices are 32-bit with 0xFFFFFFFF reserved: a tree never holds more than 2^30 slots)
  const int64_t never = std::min<int64_t>(1 + static_cast<int64_t>(cfg.max_simulations) * widest, int64_t{1} << 30);
  const int64_t slack = 32 * static_cast<int64_t>(widest);
  int64_t cap, gc_nodes = 0;
  if (cfg.max_nodes > 0 && cfg.max_nodes < never) {
    gc_nodes = cfg.max_nodes > 2 ? cfg.max_nodes : 2;
    cap = std::min<int64_t>(never, gc_nodes + slack);
  } else {
    cap = never;
  }
  if (cap < 1 + widest) cap = 1 + widest;
  if (pool_layout(cap, n, gc_nodes > 0).bytes > ctx->d_mcts_pool.size()) {
    size_t free_b = 0, total_b = 0;
    OSG_HIP(hipMemGetInfo(&free_b, &total_b));
    free_b += ctx->d_mcts_pool.size();  // the old pool is released before the new one is allocated
    if (gc_nodes > 0) {
      if (pool_layout(cap, n, true).bytes > free_b * 9 / 10)
        return set_error(OSG_ERR_NOMEM, "osg_mcts_search: max_nodes slots per root do not fit the free HBM");
    } else if (pool_layout(cap, n, false).bytes > free_b * 6 / 10) {
      cap = static_cast<int64_t>(free_b * 6 / 10 / pool_layout(1, n, true).bytes);   // (a pool that collects has a remap plane)
      if (cap < 2 + 2 * widest) cap = 2 + 2 * widest;
      gc_nodes = cap - widest;  // collect before a simulation's expansion could overrun the slots
    }
  }
  cfg.max_nodes = static_cast<int32_t>(cap);
  const PoolLayout lay = pool_layout(cap, n, gc_nodes > 0);
  if (int rc = nomem_error(ctx_grow(ctx, ctx->d_mcts_pool, lay.bytes), "MCTS node pool: ")) return rc;
  Pool pool = lay.planes(reinterpret_cast<char*>(ctx->d_mcts_pool.get()));
  pool.n = n;
  {
    const char* e = std::getenv("OSG_MCTS_ROOT_MAJOR");
    pool.root_major = e ? (e[0] == '1' ? 1 : 0) : ((widest <= 16 && cfg.max_simulations <= 128) ? 0 : 1);
  }
  pool.cap = static_cast<int>(cap);
  pool.gc_nodes = static_cast<int>(gc_nodes);

  // log(parent explore_count) from the host libm: the CPU oracle (and the reference) call
  // std::log, so sharing the table makes UCT values bit-equal.  Cached in the context.
  if (const size_t want = static_cast<size_t>(cfg.max_simulations) + 2; want > ctx->d_mcts_logs.size()) {
    std::vector<double> logs(want);
    logs[0] = 0.0;
    for (size_t i = 1; i < want; ++i) logs[i] = std::log(static_cast<double>(i));
    OSG_HIP(ctx_grow(ctx, ctx->d_mcts_logs, want));
    OSG_HIP(hipMemcpy(ctx->d_mcts_logs, logs.data(), want * sizeof(double), hipMemcpyHostToDevice));
  }
  const double* d_logs = ctx->d_mcts_logs;

  // host-side outputs are staged through scratch
  size_t off = 0;
  auto carve = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
  const size_t o_best = carve(sizeof(int32_t) * n), o_vis = carve(sizeof(int32_t) * n * A),
               o_rew = carve(sizeof(double) * n * A), o_out = carve(static_cast<size_t>(n) * A),
               o_stats = carve(sizeof(double) * n * 4);
  int32_t* d_best = best_action; int32_t* d_vis = child_visits; double* d_rew = child_reward;
  int8_t* d_out = child_outcome; double* d_stats = root_stats;
  if (on_host) {
    void* scratch = nullptr;
    int rc = osg_ctx_scratch(ctx, off, &scratch);
    if (rc) return rc;
    char* sc = static_cast<char*>(scratch);
    d_best = best_action ? reinterpret_cast<int32_t*>(sc + o_best) : nullptr;
    d_vis = child_visits ? reinterpret_cast<int32_t*>(sc + o_vis) : nullptr;
    d_rew = child_reward ? reinterpret_cast<double*>(sc + o_rew) : nullptr;
    d_out = child_outcome ? reinterpret_cast<int8_t*>(sc + o_out) : nullptr;
    d_stats = root_stats ? reinterpret_cast<double*>(sc + o_stats) : nullptr;
  }
  if (layout == 2) {
    MctsOut out{d_best, d_vis, d_rew, d_out, d_stats};
    int rc = launch_mcts_wave(roots, cfg, d_logs, pool, out);
    if (rc) return rc;
  } else {
    const unsigned grid = static_cast<unsigned>((n + kBlockM - 1) / kBlockM);
    // the expansion's shuffle stage: one entry per child of the widest node and lane (two bytes above 255 actions)
    const size_t shuffle_lds = A > 32 * 6 ? 0 : static_cast<size_t>(widest) * kBlockM;   // (HexT<8>, HexT<12> shuffle on the pool)
    if (int rc = with_bool(board, [&](auto brd) {
          return for_game(roots->spec, [&](auto g, const auto& P) {
            using G = typename decltype(g)::type;
            k_mcts<G, decltype(brd)::value><<<dim3(grid), dim3(kBlockM), shuffle_lds, ctx->stream>>>(
                P, static_cast<const typename G::word_t*>(roots->words()), n, d.num_players, A, cfg,
                d.max_utility, d_logs, pool, d_best, d_vis, d_rew, d_out, d_stats);
            return OSG_OK;
          });
        })) return rc;
    OSG_HIP(hipGetLastError());
  }
  if (on_host) {
    if (best_action) OSG_HIP(hipMemcpyAsync(best_action, d_best, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (child_visits) OSG_HIP(hipMemcpyAsync(child_visits, d_vis, sizeof(int32_t) * n * A, hipMemcpyDeviceToHost, ctx->stream));
    if (child_reward) OSG_HIP(hipMemcpyAsync(child_reward, d_rew, sizeof(double) * n * A, hipMemcpyDeviceToHost, ctx->stream));
    if (child_outcome) OSG_HIP(hipMemcpyAsync(child_outcome, d_out, static_cast<size_t>(n) * A, hipMemcpyDeviceToHost, ctx->stream));
    if (root_stats) OSG_HIP(hipMemcpyAsync(root_stats, d_stats, sizeof(double) * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return OSG_OK;
}
