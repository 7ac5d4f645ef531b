// Information-set MCTS (python/algorithms/ismcts.py ISMCTSBot with RandomRolloutEvaluator) for a batch of kuhn_poker or
// leduc_poker roots: the search of osg_ismcts.h, one root per lane.
//
// Mapping: ONE LANE PER ROOT.  A search is one chain of dependent simulations over one tree, so the unit of parallelism
// is the root, as in the lane-per-root MCTS and the alpha-beta search; every root runs the same number of simulations,
// so a lane keeps its root (and takes the next one `lanes` further on) instead of drawing tickets.  Blocks are single
// wavefronts: 2^14 roots are 256 blocks, one per compute unit, where blocks of 256 would leave three quarters idle.
//
// Node table: in the context's own workspace (kept until the next search, so that osg_ismcts_tree_* can read the trees),
// node-major / lane-minor in 8-byte words — word w of node i of lane l at [(i * W + w) * lanes + l] — like the alpha-beta
// stack, so the lanes of a wavefront that touch the same word of their nodes touch consecutive addresses.  Behind it the
// hash (32-bit slots, slot-major / lane-minor) and the kept root samples.  DESIGN.md section 5e has the sizes and
// section 13 the placements considered.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "osg_internal.h"
#include "osg_ismcts.h"

using namespace osg;

namespace {

constexpr int kIsBlock = 64;
constexpr int kIsWavesPerCu = 8;                         // the grid's cap: what is resident at the kernel's 2 wavefronts per SIMD
constexpr size_t kIsWorkspaceBudget = size_t{8} << 30;   // a large table lowers the lane count, never the table
constexpr int kIsMaxNodes = 1 << 24;                     // a path entry holds the node index in 24 bits

template <class G>
constexpr bool ismcts_served() { return std::is_same<G, Kuhn>::value || std::is_same<G, Leduc>::value; }

// The table of osg_ismcts.h in HBM.  Stores outside the table are dropped (the search never makes one: the host
// instantiation runs it over accessors that abort there).
struct IsHbmTable {
  uint64_t* nodes;     // + lane
  uint32_t* slots;     // + lane
  uint64_t* samples;   // + lane
  int64_t lanes;
  int words, max_nodes, sample_slots, sample_words;
  uint32_t hash_slots;
  OSG_D uint64_t node(int i, int w) const { return nodes[(static_cast<int64_t>(i) * words + w) * lanes]; }
  OSG_D void set_node(int i, int w, uint64_t v) {
    if (static_cast<unsigned>(i) < static_cast<unsigned>(max_nodes)) nodes[(static_cast<int64_t>(i) * words + w) * lanes] = v;
  }
  OSG_D uint32_t slot(uint32_t h) const { return slots[static_cast<int64_t>(h) * lanes]; }
  OSG_D void set_slot(uint32_t h, uint32_t v) {
    if (h < hash_slots) slots[static_cast<int64_t>(h) * lanes] = v;
  }
  OSG_D uint64_t sample(int i, int w) const { return samples[(static_cast<int64_t>(i) * sample_words + w) * lanes]; }
  OSG_D void set_sample(int i, int w, uint64_t v) {
    if (static_cast<unsigned>(i) < static_cast<unsigned>(sample_slots)) samples[(static_cast<int64_t>(i) * sample_words + w) * lanes] = v;
  }
};

struct IsOutputs {   // device addresses; any but draws / count may be null
  double* policy;
  int32_t* sampled_action;
  int32_t* child_visits;
  double* child_return_sum;
  int32_t* expansion_rank;
  int32_t* nodes;
  uint8_t* status;
  uint32_t* draws;   // the workspace's own
  int32_t* count;
};

// The first root that is not a decision node: 2 * row + (1 if terminal) into *first, by minimum.
template <class G>
__global__ void __launch_bounds__(256)
k_ismcts_check(typename G::Params p, const typename G::word_t* base, int64_t n, unsigned long long* first) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= n) return;
  const typename G::State s = G::load(p, base, n, r);
  const int cur = G::current_player(p, s);
  if (cur < 0) atomicMin(first, 2ull * static_cast<unsigned long long>(r) + (cur == kTerminalPlayer ? 1ull : 0ull));
}

template <class G>
__global__ void __launch_bounds__(kIsBlock)
k_ismcts(typename G::Params p, const typename G::word_t* base, int64_t n, IsConfig cfg, uint64_t seed, int64_t index_offset,
         uint64_t* node_words, uint32_t* slot_words, uint64_t* sample_words, int sample_slots, int actions, IsOutputs out) {
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * kIsBlock;
  const int64_t lane = static_cast<int64_t>(blockIdx.x) * kIsBlock + threadIdx.x;
  IsHbmTable table{node_words + lane, slot_words + lane, sample_words + lane, lanes, kIsNodeHead + IsRules<G>::kWords,
                   cfg.max_nodes, sample_slots, IsRules<G>::kWords, cfg.hash_slots};
  for (int64_t r = lane; r < n; r += lanes) {
    IsResult res;
    ismcts_search<G>(p, G::load(p, base, n, r), cfg, seed, static_cast<uint64_t>(index_offset + r), table, &res);
    // (static selects over the three entries: a runtime index would put the result in scratch memory)
#pragma unroll
    for (int a = 0; a < kIsActions; ++a) {
      if (a < actions) {
        if (out.policy) out.policy[r * actions + a] = res.policy[a];
        if (out.child_visits) out.child_visits[r * actions + a] = res.visits[a];
        if (out.child_return_sum) out.child_return_sum[r * actions + a] = res.return_sum[a];
        if (out.expansion_rank) out.expansion_rank[r * actions + a] = res.rank[a];
      }
    }
    if (out.sampled_action) out.sampled_action[r] = res.sampled_action;
    if (out.nodes) out.nodes[r] = res.nodes;
    if (out.status) out.status[r] = static_cast<uint8_t>(res.status);
    out.draws[r] = res.draws;
    out.count[r] = res.nodes;
  }
}

int game_node_cap(const GameSpec& spec) {   // no more information states than this exist (0: no bound worth using)
  if (spec.desc.game_kind != kKuhn) return 0;
  const int P = spec.desc.num_players;   // (P + 1) cards x at most 2^(2P-1) bettings
  return (P + 1) << (2 * P - 1);
}

int check_kept(const osg_batch* roots, const char* who) {
  if (!roots) return set_error(OSG_ERR_INVALID, std::string(who) + ": null argument");
  const IsmctsKept& k = roots->ctx->ismcts;
  if (k.n == 0 || k.n != roots->n || k.game != roots->spec.desc.canonical)
    return set_error(OSG_ERR_INVALID, std::string(who) + ": the context's last osg_ismcts_search was not over a batch of this game and size");
  return OSG_OK;
}

}  // namespace

extern "C" int osg_ismcts_search(const osg_batch* roots, const osg_ismcts_cfg* cfg_in, double* policy, int32_t* sampled_action,
                                 int32_t* child_visits, double* child_return_sum, int32_t* expansion_rank, int32_t* nodes,
                                 uint8_t* status, int on_host) {
  if (!roots || !cfg_in) return set_error(OSG_ERR_INVALID, "osg_ismcts_search: null argument");
  osg_ctx* ctx = roots->ctx;
  const osg_game_desc& d = roots->spec.desc;
  if (d.game_kind != kKuhn && d.game_kind != kLeduc)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_ismcts_search: information-set MCTS serves kuhn_poker and leduc_poker "
                                          "(the perfect-information games have osg_mcts_search)");
  if (d.num_players > kIsPlayers)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_ismcts_search: kuhn_poker and leduc_poker are searched with 2 or 3 players");
  // the leduc_poker parameters change what the search leans on (rank-keyed nodes and the resampler's "never my rank"
  // with suit_isomorphism, three legal actions and tied children with action_mapping, who owns the first level with
  // starting_player) and no run of the reference on them is recorded: refused until one is
  if (d.game_kind == kLeduc && (roots->spec.leduc.iso || roots->spec.leduc.mapping || roots->spec.leduc.starter != 0))
    return set_error(OSG_ERR_UNSUPPORTED, std::string("osg_ismcts_search: leduc_poker is searched with its default rules; ") +
                                              (roots->spec.leduc.iso ? "suit_isomorphism=True" : roots->spec.leduc.mapping ? "action_mapping=True" : "starting_player != 0") +
                                              " is not served (no recorded run of the reference pins it)");
  if (cfg_in->max_simulations < 1 || cfg_in->n_rollouts < 1)
    return set_error(OSG_ERR_INVALID, "osg_ismcts_cfg: max_simulations and n_rollouts must be >= 1");
  if (cfg_in->final_policy_type < 1 || cfg_in->final_policy_type > 3)
    return set_error(OSG_ERR_INVALID, "osg_ismcts_cfg.final_policy_type must be 1 (NORMALIZED_VISITED_COUNT), 2 (MAX_VISIT_COUNT) or 3 (MAX_VALUE)");
  if (cfg_in->child_selection_policy < 1 || cfg_in->child_selection_policy > 2)
    return set_error(OSG_ERR_INVALID, "osg_ismcts_cfg.child_selection_policy must be 1 (UCT) or 2 (PUCT)");
  if (cfg_in->max_nodes > kIsMaxNodes) return set_error(OSG_ERR_INVALID, "osg_ismcts_cfg.max_nodes must be at most 2^24");
  if (!std::isfinite(cfg_in->uct_c)) return set_error(OSG_ERR_INVALID, "osg_ismcts_cfg.uct_c must be finite");
  IsConfig cfg{cfg_in->uct_c, cfg_in->max_simulations, cfg_in->n_rollouts, cfg_in->max_world_samples, cfg_in->final_policy_type,
               cfg_in->child_selection_policy, cfg_in->max_nodes, 0u};
  if (cfg.max_nodes <= 0) {   // auto: a simulation creates at most one node
    const int cap = game_node_cap(roots->spec);
    cfg.max_nodes = std::min(cfg.max_simulations, kIsMaxNodes);
    if (cap > 0) cfg.max_nodes = std::min(cfg.max_nodes, cap);
  }
  cfg.hash_slots = is_hash_slots(cfg.max_nodes);
  const int sample_slots = is_sample_slots(cfg);
  const int64_t n = roots->n;
  ctx->ismcts.n = 0;   // whatever happens below, the trees of an earlier search are gone
  if (n == 0) return OSG_OK;
  if (ctx->num_cus == 0) {
    hipDeviceProp_t prop;
    OSG_HIP(hipGetDeviceProperties(&prop, ctx->device));
    ctx->num_cus = prop.multiProcessorCount;
  }
  const int A = d.num_distinct_actions;

  return for_game(roots->spec, [&](auto g, const auto& P) -> int {
    using G = typename decltype(g)::type;
    if constexpr (!ismcts_served<G>()) {
      return set_error(OSG_ERR_UNSUPPORTED, "osg_ismcts_search: no search for this game layout");
    } else {
      using R = IsRules<G>;
      const auto* base = static_cast<const typename G::word_t*>(roots->words());
      // every root a decision node?
      void* scratch = nullptr;
      size_t off = 0;
      auto carve = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
      const size_t o_first = carve(sizeof(unsigned long long)), o_policy = carve(on_host && policy ? sizeof(double) * n * A : 0),
                   o_sum = carve(on_host && child_return_sum ? sizeof(double) * n * A : 0),
                   o_visits = carve(on_host && child_visits ? sizeof(int32_t) * n * A : 0),
                   o_rank = carve(on_host && expansion_rank ? sizeof(int32_t) * n * A : 0),
                   o_action = carve(on_host && sampled_action ? sizeof(int32_t) * n : 0),
                   o_nodes = carve(on_host && nodes ? sizeof(int32_t) * n : 0), o_status = carve(on_host && status ? static_cast<size_t>(n) : 0);
      if (int rc = osg_ctx_scratch(ctx, off, &scratch)) return rc;
      char* sc = static_cast<char*>(scratch);
      auto* d_first = reinterpret_cast<unsigned long long*>(sc + o_first);
      OSG_HIP(hipMemsetAsync(d_first, 0xFF, sizeof(unsigned long long), ctx->stream));
      k_ismcts_check<G><<<dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(P, base, n, d_first);
      OSG_HIP(hipGetLastError());
      unsigned long long first = 0;
      OSG_HIP(hipMemcpyAsync(&first, d_first, sizeof(first), hipMemcpyDeviceToHost, ctx->stream));
      OSG_HIP(hipStreamSynchronize(ctx->stream));
      if (first != ~0ull)
        return set_error(OSG_ERR_INVALID, "osg_ismcts_search: root " + std::to_string(first >> 1) +
                         ((first & 1ull) ? " is terminal" : " is a chance node") + ": a search starts at a decision node");

      // the workspace: per root the draws and the node count, then the lanes' tables
      const int W = kIsNodeHead + R::kWords;
      const size_t per_lane = static_cast<size_t>(cfg.max_nodes) * W * 8 + static_cast<size_t>(cfg.hash_slots) * 4 +
                              static_cast<size_t>(sample_slots) * R::kWords * 8;
      int64_t blocks = std::min<int64_t>((n + kIsBlock - 1) / kIsBlock, static_cast<int64_t>(ctx->num_cus) * kIsWavesPerCu);
      blocks = std::min<int64_t>(blocks, static_cast<int64_t>(kIsWorkspaceBudget / (per_lane * kIsBlock)));
      if (blocks < 1) return set_error(OSG_ERR_NOMEM, "osg_ismcts_search: a table of max_nodes nodes per root does not fit the workspace");
      const int64_t lanes = blocks * kIsBlock;
      size_t woff = 0;
      auto wcarve = [&](size_t bytes) { size_t o = woff; woff += align_up(bytes); return o; };
      const size_t o_draws = wcarve(sizeof(uint32_t) * n), o_count = wcarve(sizeof(int32_t) * n),
                   o_table = wcarve(static_cast<size_t>(cfg.max_nodes) * W * 8 * lanes),
                   o_slots = wcarve(static_cast<size_t>(cfg.hash_slots) * 4 * lanes),
                   o_samples = wcarve(static_cast<size_t>(sample_slots) * R::kWords * 8 * lanes);
      if (int rc = nomem_error(ctx_grow(ctx, ctx->d_ismcts, woff), "IS-MCTS workspace: ")) return rc;
      char* ws = reinterpret_cast<char*>(ctx->d_ismcts.get());
      IsOutputs out;
      out.policy = on_host && policy ? reinterpret_cast<double*>(sc + o_policy) : policy;
      out.child_return_sum = on_host && child_return_sum ? reinterpret_cast<double*>(sc + o_sum) : child_return_sum;
      out.child_visits = on_host && child_visits ? reinterpret_cast<int32_t*>(sc + o_visits) : child_visits;
      out.expansion_rank = on_host && expansion_rank ? reinterpret_cast<int32_t*>(sc + o_rank) : expansion_rank;
      out.sampled_action = on_host && sampled_action ? reinterpret_cast<int32_t*>(sc + o_action) : sampled_action;
      out.nodes = on_host && nodes ? reinterpret_cast<int32_t*>(sc + o_nodes) : nodes;
      out.status = on_host && status ? reinterpret_cast<uint8_t*>(sc + o_status) : status;
      out.draws = reinterpret_cast<uint32_t*>(ws + o_draws);
      out.count = reinterpret_cast<int32_t*>(ws + o_count);
      k_ismcts<G><<<dim3(static_cast<unsigned>(blocks)), dim3(kIsBlock), 0, ctx->stream>>>(
          P, base, n, cfg, cfg_in->seed, cfg_in->index_offset, reinterpret_cast<uint64_t*>(ws + o_table),
          reinterpret_cast<uint32_t*>(ws + o_slots), reinterpret_cast<uint64_t*>(ws + o_samples), sample_slots, A, out);
      OSG_HIP(hipGetLastError());
      IsmctsKept& kept = ctx->ismcts;
      kept.n = n;
      kept.lanes = lanes;
      kept.max_nodes = cfg.max_nodes;
      kept.node_words = W;
      kept.o_draws = o_draws;
      kept.o_count = o_count;
      kept.o_table = o_table;
      kept.game = d.canonical;
      if (on_host) {
        auto back = [&](void* dst, const void* src, size_t bytes) {
          return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
        };
        OSG_HIP(back(policy, out.policy, sizeof(double) * n * A));
        OSG_HIP(back(child_return_sum, out.child_return_sum, sizeof(double) * n * A));
        OSG_HIP(back(child_visits, out.child_visits, sizeof(int32_t) * n * A));
        OSG_HIP(back(expansion_rank, out.expansion_rank, sizeof(int32_t) * n * A));
        OSG_HIP(back(sampled_action, out.sampled_action, sizeof(int32_t) * n));
        OSG_HIP(back(nodes, out.nodes, sizeof(int32_t) * n));
        OSG_HIP(back(status, out.status, static_cast<size_t>(n)));
        OSG_HIP(hipStreamSynchronize(ctx->stream));
      }
      return OSG_OK;
    }
  });
}

extern "C" int osg_ismcts_tree_sizes(const osg_batch* roots, int32_t* h_nodes, int64_t* h_draws) {
  if (int rc = check_kept(roots, "osg_ismcts_tree_sizes")) return rc;
  osg_ctx* ctx = roots->ctx;
  const IsmctsKept& k = ctx->ismcts;
  const char* ws = reinterpret_cast<const char*>(ctx->d_ismcts.get());
  std::vector<uint32_t> draws(static_cast<size_t>(k.n));
  if (h_nodes) OSG_HIP(hipMemcpyAsync(h_nodes, ws + k.o_count, sizeof(int32_t) * k.n, hipMemcpyDeviceToHost, ctx->stream));
  if (h_draws) OSG_HIP(hipMemcpyAsync(draws.data(), ws + k.o_draws, sizeof(uint32_t) * k.n, hipMemcpyDeviceToHost, ctx->stream));
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  if (h_draws) std::copy(draws.begin(), draws.end(), h_draws);
  return OSG_OK;
}

extern "C" int osg_ismcts_tree_download(const osg_batch* roots, int64_t root, int64_t cap, osg_batch* states, int32_t* h_player,
                                        int32_t* h_total_visits, int32_t* h_visits, double* h_return_sum, int32_t* h_rank) {
  if (int rc = check_kept(roots, "osg_ismcts_tree_download")) return rc;
  osg_ctx* ctx = roots->ctx;
  const IsmctsKept& k = ctx->ismcts;
  if (root < 0 || root >= k.n) return set_error(OSG_ERR_INVALID, "osg_ismcts_tree_download: root out of range");
  if (k.n > k.lanes)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_ismcts_tree_download: the search ran " + std::to_string(k.n) + " roots on " +
                     std::to_string(k.lanes) + " lanes, so a lane's table holds the last of its roots only; search fewer roots per call");
  const char* ws = reinterpret_cast<const char*>(ctx->d_ismcts.get());
  int32_t count = 0;
  OSG_HIP(hipMemcpyAsync(&count, ws + k.o_count + sizeof(int32_t) * root, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  if (count > cap) return set_error(OSG_ERR_INVALID, "osg_ismcts_tree_download: the tree has " + std::to_string(count) + " nodes, cap is " + std::to_string(cap));
  if (count == 0) return OSG_OK;
  const int W = k.node_words, SW = W - kIsNodeHead;
  if (states && (states->ctx != ctx || states->n < count || k.game != states->spec.desc.canonical))
    return set_error(OSG_ERR_INVALID, "osg_ismcts_tree_download: `states` must be a batch of the roots' game and context with a row per node");
  std::vector<uint64_t> words(static_cast<size_t>(count) * W);
  OSG_HIP(hipMemcpy2DAsync(words.data(), 8, ws + k.o_table + 8 * root, static_cast<size_t>(k.lanes) * 8, 8, static_cast<size_t>(count) * W,
                           hipMemcpyDeviceToHost, ctx->stream));
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<uint64_t> plane(static_cast<size_t>(count));
  for (int32_t i = 0; i < count; ++i) {
    const uint64_t* w = &words[static_cast<size_t>(i) * W];
    const uint32_t order = static_cast<uint32_t>(w[1] >> 32);
    if (h_player) h_player[i] = static_cast<int32_t>(w[3] >> 32);
    if (h_total_visits) h_total_visits[i] = static_cast<int32_t>(static_cast<uint32_t>(w[1]));
    for (int a = 0; a < kIsActions; ++a) {
      if (h_visits) h_visits[i * kIsActions + a] = static_cast<int32_t>(a == 0 ? static_cast<uint32_t>(w[2]) : (a == 1 ? w[2] >> 32 : static_cast<uint32_t>(w[3])));
      if (h_return_sum) std::memcpy(&h_return_sum[i * kIsActions + a], &w[4 + a], 8);
      if (h_rank) h_rank[i * kIsActions + a] = is_child_rank(order, a);
    }
  }
  if (states) {
    for (int s = 0; s < SW; ++s) {
      for (int32_t i = 0; i < count; ++i) plane[i] = words[static_cast<size_t>(i) * W + kIsNodeHead + s];
      OSG_HIP(hipMemcpyAsync(static_cast<uint64_t*>(states->words()) + static_cast<size_t>(s) * states->n, plane.data(),
                             sizeof(uint64_t) * count, hipMemcpyHostToDevice, ctx->stream));
      OSG_HIP(hipStreamSynchronize(ctx->stream));   // `plane` is reused
    }
  }
  return OSG_OK;
}
