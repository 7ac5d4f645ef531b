// algorithms::AlphaBetaSearch (open_spiel/algorithms/minimax.cc:49-137, 222-256) for a batch of roots: the exact,
// deterministic counterpart of osg_mcts_search for tic_tac_toe, connect_four and hex.
//
// Mapping: ONE LANE PER ROOT, on a persistent grid.  A search is one dependent chain (every cut-off depends on the
// values before it), so the unit of parallelism is the root, as in the lane-per-root MCTS; but tree sizes differ by
// 10^4 between the roots of one batch (a tic_tac_toe position three plies from the end against the empty board), so a
// lane that finishes takes the next root from a ticket counter instead of idling until its wavefront's largest tree
// is done.  Taking a root is one more phase of the loop body of osg_alpha_beta.h (descend / evaluate / return), so the
// lanes of a wavefront stand in different phases of different roots and still run one instruction stream.  A root's
// result depends on its state and the configuration only — not on the lane, the ticket order or the batch order.
//
// Stack: the open frame in registers, its ancestors in a workspace from osg_ctx_scratch laid out ply-major /
// lane-minor in 8-byte words (word w of ply d of lane l at [(d * W + w) * lanes + l]), so the lanes of a wavefront
// that push or pop together touch consecutive words.  DESIGN.md section 13 has the frame sizes and the placements
// considered.
#include <algorithm>

#include "osg_alpha_beta.h"
#include "osg_internal.h"

using namespace osg;

namespace {

constexpr int kAbBlock = 256;
constexpr int kAbWavesPerCu = 8;                       // persistent grid: lanes = CUs x 8 wavefronts x 64
constexpr size_t kAbStackBudget = size_t{1} << 30;     // the workspace of a deep search lowers the lane count, not the depth

template <class G> struct is_c4 : std::false_type {};
template <int R, int C, int K, class BB> struct is_c4<C4T<R, C, K, BB>> : std::true_type {};
template <class G> struct hex_words : std::integral_constant<int, 1> {};
template <int NW> struct hex_words<HexT<NW>> : std::integral_constant<int, NW> {};
// the layouts searched: every tic_tac_toe and connect_four record, hex in the 4-word mask (up to 128 actions)
template <class G>
constexpr bool ab_served() {
  return std::is_same<G, Ttt>::value || is_c4<G>::value || (is_hex<G>::value && G::kMaskW <= kMaskWords);
}

// The rules model of osg_alpha_beta.h over the device rules of osg_game_boards.h.
template <class G>
struct AbRules {
  using State = typename G::State;
  using Todo = MaskT<hex_words<G>::value>;   // one word holds every action of tic_tac_toe (9) and connect_four (<= 32 columns)
  const typename G::Params& p;
  OSG_D bool terminal(const State& s) const { return G::terminal(p, s); }
  // The mover by the position's own count — the parity of the stones (tic_tac_toe.h:127, connect_four.cc:122-128), hex's
  // to-move bit — which a finished position has too: a terminal root under maximizing_player = -1 is valued for it.
  OSG_D int mover(const State& s) const {
    if constexpr (is_hex<G>::value) return G::to_move(s);
    else return G::plies(s) & 1;
  }
  OSG_D double player_return(const State& s, int player) const {
    double r[2];
    G::returns(p, s, r);
    return player == 0 ? r[0] : r[1];
  }
  OSG_D Todo legal(const State& s) const {   // of a state that is not terminal
    Todo t;
    if constexpr (is_c4<G>::value) {
      t.w[0] = G::open_columns(p, s);
    } else {
      const auto m = G::legal(p, s);
#pragma unroll
      for (int k = 0; k < hex_words<G>::value; ++k) t.w[k] = m.w[k];
    }
    return t;
  }
  OSG_D void apply(State& s, int a) const { G::apply(p, s, a); }
  OSG_D static bool todo_any(const Todo& t) { return t.any(); }
  OSG_D static int todo_pop(Todo& t) {   // (static selects: the set stays in registers)
    int a = -1;
    bool found = false;
#pragma unroll
    for (int k = 0; k < hex_words<G>::value; ++k) {
      const bool here = !found && t.w[k] != 0u;
      a = here ? 32 * k + __builtin_ctz(t.w[k]) : a;
      t.w[k] = here ? (t.w[k] & (t.w[k] - 1u)) : t.w[k];
      found |= here;
    }
    return a;
  }
  OSG_D static void todo_clear(Todo& t) {
#pragma unroll
    for (int k = 0; k < hex_words<G>::value; ++k) t.w[k] = 0u;
  }
};

// Frames in HBM, ply-major / lane-minor, as the frame's 8-byte words.
template <class R>
struct AbHbmStack {
  static_assert(sizeof(AbFrame<R>) % 8 == 0, "a frame is a whole number of 8-byte words");
  static constexpr int kWords = static_cast<int>(sizeof(AbFrame<R>) / 8);
  uint64_t* base;   // + lane
  int64_t lanes;
  int plies;
  // (a ply beyond the workspace cannot be reached from a consistent record — a game lasts max_game_length plies —
  // and is never written: the search of an uploaded inconsistent record may be wrong, never out of bounds)
  OSG_D void store(int ply, const AbFrame<R>& f) {
    if (ply >= plies) return;
    uint64_t w[kWords];
    __builtin_memcpy(w, &f, sizeof(f));
#pragma unroll
    for (int k = 0; k < kWords; ++k) base[(static_cast<int64_t>(ply) * kWords + k) * lanes] = w[k];
  }
  OSG_D void load(int ply, AbFrame<R>& f) {
    if (ply >= plies) return;
    uint64_t w[kWords];
#pragma unroll
    for (int k = 0; k < kWords; ++k) w[k] = base[(static_cast<int64_t>(ply) * kWords + k) * lanes];
    __builtin_memcpy(&f, w, sizeof(f));
  }
};

template <class G>
__global__ void __launch_bounds__(kAbBlock)
k_alpha_beta(typename G::Params p, const typename G::word_t* base, int64_t n, AbConfig cfg, unsigned long long* ticket,
             uint64_t* stack_words, int stack_plies, double* value, int32_t* best_action, int64_t* nodes, uint8_t* status) {
  using R = AbRules<G>;
  using Stack = AbHbmStack<R>;
  const R rules{p};
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * kAbBlock;
  const int64_t lane = static_cast<int64_t>(blockIdx.x) * kAbBlock + threadIdx.x;
  Stack stack{stack_words + lane, lanes, stack_plies};
  AbSearch<R, Stack> search;
  search.done = true;
  int64_t r = -1;
  for (;;) {
    if (search.done) {   // hand in the root just finished, take the next
      if (r >= 0) {
        value[r] = search.value;
        best_action[r] = search.best_action;
        nodes[r] = search.nodes;
        status[r] = static_cast<uint8_t>(search.status);
      }
      r = static_cast<int64_t>(atomicAdd(ticket, 1ull));
      if (r >= n) break;
      search.start(rules, G::load(p, base, n, r), cfg);
      continue;
    }
    search.step(rules, stack, cfg);
  }
}

}  // namespace

extern "C" int osg_alpha_beta_search(const osg_batch* roots, const osg_ab_cfg* cfg_in, double* value, int32_t* best_action,
                                     int64_t* nodes, uint8_t* status, int on_host) {
  if (!roots || !cfg_in || !value || !best_action || !nodes || !status)
    return set_error(OSG_ERR_INVALID, "osg_alpha_beta_search: null argument");
  osg_ctx* ctx = roots->ctx;
  const osg_game_desc& d = roots->spec.desc;
  if (d.game_kind == kKuhn || d.game_kind == kLeduc)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_alpha_beta_search: the game must be deterministic (minimax.cc:232); "
                                          "kuhn_poker and leduc_poker have chance nodes");
  if (d.game_kind == kHex && roots->spec.hex_nw > kMaskWords)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_alpha_beta_search: hex is searched on boards of up to 128 cells");
  if (cfg_in->max_nodes <= 0) return set_error(OSG_ERR_INVALID, "osg_ab_cfg.max_nodes must be positive");
  if (cfg_in->maximizing_player < -1 || cfg_in->maximizing_player > 1)
    return set_error(OSG_ERR_INVALID, "osg_ab_cfg.maximizing_player must be -1 (the mover of each root), 0 or 1");
  if (cfg_in->leaf_mode != OSG_AB_LEAF_NONE && cfg_in->leaf_mode != OSG_AB_LEAF_CONSTANT)
    return set_error(OSG_ERR_INVALID, "osg_ab_cfg.leaf_mode must be OSG_AB_LEAF_NONE or OSG_AB_LEAF_CONSTANT");
  const AbConfig cfg{cfg_in->depth_limit, cfg_in->maximizing_player, cfg_in->leaf_mode, cfg_in->leaf_value, cfg_in->max_nodes};
  const int64_t n = roots->n;
  if (n == 0) return OSG_OK;
  if (ctx->num_cus == 0) {
    hipDeviceProp_t prop;
    OSG_HIP(hipGetDeviceProperties(&prop, ctx->device));
    ctx->num_cus = prop.multiProcessorCount;
  }
  // frames pushed: plies 0 .. min(depth_limit, game length) - 2; hex with the swap rule lasts one ply longer than its cells
  const int game_plies = d.max_game_length + 1;
  const int stack_plies = std::max(1, cfg.depth_limit < 0 ? game_plies : std::min(cfg.depth_limit, game_plies));

  return for_game(roots->spec, [&](auto g, const auto& P) -> int {
    using G = typename decltype(g)::type;
    if constexpr (!ab_served<G>()) {
      return set_error(OSG_ERR_UNSUPPORTED, "osg_alpha_beta_search: no search for this game layout");
    } else {
      using Stack = AbHbmStack<AbRules<G>>;
      const size_t per_lane = static_cast<size_t>(stack_plies) * Stack::kWords * 8;
      int64_t blocks = std::min<int64_t>((n + kAbBlock - 1) / kAbBlock, static_cast<int64_t>(ctx->num_cus) * kAbWavesPerCu * 64 / kAbBlock);
      blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, static_cast<int64_t>(kAbStackBudget / (per_lane * kAbBlock))));
      const int64_t lanes = blocks * kAbBlock;
      size_t off = 0;
      auto carve = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
      const size_t o_ticket = carve(sizeof(unsigned long long)), o_stack = carve(per_lane * lanes),
                   o_value = carve(on_host ? sizeof(double) * n : 0), o_nodes = carve(on_host ? sizeof(int64_t) * n : 0),
                   o_best = carve(on_host ? sizeof(int32_t) * n : 0), o_status = carve(on_host ? static_cast<size_t>(n) : 0);
      void* scratch = nullptr;
      if (int rc = osg_ctx_scratch(ctx, off, &scratch)) return rc;
      char* sc = static_cast<char*>(scratch);
      double* d_value = on_host ? reinterpret_cast<double*>(sc + o_value) : value;
      int64_t* d_nodes = on_host ? reinterpret_cast<int64_t*>(sc + o_nodes) : nodes;
      int32_t* d_best = on_host ? reinterpret_cast<int32_t*>(sc + o_best) : best_action;
      uint8_t* d_status = on_host ? reinterpret_cast<uint8_t*>(sc + o_status) : status;
      OSG_HIP(hipMemsetAsync(sc + o_ticket, 0, sizeof(unsigned long long), ctx->stream));
      k_alpha_beta<G><<<dim3(static_cast<unsigned>(blocks)), dim3(kAbBlock), 0, ctx->stream>>>(
          P, static_cast<const typename G::word_t*>(roots->words()), n, cfg,
          reinterpret_cast<unsigned long long*>(sc + o_ticket), reinterpret_cast<uint64_t*>(sc + o_stack), stack_plies,
          d_value, d_best, d_nodes, d_status);
      OSG_HIP(hipGetLastError());
      if (on_host) {
        OSG_HIP(hipMemcpyAsync(value, d_value, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        OSG_HIP(hipMemcpyAsync(best_action, d_best, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
        OSG_HIP(hipMemcpyAsync(nodes, d_nodes, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
        OSG_HIP(hipMemcpyAsync(status, d_status, static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
        OSG_HIP(hipStreamSynchronize(ctx->stream));
      }
      return OSG_OK;
    }
  });
}
