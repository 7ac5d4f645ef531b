// Random play on a batch: random steps with auto-reset, the synthetic benchmark batches and random rollouts
// (osg_random_steps, osg_synth_batch, osg_rollout).  File map: osg_batch_internal.h.
#include <algorithm>

#include "osg_batch_internal.h"

namespace {

// `steps` uniformly random env steps per state with auto-reset, the state in registers throughout.
// Persistent grid (grid-stride over the states).  The two counters are reduced per workgroup and then
// added to one of 64 partial slots — 32 768 same-address atomics (one per wavefront) were measured at
// ~12 ns each, 400 us per launch, dwarfing the steps themselves; k_fold_counters sums the slots.
template <class G>
__global__ void __launch_bounds__(kBlock)
k_random_steps(typename G::Params p, typename G::word_t* base, int64_t n, uint64_t seed, int64_t index_offset,
               int steps, unsigned long long* partials) {
  __shared__ unsigned long long s_sum[2][kBlock / 64];
  unsigned long long applied = 0, episodes = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    typename G::State s = G::load(p, base, n, i);
    Rng rng(seed, static_cast<uint64_t>(index_offset + i), 0);
    for (int t = 0; t < steps; ++t) {
      if (G::terminal(p, s)) {
        s = G::initial(p);
        ++episodes;
      }
      auto m = G::legal(p, s);
      int a = sample_action<G>(p, s, m, G::current_player(p, s), rng);
      G::apply(p, s, a);
      ++applied;
    }
    G::store(p, base, n, i, s);
  }
  unsigned long long a = applied, e = episodes;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off);
    e += __shfl_xor(e, off);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[0][threadIdx.x >> 6] = a;
    s_sum[1][threadIdx.x >> 6] = e;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long ta = 0, te = 0;
    for (int w = 0; w < kBlock / 64; ++w) { ta += s_sum[0][w]; te += s_sum[1][w]; }
    const int slot = blockIdx.x & (kCounterSlots - 1);
    atomicAdd(&partials[2 * slot], ta);
    atomicAdd(&partials[2 * slot + 1], te);
  }
}
// Adds the partial slots into the caller's two counters and clears them for the next launch.
__global__ void __launch_bounds__(64) k_fold_counters(unsigned long long* partials, unsigned long long* counters) {
  const int lane = threadIdx.x;
  unsigned long long a = partials[2 * lane], e = partials[2 * lane + 1];
  partials[2 * lane] = 0;
  partials[2 * lane + 1] = 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off);
    e += __shfl_xor(e, off);
  }
  if (lane == 0) {
    counters[0] += a;
    counters[1] += e;
  }
}

// SURVEY.md 8(d) synthetic inputs on the counter stream, so that the CPU oracle regenerates the very batch a
// benchmark times (oracle/spiel_oracle_capi.cpp osgo_synth_batch restates this loop call for call):
//   rng   = Rng(seed, global index, kSynthSub)
//   depth = rng.below(depth_mod)                                       "d_i = hash(i) mod 36"
//   play `depth` moves from the initial state, chance outcomes by their distribution, player actions
//   uniformly over LegalActions(); a trajectory that ends before `depth` moves is thrown away and
//   re-drawn from the SAME stream ("re-drawn if terminal before d_i"), up to kSynthMaxAttempts times
//   (then the state is the initial state and depth 0: never reached by the configurations served);
//   action = one more draw of the same kind at the accepted, non-terminal state.
// One flat loop per lane, "step, or judge the finished attempt", so lanes on different attempts run the same code.
constexpr uint64_t kSynthSub = 0x53594E5448ULL;  // "SYNTH"
constexpr int kSynthMaxAttempts = 1 << 14;
template <class G>
__global__ void __launch_bounds__(kBlock)
k_synth(typename G::Params p, typename G::word_t* base, int64_t n, uint64_t seed, int64_t index_offset, int depth_mod,
        uint8_t* actions, int32_t* depth_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  Rng rng(seed, static_cast<uint64_t>(index_offset + i), kSynthSub);
  int depth = static_cast<int>(rng.below(static_cast<uint32_t>(depth_mod)));
  typename G::State s = G::initial(p);
  int t = 0, attempt = 0;
  for (;;) {
    const bool term = G::terminal(p, s);
    if (t == depth || term) {
      if (!term) break;                        // accepted
      if (++attempt >= kSynthMaxAttempts) { s = G::initial(p); depth = 0; break; }
      s = G::initial(p);                       // re-draw the whole trajectory from the same stream
      t = 0;
      continue;
    }
    const auto m = G::legal(p, s);
    G::apply(p, s, sample_action<G>(p, s, m, G::current_player(p, s), rng));
    ++t;
  }
  G::store(p, base, n, i, s);
  const auto m = G::legal(p, s);
  const int a = sample_action<G>(p, s, m, G::current_player(p, s), rng);
  if (actions) actions[i] = static_cast<uint8_t>(a);
  if (depth_out) depth_out[i] = depth;
}

// RandomRolloutEvaluator::Evaluate (mcts.cc:43-72), persistent form: every lane owns a strided list of
// work items and runs ONE flat loop whose body is "step the playout, or retire it and start the next", so
// lanes in different phases of different playouts still execute the same instructions.  A work item is
// (root, share j of `group`): the lane plays rollouts j, j + group, j + 2 group, ... of that root back to
// back, adds their returns up in registers and stores the sums into its own slot [root, j]; k_rollout_fold
// then adds the `group` slots of every root in order.  No atomics: the L2 retires only ~2e10 atomics/s
// chip-wide, and one per playout and player was the whole run time of the short games.  Rollout r of
// root i always plays from the counter stream (seed, i, r), whatever the split.
template <class G>
__global__ void __launch_bounds__(kBlock)
k_rollout(typename G::Params p, const typename G::word_t* base, int64_t n, int num_players, uint64_t seed,
          int64_t index_offset, int n_rollouts, int group, double* sum_returns, int32_t* steps_out) {
  const int64_t total = n * group;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (item >= total) return;
  int64_t root = item / group;
  int r = static_cast<int>(item - root * group);  // current rollout of this share
  typename G::State s = G::load(p, base, n, root);
  Rng rng(seed, static_cast<uint64_t>(index_offset + root), static_cast<uint64_t>(r));
  double acc[kMaxPlayers];
#pragma unroll
  for (int q = 0; q < kMaxPlayers; ++q) acc[q] = 0.0;
  int plies = 0, ply = 0;  // moves of this share so far / of the running playout
  for (;;) {
    if (G::terminal(p, s) || ply >= kMaxPlayoutPlies) {
      double ret[kMaxPlayers];
      G::returns(p, s, ret);
#pragma unroll
      for (int q = 0; q < kMaxPlayers; ++q)
        if (q < num_players) acc[q] += ret[q];  // small multiples of 0.5: exact in any order
      r += group;
      if (r >= n_rollouts) {  // this share is done: hand in its sums, fetch the next item
#pragma unroll
        for (int q = 0; q < kMaxPlayers; ++q) {
          if (q < num_players) sum_returns[item * num_players + q] = acc[q];  // slot of (root, share)
          acc[q] = 0.0;
        }
        if (steps_out) steps_out[item] = plies;
        plies = 0;
        item += stride;
        if (item >= total) break;
        root = item / group;
        r = static_cast<int>(item - root * group);
      }
      s = G::load(p, base, n, root);
      rng = Rng(seed, static_cast<uint64_t>(index_offset + root), static_cast<uint64_t>(r));
      ply = 0;
      continue;
    }
    auto m = G::legal(p, s);
    int a = sample_action<G>(p, s, m, G::current_player(p, s), rng);
    G::apply(p, s, a);
    ++plies;
    ++ply;
  }
}

// The same work items for hex when nobody asks for the ply counts (round 6): a playout is HexT::fill_playout_winner —
// the stones placed with the same draws until the board is full, the winner read off by one flood — so every playout of
// a root has the same length and the loop needs no retire / refill phase.  Same sums as k_rollout.
template <class G>
__global__ void __launch_bounds__(kBlock)
k_rollout_hexfill(typename G::Params p, const typename G::word_t* base, int64_t n, uint64_t seed, int64_t index_offset,
                  int n_rollouts, int group, double* sum_returns) {
  const int64_t total = n * group;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; item < total; item += stride) {
    const int64_t root = item / group;
    const typename G::State s = G::load(p, base, n, root);
    double acc = 0.0;
    for (int r = static_cast<int>(item - root * group); r < n_rollouts; r += group) {
      if (G::terminal(p, s)) {   // a finished root: Returns() as it stands
        acc += G::result(s) == 1 ? 1.0 : -1.0;
        continue;
      }
      Rng rng(seed, static_cast<uint64_t>(index_offset + root), static_cast<uint64_t>(r));
      acc += G::fill_playout_winner(p, s, rng) == 0 ? 1.0 : -1.0;
    }
    sum_returns[item * 2] = acc;
    sum_returns[item * 2 + 1] = -acc + 0.0;
  }
}

template <class G>   // (a template so that the discarded branch is not instantiated for the other games)
void launch_rollout_hexfill(const typename G::Params& p, const void* words, int64_t n, uint64_t seed, int64_t index_offset,
                            int n_rollouts, int group, double* d_part, unsigned blocks, hipStream_t st) {
  if constexpr (is_hex<G>::value)
    k_rollout_hexfill<G><<<dim3(blocks), dim3(kBlock), 0, st>>>(p, static_cast<const typename G::word_t*>(words), n, seed,
                                                              index_offset, n_rollouts, group, d_part);
}

// Sums the `group` share slots of every root: sum_returns [n, P] and, optionally, the ply counts [n].
__global__ void __launch_bounds__(kBlock)
k_rollout_fold(const double* __restrict__ part, const int32_t* __restrict__ part_steps, int64_t n, int num_players,
               int group, double* __restrict__ sum_returns, int32_t* __restrict__ steps_out) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;  // (root, player)
  if (k >= n * num_players) return;
  const int64_t root = k / num_players;
  const int q = static_cast<int>(k - root * num_players);
  double v = 0.0;
  for (int j = 0; j < group; ++j) v += part[(root * group + j) * num_players + q];
  sum_returns[k] = v;
  if (steps_out && q == 0) {
    int32_t t = 0;
    for (int j = 0; j < group; ++j) t += part_steps[root * group + j];
    steps_out[root] = t;
  }
}

}  // namespace

extern "C" {

int osg_random_steps(osg_batch* b, uint64_t seed, int64_t index_offset, int steps, unsigned long long* d_counters) {
  osg_ctx* ctx = b->ctx;
  unsigned long long* partials = ctx->d_illegal + 1;
  int64_t blocks = (b->n + kBlock - 1) / kBlock;
  constexpr int64_t kMaxBlocks = 4096;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;  // 16 workgroups per CU (4096 measured 4 % faster than 2048), grid-strided beyond
  if (int rc = for_game(b->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_random_steps<G><<<dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, ctx->stream>>>(P,
            static_cast<typename G::word_t*>(b->words()), b->n, seed, index_offset,
            steps, partials);
        return OSG_OK;
      })) return rc;
  k_fold_counters<<<dim3(1), dim3(64), 0, ctx->stream>>>(partials, d_counters);
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

int osg_synth_batch(osg_batch* b, uint64_t seed, int64_t index_offset, int depth_mod, uint8_t* d_actions,
                    int32_t* d_depth) {
  if (!b) return set_error(OSG_ERR_INVALID, "osg_synth_batch: null batch");
  if (depth_mod < 1 || depth_mod > b->spec.desc.max_game_length)
    return set_error(OSG_ERR_INVALID, "osg_synth_batch: depth_mod must lie in [1, MaxGameLength()]");
  if (int rc = refuse_endless_playouts(b->spec, "osg_synth_batch")) return rc;
  if (d_actions && b->spec.desc.num_distinct_actions > 255)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_synth_batch: d_actions holds one byte per action; pass NULL for games with more "
                                          "than 255 actions");
  osg_ctx* ctx = b->ctx;
  if (int rc = for_game(b->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_synth<G><<<dim3(grid_for(b->n)), dim3(kBlock), 0, ctx->stream>>>(P,
            static_cast<typename G::word_t*>(b->words()), b->n, seed, index_offset, depth_mod,
            d_actions, d_depth);
        return OSG_OK;
      })) return rc;
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

int osg_rollout(const osg_batch* roots, uint64_t seed, int64_t index_offset, int n_rollouts, double* sum_returns,
                int32_t* steps, int on_host) {
  osg_ctx* ctx = roots->ctx;
  const int P_ = roots->spec.desc.num_players;
  const int64_t n = roots->n;
  if (n_rollouts <= 0) return set_error(OSG_ERR_INVALID, "n_rollouts must be positive");
  if (int rc = refuse_endless_playouts(roots->spec, "osg_rollout")) return rc;
  // Lanes per root: enough shares to fill the chip (8 waves per SIMD = 2^19 lanes), no more.
  constexpr int kLanesLog2 = 19;
  int64_t group = ((int64_t{1} << kLanesLog2) + n - 1) / std::max<int64_t>(n, 1);
  if (group > n_rollouts) group = n_rollouts;
  if (group < 1) group = 1;
  // scratch: [sums | steps] when the results go to the host, then the per-share slots when group > 1
  const size_t ret_bytes = sizeof(double) * P_ * n, step_bytes = sizeof(int32_t) * n;
  const size_t off_steps = align_up(ret_bytes), off_part = on_host ? align_up(off_steps + step_bytes) : 0;
  const size_t part_bytes = group > 1 ? ret_bytes * group : 0, off_part_steps = align_up(off_part + part_bytes);
  const size_t scratch_bytes = group > 1 ? off_part_steps + step_bytes * group : (on_host ? off_steps + step_bytes : 0);
  char* scratch = nullptr;
  if (scratch_bytes) {
    void* ptr;
    int rc = osg_ctx_scratch(ctx, scratch_bytes, &ptr);
    if (rc) return rc;
    scratch = static_cast<char*>(ptr);
  }
  double* d_sum = on_host ? reinterpret_cast<double*>(scratch) : sum_returns;
  int32_t* d_steps = steps ? (on_host ? reinterpret_cast<int32_t*>(scratch + off_steps) : steps) : nullptr;
  double* d_part = group > 1 ? reinterpret_cast<double*>(scratch + off_part) : d_sum;
  int32_t* d_part_steps = d_steps ? (group > 1 ? reinterpret_cast<int32_t*>(scratch + off_part_steps) : d_steps) : nullptr;
  const int64_t total = n * group;
  // Persistent grid: at most 8 blocks per CU x 256 CUs, grid-strided beyond that.
  int64_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > 2048) blocks = 2048;
  if (!steps && roots->spec.desc.game_kind == kHex) {
    if (int rc = for_game(roots->spec, [&](auto g, const auto& P) {
          using G = typename decltype(g)::type;
          launch_rollout_hexfill<G>(P, roots->words(), n, seed, index_offset, n_rollouts,
              static_cast<int>(group), d_part, static_cast<unsigned>(blocks), ctx->stream);
          return OSG_OK;
        })) return rc;
  } else {
  if (int rc = for_game(roots->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_rollout<G><<<dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, ctx->stream>>>(P,
            static_cast<const typename G::word_t*>(roots->words()), n, P_, seed,
            index_offset, n_rollouts, static_cast<int>(group), d_part,
            d_part_steps);
        return OSG_OK;
      })) return rc;
  }
  if (group > 1)
    k_rollout_fold<<<dim3(grid_for(n * P_)), dim3(kBlock), 0, ctx->stream>>>(d_part, d_part_steps, n, P_,
                                                                             static_cast<int>(group), d_sum, d_steps);
  OSG_HIP(hipGetLastError());
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(sum_returns, d_sum, ret_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (steps) OSG_HIP(hipMemcpyAsync(steps, d_steps, step_bytes, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return OSG_OK;
}

}  // extern "C"
