// AlphaZero self-play on the device (alpha_zero_torch/alpha_zero.cc PlayGame for a batch of environments): Dirichlet
// noise for all roots in one launch, policy targets and moves from a search's visit counts, per-environment trajectories
// staged time-major, and a ring of training rows that finished games are appended to.  The arithmetic is osg_selfplay.h.
//
//   k_root_noise        one lane per root: dirichlet_row on the root's prior (the draws parked in a [A, n] scratch plane)
//   k_sp_select<G>      one lane per environment: policy target, move, the ply into the staging area
//   k_sp_apply<G>       one lane per environment: apply the move, find the end of the game and player 0's return
//   k_sp_scan           one workgroup: exclusive sum of the finished games' lengths (no atomics), games / rows of the flush
//   k_sp_scatter        one wavefront per environment: a finished trajectory into its ring slots (lanes over the policy row)
//   k_sp_reset<G>       one lane per environment: finished environments restart; the ring's total_seen advances
//   k_replay_sample / k_replay_policy / k_replay_rows   gathers out of the ring
//
// Layouts.  Ring: the state records in an osg_batch of `capacity` states (plane k at words[k * capacity + slot]), policy
// [capacity, A] f32, value / root_value f32, player i8, action i32.  Staging: an osg_batch of T * n states with ply t of
// environment i at index t * n + i, so that one ply's writes are contiguous; the other fields likewise [T, n(, A)].
// head (device, i64): [0] total_seen, [1] games finished by the last commit, [2] rows it appended, [3] games ever finished.
#include <cmath>
#include <memory>

#include "osg_batch_internal.h"
#include "osg_selfplay.h"

struct osg_replay {
  osg_ctx* ctx = nullptr;
  osg_batch* states = nullptr;   // owned
  int64_t capacity = 0;
  int A = 0;
  DeviceArray<float> d_policy, d_value, d_root_value;
  DeviceArray<int8_t> d_player;
  DeviceArray<int32_t> d_action;
  DeviceArray<int64_t> d_head;
};

struct osg_selfplay {
  osg_ctx* ctx = nullptr;
  osg_batch* envs = nullptr;     // borrowed
  osg_replay* buf = nullptr;     // borrowed
  osg_batch* staging = nullptr;  // owned: T * n states
  osg_selfplay_cfg cfg{};
  int64_t n = 0;
  int T = 0, A = 0;
  DeviceArray<float> d_policy, d_root_value;     // [T, n, A], [T, n]
  DeviceArray<int32_t> d_action;                 // [T, n]
  DeviceArray<int8_t> d_player;                  // [T, n]
  DeviceArray<int32_t> d_len, d_cur_action, d_flen;   // [n]
  DeviceArray<int64_t> d_plyc, d_prefix;         // [n]
  DeviceArray<double> d_cur_root, d_ret0;        // [n]
  DeviceArray<uint8_t> d_finished;               // [n]
};

namespace {

template <class G>
constexpr bool kSelfPlayGame = !std::is_same_v<typename G::Params, Kuhn::Params> && !std::is_same_v<typename G::Params, Leduc::Params>;

int refuse_game(const GameSpec& spec, const char* who) {
  if (spec.desc.game_kind <= kHex && spec.desc.num_players == 2 && spec.desc.max_chance_outcomes == 0) return OSG_OK;
  return set_error(OSG_ERR_UNSUPPORTED, std::string(who) + ": self-play serves the deterministic two-player games (tic_tac_toe, "
                   "connect_four, hex); kuhn_poker and leduc_poker are searched by osg_ismcts_search");
}

__global__ void __launch_bounds__(kBlock)
k_root_noise(double* prior, const uint32_t* mask, int mask_words, const uint8_t* request, int64_t n, int A, double alpha,
             double epsilon, uint64_t seed, int64_t index_offset, uint64_t sub, double* noise) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  if (request && request[i] != 5) return;
  Rng rng(seed, static_cast<uint64_t>(index_offset + i), sub);
  dirichlet_row(prior + i * A, mask + i * mask_words, A, alpha, epsilon, rng, noise + i, n);
}

struct SelectArgs {
  const int32_t* visits;
  const int32_t* best;
  const double* root_value;
  float* policy_out;
  int32_t* action_out;
  // staging
  float* st_policy;
  float* st_root_value;
  int32_t* st_action;
  int8_t* st_player;
  const int32_t* len;
  const int64_t* plyc;
  int32_t* cur_action;
  double* cur_root;
  unsigned long long* illegal;
};

template <class G>
__global__ void __launch_bounds__(kBlock)
k_sp_select(typename G::Params p, const typename G::word_t* env, int64_t n, typename G::word_t* stage, int T, int A,
            osg_selfplay_cfg cfg, SelectArgs x) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const typename G::State s = G::load(p, env, n, i);
  const int t = x.len[i];
  const int32_t* v = x.visits + i * A;
  const bool unit_t = cfg.temperature == 1.0;
  const double inv_t = 1.0 / cfg.temperature;
  const double sum = sp_policy_sum(v, A, inv_t, unit_t);
  if (!(sum > 0.0) || t >= T || G::terminal(p, s)) {   // nothing to learn from and no move to make: counted, not recorded
    x.cur_action[i] = OSG_INVALID_ACTION;
    x.action_out[i] = OSG_INVALID_ACTION;
    if (x.policy_out)
      for (int a = 0; a < A; ++a) x.policy_out[i * A + a] = 0.0f;
    atomicAdd(x.illegal, 1ull);
    return;
  }
  const bool greedy = t >= cfg.temperature_drop;
  double z = 0.0;
  if (!greedy) {
    Rng rng(cfg.seed, static_cast<uint64_t>(cfg.index_offset + i), static_cast<uint64_t>(x.plyc[i]));
    z = rng.unit();
  }
  const int64_t at = static_cast<int64_t>(t) * n + i;
  float* sp = x.st_policy + at * A;
  float* po = x.policy_out ? x.policy_out + i * A : nullptr;
  const int drawn = sp_policy_and_draw(v, A, inv_t, unit_t, sum, !greedy, z, [&](int a, double pr) {
    const float f = static_cast<float>(pr);
    sp[a] = f;
    if (po) po[a] = f;
  });
  const int action = greedy ? x.best[i] : drawn;
  const int64_t rows = static_cast<int64_t>(T) * n;
  for (int k = 0; k < p.words; ++k) stage[k * rows + at] = env[k * n + i];
  x.st_action[at] = action;
  x.st_root_value[at] = static_cast<float>(x.root_value[i]);
  x.st_player[at] = static_cast<int8_t>(G::current_player(p, s));
  x.cur_action[i] = action;
  x.cur_root[i] = x.root_value[i];
  x.action_out[i] = action;
}

template <class G>
__global__ void __launch_bounds__(kBlock)
k_sp_apply(typename G::Params p, typename G::word_t* env, int64_t n, double cutoff_value, const int32_t* cur_action,
           const double* cur_root, int32_t* len, int64_t* plyc, uint8_t* finished, double* ret0, int32_t* flen,
           unsigned long long* illegal) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  finished[i] = 0;
  ret0[i] = 0.0;
  flen[i] = 0;
  const int a = cur_action[i];
  if (a == OSG_INVALID_ACTION) return;   // (select counted it)
  typename G::State s = G::load(p, env, n, i);
  const auto m = G::legal(p, s);
  if (a < 0 || a >= 32 * G::kMaskW || !m.test(a)) {   // a best_action the search did not have: the ply stays unplayed
    atomicAdd(illegal, 1ull);
    return;
  }
  const int mover = G::current_player(p, s);
  G::apply(p, s, a);
  G::store(p, env, n, i, s);
  const int32_t plies = len[i] + 1;
  len[i] = plies;
  plyc[i] += 1;
  if (G::terminal(p, s)) {
    double r[kMaxPlayers];
    G::returns(p, s, r);
    finished[i] = 1; ret0[i] = r[0]; flen[i] = plies;
  } else if (sp_cut_off(cur_root[i], cutoff_value)) {
    finished[i] = 1; ret0[i] = sp_cutoff_return0(cur_root[i], mover); flen[i] = plies;
  }
}

// prefix[i] = sum of flen[j], j < i, and the flush's totals: ONE workgroup; every thread owns a run of consecutive
// environments, the runs' sums are scanned in LDS.
constexpr int kScanBlock = 1024;
__global__ void __launch_bounds__(kScanBlock)
k_sp_scan(const int32_t* flen, const uint8_t* finished, int64_t n, int64_t* prefix, int64_t* head) {
  __shared__ int64_t rows[kScanBlock];
  __shared__ int32_t games[kScanBlock];
  const int tid = threadIdx.x;
  const int64_t run = (n + kScanBlock - 1) / kScanBlock;
  const int64_t lo = tid * run, hi = lo + run < n ? lo + run : n;
  int64_t sum = 0;
  int32_t g = 0;
  for (int64_t i = lo; i < hi; ++i) { sum += flen[i]; g += finished[i]; }
  rows[tid] = sum;
  games[tid] = g;
  __syncthreads();
  for (int step = 1; step < kScanBlock; step <<= 1) {   // Hillis-Steele, inclusive
    const int64_t add_r = tid >= step ? rows[tid - step] : 0;
    const int32_t add_g = tid >= step ? games[tid - step] : 0;
    __syncthreads();
    rows[tid] += add_r;
    games[tid] += add_g;
    __syncthreads();
  }
  int64_t at = rows[tid] - sum;
  for (int64_t i = lo; i < hi; ++i) { prefix[i] = at; at += flen[i]; }
  if (tid == kScanBlock - 1) {
    head[1] = games[tid];
    head[2] = rows[tid];
    head[3] += games[tid];
  }
}

struct RingRows {
  float* policy;
  float* value;
  float* root_value;
  int8_t* player;
  int32_t* action;
  int64_t capacity;
};

template <class W>
__global__ void __launch_bounds__(64)
k_sp_scatter(const W* stage, int64_t n, int T, int words, int A, const float* st_policy, const float* st_root_value,
             const int32_t* st_action, const int8_t* st_player, const uint8_t* finished, const int32_t* flen,
             const int64_t* prefix, const double* ret0, const int64_t* head, W* ring, RingRows r) {
  const int64_t i = blockIdx.x;
  if (!finished[i]) return;
  const int lane = threadIdx.x;
  const int plies = flen[i];
  const int64_t total_seen = head[0], rows = head[2], base = prefix[i];
  const int64_t stage_rows = static_cast<int64_t>(T) * n;
  for (int t = 0; t < plies; ++t) {
    const int64_t g = base + t;
    if (!ring_written(rows, g, r.capacity)) continue;   // overwritten by the same flush in the sequential order
    const int64_t slot = ring_slot(total_seen, g, r.capacity);
    const int64_t at = static_cast<int64_t>(t) * n + i;
    for (int a = lane; a < A; a += 64) r.policy[slot * A + a] = st_policy[at * A + a];
    for (int k = lane; k < words; k += 64) ring[k * r.capacity + slot] = stage[k * stage_rows + at];
    if (lane == 0) {
      r.value[slot] = static_cast<float>(ret0[i]);
      r.root_value[slot] = st_root_value[at];
      r.player[slot] = st_player[at];
      r.action[slot] = st_action[at];
    }
  }
}

template <class G>
__global__ void __launch_bounds__(kBlock)
k_sp_reset(typename G::Params p, typename G::word_t* env, int64_t n, const uint8_t* finished, int32_t* len, int64_t* head) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i == 0) head[0] += head[2];
  if (i >= n || !finished[i]) return;
  G::store(p, env, n, i, G::initial(p));
  len[i] = 0;
}

template <class W>
__global__ void __launch_bounds__(kBlock)
k_replay_sample(const W* ring, int64_t capacity, int words, W* dst, int64_t m, const int64_t* head, uint64_t seed,
                int64_t index_offset, const float* ring_value, float* value, int64_t* index) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= m) return;
  const int64_t size = ring_size(head[0], capacity);
  Rng rng(seed, static_cast<uint64_t>(index_offset + j), 0);
  const int64_t at = rng.below(static_cast<uint32_t>(size));
  index[j] = at;
  for (int k = 0; k < words; ++k) dst[k * m + j] = ring[k * capacity + at];
  if (value) value[j] = ring_value[at];
}

// out[j, a] = ring[index[j], a]: one lane per element
__global__ void __launch_bounds__(kBlock)
k_replay_policy(const float* ring_policy, const int64_t* index, int64_t capacity, int A, int64_t m, float* out) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= m * A) return;
  const int64_t j = e / A;
  const int a = static_cast<int>(e - j * A);
  const int64_t at = index[j];
  out[e] = (at >= 0 && at < capacity) ? ring_policy[at * A + a] : 0.0f;
}

__global__ void __launch_bounds__(kBlock)
k_replay_rows(RingRows r, const int64_t* index, int64_t m, float* value, float* root_value, int8_t* player, int32_t* action,
              unsigned long long* illegal) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= m) return;
  const int64_t at = index[j];
  if (at < 0 || at >= r.capacity) { atomicAdd(illegal, 1ull); return; }
  if (value) value[j] = r.value[at];
  if (root_value) root_value[j] = r.root_value[at];
  if (player) player[j] = r.player[at];
  if (action) action[j] = r.action[at];
}

RingRows ring_rows(const osg_replay* b) {
  return RingRows{b->d_policy, b->d_value, b->d_root_value, b->d_player, b->d_action, b->capacity};
}

// f(word type tag) for the game's record word (u32 or u64)
template <class F>
int with_word(const GameSpec& spec, F&& f) {
  return spec.desc.state_word_bytes == 8 ? f(TypeTag<uint64_t>{}) : f(TypeTag<uint32_t>{});
}

}  // namespace

extern "C" {

int osg_mcts_root_noise(osg_ctx* ctx, double* d_prior, const uint32_t* d_mask, int mask_words, const uint8_t* d_request,
                        int64_t n, int A, double alpha, double epsilon, uint64_t seed, int64_t index_offset, uint64_t sub) {
  if (!ctx || !d_prior || !d_mask || n < 1 || A < 1 || mask_words < 1 || A > 32 * mask_words)
    return set_error(OSG_ERR_INVALID, "osg_mcts_root_noise: bad argument");
  if (!std::isfinite(alpha) || alpha <= 0.0 || !(epsilon >= 0.0 && epsilon <= 1.0))
    return set_error(OSG_ERR_INVALID, "osg_mcts_root_noise: alpha must be finite and > 0, epsilon in [0, 1]");
  void* scratch = nullptr;
  if (int rc = osg_ctx_scratch(ctx, sizeof(double) * static_cast<size_t>(n) * A, &scratch)) return rc;
  k_root_noise<<<dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream>>>(d_prior, d_mask, mask_words, d_request, n, A, alpha, epsilon,
                                                                  seed, index_offset, sub, static_cast<double*>(scratch));
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

int osg_replay_create(osg_ctx* ctx, const char* game_string, int64_t capacity, osg_replay** out) {
  if (!ctx || !game_string || !out) return set_error(OSG_ERR_INVALID, "osg_replay_create: null argument");
  if (capacity < 1 || capacity > 0x7FFFFFFF) return set_error(OSG_ERR_INVALID, "osg_replay_create: capacity must be in [1, 2^31)");
  GameSpec spec;
  if (int rc = parse_game(game_string, &spec)) return rc;
  if (int rc = refuse_game(spec, "osg_replay_create")) return rc;
  auto b = std::make_unique<osg_replay>();
  b->ctx = ctx;
  b->capacity = capacity;
  b->A = spec.desc.num_distinct_actions;
  const size_t cap = static_cast<size_t>(capacity);
  if (int rc = nomem_error(b->d_policy.alloc(cap * b->A), "replay buffer: ")) return rc;
  if (int rc = nomem_error(b->d_value.alloc(cap), "replay buffer: ")) return rc;
  if (int rc = nomem_error(b->d_root_value.alloc(cap), "replay buffer: ")) return rc;
  if (int rc = nomem_error(b->d_player.alloc(cap), "replay buffer: ")) return rc;
  if (int rc = nomem_error(b->d_action.alloc(cap), "replay buffer: ")) return rc;
  if (int rc = nomem_error(b->d_head.alloc(4), "replay buffer: ")) return rc;
  OSG_HIP(hipMemsetAsync(b->d_policy, 0, cap * b->A * sizeof(float), ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_value, 0, cap * sizeof(float), ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_root_value, 0, cap * sizeof(float), ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_player, 0, cap, ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_action, 0, cap * sizeof(int32_t), ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_head, 0, 4 * sizeof(int64_t), ctx->stream));
  if (int rc = osg_batch_create(ctx, game_string, capacity, &b->states)) return rc;
  *out = b.release();
  return OSG_OK;
}

int osg_replay_destroy(osg_replay* buf) {
  if (!buf) return OSG_OK;
  osg_batch_destroy(buf->states);   // (waits for the stream)
  delete buf;
  return OSG_OK;
}

int osg_replay_sizes(osg_replay* buf, int64_t* size, int64_t* total_seen, int64_t* capacity) {
  if (!buf) return set_error(OSG_ERR_INVALID, "osg_replay_sizes: null argument");
  int64_t seen = 0;
  OSG_HIP(hipMemcpyAsync(&seen, buf->d_head.get(), sizeof(seen), hipMemcpyDeviceToHost, buf->ctx->stream));
  OSG_HIP(hipStreamSynchronize(buf->ctx->stream));
  if (size) *size = ring_size(seen, buf->capacity);
  if (total_seen) *total_seen = seen;
  if (capacity) *capacity = buf->capacity;
  return OSG_OK;
}

osg_batch* osg_replay_states(osg_replay* buf) { return buf ? buf->states : nullptr; }

int osg_replay_sample(osg_replay* buf, uint64_t seed, int64_t index_offset, int64_t m, osg_batch* dst_states,
                      float* d_policy, float* d_value, int64_t* d_index) {
  if (!buf || !dst_states) return set_error(OSG_ERR_INVALID, "osg_replay_sample: null argument");
  if (m < 1) return set_error(OSG_ERR_INVALID, "osg_replay_sample: m must be >= 1");
  if (!same_game(dst_states, buf->states) || dst_states->n != m)
    return set_error(OSG_ERR_INVALID, "osg_replay_sample: dst_states must be a batch of the buffer's game and of m states");
  int64_t size = 0;
  if (int rc = osg_replay_sizes(buf, &size, nullptr, nullptr)) return rc;
  if (size < 1) return set_error(OSG_ERR_INVALID, "osg_replay_sample: the buffer is empty");
  osg_ctx* ctx = buf->ctx;
  if (!d_index) {
    void* scratch = nullptr;
    if (int rc = osg_ctx_scratch(ctx, sizeof(int64_t) * static_cast<size_t>(m), &scratch)) return rc;
    d_index = static_cast<int64_t*>(scratch);
  }
  const int words = buf->states->spec.desc.state_words;
  if (int rc = with_word(buf->states->spec, [&](auto w) {
        using W = typename decltype(w)::type;
        k_replay_sample<W><<<dim3(grid_for(m)), dim3(kBlock), 0, ctx->stream>>>(
            static_cast<const W*>(buf->states->words()), buf->capacity, words, static_cast<W*>(dst_states->words()), m,
            buf->d_head, seed, index_offset, buf->d_value, d_value, d_index);
        return OSG_OK;
      })) return rc;
  OSG_HIP(hipGetLastError());
  if (d_policy) {
    k_replay_policy<<<dim3(grid_for(m * buf->A)), dim3(kBlock), 0, ctx->stream>>>(buf->d_policy, d_index, buf->capacity, buf->A, m, d_policy);
    OSG_HIP(hipGetLastError());
  }
  return OSG_OK;
}

int osg_replay_rows(osg_replay* buf, const int64_t* d_index, int64_t m, float* d_policy, float* d_value,
                    float* d_root_value, int8_t* d_player, int32_t* d_action) {
  if (!buf || !d_index || m < 1) return set_error(OSG_ERR_INVALID, "osg_replay_rows: bad argument");
  osg_ctx* ctx = buf->ctx;
  k_replay_rows<<<dim3(grid_for(m)), dim3(kBlock), 0, ctx->stream>>>(ring_rows(buf), d_index, m, d_value, d_root_value, d_player,
                                                                   d_action, ctx->d_illegal);
  OSG_HIP(hipGetLastError());
  if (d_policy) {
    k_replay_policy<<<dim3(grid_for(m * buf->A)), dim3(kBlock), 0, ctx->stream>>>(buf->d_policy, d_index, buf->capacity, buf->A, m, d_policy);
    OSG_HIP(hipGetLastError());
  }
  return OSG_OK;
}

int osg_selfplay_create(osg_batch* envs, osg_replay* buf, const osg_selfplay_cfg* cfg, osg_selfplay** out) {
  if (!envs || !buf || !cfg || !out) return set_error(OSG_ERR_INVALID, "osg_selfplay_create: null argument");
  if (int rc = refuse_game(envs->spec, "osg_selfplay_create")) return rc;
  if (!same_game(envs, buf->states) || envs->ctx != buf->ctx)
    return set_error(OSG_ERR_INVALID, "osg_selfplay_create: environments and replay buffer must share game and context");
  if (!std::isfinite(cfg->temperature) || cfg->temperature <= 0.0)
    return set_error(OSG_ERR_INVALID, "osg_selfplay_create: temperature must be finite and > 0");
  if (std::isnan(cfg->cutoff_value) || cfg->temperature_drop < 0)
    return set_error(OSG_ERR_INVALID, "osg_selfplay_create: cutoff_value must be a number, temperature_drop >= 0");
  auto sp = std::make_unique<osg_selfplay>();
  sp->ctx = envs->ctx;
  sp->envs = envs;
  sp->buf = buf;
  sp->cfg = *cfg;
  sp->n = envs->n;
  sp->T = envs->spec.desc.max_game_length;
  sp->A = envs->spec.desc.num_distinct_actions;
  const size_t n = static_cast<size_t>(sp->n), rows = n * sp->T;
  const char* who = "self-play staging: ";
  if (int rc = nomem_error(sp->d_policy.alloc(rows * sp->A), who)) return rc;
  if (int rc = nomem_error(sp->d_root_value.alloc(rows), who)) return rc;
  if (int rc = nomem_error(sp->d_action.alloc(rows), who)) return rc;
  if (int rc = nomem_error(sp->d_player.alloc(rows), who)) return rc;
  if (int rc = nomem_error(sp->d_len.alloc(n), who)) return rc;
  if (int rc = nomem_error(sp->d_cur_action.alloc(n), who)) return rc;
  if (int rc = nomem_error(sp->d_flen.alloc(n), who)) return rc;
  if (int rc = nomem_error(sp->d_plyc.alloc(n), who)) return rc;
  if (int rc = nomem_error(sp->d_prefix.alloc(n), who)) return rc;
  if (int rc = nomem_error(sp->d_cur_root.alloc(n), who)) return rc;
  if (int rc = nomem_error(sp->d_ret0.alloc(n), who)) return rc;
  if (int rc = nomem_error(sp->d_finished.alloc(n), who)) return rc;
  hipStream_t st = sp->ctx->stream;
  OSG_HIP(hipMemsetAsync(sp->d_len, 0, n * sizeof(int32_t), st));
  OSG_HIP(hipMemsetAsync(sp->d_plyc, 0, n * sizeof(int64_t), st));
  OSG_HIP(hipMemsetAsync(sp->d_cur_action, 0xFF, n * sizeof(int32_t), st));   // OSG_INVALID_ACTION: nothing selected yet
  OSG_HIP(hipMemsetAsync(sp->d_cur_root, 0, n * sizeof(double), st));
  OSG_HIP(hipMemsetAsync(sp->d_finished, 0, n, st));
  OSG_HIP(hipMemsetAsync(sp->d_ret0, 0, n * sizeof(double), st));
  if (int rc = osg_batch_create(sp->ctx, envs->spec.desc.canonical, static_cast<int64_t>(rows), &sp->staging)) return rc;
  *out = sp.release();
  return OSG_OK;
}

int osg_selfplay_destroy(osg_selfplay* sp) {
  if (!sp) return OSG_OK;
  osg_batch_destroy(sp->staging);   // (waits for the stream)
  delete sp;
  return OSG_OK;
}

int osg_selfplay_select(osg_selfplay* sp, const int32_t* d_child_visits, const int32_t* d_best_action,
                        const double* d_root_value, float* d_policy_out, int32_t* d_action_out) {
  if (!sp || !d_child_visits || !d_best_action || !d_root_value || !d_action_out)
    return set_error(OSG_ERR_INVALID, "osg_selfplay_select: null argument");
  osg_ctx* ctx = sp->ctx;
  const SelectArgs x{d_child_visits, d_best_action, d_root_value, d_policy_out, d_action_out, sp->d_policy, sp->d_root_value,
                     sp->d_action, sp->d_player, sp->d_len, sp->d_plyc, sp->d_cur_action, sp->d_cur_root, ctx->d_illegal};
  if (int rc = for_game(sp->envs->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        if constexpr (kSelfPlayGame<G>) {
          k_sp_select<G><<<dim3(grid_for(sp->n)), dim3(kBlock), 0, ctx->stream>>>(
              P, static_cast<const typename G::word_t*>(sp->envs->words()), sp->n,
              static_cast<typename G::word_t*>(sp->staging->words()), sp->T, sp->A, sp->cfg, x);
          return OSG_OK;
        } else {
          return refuse_game(sp->envs->spec, "osg_selfplay_select");
        }
      })) return rc;
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

int osg_selfplay_commit(osg_selfplay* sp, uint8_t* d_finished, double* d_returns, int64_t* h_counts) {
  if (!sp) return set_error(OSG_ERR_INVALID, "osg_selfplay_commit: null argument");
  osg_ctx* ctx = sp->ctx;
  osg_replay* buf = sp->buf;
  hipStream_t st = ctx->stream;
  const int64_t n = sp->n;
  if (int rc = for_game(sp->envs->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        if constexpr (kSelfPlayGame<G>) {
          using W = typename G::word_t;
          k_sp_apply<G><<<dim3(grid_for(n)), dim3(kBlock), 0, st>>>(
              P, static_cast<W*>(sp->envs->words()), n, sp->cfg.cutoff_value, sp->d_cur_action, sp->d_cur_root, sp->d_len,
              sp->d_plyc, sp->d_finished, sp->d_ret0, sp->d_flen, ctx->d_illegal);
          k_sp_scan<<<dim3(1), dim3(kScanBlock), 0, st>>>(sp->d_flen, sp->d_finished, n, sp->d_prefix, buf->d_head);
          k_sp_scatter<W><<<dim3(static_cast<unsigned>(n)), dim3(64), 0, st>>>(
              static_cast<const W*>(sp->staging->words()), n, sp->T, P.words, sp->A, sp->d_policy, sp->d_root_value, sp->d_action,
              sp->d_player, sp->d_finished, sp->d_flen, sp->d_prefix, sp->d_ret0, buf->d_head,
              static_cast<W*>(buf->states->words()), ring_rows(buf));
          k_sp_reset<G><<<dim3(grid_for(n)), dim3(kBlock), 0, st>>>(P, static_cast<W*>(sp->envs->words()), n, sp->d_finished,
                                                                   sp->d_len, buf->d_head);
          return OSG_OK;
        } else {
          return refuse_game(sp->envs->spec, "osg_selfplay_commit");
        }
      })) return rc;
  OSG_HIP(hipGetLastError());
  // one selection is played once: a commit without a new select moves nothing
  OSG_HIP(hipMemsetAsync(sp->d_cur_action, 0xFF, static_cast<size_t>(n) * sizeof(int32_t), st));
  if (d_finished) OSG_HIP(hipMemcpyAsync(d_finished, sp->d_finished.get(), static_cast<size_t>(n), hipMemcpyDeviceToDevice, st));
  if (d_returns) OSG_HIP(hipMemcpyAsync(d_returns, sp->d_ret0.get(), static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (h_counts) {
    OSG_HIP(hipMemcpyAsync(h_counts, buf->d_head.get() + 1, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    OSG_HIP(hipStreamSynchronize(st));
  }
  return OSG_OK;
}

int osg_selfplay_staged(osg_selfplay* sp, int t, osg_batch* dst_states, float* d_policy, int32_t* d_action,
                        float* d_root_value, int8_t* d_player, int32_t* d_length, int64_t* d_ply_counter) {
  if (!sp || t < 0 || t >= sp->T) return set_error(OSG_ERR_INVALID, "osg_selfplay_staged: bad argument");
  hipStream_t st = sp->ctx->stream;
  const size_t n = static_cast<size_t>(sp->n), at = static_cast<size_t>(t) * n;
  if (dst_states) {
    if (!same_game(dst_states, sp->envs) || dst_states->n != sp->n)
      return set_error(OSG_ERR_INVALID, "osg_selfplay_staged: dst_states must be a batch of the game and of n states");
    const size_t wb = sp->envs->spec.desc.state_word_bytes, rows = n * sp->T;
    const char* src = static_cast<const char*>(sp->staging->words());
    char* dst = static_cast<char*>(dst_states->words());
    for (int k = 0; k < sp->envs->spec.desc.state_words; ++k)
      OSG_HIP(hipMemcpyAsync(dst + k * n * wb, src + (k * rows + at) * wb, n * wb, hipMemcpyDeviceToDevice, st));
  }
  if (d_policy) OSG_HIP(hipMemcpyAsync(d_policy, sp->d_policy.get() + at * sp->A, n * sp->A * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (d_action) OSG_HIP(hipMemcpyAsync(d_action, sp->d_action.get() + at, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (d_root_value) OSG_HIP(hipMemcpyAsync(d_root_value, sp->d_root_value.get() + at, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (d_player) OSG_HIP(hipMemcpyAsync(d_player, sp->d_player.get() + at, n, hipMemcpyDeviceToDevice, st));
  if (d_length) OSG_HIP(hipMemcpyAsync(d_length, sp->d_len.get(), n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (d_ply_counter) OSG_HIP(hipMemcpyAsync(d_ply_counter, sp->d_plyc.get(), n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  return OSG_OK;
}

}  // extern "C"
