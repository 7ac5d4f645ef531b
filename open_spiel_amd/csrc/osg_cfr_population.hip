// Payoff-tensor cells and policy aggregation for a population of policy tables on the flattened tree (policy_value,
// expected_game_score.py:35-58; PolicyAggregator.aggregate, policy_aggregator.py:130-265): the arithmetic is
// osg_population.h's.
//   k_pop_plans      one thread per (table, infostate): the row of the table's realization plan, own reach x policy
//   k_pop_returns    one workgroup of four wavefronts per tile of up to kPopTile profiles (fewer per tile while the
//                    tiles would not fill the device twice over).  The terminals pass through LDS in
//                    chunks of kPopChunk: a chunk's plan indices, chance products and returns are staged ONCE per tile,
//                    every thread forms its terminal's weight for each profile of the tile (P gathers from the plans,
//                    which stay in L2), the wavefronts add their 64 terms by shuffles and one thread per (profile,
//                    player) adds the chunk's sum to its total: chunks in ascending order.  No floating-point atomics.
//   k_pop_aggregate  one thread per infostate row: the members in member order, the tables ascending per member
//   k_pop_check_*    on_host = 0 only: the value checks the host cannot make without waiting.  They raise the call's
//                    `refused` word, which makes the kernels behind them write nothing, and the pinned copy of it that
//                    the next population call on the solver reports.
// One form each: a profile's returns are its own workgroup-local sum whatever else the call holds, so their bits depend
// on the game and the profile's P tables alone.
#include "osg_cfr_internal.h"
#include "osg_population.h"

namespace {

constexpr int kPopThreads = kPopChunk;   // k_pop_returns: a terminal of the chunk per thread
constexpr int kPopTile = 8;              // profiles per workgroup at the most
constexpr int kPopRowThreads = 256;
// The limits of a call: sizes beyond them are refused, nothing grows without bound.
constexpr int64_t kPopMaxProfiles = int64_t{1} << 22;        // per call
constexpr size_t kPopMaxStackBytes = size_t{1} << 30;        // n_tables * I * Amax * 8 (the plans take as much again)
static_assert(kPopTile * kMaxPlayers <= kPopThreads, "one accumulating thread per (profile of the tile, player)");

struct PopReturns {
  int T, P, n_tables;
  size_t IA;
  const int32_t* term_seq;
  const double* term_chance;
  const double* term_ret;
  const double* plans;       // [n_tables, I, A]
  const int32_t* profiles;   // [n_profiles, P]
  int64_t n_profiles;
  int tile;                  // profiles per workgroup, 1 .. kPopTile
  double* returns;           // [n_profiles, P]
  const unsigned int* refused;
};

struct PopAggregate {
  const int32_t* path_off;
  const int32_t* path;
  const double* tables;      // [n_tables, I, A]
  int n_tables;
  const double* weights;     // [P, n_tables]
  double epsilon;
  double* out;               // [I, A]
  const unsigned int* refused;
};

__global__ void __launch_bounds__(kPopRowThreads) k_pop_check_profiles(const int32_t* profiles, int64_t n, int n_tables,
                                                                       unsigned int* refused, unsigned int* h_refused) {
  const int64_t x = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (x >= n) return;
  if (profiles[x] < 0 || profiles[x] >= n_tables) { *refused = 1u; *h_refused = 1u; }
}
__global__ void __launch_bounds__(kPopRowThreads) k_pop_check_weights(const double* weights, int n, unsigned int* refused,
                                                                      unsigned int* h_refused) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n) return;
  const double w = weights[x];
  if (!(w >= 0.0) || w > 1.7976931348623157e308) { *refused = 1u; *h_refused = 2u; }
}

__global__ void __launch_bounds__(kPopRowThreads) k_pop_plans(Tree t, const int32_t* path_off, const int32_t* path,
                                                              const double* tables, int n_tables, double* plans) {
  const int64_t x = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (x >= static_cast<int64_t>(n_tables) * t.I) return;
  const int k = static_cast<int>(x / t.I), i = static_cast<int>(x % t.I);
  const size_t IA = static_cast<size_t>(t.I) * t.A;
  const double* pol = tables + k * IA;
  const int m0 = t.mem_off[i];
  const double own = t.mem_off[i + 1] > m0 ? pop_own_reach(path, path_off[m0], path_off[m0 + 1], t.info_player[i], pol, 1.0) : 0.0;
  pop_plan_row(own, pol + static_cast<size_t>(i) * t.A, t.nact[i], t.A, plans + k * IA + static_cast<size_t>(i) * t.A);
}

__global__ void __launch_bounds__(kPopThreads) k_pop_returns(PopReturns c) {
  __shared__ int32_t s_seq[kPopChunk * kMaxPlayers];
  __shared__ double s_ret[kPopChunk * kMaxPlayers];
  __shared__ double s_chance[kPopChunk];
  __shared__ double s_wave[kPopThreads / 64][kPopTile * kMaxPlayers];
  __shared__ int32_t s_table[kPopTile * kMaxPlayers];
  if (*c.refused) return;   // (uniform)
  const int P = c.P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * c.tile;
  const int tile = static_cast<int>(c.n_profiles - m0 < c.tile ? c.n_profiles - m0 : c.tile);
  if (tid < tile * P) {   // (an index the checks let through is in range; the clamp keeps every gather inside the plans regardless)
    const int k = c.profiles[m0 * P + tid];
    s_table[tid] = k < 0 ? 0 : (k >= c.n_tables ? c.n_tables - 1 : k);
  }
  double total = 0.0;   // thread j * P + q: player q's return under profile j of the tile
  for (int t0 = 0; t0 < c.T; t0 += kPopChunk) {
    const int here = c.T - t0 < kPopChunk ? c.T - t0 : kPopChunk;
    for (int x = tid; x < here * P; x += kPopThreads) {
      s_seq[x] = c.term_seq[static_cast<size_t>(t0) * P + x];
      s_ret[x] = c.term_ret[static_cast<size_t>(t0) * P + x];
    }
    if (tid < here) s_chance[tid] = c.term_chance[t0 + tid];
    __syncthreads();
    for (int j = 0; j < tile; ++j) {
      double w = 0.0;
      if (tid < here)
        w = pop_terminal_weight(s_chance[tid], s_seq + tid * P, P, [&](int p) { return c.plans + s_table[j * P + p] * c.IA; });
      for (int q = 0; q < P; ++q) {
        double sum = tid < here ? pop_return_term(s_ret[tid * P + q], w) : 0.0;
        for (int off = 32; off >= 1; off >>= 1) sum = sum + __shfl_down(sum, off, 64);   // lane 0: pop_wave_sum
        if (lane == 0) s_wave[wave][j * P + q] = sum;
      }
    }
    __syncthreads();
    if (tid < tile * P) total += pop_chunk_sum(s_wave[0][tid], s_wave[1][tid], s_wave[2][tid], s_wave[3][tid]);
  }
  if (tid < tile * P) c.returns[m0 * P + tid] = total;
}

__global__ void __launch_bounds__(kPopRowThreads) k_pop_aggregate(Tree t, PopAggregate c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.I || *c.refused) return;
  const int p = t.info_player[i];
  pop_aggregate_row(i, p, t.nact[i], t.A, t.mem_off[i], t.mem_off[i + 1], c.path_off, c.path, c.tables, c.n_tables,
                    static_cast<size_t>(t.I) * t.A, c.weights + static_cast<size_t>(p) * c.n_tables, c.epsilon,
                    c.out + static_cast<size_t>(i) * t.A);
}

dim3 blocks_of(size_t n, int threads) { return dim3(static_cast<unsigned>(std::max<size_t>((n + threads - 1) / threads, 1))); }

// The terminals' plan indices, chance products and returns: one pass over the histories, parents before children.
int build_population_plan(osg_cfr* s) {
  PopulationPlan& pp = s->population;
  if (pp.built) return OSG_OK;
  const int H = s->H, P = s->P, A = s->A;
  std::vector<int32_t> last(static_cast<size_t>(H) * P, -1), seq;
  std::vector<double> chance(H, 1.0), term_chance, term_ret;
  for (int h = 1; h < H; ++h) {
    const int par = s->parent[h];
    std::copy_n(last.begin() + static_cast<size_t>(par) * P, P, last.begin() + static_cast<size_t>(h) * P);
    chance[h] = chance[par];
    if (s->kind[par] == kChanceNode) chance[h] = chance[par] * s->edge_prob[h];
    else last[static_cast<size_t>(h) * P + s->actor[par]] = s->info[par] * A + s->aidx[h];
  }
  for (int h = 0; h < H; ++h) {
    if (s->kind[h] != kTerminalNode) continue;
    seq.insert(seq.end(), last.begin() + static_cast<size_t>(h) * P, last.begin() + static_cast<size_t>(h + 1) * P);
    term_chance.push_back(chance[h]);
    term_ret.insert(term_ret.end(), s->term_ret.begin() + static_cast<size_t>(h) * P, s->term_ret.begin() + static_cast<size_t>(h + 1) * P);
  }
  const size_t T = term_chance.size();
  OSG_HIP(pp.term_seq.alloc(T * P));
  OSG_HIP(pp.term_chance.alloc(T));
  OSG_HIP(pp.term_ret.alloc(T * P));
  OSG_HIP(pp.refused.alloc(1));
  OSG_HIP(pp.h_refused.alloc(1));
  *pp.h_refused.get() = 0u;
  OSG_HIP(hipMemcpy(pp.term_seq, seq.data(), sizeof(int32_t) * T * P, hipMemcpyHostToDevice));
  OSG_HIP(hipMemcpy(pp.term_chance, term_chance.data(), sizeof(double) * T, hipMemcpyHostToDevice));
  OSG_HIP(hipMemcpy(pp.term_ret, term_ret.data(), sizeof(double) * T * P, hipMemcpyHostToDevice));
  OSG_HIP(hipDeviceGetAttribute(&pp.compute_units, hipDeviceAttributeMultiprocessorCount, s->ctx->device));
  pp.T = static_cast<int>(T);
  pp.built = true;
  return OSG_OK;
}

// What both entry points ask first.  stack_doubles: n_tables * I * A.
int population_call(osg_cfr* s, const char* who, const void* a, const void* b, const void* c, int n_tables, size_t* stack_doubles) {
  const std::string name(who);
  if (!s || !a || !b || !c) return set_error(OSG_ERR_INVALID, name + ": null argument");
  if (n_tables < 1) return set_error(OSG_ERR_INVALID, name + ": n_tables must be at least 1");
  if (!s->path_kernel || s->P > kMaxPlayers)
    return set_error(OSG_ERR_UNSUPPORTED, name + ": the tree's root paths do not fit their codes");
  // the leduc_poker parameters change what the realization plans lean on (unequal chance weights with suit_isomorphism,
  // several own sequences per information state with action_mapping, the owner of the first level with
  // starting_player) and no run of the reference on them is recorded: refused until one is
  if (s->spec.desc.game_kind == kLeduc && (s->spec.leduc.iso || s->spec.leduc.mapping || s->spec.leduc.starter != 0))
    return set_error(OSG_ERR_UNSUPPORTED, name + ": leduc_poker populations are served with its default rules; " +
                                              (s->spec.leduc.iso ? "suit_isomorphism=True" : s->spec.leduc.mapping ? "action_mapping=True" : "starting_player != 0") +
                                              " is not served (no recorded run of the reference pins it)");
  const size_t IA = static_cast<size_t>(s->I) * s->A;
  if (static_cast<size_t>(n_tables) > kPopMaxStackBytes / (sizeof(double) * std::max<size_t>(IA, 1)))
    return set_error(OSG_ERR_UNSUPPORTED, name + ": " + std::to_string(n_tables) + " tables of " + std::to_string(IA) +
                                              " cells exceed the limit of " + std::to_string(kPopMaxStackBytes) + " bytes per table stack");
  if (int rc = build_population_plan(s)) return rc;
  if (const unsigned int why = *s->population.h_refused.get()) {
    *s->population.h_refused.get() = 0u;
    return set_error(OSG_ERR_INVALID, name + ": an earlier on_host = 0 call on this solver was refused on the device and wrote nothing (" +
                                          (why == 1u ? "a profile index outside [0, n_tables)" : "a negative or non-finite weight") + ")");
  }
  *stack_doubles = static_cast<size_t>(n_tables) * IA;
  return OSG_OK;
}

}  // namespace

extern "C" {

int osg_cfr_profile_returns(osg_cfr* s, const double* tables, int n_tables, const int32_t* profiles, int64_t n_profiles,
                            int on_host, double* returns) {
  const char* who = "osg_cfr_profile_returns";
  if (n_profiles < 0) return set_error(OSG_ERR_INVALID, std::string(who) + ": n_profiles is negative");
  if (n_profiles > kPopMaxProfiles)
    return set_error(OSG_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(n_profiles) + " profiles exceed the limit of " +
                                              std::to_string(kPopMaxProfiles) + " per call");
  size_t stack = 0;
  if (int rc = population_call(s, who, tables, profiles, returns, n_tables, &stack)) return rc;
  const int P = s->P;
  const size_t cells = static_cast<size_t>(n_profiles) * P;
  if (on_host)
    for (size_t x = 0; x < cells; ++x)
      if (profiles[x] < 0 || profiles[x] >= n_tables)
        return set_error(OSG_ERR_INVALID, std::string(who) + ": profile " + std::to_string(x / P) + " names table " +
                                              std::to_string(profiles[x]) + " of " + std::to_string(n_tables));
  if (n_profiles == 0) return OSG_OK;
  PopulationPlan& pp = s->population;
  hipStream_t st = s->ctx->stream;
  OSG_HIP(pp.plans.ensure(stack));
  OSG_HIP(hipMemsetAsync(pp.refused, 0, sizeof(unsigned int), st));
  PopReturns c;
  c.T = pp.T; c.P = P; c.n_tables = n_tables; c.IA = static_cast<size_t>(s->I) * s->A;
  c.term_seq = pp.term_seq; c.term_chance = pp.term_chance; c.term_ret = pp.term_ret;
  c.plans = pp.plans; c.n_profiles = n_profiles; c.refused = pp.refused;
  if (on_host) {
    OSG_HIP(pp.tables.ensure(stack));
    OSG_HIP(pp.profiles.ensure(cells));
    OSG_HIP(pp.out.ensure(cells));
    OSG_HIP(hipMemcpyAsync(pp.tables, tables, sizeof(double) * stack, hipMemcpyHostToDevice, st));
    OSG_HIP(hipMemcpyAsync(pp.profiles, profiles, sizeof(int32_t) * cells, hipMemcpyHostToDevice, st));
    tables = pp.tables;
    c.profiles = pp.profiles; c.returns = pp.out;
  } else {
    c.profiles = profiles; c.returns = returns;
    k_pop_check_profiles<<<blocks_of(cells, kPopRowThreads), dim3(kPopRowThreads), 0, st>>>(profiles, static_cast<int64_t>(cells), n_tables,
                                                                                          pp.refused, pp.h_refused);
  }
  k_pop_plans<<<blocks_of(static_cast<size_t>(n_tables) * s->I, kPopRowThreads), dim3(kPopRowThreads), 0, st>>>(
      s->tree(), s->d_path_off, s->d_path, tables, n_tables, pp.plans);
  // The widest tile that still leaves two workgroups per compute unit: a tile saves staging, workgroups fill the device.
  // A profile's sum is its own whatever the tile, so the choice changes no bit.
  c.tile = kPopTile;
  while (c.tile > 1 && (n_profiles + c.tile - 1) / c.tile < 2 * static_cast<int64_t>(pp.compute_units)) c.tile /= 2;
  k_pop_returns<<<blocks_of(static_cast<size_t>(n_profiles), c.tile), dim3(kPopThreads), 0, st>>>(c);
  OSG_HIP(hipGetLastError());
  s->last_eval_kernel = "k_pop_returns";
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(returns, pp.out, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipStreamSynchronize(st));
  }
  return OSG_OK;
}

int osg_cfr_aggregate_policies(osg_cfr* s, const double* tables, int n_tables, const double* weights, double epsilon,
                               int on_host, double* out_table) {
  const char* who = "osg_cfr_aggregate_policies";
  if (!(epsilon >= 0.0)) return set_error(OSG_ERR_INVALID, std::string(who) + ": epsilon must be >= 0");
  size_t stack = 0;
  if (int rc = population_call(s, who, tables, weights, out_table, n_tables, &stack)) return rc;
  if (s->A > kPopMaxActions)
    return set_error(OSG_ERR_UNSUPPORTED, std::string(who) + ": rows of " + std::to_string(s->A) + " actions exceed the limit of " +
                                              std::to_string(kPopMaxActions));
  const size_t IA = static_cast<size_t>(s->I) * s->A, W = static_cast<size_t>(s->P) * n_tables;
  if (on_host)
    for (size_t x = 0; x < W; ++x)
      if (!(weights[x] >= 0.0) || std::isinf(weights[x]))
        return set_error(OSG_ERR_INVALID, std::string(who) + ": weight " + std::to_string(x % n_tables) + " of player " +
                                              std::to_string(x / n_tables) + " is negative or not finite");
  PopulationPlan& pp = s->population;
  hipStream_t st = s->ctx->stream;
  OSG_HIP(hipMemsetAsync(pp.refused, 0, sizeof(unsigned int), st));
  PopAggregate c;
  c.path_off = s->d_path_off; c.path = s->d_path; c.n_tables = n_tables; c.epsilon = epsilon; c.refused = pp.refused;
  if (on_host) {
    OSG_HIP(pp.tables.ensure(stack));
    OSG_HIP(pp.weights.ensure(W));
    OSG_HIP(pp.out.ensure(IA));
    OSG_HIP(hipMemcpyAsync(pp.tables, tables, sizeof(double) * stack, hipMemcpyHostToDevice, st));
    OSG_HIP(hipMemcpyAsync(pp.weights, weights, sizeof(double) * W, hipMemcpyHostToDevice, st));
    c.tables = pp.tables; c.weights = pp.weights; c.out = pp.out;
  } else {
    c.tables = tables; c.weights = weights; c.out = out_table;
    k_pop_check_weights<<<blocks_of(W, kPopRowThreads), dim3(kPopRowThreads), 0, st>>>(weights, static_cast<int>(W), pp.refused, pp.h_refused);
  }
  k_pop_aggregate<<<blocks_of(s->I, kPopRowThreads), dim3(kPopRowThreads), 0, st>>>(s->tree(), c);
  OSG_HIP(hipGetLastError());
  s->last_eval_kernel = "k_pop_aggregate";
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(out_table, pp.out, sizeof(double) * IA, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipStreamSynchronize(st));
  }
  return OSG_OK;
}

}  // extern "C"
