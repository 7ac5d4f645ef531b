// NFSP data collection on the device (open_spiel/python/pytorch/nfsp.py with dqn.py, under the loop of
// examples/kuhn_nfsp.py): self-play episodes over the flattened tree against an [I, A] table of Q-network outputs and an
// [I, A] table of average-policy probabilities that are frozen for the call, the DQN transitions they close and the
// supervised rows of the BEST_RESPONSE decisions, a ring of transitions (dqn.ReplayBuffer) and the appends to it and to
// the players' reservoirs (osg_deep_cfr.hip).  The arithmetic is osg_nfsp.h.
//
// Order is the contract.  The reference plays one episode after another and appends one row at a time; here one lane
// plays one episode and stages its rows per player, an exclusive scan of the per-(player, episode) counts gives every
// row the position that loop would have given it in its player's buffer, and the buffers resolve the rows of a call
// that meet in one slot by position: the reservoir with its integer atomicMax, the ring with no atomic at all (row r of
// m stays iff r + capacity >= m).  No floating-point atomics, no dependence on the launch geometry, one host wait per
// call (on the row totals, which size the appends).
//
// Where the tables live: the two [I, A] float32 tables are read once per decision at an address the lanes do not share
// (each episode is somewhere else in the tree), tens of kilobytes that stay in the L2 and mostly in a CU's vector cache.
// k_nfsp_collect<true> copies them to LDS first (OSG_NFSP_TABLES=lds; refused where they do not fit in 64 KB);
// profiles/nfsp_probe.txt has both rates and DESIGN.md section 6 the choice.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "osg_cfr_internal.h"
#include "osg_nfsp.h"

struct osg_transition_ring {
  osg_ctx* ctx = nullptr;
  int64_t capacity = 0, entry_index = 0;
  DeviceArray<int32_t> d_info, d_action, d_next;
  DeviceArray<float> d_reward;
  DeviceArray<uint8_t> d_final;
  // sampling scratch, grow-only
  DeviceArray<uint64_t> d_key_in, d_key_out;
  DeviceArray<int64_t> d_slot_in, d_slot_out;
  DeviceArray<unsigned char> d_tmp;
};

namespace {

constexpr int kThreads = 256;
constexpr size_t kLdsTableBytes = 64 * 1024;
inline unsigned blocks_for(int64_t n) { return static_cast<unsigned>((n + kThreads - 1) / kThreads); }

struct RingRows {   // device pointers, one column each
  int32_t* info;
  int32_t* action;
  float* reward;
  int32_t* next;
  uint8_t* final_;
};

// ---- ring -----------------------------------------------------------------------------------------------------------------
// Rows [r0, m) of the call are the ones that stay (r0 = max(0, m - capacity)): each has its slot to itself.
__global__ void k_ring_commit(RingRows ring, int64_t capacity, int64_t entry0, int64_t m, int64_t r0, RingRows src) {
  const int64_t r = r0 + static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= m || !nfsp_ring_row_stays(r, m, capacity)) return;
  const int64_t slot = nfsp_ring_slot(entry0 + r, capacity);
  ring.info[slot] = src.info[r];
  ring.action[slot] = src.action[r];
  ring.reward[slot] = src.reward[r];
  ring.next[slot] = src.next[r];
  ring.final_[slot] = src.final_[r];
}
__global__ void k_ring_rows(RingRows ring, int64_t capacity, const int64_t* __restrict__ slots, int64_t m, RingRows out) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int64_t slot = slots[j];
  const bool ok = slot >= 0 && slot < capacity;
  if (out.info) out.info[j] = ok ? ring.info[slot] : -1;
  if (out.action) out.action[j] = ok ? ring.action[slot] : -1;
  if (out.reward) out.reward[j] = ok ? ring.reward[slot] : 0.0f;
  if (out.next) out.next[j] = ok ? ring.next[slot] : -1;
  if (out.final_) out.final_[j] = ok ? ring.final_[slot] : 0;
}
__global__ void k_ring_keys(uint64_t* key, int64_t* slot, uint64_t seed, uint64_t stream, int64_t size) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= size) return;
  key[k] = dcfr_sample_key(seed, stream, k);
  slot[k] = k;
}

RingRows rows_of(osg_transition_ring* b) { return RingRows{b->d_info, b->d_action, b->d_reward, b->d_next, b->d_final}; }

int ring_append(osg_transition_ring* b, int64_t m, RingRows src) {
  if (m == 0) return OSG_OK;
  const int64_t r0 = m > b->capacity ? m - b->capacity : 0;
  k_ring_commit<<<dim3(blocks_for(m - r0)), dim3(kThreads), 0, b->ctx->stream>>>(rows_of(b), b->capacity, b->entry_index, m, r0, src);
  OSG_HIP(hipGetLastError());
  b->entry_index += m;
  return OSG_OK;
}

// ---- collection -----------------------------------------------------------------------------------------------------------
struct NfspState {   // what a solver holds for NFSP, built at the first call
  DeviceArray<int32_t> d_legal;     // [I, A] legal action ids, -1 padded
  std::vector<int64_t> bounds;      // per player: the most decisions on one path
  int64_t bound = 1;                // their maximum: rows staged per (player, episode)
  // the last call: staged rows per (player, episode), then compacted in sequence order
  int64_t E = 0, ring_rows = 0, sl_rows = 0;
  DeviceArray<int32_t> st_info, st_action, st_next, st_sl_info, c_info, c_action, c_next, c_sl_info, draws, modes;
  DeviceArray<float> st_reward, st_sl_probs, c_reward, c_sl_probs;
  DeviceArray<uint8_t> st_final, c_final;
  DeviceArray<int64_t> counts, offsets;   // [2, P E] and [2, P E + 1]: transitions, then supervised rows
  DeviceArray<unsigned char> tmp;
  DeviceArray<unsigned int> d_flag;
  PinnedArray<int64_t> h_totals;    // per player: transitions, supervised rows, BEST_RESPONSE episodes; then the flag
};

struct DeviceTree {
  Tree t;
  int P, A;
  OSG_D int kind(int h) const { return t.kind[h]; }
  OSG_D int nchild(int h) const { return t.nchild[h]; }
  OSG_D int child(int h, int c) const { return t.first_child[h] + c; }
  OSG_D double prob(int h) const { return t.edge_prob[h]; }
  OSG_D int info(int h) const { return t.info[h]; }
  OSG_D int actor(int h) const { return t.actor[h]; }
  OSG_D double ret(int h, int p) const { return t.term_ret[h * P + p]; }
};

// The lane's staging ranges: rows [(p E + j) B, + B) of every column.  A row at or beyond the bound raises `bad` and
// is not written.
struct StageSink {
  int64_t E, B, j;
  int A;
  RingRows ring;
  int32_t* sl_info;
  float* sl_probs;
  bool bad = false;
  OSG_D void open(int p, int n, int32_t info, int32_t action) {
    if (n >= B) { bad = true; return; }
    const int64_t at = (p * E + j) * B + n;
    ring.info[at] = info;
    ring.action[at] = action;
  }
  OSG_D void close(int p, int n, float reward, int32_t next, int final_) {
    if (n >= B) { bad = true; return; }
    const int64_t at = (p * E + j) * B + n;
    ring.reward[at] = reward;
    ring.next[at] = next;
    ring.final_[at] = static_cast<uint8_t>(final_);
  }
  OSG_D void supervised(int p, int n, int32_t info, const float* row) {
    if (n >= B) { bad = true; return; }
    const int64_t at = (p * E + j) * B + n;
    sl_info[at] = info;
    for (int a = 0; a < A; ++a) sl_probs[at * A + a] = row[a];
  }
};

// One lane per episode.  kLds: the block first copies q and avg ([I, A] float32 each) to LDS.
template <bool kLds>
__global__ void __launch_bounds__(kThreads)
k_nfsp_collect(Tree t, const int32_t* __restrict__ legal, const float* __restrict__ q, const float* __restrict__ avg, NfspParams prm,
               uint64_t seed, int64_t first, int64_t count, int64_t bound, RingRows st_ring, int32_t* st_sl_info, float* st_sl_probs,
               int64_t* counts, int32_t* draws, int32_t* modes, unsigned int* flag) {
  extern __shared__ __attribute__((aligned(16))) float lds_tables[];
  const float* qt = q;
  const float* at = avg;
  if (kLds) {
    const int n = t.I * t.A;
    for (int x = threadIdx.x; x < n; x += blockDim.x) { lds_tables[x] = q[x]; lds_tables[n + x] = avg[x]; }
    __syncthreads();
    qt = lds_tables;
    at = lds_tables + n;
  }
  const int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const DeviceTree tree{t, t.P, t.A};
  StageSink sink{count, bound, j, t.A, st_ring, st_sl_info, st_sl_probs};
  const NfspEpisode ep = nfsp_episode(tree, legal, qt, at, prm, seed, static_cast<uint64_t>(first + j), sink);
  if (sink.bad) atomicOr(flag, 1u);
  for (int p = 0; p < t.P; ++p) {
    counts[p * count + j] = sink.bad ? 0 : nfsp_rows_of(ep.transitions, p);
    counts[(t.P + p) * count + j] = sink.bad ? 0 : nfsp_rows_of(ep.supervised, p);
  }
  draws[j] = ep.draws;
  modes[j] = static_cast<int32_t>(ep.modes);
}

// Staged rows to their sequence positions: row r of (player, episode) x goes to offsets[x] + r.
__global__ void k_nfsp_compact_ring(const int64_t* __restrict__ counts, const int64_t* __restrict__ offsets, int64_t X, int64_t bound,
                                    RingRows st, RingRows c) {
  const int64_t y = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (y >= X * bound) return;
  const int64_t x = y / bound, r = y % bound;
  if (r >= counts[x]) return;
  const int64_t to = offsets[x] + r;
  c.info[to] = st.info[y];
  c.action[to] = st.action[y];
  c.reward[to] = st.reward[y];
  c.next[to] = st.next[y];
  c.final_[to] = st.final_[y];
}
__global__ void k_nfsp_compact_sl(const int64_t* __restrict__ counts, const int64_t* __restrict__ offsets, int64_t X, int64_t bound,
                                  int A, const int32_t* __restrict__ st_info, const float* __restrict__ st_probs, int32_t* c_info,
                                  float* c_probs) {
  const int64_t y = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (y >= X * bound) return;
  const int64_t x = y / bound, r = y % bound;
  if (r >= counts[x]) return;
  const int64_t to = offsets[x] + r;
  c_info[to] = st_info[y];
  for (int a = 0; a < A; ++a) c_probs[to * A + a] = st_probs[y * A + a];
}
// One workgroup: closes both offset arrays with their totals, counts every player's BEST_RESPONSE episodes (integer adds
// in LDS) and hands the totals and the flag to the host.  totals: [P][3] transitions, supervised rows, BEST_RESPONSE
// episodes; then the flag.
__global__ void __launch_bounds__(kThreads)
k_nfsp_totals(const int64_t* counts, int64_t* offsets, int64_t E, int P, const int32_t* __restrict__ modes, const unsigned int* flag,
              int64_t* totals) {
  __shared__ unsigned long long best[kNfspMaxP];
  if (threadIdx.x < kNfspMaxP) best[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned int mine[kNfspMaxP];
#pragma unroll
  for (int p = 0; p < kNfspMaxP; ++p) mine[p] = 0u;
  for (int64_t j = threadIdx.x; j < E; j += blockDim.x) {
    const uint32_t m = static_cast<uint32_t>(modes[j]);
#pragma unroll
    for (int p = 0; p < kNfspMaxP; ++p) mine[p] += (m >> p) & 1u;
  }
#pragma unroll
  for (int p = 0; p < kNfspMaxP; ++p)
    if (mine[p]) atomicAdd(&best[p], static_cast<unsigned long long>(mine[p]));
  __syncthreads();
  if (threadIdx.x) return;
  const int64_t X = static_cast<int64_t>(P) * E;
  for (int w = 0; w < 2; ++w) offsets[w * (X + 1) + X] = offsets[w * (X + 1) + X - 1] + counts[w * X + X - 1];
  for (int p = 0; p < P; ++p) {
    for (int w = 0; w < 2; ++w) totals[3 * p + w] = offsets[w * (X + 1) + (p + 1) * E] - offsets[w * (X + 1) + p * E];
    totals[3 * p + 2] = static_cast<int64_t>(best[p]);
  }
  totals[3 * P] = *flag;
}

int nfsp_state(osg_cfr* s, NfspState** out) {
  if (!s->nfsp) {
    auto d = std::make_shared<NfspState>();
    hipStream_t st = s->ctx->stream;
    int rc = upload(s->legal, d->d_legal, st);
    if (rc) return rc;
    OSG_HIP(d->d_flag.alloc(1));
    OSG_HIP(d->h_totals.alloc(3 * kNfspMaxP + 1));
    std::vector<int64_t> work(static_cast<size_t>(s->H));
    for (int p = 0; p < s->P; ++p) {
      d->bounds.push_back(nfsp_row_bound(s->H, s->kind.data(), s->nchild.data(), s->actor.data(), p,
                                         [&](int h, int c) { return s->first_child[h] + c; }, work.data()));
      d->bound = std::max(d->bound, d->bounds.back());
    }
    OSG_HIP(hipStreamSynchronize(st));
    s->nfsp = d;
  }
  *out = static_cast<NfspState*>(s->nfsp.get());
  return OSG_OK;
}

bool tables_in_lds() {   // read at every call
  const char* e = getenv("OSG_NFSP_TABLES");
  return e && strcmp(e, "lds") == 0;
}

}  // namespace

extern "C" {

int osg_transition_ring_create(osg_ctx* ctx, int64_t capacity, osg_transition_ring** out) {
  if (!ctx || !out || capacity < 1) return set_error(OSG_ERR_INVALID, "osg_transition_ring_create: bad argument");
  if (capacity >= (int64_t{1} << 31)) return set_error(OSG_ERR_UNSUPPORTED, "osg_transition_ring_create: capacity of 2^31 rows or more");
  auto b = std::make_unique<osg_transition_ring>();
  b->ctx = ctx; b->capacity = capacity;
  int rc;
  const char* who = "osg_transition_ring_create: ";
  if ((rc = nomem_error(b->d_info.alloc(capacity), who)) || (rc = nomem_error(b->d_action.alloc(capacity), who)) ||
      (rc = nomem_error(b->d_reward.alloc(capacity), who)) || (rc = nomem_error(b->d_next.alloc(capacity), who)) ||
      (rc = nomem_error(b->d_final.alloc(capacity), who)))
    return rc;
  OSG_HIP(hipMemsetAsync(b->d_info, 0xFF, sizeof(int32_t) * capacity, ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_action, 0xFF, sizeof(int32_t) * capacity, ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_reward, 0, sizeof(float) * capacity, ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_next, 0xFF, sizeof(int32_t) * capacity, ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_final, 0, sizeof(uint8_t) * capacity, ctx->stream));
  *out = b.release();
  return OSG_OK;
}

int osg_transition_ring_destroy(osg_transition_ring* ring) {
  if (!ring) return OSG_OK;
  (void)hipStreamSynchronize(ring->ctx->stream);
  delete ring;
  return OSG_OK;
}

int osg_transition_ring_sizes(osg_transition_ring* ring, int64_t* size, int64_t* entry_index, int64_t* capacity) {
  if (!ring) return set_error(OSG_ERR_INVALID, "osg_transition_ring_sizes: null argument");
  if (size) *size = std::min(ring->entry_index, ring->capacity);
  if (entry_index) *entry_index = ring->entry_index;
  if (capacity) *capacity = ring->capacity;
  return OSG_OK;
}

int osg_transition_ring_clear(osg_transition_ring* ring) {
  if (!ring) return set_error(OSG_ERR_INVALID, "osg_transition_ring_clear: null argument");
  ring->entry_index = 0;   // the rows stay, the count starts again
  return OSG_OK;
}

int osg_transition_ring_append(osg_transition_ring* ring, int64_t m, const int32_t* d_info, const int32_t* d_action,
                               const float* d_reward, const int32_t* d_next_info, const uint8_t* d_final) {
  if (!ring || m < 0 || (m > 0 && (!d_info || !d_action || !d_reward || !d_next_info || !d_final)))
    return set_error(OSG_ERR_INVALID, "osg_transition_ring_append: bad argument");
  return ring_append(ring, m, RingRows{const_cast<int32_t*>(d_info), const_cast<int32_t*>(d_action), const_cast<float*>(d_reward),
                                       const_cast<int32_t*>(d_next_info), const_cast<uint8_t*>(d_final)});
}

int osg_transition_ring_rows(osg_transition_ring* ring, const int64_t* d_slots, int64_t m, int32_t* d_info, int32_t* d_action,
                             float* d_reward, int32_t* d_next_info, uint8_t* d_final) {
  if (!ring || m < 0 || (m > 0 && !d_slots)) return set_error(OSG_ERR_INVALID, "osg_transition_ring_rows: bad argument");
  if (m == 0) return OSG_OK;
  k_ring_rows<<<dim3(blocks_for(m)), dim3(kThreads), 0, ring->ctx->stream>>>(rows_of(ring), ring->capacity, d_slots, m,
                                                                            RingRows{d_info, d_action, d_reward, d_next_info, d_final});
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

int osg_transition_ring_sample(osg_transition_ring* ring, uint64_t seed, uint64_t stream, int64_t m, int64_t* d_slots) {
  if (!ring || m < 1 || !d_slots) return set_error(OSG_ERR_INVALID, "osg_transition_ring_sample: bad argument");
  const int64_t size = std::min(ring->entry_index, ring->capacity);
  if (m > size) return set_error(OSG_ERR_INVALID, "osg_transition_ring_sample: more rows asked for than the ring holds");
  hipStream_t st = ring->ctx->stream;
  OSG_HIP(ring->d_key_in.ensure(size));
  OSG_HIP(ring->d_key_out.ensure(size));
  OSG_HIP(ring->d_slot_in.ensure(size));
  OSG_HIP(ring->d_slot_out.ensure(size));
  k_ring_keys<<<dim3(blocks_for(size)), dim3(kThreads), 0, st>>>(ring->d_key_in, ring->d_slot_in, seed, stream, size);
  size_t bytes = 0;
  OSG_HIP(rocprim::radix_sort_pairs(nullptr, bytes, ring->d_key_in.get(), ring->d_key_out.get(), ring->d_slot_in.get(),
                                    ring->d_slot_out.get(), static_cast<size_t>(size), 0u, 64u, st));
  OSG_HIP(ring->d_tmp.ensure(bytes));
  OSG_HIP(rocprim::radix_sort_pairs(ring->d_tmp.get(), bytes, ring->d_key_in.get(), ring->d_key_out.get(), ring->d_slot_in.get(),
                                    ring->d_slot_out.get(), static_cast<size_t>(size), 0u, 64u, st));
  OSG_HIP(hipMemcpyAsync(d_slots, ring->d_slot_out.get(), sizeof(int64_t) * m, hipMemcpyDeviceToDevice, st));
  return OSG_OK;
}

int osg_nfsp_collect(osg_cfr* s, const float* d_q, const float* d_avg_probs, const double* eps, const double* anticipatory,
                     uint64_t seed, int64_t first_episode, int64_t episodes, osg_transition_ring* const* rings,
                     osg_reservoir* const* reservoirs, int64_t* totals) {
  if (!s || !d_q || !d_avg_probs || !eps || !anticipatory || episodes < 0 || first_episode < 0)
    return set_error(OSG_ERR_INVALID, "osg_nfsp_collect: bad argument");
  int rc = deep_supported(s, "osg_nfsp_collect");
  if (rc) return rc;
  const int P = s->P, A = s->A;
  if (P > kNfspMaxP) return set_error(OSG_ERR_UNSUPPORTED, "osg_nfsp_collect: more than 8 players");
  for (int p = 0; p < P; ++p) {
    if (rings && rings[p] && rings[p]->ctx != s->ctx) return set_error(OSG_ERR_INVALID, "osg_nfsp_collect: a ring of another context");
    if (reservoirs && reservoirs[p] && !reservoir_serves(reservoirs[p], s))
      return set_error(OSG_ERR_INVALID, "osg_nfsp_collect: a reservoir of another row width or context");
  }
  NfspState* d = nullptr;
  if ((rc = nfsp_state(s, &d))) return rc;
  const int64_t E = episodes, B = d->bound, X = static_cast<int64_t>(P) * E;
  if (B > kNfspMaxRows) return set_error(OSG_ERR_UNSUPPORTED, "osg_nfsp_collect: more than 15 decisions of one player on a path");
  if (X * B >= (int64_t{1} << 31) - 1) return set_error(OSG_ERR_UNSUPPORTED, "osg_nfsp_collect: 2^31 rows or more in one call");
  const bool lds = tables_in_lds();
  const size_t lds_bytes = lds ? 2 * sizeof(float) * static_cast<size_t>(s->I) * A : 0;
  if (lds_bytes > kLdsTableBytes) return set_error(OSG_ERR_UNSUPPORTED, "osg_nfsp_collect: the tables do not fit in 64 KB of LDS");
  hipStream_t st = s->ctx->stream;
  d->E = E; d->ring_rows = d->sl_rows = 0;
  if (totals) std::fill(totals, totals + 4 * P, int64_t{0});
  if (E == 0) return OSG_OK;
  NfspParams prm{};
  for (int p = 0; p < P; ++p) { prm.eps[p] = eps[p]; prm.anticipatory[p] = anticipatory[p]; }
  const size_t rows = static_cast<size_t>(X * B);
  OSG_HIP(d->st_info.ensure(rows)); OSG_HIP(d->st_action.ensure(rows)); OSG_HIP(d->st_reward.ensure(rows));
  OSG_HIP(d->st_next.ensure(rows)); OSG_HIP(d->st_final.ensure(rows));
  OSG_HIP(d->st_sl_info.ensure(rows)); OSG_HIP(d->st_sl_probs.ensure(rows * A));
  OSG_HIP(d->c_info.ensure(rows)); OSG_HIP(d->c_action.ensure(rows)); OSG_HIP(d->c_reward.ensure(rows));
  OSG_HIP(d->c_next.ensure(rows)); OSG_HIP(d->c_final.ensure(rows));
  OSG_HIP(d->c_sl_info.ensure(rows)); OSG_HIP(d->c_sl_probs.ensure(rows * A));
  OSG_HIP(d->counts.ensure(2 * X));
  OSG_HIP(d->offsets.ensure(2 * (X + 1)));
  OSG_HIP(d->draws.ensure(E));
  OSG_HIP(d->modes.ensure(E));
  OSG_HIP(hipMemsetAsync(d->d_flag, 0, sizeof(unsigned int), st));
  const RingRows st_ring{d->st_info, d->st_action, d->st_reward, d->st_next, d->st_final};
  const RingRows c_ring{d->c_info, d->c_action, d->c_reward, d->c_next, d->c_final};
  if (lds)
    k_nfsp_collect<true><<<dim3(blocks_for(E)), dim3(kThreads), lds_bytes, st>>>(
        s->tree(), d->d_legal, d_q, d_avg_probs, prm, seed, first_episode, E, B, st_ring, d->st_sl_info, d->st_sl_probs, d->counts,
        d->draws, d->modes, d->d_flag);
  else
    k_nfsp_collect<false><<<dim3(blocks_for(E)), dim3(kThreads), 0, st>>>(
        s->tree(), d->d_legal, d_q, d_avg_probs, prm, seed, first_episode, E, B, st_ring, d->st_sl_info, d->st_sl_probs, d->counts,
        d->draws, d->modes, d->d_flag);
  OSG_HIP(hipGetLastError());
  for (int w = 0; w < 2; ++w) {
    int64_t* in = d->counts.get() + w * X;
    int64_t* out = d->offsets.get() + w * (X + 1);
    size_t bytes = 0;
    OSG_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, int64_t{0}, static_cast<size_t>(X), rocprim::plus<int64_t>(), st));
    OSG_HIP(d->tmp.ensure(bytes));
    OSG_HIP(rocprim::exclusive_scan(d->tmp.get(), bytes, in, out, int64_t{0}, static_cast<size_t>(X), rocprim::plus<int64_t>(), st));
  }
  k_nfsp_totals<<<dim3(1), dim3(kThreads), 0, st>>>(d->counts, d->offsets, E, P, d->modes, d->d_flag, d->h_totals);
  k_nfsp_compact_ring<<<dim3(blocks_for(X * B)), dim3(kThreads), 0, st>>>(d->counts, d->offsets, X, B, st_ring, c_ring);
  k_nfsp_compact_sl<<<dim3(blocks_for(X * B)), dim3(kThreads), 0, st>>>(d->counts.get() + X, d->offsets.get() + (X + 1), X, B, A,
                                                                        d->st_sl_info, d->st_sl_probs, d->c_sl_info, d->c_sl_probs);
  OSG_HIP(hipGetLastError());
  OSG_HIP(hipStreamSynchronize(st));   // the row totals size the appends
  if (d->h_totals[3 * P]) {
    d->E = 0;
    return set_error(OSG_ERR_INVALID, "osg_nfsp_collect: an episode passed its row bound (internal error)");
  }
  int64_t ring_at = 0, sl_at = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t m = d->h_totals[3 * p], ms = d->h_totals[3 * p + 1], best = d->h_totals[3 * p + 2];
    if (rings && rings[p] &&
        (rc = ring_append(rings[p], m, RingRows{d->c_info.get() + ring_at, d->c_action.get() + ring_at, d->c_reward.get() + ring_at,
                                                d->c_next.get() + ring_at, d->c_final.get() + ring_at})))
      return rc;
    if (reservoirs && reservoirs[p] &&
        (rc = reservoir_append(reservoirs[p], ms, d->c_sl_info.get() + sl_at, 0, d->c_sl_probs.get() + sl_at * A)))
      return rc;
    if (totals) { totals[4 * p] = m; totals[4 * p + 1] = ms; totals[4 * p + 2] = ms + best; totals[4 * p + 3] = m + E; }
    ring_at += m;
    sl_at += ms;
  }
  d->ring_rows = ring_at;
  d->sl_rows = sl_at;
  s->last_kernel = lds ? "k_nfsp_collect<lds>" : "k_nfsp_collect";
  return OSG_OK;
}

int osg_nfsp_staged(osg_cfr* s, int64_t* sizes, int64_t* d_ring_offsets, int32_t* d_ring_info, int32_t* d_ring_action,
                    float* d_ring_reward, int32_t* d_ring_next_info, uint8_t* d_ring_final, int64_t* d_sl_offsets,
                    int32_t* d_sl_info, float* d_sl_probs, int32_t* d_draws, int32_t* d_modes) {
  if (!s) return set_error(OSG_ERR_INVALID, "osg_nfsp_staged: null argument");
  NfspState* d = static_cast<NfspState*>(s->nfsp.get());
  if (sizes) {
    sizes[0] = d ? d->E : 0; sizes[1] = d ? d->ring_rows : 0; sizes[2] = d ? d->sl_rows : 0; sizes[3] = d ? d->bound : 0;
    for (int p = 0; p < s->P && p < kNfspMaxP; ++p) sizes[4 + p] = d ? d->bounds[p] : 0;
  }
  if (!d || d->E == 0) return OSG_OK;
  hipStream_t st = s->ctx->stream;
  const int64_t X = static_cast<int64_t>(s->P) * d->E;
  const int A = s->A;
  auto copy = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
  };
  OSG_HIP(copy(d_ring_offsets, d->offsets.get(), sizeof(int64_t) * (X + 1)));
  OSG_HIP(copy(d_sl_offsets, d->offsets.get() + (X + 1), sizeof(int64_t) * (X + 1)));
  OSG_HIP(copy(d_ring_info, d->c_info.get(), sizeof(int32_t) * d->ring_rows));
  OSG_HIP(copy(d_ring_action, d->c_action.get(), sizeof(int32_t) * d->ring_rows));
  OSG_HIP(copy(d_ring_reward, d->c_reward.get(), sizeof(float) * d->ring_rows));
  OSG_HIP(copy(d_ring_next_info, d->c_next.get(), sizeof(int32_t) * d->ring_rows));
  OSG_HIP(copy(d_ring_final, d->c_final.get(), sizeof(uint8_t) * d->ring_rows));
  OSG_HIP(copy(d_sl_info, d->c_sl_info.get(), sizeof(int32_t) * d->sl_rows));
  OSG_HIP(copy(d_sl_probs, d->c_sl_probs.get(), sizeof(float) * d->sl_rows * A));
  OSG_HIP(copy(d_draws, d->draws.get(), sizeof(int32_t) * d->E));
  OSG_HIP(copy(d_modes, d->modes.get(), sizeof(int32_t) * d->E));
  return OSG_OK;
}

}  // extern "C"
