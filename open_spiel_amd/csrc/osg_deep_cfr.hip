// Deep CFR on the device (open_spiel/python/pytorch/deep_cfr.py): the infostate tensors of a flattened tree, reservoir
// buffers of (infostate, iteration, values) rows, and _traverse_game_tree x trajectories against an [I, A] table of
// advantage-network outputs that is frozen for the call.  The arithmetic is osg_deep_cfr.h.
//
// Order is the contract.  The reference appends one row at a time; here every row of a call gets the sequence position
// the reference would have given it — trajectories in index order, a trajectory's advantage rows post-order, its
// strategy rows pre-order — by an exclusive scan of the per-trajectory counts, and the reservoir resolves the rows of a
// call that meet in one slot by position (the last one wins, as a sequential loop leaves it): an integer atomicMax per
// slot, then a copy by the winners.  No floating-point atomics, no dependence on the launch geometry.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "osg_cfr_internal.h"
#include "osg_deep_cfr.h"

struct osg_reservoir {
  osg_ctx* ctx = nullptr;
  int A = 0;
  int64_t capacity = 0, add_calls = 0;
  uint64_t seed = 0, stream = 0;
  DeviceArray<int32_t> d_info, d_iter;
  DeviceArray<float> d_vals;
  DeviceArray<unsigned int> d_winner;   // [capacity] 1 + the position of the call's last row for the slot; zero between calls
  // sampling scratch, grow-only
  DeviceArray<uint64_t> d_key_in, d_key_out;
  DeviceArray<int64_t> d_slot_in, d_slot_out;
  DeviceArray<unsigned char> d_tmp;
};

namespace {

constexpr int kThreads = 256;
inline unsigned blocks_for(int64_t n) { return static_cast<unsigned>((n + kThreads - 1) / kThreads); }

// ---- reservoir ------------------------------------------------------------------------------------------------------------
__global__ void k_res_claim(unsigned int* winner, uint64_t seed, uint64_t stream, int64_t add0, int64_t capacity, int64_t m) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int64_t slot = dcfr_reservoir_slot(seed, stream, add0 + r, capacity);
  if (slot >= 0) atomicMax(&winner[slot], static_cast<unsigned int>(r) + 1u);
}
__global__ void k_res_commit(unsigned int* winner, int32_t* info, int32_t* iter, float* vals, int A, uint64_t seed,
                             uint64_t stream, int64_t add0, int64_t capacity, int64_t m, const int32_t* __restrict__ src_info,
                             int32_t iteration, const float* __restrict__ src_vals) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int64_t slot = dcfr_reservoir_slot(seed, stream, add0 + r, capacity);
  if (slot < 0 || winner[slot] != static_cast<unsigned int>(r) + 1u) return;   // only the winner sees its own mark
  info[slot] = src_info[r];
  iter[slot] = iteration;
  for (int a = 0; a < A; ++a) vals[slot * A + a] = src_vals[r * A + a];
  winner[slot] = 0u;
}
__global__ void k_res_rows(const int32_t* info, const int32_t* iter, const float* vals, int A, int64_t capacity,
                           const int64_t* __restrict__ slots, int64_t m, int32_t* o_info, int32_t* o_iter, float* o_vals) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int64_t slot = slots[j];
  const bool ok = slot >= 0 && slot < capacity;
  if (o_info) o_info[j] = ok ? info[slot] : -1;
  if (o_iter) o_iter[j] = ok ? iter[slot] : 0;
  if (o_vals)
    for (int a = 0; a < A; ++a) o_vals[j * A + a] = ok ? vals[slot * A + a] : 0.0f;
}
__global__ void k_res_keys(uint64_t* key, int64_t* slot, uint64_t seed, uint64_t stream, int64_t size) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= size) return;
  key[k] = dcfr_sample_key(seed, stream, k);
  slot[k] = k;
}

}  // namespace

namespace osg_cfr_impl {
bool reservoir_serves(const osg_reservoir* b, const osg_cfr* s) { return b->A == s->A && b->ctx == s->ctx; }

int reservoir_append(osg_reservoir* b, int64_t m, const int32_t* d_info, int32_t iteration, const float* d_values) {
  if (m == 0) return OSG_OK;
  hipStream_t st = b->ctx->stream;
  k_res_claim<<<dim3(blocks_for(m)), dim3(kThreads), 0, st>>>(b->d_winner, b->seed, b->stream, b->add_calls, b->capacity, m);
  k_res_commit<<<dim3(blocks_for(m)), dim3(kThreads), 0, st>>>(b->d_winner, b->d_info, b->d_iter, b->d_vals, b->A, b->seed,
                                                               b->stream, b->add_calls, b->capacity, m, d_info, iteration,
                                                               d_values);
  OSG_HIP(hipGetLastError());
  b->add_calls += m;
  return OSG_OK;
}
}  // namespace osg_cfr_impl

namespace {

// ---- traversal ------------------------------------------------------------------------------------------------------------
struct DeepState {   // what a solver holds for Deep CFR, built at the first call
  DeviceArray<int32_t> d_legal;       // [I, A] legal action ids, -1 padded
  DeviceArray<double> d_strategy;     // [I, A] by action id: the launch's strategy table
  std::vector<DcfrBounds> bounds;     // per traverser
  // the last call: staged rows per trajectory, then compacted in sequence order
  int64_t T = 0, adv_bound = 0, strat_bound = 0, adv_rows = 0, strat_rows = 0;
  DeviceArray<int32_t> st_adv_info, st_strat_info, c_adv_info, c_strat_info, draws;
  DeviceArray<float> st_adv_vals, st_strat_vals, c_adv_vals, c_strat_vals;
  DeviceArray<int64_t> counts, offsets;   // [2, T] and [2, T + 1]
  DeviceArray<unsigned char> tmp;
  DeviceArray<unsigned int> d_flag;
  PinnedArray<int64_t> h_totals;      // adv rows, strat rows, flag
};

__global__ void k_dcfr_strategy(const float* __restrict__ adv, const int32_t* __restrict__ legal, const int32_t* __restrict__ nact,
                                int I, int A, double* strategy) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  float row[kDcfrMaxA];
  int32_t ids[kDcfrMaxA];
  double p[kDcfrMaxA];
  for (int a = 0; a < A; ++a) { row[a] = adv[i * A + a]; ids[a] = legal[i * A + a]; }
  dcfr_strategy(row, ids, nact[i], A, p);
  for (int a = 0; a < A; ++a) strategy[i * A + a] = p[a];
}

// One lane per trajectory (k_mccfr's frame stack).  Rows go to the lane's own staging ranges, within the exact bounds
// the host computed from the tree; a lane that would pass one raises the flag and writes nothing more.
__global__ void __launch_bounds__(kThreads)
k_dcfr_traverse(Tree t, const int32_t* __restrict__ legal, const double* __restrict__ strategy, int trav, uint64_t seed,
                int64_t first, int64_t count, int64_t adv_bound, int64_t strat_bound, int32_t* adv_info, float* adv_vals,
                int32_t* strat_info, float* strat_vals, int64_t* counts, int32_t* draws, unsigned int* flag) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const int A = t.A, P = t.P;
  Rng rng(seed, static_cast<uint64_t>(first + j), 0);
  int n_draws = 0;
  int64_t n_adv = 0, n_strat = 0;
  int f_node[kMaxFrames];
  int f_a[kMaxFrames];
  double f_cv[kMaxFrames][kMaxA];
  int sp = 0;
  int node = 0;
  bool bad = false;
  for (;;) {
    double ret;
    for (;;) {   // descend to a terminal, pushing a frame at every node of the traverser
      const int k = t.kind[node];
      if (k == kTerminalNode) { ret = t.term_ret[node * P + trav]; break; }
      const int fc = t.first_child[node], nc = t.nchild[node];
      if (k == kChanceNode) {
        const double u = rng.unit();
        ++n_draws;
        node = fc + dcfr_choice(nc, u, [&](int c) { return t.edge_prob[fc + c]; });
        continue;
      }
      const int i = t.info[node];
      if (t.actor[node] != trav) {
        double p[kDcfrMaxA];
        for (int a = 0; a < A; ++a) p[a] = strategy[i * A + a];
        if (n_strat < strat_bound) {   // the row is appended at the visit (pre-order)
          const int64_t at = j * strat_bound + n_strat;
          strat_info[at] = i;
          for (int a = 0; a < A; ++a) strat_vals[at * A + a] = static_cast<float>(p[a]);
        } else {
          bad = true;
        }
        ++n_strat;
        const double u = rng.unit();
        ++n_draws;
        const int id = dcfr_opponent_draw(p, A, u);
        int pick = 0;
        for (int c = 0; c < nc; ++c)
          if (legal[i * A + c] == id) pick = c;
        node = fc + pick;
        continue;
      }
      if (sp >= kMaxFrames) { bad = true; ret = 0.0; break; }
      f_node[sp] = node;
      f_a[sp] = 0;
      ++sp;
      node = fc;
    }
    bool done = false;
    for (;;) {   // ascend: hand `ret` to the innermost open frame
      if (sp == 0) { done = true; break; }
      const int fn = f_node[sp - 1];
      const int nc = t.nchild[fn];
      const int a = f_a[sp - 1];
      f_cv[sp - 1][a] = ret;
      if (a + 1 < nc) {
        f_a[sp - 1] = a + 1;
        node = t.first_child[fn] + a + 1;
        break;
      }
      const int i = t.info[fn];
      double p[kDcfrMaxA];
      int32_t ids[kDcfrMaxA];
      float row[kDcfrMaxA];
      for (int b = 0; b < A; ++b) { p[b] = strategy[i * A + b]; ids[b] = legal[i * A + b]; }
      ret = dcfr_advantage_row(p, f_cv[sp - 1], ids, nc, A, row);
      if (n_adv < adv_bound) {   // appended after the children returned (post-order)
        const int64_t at = j * adv_bound + n_adv;
        adv_info[at] = i;
        for (int b = 0; b < A; ++b) adv_vals[at * A + b] = row[b];
      } else {
        bad = true;
      }
      ++n_adv;
      --sp;
    }
    if (done || bad) break;
  }
  if (bad) { atomicOr(flag, 1u); n_adv = 0; n_strat = 0; }
  counts[j] = n_adv;
  counts[count + j] = n_strat;
  draws[j] = n_draws;
}

// Staged rows to their sequence positions: row r of trajectory j goes to offsets[j] + r.
__global__ void k_dcfr_compact(const int64_t* __restrict__ counts, const int64_t* __restrict__ offsets, int64_t T, int64_t bound,
                               int A, const int32_t* __restrict__ st_info, const float* __restrict__ st_vals, int32_t* c_info,
                               float* c_vals) {
  const int64_t x = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (x >= T * bound) return;
  const int64_t j = x / bound, r = x % bound;
  if (r >= counts[j]) return;
  const int64_t to = offsets[j] + r;
  c_info[to] = st_info[x];
  for (int a = 0; a < A; ++a) c_vals[to * A + a] = st_vals[x * A + a];
}
// Closes both offset arrays with their totals and hands the totals and the flag to the host.
__global__ void k_dcfr_totals(const int64_t* counts, int64_t* offsets, int64_t T, const unsigned int* flag, int64_t* totals) {
  if (threadIdx.x || blockIdx.x) return;
  for (int w = 0; w < 2; ++w) {
    const int64_t total = offsets[w * (T + 1) + T - 1] + counts[w * T + T - 1];
    offsets[w * (T + 1) + T] = total;
    totals[w] = total;
  }
  totals[2] = *flag;
}

int deep_state(osg_cfr* s, DeepState** out) {
  if (!s->deep) {
    auto d = std::make_shared<DeepState>();
    hipStream_t st = s->ctx->stream;
    int rc = upload(s->legal, d->d_legal, st);
    if (rc) return rc;
    OSG_HIP(d->d_strategy.alloc(static_cast<size_t>(s->I) * s->A));
    OSG_HIP(d->d_flag.alloc(1));
    OSG_HIP(d->h_totals.alloc(4));
    std::vector<int64_t> work(3 * static_cast<size_t>(s->H));
    for (int p = 0; p < s->P; ++p)
      d->bounds.push_back(dcfr_row_bounds(s->H, s->kind.data(), s->nchild.data(), s->actor.data(), p,
                                          [&](int h, int c) { return s->first_child[h] + c; }, work.data()));
    OSG_HIP(hipStreamSynchronize(st));
    s->deep = d;
  }
  *out = static_cast<DeepState*>(s->deep.get());
  return OSG_OK;
}

}  // namespace

namespace osg_cfr_impl {
int deep_supported(const osg_cfr* s, const char* who) {
  if (s->A > kMaxA || s->A > kDcfrMaxA)
    return set_error(OSG_ERR_UNSUPPORTED, std::string(who) + ": decision nodes wider than 4 actions");
  for (int32_t id : s->legal)
    if (id >= s->A) return set_error(OSG_ERR_UNSUPPORTED, std::string(who) + ": an action id beyond the table's width");
  return OSG_OK;
}
}  // namespace osg_cfr_impl

extern "C" {

int osg_cfr_infostate_tensors(osg_cfr* s, float* out, int on_host) {
  if (!s || !out) return set_error(OSG_ERR_INVALID, "osg_cfr_infostate_tensors: null argument");
  const int E = s->spec.desc.info_size;
  if (E < 1) return set_error(OSG_ERR_UNSUPPORTED, "osg_cfr_infostate_tensors: the game has no information state tensor");
  // one member history per infostate, replayed from the root: ply d of every path in one osg_apply
  std::vector<std::vector<int32_t>> paths(s->I);
  size_t depth = 0;
  for (int i = 0; i < s->I; ++i) {
    for (int32_t v = s->mem[s->mem_off[i]]; s->parent[v] >= 0; v = s->parent[v]) paths[i].push_back(s->edge_action[v]);
    depth = std::max(depth, paths[i].size());
  }
  osg_batch* b = nullptr;
  int rc = osg_batch_create(s->ctx, s->spec.desc.canonical, s->I, &b);
  if (rc) return rc;
  std::vector<int32_t> acts(s->I);
  for (size_t d = 0; d < depth && !rc; ++d) {
    for (int i = 0; i < s->I; ++i) acts[i] = d < paths[i].size() ? paths[i][paths[i].size() - 1 - d] : -1;
    int64_t illegal = 0;
    rc = osg_apply(b, acts.data(), 1, &illegal);
    if (!rc && illegal) rc = set_error(OSG_ERR_ILLEGAL, "osg_cfr_infostate_tensors: a member history did not replay");
  }
  if (!rc) rc = osg_observation(b, -1, 1, out, on_host);   // the current player of a member history is the infostate's
  if (!rc) rc = osg_ctx_synchronize(s->ctx);
  osg_batch_destroy(b);
  return rc;
}

int osg_reservoir_create(osg_ctx* ctx, int num_actions, int64_t capacity, uint64_t seed, uint64_t stream, osg_reservoir** out) {
  if (!ctx || !out || num_actions < 1 || capacity < 1) return set_error(OSG_ERR_INVALID, "osg_reservoir_create: bad argument");
  if (capacity >= (int64_t{1} << 31)) return set_error(OSG_ERR_UNSUPPORTED, "osg_reservoir_create: capacity of 2^31 rows or more");
  auto b = std::make_unique<osg_reservoir>();
  b->ctx = ctx; b->A = num_actions; b->capacity = capacity; b->seed = seed; b->stream = stream;
  int rc;
  if ((rc = nomem_error(b->d_info.alloc(capacity), "osg_reservoir_create: ")) || (rc = nomem_error(b->d_iter.alloc(capacity), "osg_reservoir_create: ")) ||
      (rc = nomem_error(b->d_vals.alloc(static_cast<size_t>(capacity) * num_actions), "osg_reservoir_create: ")) ||
      (rc = nomem_error(b->d_winner.alloc(capacity), "osg_reservoir_create: ")))
    return rc;
  OSG_HIP(hipMemsetAsync(b->d_winner, 0, sizeof(unsigned int) * capacity, ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_info, 0xFF, sizeof(int32_t) * capacity, ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_iter, 0, sizeof(int32_t) * capacity, ctx->stream));
  OSG_HIP(hipMemsetAsync(b->d_vals, 0, sizeof(float) * capacity * num_actions, ctx->stream));
  *out = b.release();
  return OSG_OK;
}

int osg_reservoir_destroy(osg_reservoir* buf) {
  if (!buf) return OSG_OK;
  (void)hipStreamSynchronize(buf->ctx->stream);
  delete buf;
  return OSG_OK;
}

int osg_reservoir_sizes(osg_reservoir* buf, int64_t* size, int64_t* add_calls, int64_t* capacity) {
  if (!buf) return set_error(OSG_ERR_INVALID, "osg_reservoir_sizes: null argument");
  if (size) *size = std::min(buf->add_calls, buf->capacity);
  if (add_calls) *add_calls = buf->add_calls;
  if (capacity) *capacity = buf->capacity;
  return OSG_OK;
}

int osg_reservoir_clear(osg_reservoir* buf) {
  if (!buf) return set_error(OSG_ERR_INVALID, "osg_reservoir_clear: null argument");
  buf->add_calls = 0;   // ReservoirBuffer.clear (deep_cfr.py:211-213): the rows stay, the count starts again
  return OSG_OK;
}

int osg_reservoir_append(osg_reservoir* buf, int64_t m, const int32_t* d_info, int32_t iteration, const float* d_values) {
  if (!buf || m < 0 || (m > 0 && (!d_info || !d_values))) return set_error(OSG_ERR_INVALID, "osg_reservoir_append: bad argument");
  if (m >= (int64_t{1} << 31) - 1) return set_error(OSG_ERR_UNSUPPORTED, "osg_reservoir_append: 2^31 rows or more in one call");
  return reservoir_append(buf, m, d_info, iteration, d_values);
}

int osg_reservoir_rows(osg_reservoir* buf, const int64_t* d_slots, int64_t m, int32_t* d_info, int32_t* d_iteration,
                       float* d_values) {
  if (!buf || m < 0 || (m > 0 && !d_slots)) return set_error(OSG_ERR_INVALID, "osg_reservoir_rows: bad argument");
  if (m == 0) return OSG_OK;
  k_res_rows<<<dim3(blocks_for(m)), dim3(kThreads), 0, buf->ctx->stream>>>(buf->d_info, buf->d_iter, buf->d_vals, buf->A,
                                                                           buf->capacity, d_slots, m, d_info, d_iteration, d_values);
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

int osg_reservoir_sample(osg_reservoir* buf, uint64_t seed, uint64_t stream, int64_t m, int64_t* d_slots) {
  if (!buf || m < 1 || !d_slots) return set_error(OSG_ERR_INVALID, "osg_reservoir_sample: bad argument");
  const int64_t size = std::min(buf->add_calls, buf->capacity);
  if (m > size) return set_error(OSG_ERR_INVALID, "osg_reservoir_sample: more rows asked for than the buffer holds");
  hipStream_t st = buf->ctx->stream;
  OSG_HIP(buf->d_key_in.ensure(size));
  OSG_HIP(buf->d_key_out.ensure(size));
  OSG_HIP(buf->d_slot_in.ensure(size));
  OSG_HIP(buf->d_slot_out.ensure(size));
  k_res_keys<<<dim3(blocks_for(size)), dim3(kThreads), 0, st>>>(buf->d_key_in, buf->d_slot_in, seed, stream, size);
  size_t bytes = 0;
  OSG_HIP(rocprim::radix_sort_pairs(nullptr, bytes, buf->d_key_in.get(), buf->d_key_out.get(), buf->d_slot_in.get(),
                                    buf->d_slot_out.get(), static_cast<size_t>(size), 0u, 64u, st));
  OSG_HIP(buf->d_tmp.ensure(bytes));
  OSG_HIP(rocprim::radix_sort_pairs(buf->d_tmp.get(), bytes, buf->d_key_in.get(), buf->d_key_out.get(), buf->d_slot_in.get(),
                                    buf->d_slot_out.get(), static_cast<size_t>(size), 0u, 64u, st));
  OSG_HIP(hipMemcpyAsync(d_slots, buf->d_slot_out.get(), sizeof(int64_t) * m, hipMemcpyDeviceToDevice, st));
  return OSG_OK;
}

int osg_deep_cfr_traverse(osg_cfr* s, const float* d_advantages, int player, int iteration, uint64_t seed,
                          int64_t first_trajectory, int64_t trajectories, osg_reservoir* adv_buf, osg_reservoir* strat_buf,
                          int64_t* h_counts) {
  if (!s || !d_advantages || trajectories < 0 || first_trajectory < 0)
    return set_error(OSG_ERR_INVALID, "osg_deep_cfr_traverse: bad argument");
  if (player < 0 || player >= s->P) return set_error(OSG_ERR_INVALID, "osg_deep_cfr_traverse: no such player");
  int rc = deep_supported(s, "osg_deep_cfr_traverse");
  if (rc) return rc;
  for (osg_reservoir* b : {adv_buf, strat_buf})
    if (b && (b->A != s->A || b->ctx != s->ctx))
      return set_error(OSG_ERR_INVALID, "osg_deep_cfr_traverse: a buffer of another row width or context");
  DeepState* d = nullptr;
  if ((rc = deep_state(s, &d))) return rc;
  const DcfrBounds bd = d->bounds[player];
  if (bd.frames > kMaxFrames) return set_error(OSG_ERR_UNSUPPORTED, "osg_deep_cfr_traverse: more than 24 traverser nodes on a path");
  const int64_t T = trajectories, ab = std::max<int64_t>(bd.adv, 1), sb = std::max<int64_t>(bd.strat, 1);
  if (T * std::max(ab, sb) >= (int64_t{1} << 31) - 1)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_deep_cfr_traverse: 2^31 rows or more in one call");
  hipStream_t st = s->ctx->stream;
  const int A = s->A;
  d->T = T; d->adv_bound = ab; d->strat_bound = sb; d->adv_rows = d->strat_rows = 0;
  if (h_counts) h_counts[0] = h_counts[1] = 0;
  if (T == 0) return OSG_OK;
  OSG_HIP(d->st_adv_info.ensure(T * ab));
  OSG_HIP(d->st_adv_vals.ensure(T * ab * A));
  OSG_HIP(d->c_adv_info.ensure(T * ab));
  OSG_HIP(d->c_adv_vals.ensure(T * ab * A));
  OSG_HIP(d->st_strat_info.ensure(T * sb));
  OSG_HIP(d->st_strat_vals.ensure(T * sb * A));
  OSG_HIP(d->c_strat_info.ensure(T * sb));
  OSG_HIP(d->c_strat_vals.ensure(T * sb * A));
  OSG_HIP(d->counts.ensure(2 * T));
  OSG_HIP(d->offsets.ensure(2 * (T + 1)));
  OSG_HIP(d->draws.ensure(T));
  OSG_HIP(hipMemsetAsync(d->d_flag, 0, sizeof(unsigned int), st));
  k_dcfr_strategy<<<dim3(blocks_for(s->I)), dim3(kThreads), 0, st>>>(d_advantages, d->d_legal, s->d_nact, s->I, A, d->d_strategy);
  k_dcfr_traverse<<<dim3(blocks_for(T)), dim3(kThreads), 0, st>>>(s->tree(), d->d_legal, d->d_strategy, player, seed,
                                                                  first_trajectory, T, ab, sb, d->st_adv_info, d->st_adv_vals,
                                                                  d->st_strat_info, d->st_strat_vals, d->counts, d->draws, d->d_flag);
  OSG_HIP(hipGetLastError());
  for (int w = 0; w < 2; ++w) {
    int64_t* in = d->counts.get() + w * T;
    int64_t* out = d->offsets.get() + w * (T + 1);
    size_t bytes = 0;
    OSG_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, int64_t{0}, static_cast<size_t>(T), rocprim::plus<int64_t>(), st));
    OSG_HIP(d->tmp.ensure(bytes));
    OSG_HIP(rocprim::exclusive_scan(d->tmp.get(), bytes, in, out, int64_t{0}, static_cast<size_t>(T), rocprim::plus<int64_t>(), st));
  }
  k_dcfr_totals<<<dim3(1), dim3(64), 0, st>>>(d->counts, d->offsets, T, d->d_flag, d->h_totals);
  k_dcfr_compact<<<dim3(blocks_for(T * ab)), dim3(kThreads), 0, st>>>(d->counts, d->offsets, T, ab, A, d->st_adv_info, d->st_adv_vals,
                                                                      d->c_adv_info, d->c_adv_vals);
  k_dcfr_compact<<<dim3(blocks_for(T * sb)), dim3(kThreads), 0, st>>>(d->counts.get() + T, d->offsets.get() + (T + 1), T, sb, A,
                                                                      d->st_strat_info, d->st_strat_vals, d->c_strat_info, d->c_strat_vals);
  OSG_HIP(hipGetLastError());
  OSG_HIP(hipStreamSynchronize(st));   // the row totals size the appends
  if (d->h_totals[2]) {
    d->T = 0;
    return set_error(OSG_ERR_INVALID, "osg_deep_cfr_traverse: a trajectory passed its row bound (internal error)");
  }
  d->adv_rows = d->h_totals[0];
  d->strat_rows = d->h_totals[1];
  if (adv_buf && (rc = reservoir_append(adv_buf, d->adv_rows, d->c_adv_info, iteration, d->c_adv_vals))) return rc;
  if (strat_buf && (rc = reservoir_append(strat_buf, d->strat_rows, d->c_strat_info, iteration, d->c_strat_vals))) return rc;
  if (h_counts) { h_counts[0] = d->adv_rows; h_counts[1] = d->strat_rows; }
  s->last_kernel = "k_dcfr_traverse";
  return OSG_OK;
}

int osg_deep_cfr_staged(osg_cfr* s, int64_t* sizes, int64_t* d_adv_offsets, int32_t* d_adv_info, float* d_adv_values,
                        int64_t* d_strat_offsets, int32_t* d_strat_info, float* d_strat_values, int32_t* d_draws) {
  if (!s) return set_error(OSG_ERR_INVALID, "osg_deep_cfr_staged: null argument");
  DeepState* d = static_cast<DeepState*>(s->deep.get());
  if (sizes) { sizes[0] = d ? d->T : 0; sizes[1] = d ? d->adv_rows : 0; sizes[2] = d ? d->strat_rows : 0; sizes[3] = d ? d->adv_bound : 0; sizes[4] = d ? d->strat_bound : 0; }
  if (!d || d->T == 0) return OSG_OK;
  hipStream_t st = s->ctx->stream;
  const int64_t T = d->T;
  const int A = s->A;
  auto copy = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
  };
  OSG_HIP(copy(d_adv_offsets, d->offsets.get(), sizeof(int64_t) * (T + 1)));
  OSG_HIP(copy(d_strat_offsets, d->offsets.get() + (T + 1), sizeof(int64_t) * (T + 1)));
  OSG_HIP(copy(d_adv_info, d->c_adv_info.get(), sizeof(int32_t) * d->adv_rows));
  OSG_HIP(copy(d_adv_values, d->c_adv_vals.get(), sizeof(float) * d->adv_rows * A));
  OSG_HIP(copy(d_strat_info, d->c_strat_info.get(), sizeof(int32_t) * d->strat_rows));
  OSG_HIP(copy(d_strat_values, d->c_strat_vals.get(), sizeof(float) * d->strat_rows * A));
  OSG_HIP(copy(d_draws, d->draws.get(), sizeof(int32_t) * T));
  return OSG_OK;
}

}  // extern "C"
