// algorithms::GetAllStates (open_spiel/algorithms/get_all_states.cc:28-91) and algorithms::ValueIteration
// (open_spiel/algorithms/value_iteration.cc:84-138) for tic_tac_toe, connect_four and hex without the swap move:
// every reachable position once, its game-theoretic value, the optimal moves and the distance to the end.
//
// Forward, one level (= ply = stone count) at a time:
//   k_solve_count    legal actions per position (0 at a terminal one); an exclusive scan gives the edge offsets
//   k_solve_expand   ONE THREAD PER EDGE: the parent by binary search in the offsets, the k-th legal action, the child
//                    record, its canonical key (osg_solve.h) — child order = (parent, action ascending), fixed by the
//                    offsets, no atomics
//   radix sort       (key, edge index) pairs, stable: rocPRIM, 64 bits at a time (low word, then high word)
//   k_solve_heads    first of each run of equal keys; an exclusive scan numbers the survivors
//   k_solve_compact  the survivors' records and keys become level d + 1 (ascending by key), and every edge learns the
//                    index of its child
// Backward, one launch per level: k_solve_level folds the children's values (SolveFold).
// Workspaces live for one level (the children before merging, the sort's buffers); what stays is the records and keys
// per level and the edge table.
#include <string.h>

#include <memory>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "osg_internal.h"
#include "osg_solve.h"

using namespace osg;

namespace {

constexpr int kSolveBlock = 256;
inline unsigned solve_grid(int64_t n) { return static_cast<unsigned>((n + kSolveBlock - 1) / kSolveBlock); }

template <class G> struct is_c4 : std::false_type {};
template <int R, int C, int K, class BB> struct is_c4<C4T<R, C, K, BB>> : std::true_type {};
template <class G> struct solve_hex_nw : std::integral_constant<int, 0> {};
template <int NW> struct solve_hex_nw<HexT<NW>> : std::integral_constant<int, NW> {};
template <class G>
constexpr bool solve_served() {
  return std::is_same<G, Ttt>::value || is_c4<G>::value || (solve_hex_nw<G>::value >= 1 && solve_hex_nw<G>::value <= 2);
}

using Bytes = DeviceArray<unsigned char>;   // state records (their word type comes with the game) and rocprim's scratch
template <class W> W* words_of(const Bytes& b) { return reinterpret_cast<W*>(b.get()); }
template <class T>
int dev_alloc(DeviceArray<T>& buf, size_t n) { return nomem_error(buf.alloc(n), "osg_solve: "); }

struct Level {
  int64_t n = 0, edges = 0;
  Bytes words;                        // the records (SoA, stride n), ascending by key
  DeviceArray<uint64_t> key_lo, key_hi;
  DeviceArray<int64_t> edge_off, edge_child;   // [n + 1] (level-local), [edges] (global, -1 dropped)
  DeviceArray<int32_t> edge_action;            // [edges]
};

template <class G>
__global__ void __launch_bounds__(kSolveBlock)
k_solve_root(typename G::Params p, typename G::word_t* words, uint64_t* key_lo, uint64_t* key_hi) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const typename G::State s = G::initial(p);
  G::store(p, words, 1, 0, s);
  const SolveKey k = SolveTraits<G>::key(p, s);
  key_lo[0] = k.lo;
  if (key_hi) key_hi[0] = k.hi;
}

template <class G>
__global__ void __launch_bounds__(kSolveBlock)
k_solve_count(typename G::Params p, const typename G::word_t* words, int64_t n, int64_t* count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSolveBlock + threadIdx.x;
  if (i > n) return;
  if (i == n) { count[n] = 0; return; }
  const typename G::State s = G::load(p, words, n, i);
  count[i] = G::terminal(p, s) ? 0 : solve_legal<G>(p, s).count();
}

template <class G>
__global__ void __launch_bounds__(kSolveBlock)
k_solve_expand(typename G::Params p, const typename G::word_t* words, int64_t n, const int64_t* off, int64_t m, int depth,
               int depth_limit, int include_terminals, typename G::word_t* child_words, uint64_t* key_lo, uint64_t* key_hi,
               int32_t* action, uint32_t* index) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kSolveBlock + threadIdx.x;
  if (e >= m) return;
  const int64_t i = solve_edge_parent(off, n, e);
  const typename G::State s = G::load(p, words, n, i);
  int a;
  typename G::State c;
  SolveKey k;
  solve_expand<G>(p, s, depth, static_cast<int>(e - off[i]), depth_limit, include_terminals != 0, &a, &c, &k);
  G::store(p, child_words, m, e, c);
  key_lo[e] = k.lo;
  if (key_hi) key_hi[e] = k.hi;
  action[e] = a;
  index[e] = static_cast<uint32_t>(e);
}

__global__ void __launch_bounds__(kSolveBlock)
k_solve_gather(const uint64_t* src, const uint32_t* index, int64_t m, uint64_t* dst) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kSolveBlock + threadIdx.x;
  if (j < m) dst[j] = src[index[j]];
}

// head[j] = 1 where sorted key j opens a run of a key that is kept; head[m] = 0 (the scan's total lands there)
__global__ void __launch_bounds__(kSolveBlock)
k_solve_heads(const uint64_t* lo, const uint64_t* hi, int64_t m, int64_t* head) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kSolveBlock + threadIdx.x;
  if (j > m) return;
  if (j == m) { head[m] = 0; return; }
  const SolveKey k{lo[j], hi ? hi[j] : ~0ull};
  bool h = !solve_key_equal(k, solve_key_dropped());
  if (h && j > 0) h = !solve_key_equal(k, SolveKey{lo[j - 1], hi ? hi[j - 1] : ~0ull});
  head[j] = h ? 1 : 0;
}

template <class G>
__global__ void __launch_bounds__(kSolveBlock)
k_solve_compact(typename G::Params p, const typename G::word_t* child_words, int64_t m, const uint32_t* index,
                const uint64_t* lo, const uint64_t* hi, const int64_t* pos, int64_t u, int64_t next_base,
                typename G::word_t* next_words, uint64_t* next_lo, uint64_t* next_hi, int64_t* edge_child) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kSolveBlock + threadIdx.x;
  if (j >= m) return;
  const int64_t e = index[j];
  const SolveKey k{lo[j], hi ? hi[j] : ~0ull};
  if (solve_key_equal(k, solve_key_dropped())) { edge_child[e] = -1; return; }
  const bool head = pos[j + 1] != pos[j];
  const int64_t q = head ? pos[j] : pos[j] - 1;
  edge_child[e] = next_base + q;
  if (head && q < u) {
    G::store(p, next_words, u, q, G::load(p, child_words, m, e));
    next_lo[q] = k.lo;
    if (next_hi) next_hi[q] = k.hi;
  }
}

__global__ void __launch_bounds__(kSolveBlock)
k_solve_shift(const int64_t* src, int64_t n, int64_t add, int64_t* dst) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSolveBlock + threadIdx.x;
  if (i < n) dst[i] = src[i] + add;
}

template <class G>
__global__ void __launch_bounds__(kSolveBlock)
k_solve_level(typename G::Params p, const typename G::word_t* words, int64_t n, int64_t base, const int64_t* edge_off,
              const int32_t* edge_action, const int64_t* edge_child, double* value, uint32_t* optimal, int mask_words,
              int32_t* distance, unsigned long long* terminals) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSolveBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t g = base + i;
  const typename G::State s = G::load(p, words, n, i);
  MaskT<G::kMaskW> best;
  if (G::terminal(p, s)) {
    double r[2];
    G::returns(p, s, r);
    value[g] = r[0];
    distance[g] = 0;
    atomicAdd(terminals, 1ull);   // a count: the order of arrival decides nothing
  } else {
    SolveFold f;
    f.start(SolveTraits<G>::mover(s));
    const int64_t e0 = edge_off[g], e1 = edge_off[g + 1];
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t c = edge_child[e];
      f.fold(c < 0 ? 0.0 : value[c], c < 0 ? 0 : distance[c]);
    }
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t c = edge_child[e];
      if ((c < 0 ? 0.0 : value[c]) == f.value) best.set(edge_action[e]);
    }
    value[g] = f.value;
    distance[g] = f.result_distance();
  }
#pragma unroll
  for (int k = 0; k < G::kMaskW; ++k)
    if (k < mask_words) optimal[g * mask_words + k] = best.w[k];   // the layout of osg_legal_mask: desc.mask_words per state
}

template <class G>
__global__ void __launch_bounds__(kSolveBlock)
k_solve_lookup(typename G::Params p, const typename G::word_t* words, int64_t nq, const int64_t* level_off, int levels,
               const uint64_t* key_lo, const uint64_t* key_hi, int64_t* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSolveBlock + threadIdx.x;
  if (i >= nq) return;
  const typename G::State s = G::load(p, words, nq, i);
  const int d = SolveTraits<G>::plies(s);
  out[i] = d < levels ? solve_find(key_lo, key_hi, level_off[d], level_off[d + 1], SolveTraits<G>::key(p, s)) : -1;
}

}  // namespace

struct osg_solve {
  struct CtxRef { osg_ctx* ctx = nullptr; ~CtxRef() { if (ctx) ctx_release(ctx); } } held;   // first member: dropped last, after every buffer
  osg_ctx* ctx = nullptr;
  GameSpec spec;
  int depth_limit = -1;
  bool include_terminals = true;
  int mask_words = kMaskWords;
  int64_t n = 0, edges = 0, terminals = 0;
  std::vector<int64_t> level_off;    // [levels + 1]
  std::vector<Bytes> level_words;    // the records of each level (SoA, stride = the level's size)
  DeviceArray<uint64_t> key_lo, key_hi;
  DeviceArray<int64_t> d_level_off, edge_off, edge_child;
  DeviceArray<int32_t> edge_action, distance;
  DeviceArray<double> value;
  DeviceArray<uint32_t> optimal;
  bool wide = false;
  ~osg_solve() { if (ctx) (void)hipStreamSynchronize(ctx->stream); }   // (then the buffers go, then the context reference)
};

namespace {

int read_i64(osg_ctx* ctx, const int64_t* d, int64_t* h) {
  OSG_HIP(hipMemcpyAsync(h, d, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  return OSG_OK;
}

int scan_i64(osg_ctx* ctx, const int64_t* in, int64_t* out, int64_t count) {
  size_t bytes = 0;
  OSG_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, int64_t{0}, static_cast<size_t>(count), rocprim::plus<int64_t>(), ctx->stream));
  Bytes tmp;
  if (int rc = dev_alloc(tmp, bytes)) return rc;
  OSG_HIP(rocprim::exclusive_scan(tmp.get(), bytes, in, out, int64_t{0}, static_cast<size_t>(count), rocprim::plus<int64_t>(), ctx->stream));
  OSG_HIP(hipStreamSynchronize(ctx->stream));   // tmp goes with this scope
  return OSG_OK;
}

int sort_pairs(osg_ctx* ctx, const uint64_t* k_in, uint64_t* k_out, const uint32_t* v_in, uint32_t* v_out, int64_t m, int bits) {
  size_t bytes = 0;
  OSG_HIP(rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, static_cast<size_t>(m), 0u, static_cast<unsigned>(bits), ctx->stream));
  Bytes tmp;
  if (int rc = dev_alloc(tmp, bytes)) return rc;
  OSG_HIP(rocprim::radix_sort_pairs(tmp.get(), bytes, k_in, k_out, v_in, v_out, static_cast<size_t>(m), 0u, static_cast<unsigned>(bits), ctx->stream));
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  return OSG_OK;
}

template <class G>
int solve_run(osg_solve* s, const typename G::Params& P, int64_t max_states) {
  using W = typename G::word_t;
  osg_ctx* ctx = s->ctx;
  hipStream_t st = ctx->stream;
  const int state_words = s->spec.desc.state_words;
  const int key_bits = SolveTraits<G>::key_bits(P);
  const bool wide = key_bits > 64;
  // the dropped key has bit `key_bits` set, which no position's key has: one more bit than the key takes part
  const int bits_lo = wide ? 64 : std::min(64, key_bits + 1), bits_hi = wide ? std::min(64, key_bits - 64 + 1) : 0;
  s->wide = wide;
  s->mask_words = std::min<int>(s->spec.desc.mask_words, G::kMaskW);
  if (max_states < 1) return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: the game has more states than max_states");

  std::vector<Level> levels(1);
  {
    Level& L = levels[0];
    L.n = 1;
    if (int rc = dev_alloc(L.words, sizeof(W) * state_words)) return rc;
    if (int rc = dev_alloc(L.key_lo, 1)) return rc;
    if (wide) if (int rc = dev_alloc(L.key_hi, 1)) return rc;
    k_solve_root<G><<<dim3(1), dim3(kSolveBlock), 0, st>>>(P, words_of<W>(L.words), L.key_lo.get(), L.key_hi.get());
    OSG_HIP(hipGetLastError());
  }
  int64_t total = 1, total_edges = 0;
  for (int d = 0;; ++d) {
    Level& L = levels[d];
    DeviceArray<int64_t> count;
    if (int rc = dev_alloc(count, L.n + 1)) return rc;
    if (int rc = dev_alloc(L.edge_off, L.n + 1)) return rc;
    k_solve_count<G><<<dim3(solve_grid(L.n + 1)), dim3(kSolveBlock), 0, st>>>(P, words_of<W>(L.words), L.n, count.get());
    OSG_HIP(hipGetLastError());
    if (int rc = scan_i64(ctx, count.get(), L.edge_off.get(), L.n + 1)) return rc;
    count.reset();
    int64_t m = 0;
    if (int rc = read_i64(ctx, L.edge_off.get() + L.n, &m)) return rc;
    L.edges = m;
    total_edges += m;
    if (m == 0) break;
    // Before the level's workspaces are allocated: a position of level d + 1 has as many parents as it has stones
    // that could have been placed last — at most the stones of the player who moved, ceil((d + 1) / 2) — so where the
    // limits drop no child of this level, at least m / ceil((d + 1) / 2) positions survive the merge.
    const bool none_dropped = s->include_terminals && (s->depth_limit < 0 || d + 1 <= s->depth_limit);
    const int64_t max_parents = (d + 2) / 2;
    if (none_dropped && total + (m + max_parents - 1) / max_parents > max_states)
      return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: the game has more states than max_states (" + std::to_string(max_states) +
                                            "): at least " + std::to_string(total + (m + max_parents - 1) / max_parents) + " after " +
                                            std::to_string(d + 1) + " plies");
    if (m > (int64_t{1} << 31) - 1)   // edge indices are 32-bit values of the sort
      return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: a level with 2^31 or more children is not enumerated");
    if (int rc = dev_alloc(L.edge_action, m)) return rc;
    if (int rc = dev_alloc(L.edge_child, m)) return rc;
    Bytes child_words;
    DeviceArray<uint64_t> lo, hi, lo_s, hi_s;
    DeviceArray<uint32_t> index, index_s;
    if (int rc = dev_alloc(child_words, sizeof(W) * state_words * m)) return rc;
    if (int rc = dev_alloc(lo, m)) return rc;
    if (int rc = dev_alloc(index, m)) return rc;
    if (int rc = dev_alloc(lo_s, m)) return rc;
    if (int rc = dev_alloc(index_s, m)) return rc;
    if (wide) { if (int rc = dev_alloc(hi, m)) return rc; if (int rc = dev_alloc(hi_s, m)) return rc; }
    k_solve_expand<G><<<dim3(solve_grid(m)), dim3(kSolveBlock), 0, st>>>(
        P, words_of<W>(L.words), L.n, L.edge_off.get(), m, d, s->depth_limit, s->include_terminals ? 1 : 0, words_of<W>(child_words),
        lo.get(), hi.get(), L.edge_action.get(), index.get());
    OSG_HIP(hipGetLastError());
    if (int rc = sort_pairs(ctx, lo.get(), lo_s.get(), index.get(), index_s.get(), m, bits_lo)) return rc;
    if (wide) {   // least significant word first; the second, stable pass orders by the high word
      DeviceArray<uint64_t> hi_g;
      if (int rc = dev_alloc(hi_g, m)) return rc;
      k_solve_gather<<<dim3(solve_grid(m)), dim3(kSolveBlock), 0, st>>>(hi.get(), index_s.get(), m, hi_g.get());
      OSG_HIP(hipGetLastError());
      if (int rc = sort_pairs(ctx, hi_g.get(), hi_s.get(), index_s.get(), index.get(), m, bits_hi)) return rc;
      k_solve_gather<<<dim3(solve_grid(m)), dim3(kSolveBlock), 0, st>>>(lo.get(), index.get(), m, lo_s.get());
      OSG_HIP(hipGetLastError());
      std::swap(index, index_s);
    }
    DeviceArray<int64_t> head, pos;
    if (int rc = dev_alloc(head, m + 1)) return rc;
    if (int rc = dev_alloc(pos, m + 1)) return rc;
    k_solve_heads<<<dim3(solve_grid(m + 1)), dim3(kSolveBlock), 0, st>>>(lo_s.get(), hi_s.get(), m, head.get());
    OSG_HIP(hipGetLastError());
    if (int rc = scan_i64(ctx, head.get(), pos.get(), m + 1)) return rc;
    int64_t u = 0;
    if (int rc = read_i64(ctx, pos.get() + m, &u)) return rc;
    if (total + u > max_states)
      return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: the game has more states than max_states (" + std::to_string(max_states) +
                                            "): " + std::to_string(total + u) + " after " + std::to_string(d + 1) + " plies");
    Level N;
    N.n = u;
    if (int rc = dev_alloc(N.words, sizeof(W) * state_words * u)) return rc;
    if (int rc = dev_alloc(N.key_lo, u)) return rc;
    if (wide) if (int rc = dev_alloc(N.key_hi, u)) return rc;
    k_solve_compact<G><<<dim3(solve_grid(m)), dim3(kSolveBlock), 0, st>>>(
        P, words_of<W>(child_words), m, index_s.get(), lo_s.get(), hi_s.get(), pos.get(), u, total,
        words_of<W>(N.words), N.key_lo.get(), N.key_hi.get(), L.edge_child.get());
    OSG_HIP(hipGetLastError());
    OSG_HIP(hipStreamSynchronize(st));   // the level's workspaces go here
    if (u == 0) break;
    total += u;
    levels.push_back(std::move(N));
  }

  // the result: keys and the edge table in (level, key) order, the records stay per level
  const int nl = static_cast<int>(levels.size());
  s->n = total;
  s->edges = total_edges;
  s->level_off.assign(nl + 1, 0);
  for (int d = 0; d < nl; ++d) s->level_off[d + 1] = s->level_off[d] + levels[d].n;
  if (int rc = dev_alloc(s->key_lo, total)) return rc;
  if (wide) if (int rc = dev_alloc(s->key_hi, total)) return rc;
  if (int rc = dev_alloc(s->d_level_off, nl + 1)) return rc;
  if (int rc = dev_alloc(s->edge_off, total + 1)) return rc;
  if (int rc = dev_alloc(s->edge_action, total_edges)) return rc;
  if (int rc = dev_alloc(s->edge_child, total_edges)) return rc;
  if (int rc = dev_alloc(s->value, total)) return rc;
  if (int rc = dev_alloc(s->optimal, s->mask_words * total)) return rc;
  if (int rc = dev_alloc(s->distance, total)) return rc;
  OSG_HIP(hipMemcpyAsync(s->d_level_off.get(), s->level_off.data(), sizeof(int64_t) * (nl + 1), hipMemcpyHostToDevice, st));
  int64_t ebase = 0;
  for (int d = 0; d < nl; ++d) {
    Level& L = levels[d];
    const int64_t o = s->level_off[d];
    OSG_HIP(hipMemcpyAsync(s->key_lo.get() + o, L.key_lo.get(), sizeof(uint64_t) * L.n, hipMemcpyDeviceToDevice, st));
    if (wide) OSG_HIP(hipMemcpyAsync(s->key_hi.get() + o, L.key_hi.get(), sizeof(uint64_t) * L.n, hipMemcpyDeviceToDevice, st));
    k_solve_shift<<<dim3(solve_grid(L.n + 1)), dim3(kSolveBlock), 0, st>>>(L.edge_off.get(), L.n + 1, ebase, s->edge_off.get() + o);
    OSG_HIP(hipGetLastError());
    if (L.edges > 0) {
      OSG_HIP(hipMemcpyAsync(s->edge_action.get() + ebase, L.edge_action.get(), sizeof(int32_t) * L.edges, hipMemcpyDeviceToDevice, st));
      OSG_HIP(hipMemcpyAsync(s->edge_child.get() + ebase, L.edge_child.get(), sizeof(int64_t) * L.edges, hipMemcpyDeviceToDevice, st));
    }
    ebase += L.edges;
  }
  OSG_HIP(hipStreamSynchronize(st));
  s->level_words.resize(nl);
  for (int d = 0; d < nl; ++d) {
    s->level_words[d] = std::move(levels[d].words);
    levels[d] = Level();   // its keys and edges are in the result now
  }

  // backward
  DeviceArray<unsigned long long> term;
  if (int rc = dev_alloc(term, 1)) return rc;
  OSG_HIP(hipMemsetAsync(term.get(), 0, sizeof(unsigned long long), st));
  for (int d = nl - 1; d >= 0; --d) {
    const int64_t n = s->level_off[d + 1] - s->level_off[d];
    k_solve_level<G><<<dim3(solve_grid(n)), dim3(kSolveBlock), 0, st>>>(
        P, words_of<W>(s->level_words[d]), n, s->level_off[d], s->edge_off.get(), s->edge_action.get(),
        s->edge_child.get(), s->value.get(), s->optimal.get(), s->mask_words, s->distance.get(),
        term.get());
    OSG_HIP(hipGetLastError());
  }
  unsigned long long h_term = 0;
  OSG_HIP(hipMemcpyAsync(&h_term, term.get(), sizeof(h_term), hipMemcpyDeviceToHost, st));
  OSG_HIP(hipStreamSynchronize(st));
  s->terminals = static_cast<int64_t>(h_term);
  return OSG_OK;
}

int copy_out(osg_solve* s, void* dst, const void* src, size_t bytes, int on_host) {
  OSG_HIP(hipMemcpyAsync(dst, src, bytes, on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s->ctx->stream));
  if (on_host) OSG_HIP(hipStreamSynchronize(s->ctx->stream));
  return OSG_OK;
}

}  // namespace

extern "C" int osg_solve_create(osg_ctx* ctx, const char* game_string, int32_t depth_limit, int32_t include_terminals,
                                int64_t max_states, osg_solve** out) {
  if (!ctx || !game_string || !out) return set_error(OSG_ERR_INVALID, "osg_solve_create: null argument");
  if (ctx->closed) return set_error(OSG_ERR_INVALID, "osg_solve_create: the context was destroyed");
  if (max_states <= 0) max_states = int64_t{1} << 26;
  std::unique_ptr<osg_solve> s(new osg_solve);
  if (int rc = parse_game(game_string, &s->spec)) return rc;
  const osg_game_desc& d = s->spec.desc;
  if (d.game_kind == kKuhn || d.game_kind == kLeduc)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: the game must be a deterministic perfect-information game "
                                          "(value_iteration.cc:95-98); kuhn_poker and leduc_poker have chance nodes and hidden cards");
  if (d.game_kind == kHex) {
    int swap = 0;
    for_hex(s->spec, [&](auto, const auto& p) { swap = p.swap; return 0; });
    if (swap)
      return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: hex with swap=true is not enumerated (after the swap move the "
                                            "stone count is no longer the ply)");
    if (s->spec.hex_nw > kMaskWords)
      return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: hex is enumerated on boards of up to 128 cells");
    if (s->spec.hex_nw > 2)
      return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: the canonical key of a hex board above 64 cells is wider than 128 bits");
    if (s->spec.hex_explicit)
      return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: hex(string_rep=explicit) prints the edge labels, which the "
                                            "canonical key (the stones) does not separate");
  }
  s->ctx = ctx;
  ctx_retain(ctx);
  s->held.ctx = ctx;
  s->depth_limit = depth_limit;
  s->include_terminals = include_terminals != 0;
  osg_solve* raw = s.get();
  const int rc = for_game(raw->spec, [&](auto g, const auto& P) -> int {
    using G = typename decltype(g)::type;
    if constexpr (!solve_served<G>()) return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_create: no enumeration for this game layout");
    else return solve_run<G>(raw, P, max_states);
  });
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;   // (s frees what was allocated)
  }
  *out = s.release();
  return OSG_OK;
}

extern "C" int osg_solve_destroy(osg_solve* s) {
  delete s;
  return OSG_OK;
}

extern "C" int osg_solve_sizes(const osg_solve* s, int64_t* states, int32_t* levels, int64_t* edges, int64_t* terminals) {
  if (!s) return set_error(OSG_ERR_INVALID, "osg_solve_sizes: null argument");
  if (states) *states = s->n;
  if (levels) *levels = static_cast<int32_t>(s->level_off.size()) - 1;
  if (edges) *edges = s->edges;
  if (terminals) *terminals = s->terminals;
  return OSG_OK;
}

extern "C" int osg_solve_level_offsets(const osg_solve* s, int64_t* h_offsets) {
  if (!s || !h_offsets) return set_error(OSG_ERR_INVALID, "osg_solve_level_offsets: null argument");
  for (size_t i = 0; i < s->level_off.size(); ++i) h_offsets[i] = s->level_off[i];
  return OSG_OK;
}

extern "C" int osg_solve_states(const osg_solve* s, osg_batch* dst) {
  if (!s || !dst) return set_error(OSG_ERR_INVALID, "osg_solve_states: null argument");
  if (dst->n != s->n || std::string(dst->spec.desc.canonical) != s->spec.desc.canonical)
    return set_error(OSG_ERR_INVALID, "osg_solve_states: the batch must be of the solved game and hold as many states as the result");
  const size_t wb = static_cast<size_t>(s->spec.desc.state_word_bytes);
  const int planes = s->spec.desc.state_words;
  for (size_t d = 0; d + 1 < s->level_off.size(); ++d) {
    const int64_t o = s->level_off[d], n = s->level_off[d + 1] - o;
    for (int k = 0; k < planes; ++k)
      OSG_HIP(hipMemcpyAsync(static_cast<char*>(dst->words()) + (static_cast<size_t>(k) * s->n + o) * wb,
                             words_of<char>(s->level_words[d]) + static_cast<size_t>(k) * n * wb, static_cast<size_t>(n) * wb,
                             hipMemcpyDeviceToDevice, dst->ctx->stream));
  }
  return OSG_OK;
}

extern "C" int osg_solve_values(const osg_solve* s, double* value, int on_host) {
  if (!s || !value) return set_error(OSG_ERR_INVALID, "osg_solve_values: null argument");
  return copy_out(const_cast<osg_solve*>(s), value, s->value.get(), sizeof(double) * s->n, on_host);
}

extern "C" int osg_solve_optimal(const osg_solve* s, uint32_t* mask, int32_t* distance, int on_host) {
  if (!s) return set_error(OSG_ERR_INVALID, "osg_solve_optimal: null argument");
  osg_solve* m = const_cast<osg_solve*>(s);
  if (mask) if (int rc = copy_out(m, mask, s->optimal.get(), sizeof(uint32_t) * s->mask_words * s->n, on_host)) return rc;
  if (distance) if (int rc = copy_out(m, distance, s->distance.get(), sizeof(int32_t) * s->n, on_host)) return rc;
  return OSG_OK;
}

extern "C" int osg_solve_edges(const osg_solve* s, int64_t* edge_off, int32_t* action, int64_t* child, int on_host) {
  if (!s) return set_error(OSG_ERR_INVALID, "osg_solve_edges: null argument");
  osg_solve* m = const_cast<osg_solve*>(s);
  if (edge_off) if (int rc = copy_out(m, edge_off, s->edge_off.get(), sizeof(int64_t) * (s->n + 1), on_host)) return rc;
  if (action && s->edges) if (int rc = copy_out(m, action, s->edge_action.get(), sizeof(int32_t) * s->edges, on_host)) return rc;
  if (child && s->edges) if (int rc = copy_out(m, child, s->edge_child.get(), sizeof(int64_t) * s->edges, on_host)) return rc;
  return OSG_OK;
}

extern "C" int osg_solve_lookup(const osg_solve* s, const osg_batch* query, int64_t* index, int on_host) {
  if (!s || !query || !index) return set_error(OSG_ERR_INVALID, "osg_solve_lookup: null argument");
  if (std::string(query->spec.desc.canonical) != s->spec.desc.canonical)
    return set_error(OSG_ERR_INVALID, "osg_solve_lookup: the batch is of another game");
  const int64_t nq = query->n;
  if (nq == 0) return OSG_OK;
  osg_ctx* ctx = s->ctx;
  int64_t* d_index = index;
  if (on_host) {
    void* scratch = nullptr;
    if (int rc = osg_ctx_scratch(ctx, sizeof(int64_t) * nq, &scratch)) return rc;
    d_index = static_cast<int64_t*>(scratch);
  }
  const int levels = static_cast<int>(s->level_off.size()) - 1;
  if (int rc = for_game(s->spec, [&](auto g, const auto& P) -> int {
        using G = typename decltype(g)::type;
        if constexpr (!solve_served<G>()) return set_error(OSG_ERR_UNSUPPORTED, "osg_solve_lookup: no enumeration for this game layout");
        else {
          k_solve_lookup<G><<<dim3(solve_grid(nq)), dim3(kSolveBlock), 0, ctx->stream>>>(
              P, static_cast<const typename G::word_t*>(query->words()), nq, s->d_level_off.get(), levels,
              s->key_lo.get(), s->wide ? s->key_hi.get() : nullptr, d_index);
          return OSG_OK;
        }
      })) return rc;
  OSG_HIP(hipGetLastError());
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(index, d_index, sizeof(int64_t) * nq, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return OSG_OK;
}
