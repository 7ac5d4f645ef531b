// The batch itself: its lifetime, copies between batches and to / from the host, and the per-state queries (legal
// mask, apply, status, chance probabilities).  File map: osg_batch_internal.h.
#include <memory>

#include "osg_batch_internal.h"

namespace {

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
template <class G>
__global__ void __launch_bounds__(kBlock) k_init(typename G::Params p, typename G::word_t* base, int64_t n) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  G::store(p, base, n, i, G::initial(p));
}

// 16 bytes per lane, 4 KiB per workgroup: the plain-copy ceiling (osg_copy_bytes).
__global__ void __launch_bounds__(256) k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  // non-temporal stores, like the kernels it is the ceiling of (a copy with plain stores is slower: §9)
  if (i < n16) {
    const uint4 v = src[i];
    __builtin_nontemporal_store(v.x, &dst[i].x);
    __builtin_nontemporal_store(v.y, &dst[i].y);
    __builtin_nontemporal_store(v.z, &dst[i].z);
    __builtin_nontemporal_store(v.w, &dst[i].w);
  }
}

template <class G>
__global__ void __launch_bounds__(kBlock)
k_gather(typename G::Params p, typename G::word_t* dst, int64_t nd, const typename G::word_t* src, int64_t ns,
         const int64_t* index, unsigned long long* illegal) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= nd) return;
  int64_t j = index[i];
  if (j < 0 || j >= ns) {  // device-resident indices cannot be checked on the host: initial state + counted
    G::store(p, dst, nd, i, G::initial(p));
    atomicAdd(illegal, 1ull);
    return;
  }
  for (int k = 0; k < p.words; ++k) dst[k * nd + i] = src[k * ns + j];
}

template <class G>
__global__ void __launch_bounds__(kBlock)
k_legal_mask(typename G::Params p, const typename G::word_t* base, int64_t n, uint32_t* mask, int mask_words) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  auto m = G::legal(p, G::load(p, base, n, i));
#pragma unroll
  for (int w = 0; w < G::kMaskW; ++w)  // static indices only: a runtime index would spill the mask to scratch
    if (w < mask_words) mask[i * mask_words + w] = m.w[w];
}

template <class G>
__global__ void __launch_bounds__(kBlock)
k_apply(typename G::Params p, typename G::word_t* base, int64_t n, const int32_t* actions,
        unsigned long long* illegal) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  int a = actions[i];
  if (a == OSG_INVALID_ACTION) return;
  typename G::State s = G::load(p, base, n, i);
  auto m = G::legal(p, s);
  if (a < 0 || a >= 32 * G::kMaskW || !m.test(a)) {
    atomicAdd(illegal, 1ull);  // the compiler folds this into one add per wave
    return;
  }
  G::apply(p, s, a);
  G::store(p, base, n, i, s);
}

template <class G>
__global__ void __launch_bounds__(kBlock)
k_status(typename G::Params p, const typename G::word_t* base, int64_t n, int num_players, int8_t* cur,
         uint8_t* term, double* rets) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  typename G::State s = G::load(p, base, n, i);
  if (cur) cur[i] = static_cast<int8_t>(G::current_player(p, s));
  if (term) term[i] = G::terminal(p, s) ? 1 : 0;
  if (rets) {
    double r[kMaxPlayers];
    G::returns(p, s, r);
    for (int q = 0; q < num_players; ++q) rets[i * num_players + q] = r[q];
  }
}

template <class G>
__global__ void __launch_bounds__(kBlock)
k_chance_probs(typename G::Params p, const typename G::word_t* base, int64_t n, int max_chance, double* probs) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  typename G::State s = G::load(p, base, n, i);
  bool chance = G::current_player(p, s) == kChancePlayer;
  auto m = G::legal(p, s);
  for (int o = 0; o < max_chance; ++o)
    probs[i * max_chance + o] = (chance && m.test(o)) ? G::chance_prob(p, s, o) : 0.0;
}

// ---------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------
int stage_in(osg_ctx* ctx, const void* ptr, size_t bytes, int on_host, size_t scratch_offset, const void** dev) {
  if (!on_host) { *dev = ptr; return OSG_OK; }
  void* scratch = nullptr;
  int rc = osg_ctx_scratch(ctx, scratch_offset + bytes, &scratch);
  if (rc) return rc;
  void* d = static_cast<char*>(scratch) + scratch_offset;
  OSG_HIP(hipMemcpyAsync(d, ptr, bytes, hipMemcpyHostToDevice, ctx->stream));
  *dev = d;
  return OSG_OK;
}

}  // namespace

// One thread builds the position from its cells with the game's own rules and stores it in the batch's layout.
template <class G>
__global__ void k_set_cells(typename G::Params P, typename G::word_t* words, int64_t n, int64_t index,
                            const unsigned char* cells, int n_cells, int* err) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  typename G::State s;
  const int e = G::from_cells(P, cells, n_cells, s);
  *err = e;
  if (e == 0) G::store(P, words, n, index, s);
}

extern "C" {

int osg_batch_create(osg_ctx* ctx, const char* game_string, int64_t n, osg_batch** out) {
  if (!ctx || !out || n <= 0) return set_error(OSG_ERR_INVALID, "osg_batch_create: bad argument");
  if (ctx->closed) return set_error(OSG_ERR_INVALID, "osg_batch_create: the context was destroyed");
  auto b = std::make_unique<osg_batch>();
  int rc = parse_game(game_string, &b->spec);
  if (rc) return rc;
  b->ctx = ctx;
  b->n = n;
  rc = nomem_error(b->d_words.alloc(static_cast<size_t>(n) * b->spec.desc.state_words * b->spec.desc.state_word_bytes));
  if (rc) return rc;
  rc = osg_batch_reset(b.get());
  if (rc) return rc;
  osg::ctx_retain(ctx);
  *out = b.release();
  return OSG_OK;
}

int osg_batch_destroy(osg_batch* b) {
  if (!b) return OSG_OK;
  (void)hipStreamSynchronize(b->ctx->stream);
  osg_ctx* ctx = b->ctx;
  delete b;  // frees the planes
  osg::ctx_release(ctx);
  return OSG_OK;
}
int64_t osg_batch_size(const osg_batch* b) { return b->n; }
int osg_batch_describe(const osg_batch* b, osg_game_desc* out) { *out = b->spec.desc; return OSG_OK; }
void* osg_batch_device_ptr(osg_batch* b) { return b->words(); }

int osg_batch_reset(osg_batch* b) {
  if (int rc = for_game(b->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_init<G><<<dim3(grid_for(b->n)), dim3(kBlock), 0, b->ctx->stream>>>(P,
            static_cast<typename G::word_t*>(b->words()), b->n);
        return OSG_OK;
      })) return rc;
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

int osg_batch_copy(osg_batch* dst, const osg_batch* src) {
  if (!same_game(dst, src) || dst->n != src->n) return set_error(OSG_ERR_INVALID, "osg_batch_copy: shape mismatch");
  OSG_HIP(hipMemcpyAsync(dst->words(), src->words(), src->d_words.size(), hipMemcpyDeviceToDevice, dst->ctx->stream));
  return OSG_OK;
}

int osg_batch_gather(osg_batch* dst, const osg_batch* src, const int64_t* index, int on_host) {
  if (!same_game(dst, src)) return set_error(OSG_ERR_INVALID, "osg_batch_gather: different games");
  if (!index) return set_error(OSG_ERR_INVALID, "osg_batch_gather: null index");
  if (on_host)
    for (int64_t i = 0; i < dst->n; ++i)
      if (index[i] < 0 || index[i] >= src->n) return set_error(OSG_ERR_INVALID, "osg_batch_gather: index out of range");
  const void* d_index = nullptr;
  int rc = stage_in(dst->ctx, index, sizeof(int64_t) * dst->n, on_host, 0, &d_index);
  if (rc) return rc;
  if (int rc = for_game(dst->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_gather<G><<<dim3(grid_for(dst->n)), dim3(kBlock), 0, dst->ctx->stream>>>(P,
            static_cast<typename G::word_t*>(dst->words()), dst->n,
            static_cast<const typename G::word_t*>(src->words()), src->n,
            static_cast<const int64_t*>(d_index), dst->ctx->d_illegal);
        return OSG_OK;
      })) return rc;
  OSG_HIP(hipGetLastError());
  if (on_host) OSG_HIP(hipStreamSynchronize(dst->ctx->stream));
  return OSG_OK;
}

int osg_copy_bytes(osg_ctx* ctx, void* d_dst, const void* d_src, int64_t bytes) {
  if (!ctx || !d_dst || !d_src || bytes < 0 || (bytes & 15) || (reinterpret_cast<uintptr_t>(d_dst) & 15) ||
      (reinterpret_cast<uintptr_t>(d_src) & 15))
    return set_error(OSG_ERR_INVALID, "osg_copy_bytes: null / unaligned argument");
  const int64_t n16 = bytes / 16;
  if (n16 == 0) return OSG_OK;
  k_copy16<<<dim3(static_cast<unsigned>((n16 + 255) / 256)), dim3(256), 0, ctx->stream>>>(
      static_cast<const uint4*>(d_src), static_cast<uint4*>(d_dst), n16);
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

int osg_batch_download(const osg_batch* b, void* h_words) {
  OSG_HIP(hipMemcpyAsync(h_words, b->words(), b->d_words.size(), hipMemcpyDeviceToHost, b->ctx->stream));
  OSG_HIP(hipStreamSynchronize(b->ctx->stream));
  return OSG_OK;
}
int osg_batch_upload(osg_batch* b, const void* h_words) {
  OSG_HIP(hipMemcpyAsync(b->words(), h_words, b->d_words.size(), hipMemcpyHostToDevice, b->ctx->stream));
  OSG_HIP(hipStreamSynchronize(b->ctx->stream));
  return OSG_OK;
}

int osg_batch_set_cells(osg_batch* b, int64_t index, const char* cells, int n_cells) {
  if (!b || !cells || index < 0 || index >= b->n || n_cells <= 0 || n_cells > 4096)
    return osg::set_error(OSG_ERR_INVALID, "osg_batch_set_cells: bad argument");
  osg_ctx* ctx = b->ctx;
  void* scratch;
  if (int rc = osg_ctx_scratch(ctx, 4096 + sizeof(int), &scratch)) return rc;
  unsigned char* d_cells = static_cast<unsigned char*>(scratch);
  int* d_err = reinterpret_cast<int*>(d_cells + 4096);
  OSG_HIP(hipMemcpyAsync(d_cells, cells, static_cast<size_t>(n_cells), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = for_game(b->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        if constexpr (std::is_same_v<G, Ttt> || std::is_same_v<typename G::Params, C4::Params>) {
          k_set_cells<G><<<dim3(1), dim3(64), 0, ctx->stream>>>(P, static_cast<typename G::word_t*>(b->words()), b->n, index,
                                                                d_cells, n_cells, d_err);
          return OSG_OK;
        } else {
          return osg::set_error(OSG_ERR_UNSUPPORTED, "osg_batch_set_cells: tic_tac_toe and connect_four positions (the games whose "
                                                     "reference State has a constructor from a board)");
        }
      })) return rc;
  OSG_HIP(hipGetLastError());
  int err = 0;
  OSG_HIP(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  switch (err) {
    case 0: return OSG_OK;
    case 1: return osg::set_error(OSG_ERR_INVALID, "osg_batch_set_cells: the board does not have the game's number of cells");
    case 2: return osg::set_error(OSG_ERR_INVALID, "osg_batch_set_cells: a cell is not one of '.', 'x', 'o'");
    case 3: return osg::set_error(OSG_ERR_INVALID, "Invalid board: gap in a column. Pieces must be stacked from the bottom with no gaps.");
    default: return osg::set_error(OSG_ERR_INVALID, "Invalid board state: both players have a winning line.");
  }
}

int osg_legal_mask(const osg_batch* b, uint32_t* mask, int on_host) {
  osg_ctx* ctx = b->ctx;
  const int W = b->spec.desc.mask_words;
  size_t bytes = sizeof(uint32_t) * W * b->n;
  uint32_t* d_mask = mask;
  if (on_host) {
    void* scratch;
    int rc = osg_ctx_scratch(ctx, bytes, &scratch);
    if (rc) return rc;
    d_mask = static_cast<uint32_t*>(scratch);
  }
  if (int rc = for_game(b->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_legal_mask<G><<<dim3(grid_for(b->n)), dim3(kBlock), 0, ctx->stream>>>(P,
            static_cast<const typename G::word_t*>(b->words()), b->n, d_mask, W);
        return OSG_OK;
      })) return rc;
  OSG_HIP(hipGetLastError());
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(mask, d_mask, bytes, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return OSG_OK;
}

int osg_apply(osg_batch* b, const int32_t* actions, int on_host, int64_t* h_illegal) {
  osg_ctx* ctx = b->ctx;
  const void* d_actions = nullptr;
  int rc = stage_in(ctx, actions, sizeof(int32_t) * b->n, on_host, 0, &d_actions);
  if (rc) return rc;
  if (int rc = for_game(b->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_apply<G><<<dim3(grid_for(b->n)), dim3(kBlock), 0, ctx->stream>>>(P,
            static_cast<typename G::word_t*>(b->words()), b->n,
            static_cast<const int32_t*>(d_actions), ctx->d_illegal);
        return OSG_OK;
      })) return rc;
  OSG_HIP(hipGetLastError());
  if (on_host || h_illegal) return check_illegal(ctx, h_illegal);
  return OSG_OK;
}

int osg_status_query(const osg_batch* b, int8_t* cur_player, uint8_t* terminal, double* returns, int on_host) {
  osg_ctx* ctx = b->ctx;
  const int P_ = b->spec.desc.num_players;
  int8_t* d_cur = cur_player;
  uint8_t* d_term = terminal;
  double* d_ret = returns;
  size_t off_term = align_up(b->n), off_ret = off_term + align_up(b->n);
  if (on_host) {
    void* scratch;
    int rc = osg_ctx_scratch(ctx, off_ret + sizeof(double) * P_ * b->n, &scratch);
    if (rc) return rc;
    char* sc = static_cast<char*>(scratch);
    d_cur = cur_player ? reinterpret_cast<int8_t*>(sc) : nullptr;
    d_term = terminal ? reinterpret_cast<uint8_t*>(sc + off_term) : nullptr;
    d_ret = returns ? reinterpret_cast<double*>(sc + off_ret) : nullptr;
  }
  if (int rc = for_game(b->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_status<G><<<dim3(grid_for(b->n)), dim3(kBlock), 0, ctx->stream>>>(P,
            static_cast<const typename G::word_t*>(b->words()), b->n, P_, d_cur,
            d_term, d_ret);
        return OSG_OK;
      })) return rc;
  OSG_HIP(hipGetLastError());
  if (on_host) {
    if (cur_player) OSG_HIP(hipMemcpyAsync(cur_player, d_cur, b->n, hipMemcpyDeviceToHost, ctx->stream));
    if (terminal) OSG_HIP(hipMemcpyAsync(terminal, d_term, b->n, hipMemcpyDeviceToHost, ctx->stream));
    if (returns) OSG_HIP(hipMemcpyAsync(returns, d_ret, sizeof(double) * P_ * b->n, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return OSG_OK;
}

int osg_chance_probs(const osg_batch* b, double* probs, int on_host) {
  osg_ctx* ctx = b->ctx;
  const int C = b->spec.desc.max_chance_outcomes;
  if (C == 0) return OSG_OK;
  size_t bytes = sizeof(double) * C * b->n;
  double* d_probs = probs;
  if (on_host) {
    void* scratch;
    int rc = osg_ctx_scratch(ctx, bytes, &scratch);
    if (rc) return rc;
    d_probs = static_cast<double*>(scratch);
  }
  if (int rc = for_game(b->spec, [&](auto g, const auto& P) {
        using G = typename decltype(g)::type;
        k_chance_probs<G><<<dim3(grid_for(b->n)), dim3(kBlock), 0, ctx->stream>>>(P,
            static_cast<const typename G::word_t*>(b->words()), b->n, C, d_probs);
        return OSG_OK;
      })) return rc;
  OSG_HIP(hipGetLastError());
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(probs, d_probs, bytes, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return OSG_OK;
}

}  // extern "C"
