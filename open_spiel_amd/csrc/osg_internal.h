// Library-internal declarations shared by the .hip translation units.
#ifndef OSG_INTERNAL_H_
#define OSG_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/osg_abi.h"
#include "osg_common.h"
#include "osg_device_buffer.h"
#include "osg_game_boards.h"
#include "osg_game_poker.h"
#include "osg_sample.h"

namespace osg {

enum GameKind { kTtt = 0, kC4 = 1, kHex = 2, kKuhn = 3, kLeduc = 4 };

// A parsed, validated game: description + the device parameter block.
struct GameSpec {
  osg_game_desc desc;
  int hex_nw = 0;  // u32 words per hex bit plane: 1..4 (boards of up to 128 actions), 6 / 8 / 12 (up to 19 x 19)
  bool hex_fold = false;  // cells <= 32 * hex_nw - 5: the meta word folded into the planes' spare bits (a 4 * hex_nw word record)
  bool c4_std = false;  // connect_four with the default 6x7x4 geometry (constant-folded kernels)
  bool c4_wide = false;  // connect_four above 64 board bits: two plane words per colour (C4Wide)
  bool leduc_big = false;  // leduc_poker with 4 to 10 players: the five-plane record (LeducBig)
  bool hex_explicit = false;  // hex(string_rep=explicit): edge-connection glyphs in the board string
  Ttt::Params ttt;
  C4::Params c4;
  HexT<1>::Params hex1;
  HexT<2>::Params hex2;
  HexT<3>::Params hex3;
  HexT<4>::Params hex4;
  HexT<6>::Params hex6;    // 13 x 13 (169 cells)
  HexT<8>::Params hex8;    // 15 x 15 (225 cells)
  HexT<12>::Params hex12;  // 19 x 19 (361 cells)
  Kuhn::Params kuhn;
  Leduc::Params leduc;
  std::map<std::string, std::string> params;  // as given + defaults (strings)
};

int set_error(int code, const std::string& msg);

template <class T> struct TypeTag { using type = T; };

// Run-time value -> template argument, as ordinary calls: each hands the visitor `f` a tag whose type carries the
// constant and returns f's int.  A visitor is instantiated for every tag it can be handed; where a kernel exists for a
// part of the range only, the visitor guards the rest with `if constexpr`.
template <class F>
int with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// `v` among the listed constants; a value that is none of them takes the last.
template <int First, int... Rest, class F>
int with_int(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, First>{});
  else return v == First ? f(std::integral_constant<int, First>{}) : with_int<Rest...>(v, f);
}
// The hex layout in use: f(integral_constant<int, NW>, its HexT<NW>::Params).  The one place that pairs hex_nw with
// the members of GameSpec (parse_game fills through it, hence the deduced Spec).
template <class Spec, class F>
int for_hex(Spec& spec, F&& f) {
  switch (spec.hex_nw) {
    case 1: return f(std::integral_constant<int, 1>{}, spec.hex1);
    case 2: return f(std::integral_constant<int, 2>{}, spec.hex2);
    case 3: return f(std::integral_constant<int, 3>{}, spec.hex3);
    case 4: return f(std::integral_constant<int, 4>{}, spec.hex4);
    case 6: return f(std::integral_constant<int, 6>{}, spec.hex6);
    case 8: return f(std::integral_constant<int, 8>{}, spec.hex8);
    default: return f(std::integral_constant<int, 12>{}, spec.hex12);
  }
}
// The concrete game type a spec names: f(TypeTag<G>, its G::Params).  Every layout is here (the hex boards above 128
// actions, connect_four above 64 board bits and leduc_poker with 4+ players included): the batch entry points of
// osg_batch_internal.h's units — states, masks, steps, tensors, random steps, rollouts, environment steps — and the lane-per-root
// searches of osg_mcts.hip / osg_mcts_step.hip go through it.  The wave-per-root search and the solvers' tree builder
// serve fewer layouts and keep switches of their own.
template <class F>
int for_game(const GameSpec& spec, F&& f) {
  switch (spec.desc.game_kind) {
    case kTtt: return f(TypeTag<Ttt>{}, spec.ttt);
    case kC4:
      if (spec.c4_std) return f(TypeTag<C4Std>{}, spec.c4);
      if (spec.c4_wide) return f(TypeTag<C4Wide>{}, spec.c4);
      return f(TypeTag<C4>{}, spec.c4);
    case kKuhn: return f(TypeTag<Kuhn>{}, spec.kuhn);
    case kLeduc:
      if (spec.leduc_big) return f(TypeTag<LeducBig>{}, spec.leduc);
      return f(TypeTag<Leduc>{}, spec.leduc);
    case kHex: return for_hex(spec, [&](auto nw, const auto& p) { return f(TypeTag<HexT<nw.value>>{}, p); });
    default: return set_error(OSG_ERR_INVALID, "bad game kind");
  }
}

// hipFuncAttributeMaxDynamicSharedMemorySize is one value per KERNEL, not per solver / tree: a second user with a
// smaller footprint must not lower the cap under a first one that is still in use.  Raises only; asked of the runtime
// once per (device, kernel) and size step, not per launch.
inline hipError_t raise_lds_cap(const void* kernel, int bytes) {
  static std::mutex mu;
  static std::unordered_map<std::string, int> cap;   // per (device, kernel)
  int device = 0;
  (void)hipGetDevice(&device);
  std::lock_guard<std::mutex> lock(mu);
  int& have = cap[std::to_string(device) + ":" + std::to_string(reinterpret_cast<uintptr_t>(kernel))];
  if (bytes <= have) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}

// Random playouts of hex on a one-row or one-column board never end: with the reference's `else if` between a
// colour's two edges (hex.cc:122-126,146-150) a stone on such a board can only ever carry ONE edge label, so that
// colour never wins and a filled board is a state that is not terminal and has no legal action.  (The reference's
// RandomRolloutEvaluator would index an empty LegalActions() there.)  Entry points that play out refuse these
// boards instead of hanging the device.
inline void hex_dims(const GameSpec& spec, int* rows, int* cols, int* cells) {
  for_hex(spec, [&](auto, const auto& p) { *rows = p.rows; *cols = p.cols; *cells = p.cells; return 0; });
}
inline int refuse_endless_playouts(const GameSpec& spec, const char* who) {
  if (spec.desc.game_kind != kHex) return OSG_OK;
  int rows = 0, cols = 0, cells = 0;
  hex_dims(spec, &rows, &cols, &cells);
  if (rows >= 2 && cols >= 2) return OSG_OK;
  return set_error(OSG_ERR_UNSUPPORTED, std::string(who) + ": hex on a board with a single row or column has states that are "
                   "neither terminal nor have a legal action (one colour can never win): playouts would not end");
}
int parse_game(const char* game_string, GameSpec* out);

}  // namespace osg

namespace osg {
// What osg_ismcts_tree_* need of the context's last osg_ismcts_search (n == 0: none): its trees stay in d_ismcts.
struct IsmctsKept {
  int64_t n = 0, lanes = 0;   // roots searched; lanes of the launch (lane l held roots l, l + lanes, ...)
  int max_nodes = 0, node_words = 0;
  size_t o_draws = 0, o_count = 0, o_table = 0;   // offsets in d_ismcts: draws [n] u32, node counts [n] i32, the tables
  std::string game;   // canonical string of the roots' game
};
}  // namespace osg

struct osg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  osg::DeviceArray<unsigned long long> d_illegal;  // device counter of illegal applies
  // Grow-only, reused from call to call (osg::ctx_grow); osg_ctx_trim gives the scratch, the pools and the queue back.
  osg::DeviceArray<unsigned char> d_scratch;       // reusable staging buffer
  osg::DeviceArray<unsigned char> d_mcts_pool;     // MCTS node pool, reused across searches
  osg::DeviceArray<double> d_mcts_logs;            // log(n) table shared with the host libm
  osg::DeviceArray<int32_t> d_mcts_queue;          // wave-per-root search as a work queue: [0] next ticket, [1..256] the cost
                                                   // histogram / bucket offsets, then the root order [roots]
  osg::DeviceArray<unsigned char> d_ismcts;        // IS-MCTS node tables, hashes and root samples; kept for osg_ismcts_tree_*
  osg::IsmctsKept ismcts;
  int num_cus = 0;
  // Lifetime: the creator holds one reference, every batch / solver / communicator made on the context
  // another; osg_ctx_destroy drops the creator's, and the device resources go with the last one, so a
  // batch destroyed after its context (garbage-collection order in a binding) never touches freed memory.
  int refs = 1;
  bool closed = false;
};
namespace osg {
void ctx_retain(osg_ctx* ctx);
void ctx_release(osg_ctx* ctx);
// Growth of one of the context's grow-only buffers: a request beyond the capacity waits for the context's stream (a
// queued kernel may still use the old block) and reallocates, contents lost; any other request does nothing.
template <class T>
hipError_t ctx_grow(osg_ctx* ctx, DeviceArray<T>& buf, size_t n);
}

struct osg_batch {
  osg_ctx* ctx = nullptr;
  osg::GameSpec spec;
  int64_t n = 0;
  osg::DeviceArray<unsigned char> d_words;  // state_words planes of n elements (u32 or u64: the game's word type)
  void* words() const { return d_words.get(); }
};

#define OSG_HIP(call)                                                              \
  do {                                                                             \
    hipError_t e__ = (call);                                                       \
    if (e__ != hipSuccess)                                                         \
      return osg::set_error(OSG_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

namespace osg {
// A failed allocation as the project's codes: a call site that reported OSG_ERR_HIP goes through OSG_HIP(buf.alloc(n))
// as before; one that reported OSG_ERR_NOMEM with the runtime's text goes through this.
inline int nomem_error(hipError_t e, const std::string& who = std::string()) {
  return e == hipSuccess ? OSG_OK : set_error(OSG_ERR_NOMEM, who + hipGetErrorString(e));
}
// A host vector into a fresh device array of the same length.
template <class T>
int upload(const std::vector<T>& v, DeviceArray<T>& d, hipStream_t stream) {
  OSG_HIP(d.alloc(v.size()));
  if (!v.empty()) {
    OSG_HIP(hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    // The callers pass vectors that die when they return, and a large copy from pageable memory may still be reading
    // the host buffer after the call (seen once as a GPU fault at a host address with an 87 MB vector): wait.
    if (v.size() * sizeof(T) > (64u << 10)) OSG_HIP(hipStreamSynchronize(stream));
  }
  return OSG_OK;
}
}  // namespace osg

// The context's staging buffer, at least `bytes` long (grows by half again beyond a request it cannot hold).
int osg_ctx_scratch(osg_ctx* ctx, size_t bytes, void** out);
namespace osg {
// Offsets of the pieces a caller carves out of it: multiples of 256 bytes, like the allocation itself.
inline size_t align_up(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
// The LDS one workgroup may have on `device`, from its properties (asked once per device).
inline int workgroup_lds_limit(int device, size_t* out) {
  static std::mutex mu;
  static std::map<int, size_t> known;
  std::lock_guard<std::mutex> lock(mu);
  auto it = known.find(device);
  if (it == known.end()) {
    hipDeviceProp_t prop;
    OSG_HIP(hipGetDeviceProperties(&prop, device));
    it = known.emplace(device, prop.sharedMemPerBlockOptin ? prop.sharedMemPerBlockOptin : prop.sharedMemPerBlock).first;
  }
  *out = it->second;
  return OSG_OK;
}
}  // namespace osg

#endif  // OSG_INTERNAL_H_
