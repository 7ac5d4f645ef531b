// The fused step: successor record, legal mask and status byte of every state in one launch (osg_step).
// File map: osg_batch_internal.h.
#include "osg_batch_internal.h"
#include "osg_c4_step.h"
#include "step/osg_c4_step_split.h"
#include "osg_ttt_step.h"

namespace {

// The fused headline kernel (connect_four = 35 B per state:
// 16 B state in + 16 B out + 1 B action + 1 B mask + 1 B status).
OSG_D uint8_t encode_status(bool terminal, bool illegal, int cur, int outcome) {
  uint8_t v = illegal ? 0x40 : 0;
  if (terminal) return v | 0x80 | static_cast<uint8_t>(outcome & 7);
  return v | static_cast<uint8_t>((cur + 1) & 15);
}
// (connect_four geometries without a stored result take C4T::fused_step: one pass instead of the generic sequence)
template <class G> struct has_fused_step : std::false_type {};
template <int R, int C, int K, class BB> struct has_fused_step<C4T<R, C, K, BB>> : std::integral_constant<bool, !C4T<R, C, K, BB>::kStored> {};
template <class G, typename MaskT>
__global__ void __launch_bounds__(kBlock)
k_step(typename G::Params p, const typename G::word_t* src, typename G::word_t* dst, int64_t n,
       const uint8_t* actions, MaskT* mask_out, int mask_elems, uint8_t* status) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  typename G::State s = G::load(p, src, n, i);
  int a = actions[i];
  if constexpr (has_fused_step<G>::value) {
    bool illegal_f, term_f;
    int outcome_f;
    const uint32_t open = G::fused_step(p, s, a, illegal_f, term_f, outcome_f);
    G::store(p, dst, n, i, s);
    if (sizeof(MaskT) < 4) {
      mask_out[i] = static_cast<MaskT>(open);
    } else {
#pragma unroll
      for (int w = 0; w < G::kMaskW; ++w)
        if (w < mask_elems) mask_out[i * mask_elems + w] = static_cast<MaskT>(w == 0 ? open : 0u);
    }
    status[i] = encode_status(term_f, illegal_f, term_f ? 0 : (G::plies(s) & 1), term_f ? outcome_f : 0);
    return;
  }
  bool illegal = false;
  if (a != 0xFF) {
    auto before = G::legal(p, s);
    if (a < 32 * G::kMaskW && before.test(a)) G::apply(p, s, a); else illegal = true;
  }
  G::store(p, dst, n, i, s);  // (plain stores: non-temporal ones measured mixed here — hex 22.8 -> 24.6 us at 2^20, 118 -> 104 at 2^22)
  bool term = G::terminal(p, s);
  auto after = G::legal(p, s);
  if (sizeof(MaskT) < 4) {
    mask_out[i] = static_cast<MaskT>(after.w[0]);
  } else {
#pragma unroll
    for (int w = 0; w < G::kMaskW; ++w)  // static indices only (see k_legal_mask)
      if (w < mask_elems) mask_out[i * mask_elems + w] = static_cast<MaskT>(after.w[w]);
  }
  status[i] = encode_status(term, illegal, term ? 0 : G::current_player(p, s), term ? G::outcome_code(p, s) : 0);
}

// The fused step for the games whose state is one or two words (tic_tac_toe 4 B, kuhn_poker 8 B, leduc_poker
// 2 x 8 B): V consecutive states per thread so that every plane access is ONE 16-byte vector load / store per lane
// (1 KiB per wave-instruction) instead of V narrow ones, and the V actions / masks / statuses move as one word.
// The per-state code is the generic one (G::legal / apply / terminal) on a register-resident mini-batch.
template <class G, typename MaskT, int V, int W>  // W = words per state
__global__ void __launch_bounds__(kBlock)
k_step_vec(typename G::Params p, const typename G::word_t* src, typename G::word_t* dst, int64_t n,  // src may BE dst (in-place step)
           const uint8_t* __restrict__ actions, MaskT* __restrict__ mask_out, uint8_t* __restrict__ status) {
  using word_t = typename G::word_t;
  typedef word_t wvec __attribute__((ext_vector_type(V)));
  typedef uint8_t bvec __attribute__((ext_vector_type(V)));
  typedef MaskT mvec __attribute__((ext_vector_type(V)));
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (i >= n) return;
  word_t tmp[W * V];  // plane-major mini-batch: G::load(p, tmp, V, j) reads tmp[w * V + j]
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const wvec v = *reinterpret_cast<const wvec*>(src + w * n + i);
#pragma unroll
    for (int j = 0; j < V; ++j) tmp[w * V + j] = v[j];
  }
  const bvec av = *reinterpret_cast<const bvec*>(actions + i);
  bvec sv;
  mvec mv;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if constexpr (std::is_same<G, Ttt>::value) {
      // the whole step as straight-line code on the packed word, both players' lines in one pass (osg_ttt_step.h)
      const uint32_t r = ttt_fused_step(tmp[j], av[j]);
      mv[j] = static_cast<MaskT>(r & 0xFFFFu);
      sv[j] = static_cast<uint8_t>(r >> 16);
      continue;
    }
    typename G::State s = G::load(p, tmp, V, j);
    const int a = av[j];
    bool illegal = false;
    if (a != 0xFF) {
      const auto before = G::legal(p, s);
      if (a < 32 * G::kMaskW && before.test(a)) G::apply(p, s, a); else illegal = true;
    }
    G::store(p, tmp, V, j, s);
    const bool term = G::terminal(p, s);
    const auto after = G::legal(p, s);
    mv[j] = static_cast<MaskT>(after.w[0]);
    sv[j] = encode_status(term, illegal, term ? 0 : G::current_player(p, s), term ? G::outcome_code(p, s) : 0);
  }
#pragma unroll
  for (int w = 0; w < W; ++w) {
    wvec v;
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = tmp[w * V + j];
    // non-temporal, as in k_step_c4std (2^24 states: kuhn 52.6 -> 49.4 us, leduc 103.1 -> 92.9 us, tic_tac_toe unchanged)
    __builtin_nontemporal_store(v, reinterpret_cast<wvec*>(dst + w * n + i));
  }
  __builtin_nontemporal_store(mv, reinterpret_cast<mvec*>(mask_out + i));
  __builtin_nontemporal_store(sv, reinterpret_cast<bvec*>(status + i));
}

// hex: the fused step with V consecutive states per thread.  A hex(9) state is 13 planes of 32-bit words: with one
// state per thread every plane access moves 4 bytes per lane (256 B per wave-instruction, 26 such streams per launch);
// with V = 2 it is 8 bytes per lane and plane, and the V legal masks of a thread (NW words each, rows of the [n, NW]
// output) are one contiguous span written as NW vectors.  kNt: the successor records, masks and status bytes leave
// through non-temporal stores (batches beyond the Infinity Cache).  The rules are the generic HexT<NW>::legal /
// apply on a register-resident mini-batch (the flood runs only for a placement that touches an edge-connected
// group or an edge, hex.cc:253-276).  Measured (MI355X, 118 B per step, profiles/r03_hex_step.log; V:nt):
//   2^20 states  1:0 22.2 us   2:0 20.1 us   2:1 23.4   4:0 23.2   4:1 29.0
//   2^22 states  1:0 90.2 us   2:0 97.0      2:1 80.8   4:0 99.5   4:1 96.3
//   2^24 states  1:0 334.7 us  2:0 335.3     2:1 330.1  4:0 337.7  4:1 350.7   (0.74-0.75 of 8 TB/s: DRAM)
// Four states per thread (94 vector registers, four divergent floods in a row) never pays; two do, with ordinary
// stores while the batch fits the Infinity Cache and non-temporal ones beyond.
// kMask = false (round 5; osg_step with d_mask == NULL): the successor's mask row is not written — on a hex board it
// is ~occupied of the successor record, which the caller holds anyway (SURVEY.md 8(d) prices the hex step without
// it: 109 B instead of 118 B moved for hex(9)).
template <int NW, int V, bool kNt, bool kMask = true, bool kFold = false>
__global__ void __launch_bounds__(kBlock)
k_step_hexvec(typename HexT<NW>::Params p, const uint32_t* src, uint32_t* dst, int64_t n,  // src may BE dst
              const uint8_t* __restrict__ actions, uint32_t* __restrict__ mask_out, uint8_t* __restrict__ status) {
  using G = HexT<NW>;
  constexpr int W = kFold ? 4 * NW : 4 * NW + 1;   // (folded: the meta word rides in the planes' spare bits; hex(9): 12)
  typedef uint32_t wvec __attribute__((ext_vector_type(V)));
  typedef uint8_t bvec __attribute__((ext_vector_type(V)));
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (i >= n) return;
  uint32_t tmp[W * V];  // plane-major mini-batch: G::load(p, tmp, V, j) reads tmp[w * V + j]
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const wvec v = *reinterpret_cast<const wvec*>(src + w * n + i);
#pragma unroll
    for (int j = 0; j < V; ++j) tmp[w * V + j] = v[j];
  }
  const bvec av = *reinterpret_cast<const bvec*>(actions + i);
  uint32_t mk[NW * V];  // the thread's V mask rows, in output order
  bvec sv;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    typename G::State s = G::template load_as<kFold>(tmp, V, j);
    const int a = av[j];
    bool illegal = false;
    if (a != 0xFF) {
      const auto before = G::legal(p, s);
      if (a < 32 * G::kMaskW && before.test(a)) G::apply(p, s, a); else illegal = true;
    }
    G::template store_as<kFold>(tmp, V, j, s);
    const bool term = G::terminal(p, s);
    if constexpr (kMask) {
      const auto after = G::legal(p, s);
#pragma unroll
      for (int w = 0; w < NW; ++w) mk[j * NW + w] = after.w[w];
    }
    sv[j] = encode_status(term, illegal, term ? 0 : G::current_player(p, s), term ? G::outcome_code(p, s) : 0);
  }
#pragma unroll
  for (int w = 0; w < W; ++w) {
    wvec v;
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = tmp[w * V + j];
    if constexpr (kNt) __builtin_nontemporal_store(v, reinterpret_cast<wvec*>(dst + w * n + i));
    else *reinterpret_cast<wvec*>(dst + w * n + i) = v;
  }
  if constexpr (kMask) {
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      wvec v;
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = mk[k * V + j];
      if constexpr (kNt) __builtin_nontemporal_store(v, reinterpret_cast<wvec*>(mask_out + i * NW) + k);
      else reinterpret_cast<wvec*>(mask_out + i * NW)[k] = v;
    }
  }
  if constexpr (kNt) __builtin_nontemporal_store(sv, reinterpret_cast<bvec*>(status + i));
  else *reinterpret_cast<bvec*>(status + i) = sv;
}

// connect_four, other geometries than 6 x 7 x 4: TWO consecutive states per thread so that every state access is
// one 16-byte vector load/store per lane per plane; actions / masks / statuses move as u16.
constexpr int kC4StepBlock = 128;
template <class G>
__global__ void __launch_bounds__(kC4StepBlock)
k_step_c4x2(typename G::Params p, const uint64_t* src, uint64_t* dst, int64_t n,  // src may BE dst (in-place step)
            const uint8_t* __restrict__ actions, uint8_t* __restrict__ mask_out, uint8_t* __restrict__ status) {
  const int64_t pair = static_cast<int64_t>(blockIdx.x) * kC4StepBlock + threadIdx.x;
  const int64_t i = pair * 2;
  if (i >= n) return;
  const ulonglong2 xs = *reinterpret_cast<const ulonglong2*>(src + i);
  const ulonglong2 os = *reinterpret_cast<const ulonglong2*>(src + n + i);
  const uint32_t a2 = *reinterpret_cast<const uint16_t*>(actions + i);
  uint64_t x[2] = {xs.x, xs.y}, o[2] = {os.x, os.y};
  uint32_t m2 = 0, s2 = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    typename G::State s = G::unpack(x[j], o[j]);
    const int a = (a2 >> (8 * j)) & 0xFF;
    bool term = G::terminal(p, s);
    bool illegal = false;
    if (a != 0xFF) {
      if (!term && G::column_has_room(p, s, a)) {
        G::apply(p, s, a);
        term = G::terminal(p, s);
      } else {
        illegal = true;
      }
    }
    const uint32_t open = G::open_columns(p, s);
    const int to_move = G::plies(s) & 1;
    x[j] = G::pack0(s);
    o[j] = s.o;
    m2 |= (term ? 0u : (open & 0xFFu)) << (8 * j);
    s2 |= static_cast<uint32_t>(encode_status(term, illegal, to_move, term ? G::outcome_code(p, s) : 0)) << (8 * j);
  }
  *reinterpret_cast<ulonglong2*>(dst + i) = make_ulonglong2(x[0], x[1]);
  *reinterpret_cast<ulonglong2*>(dst + n + i) = make_ulonglong2(o[0], o[1]);
  *reinterpret_cast<uint16_t*>(mask_out + i) = static_cast<uint16_t>(m2);
  *reinterpret_cast<uint16_t*>(status + i) = static_cast<uint16_t>(s2);
}

// THE HEADLINE KERNEL (with k_step_c4std2 below): the fused step of the standard connect_four board (6 x 7, four in a
// row), one state per thread, workgroups of 128.  The step is c4_place + c4_finish (step/osg_c4_step_split.h:
// c4_fused_step of osg_c4_step.h cut where the o plane is final and written on the planes' 32-bit halves — ONE line
// test, the mover's, as funnel shifts of the low word; the successor's legal mask gathered by two 24-bit multiplies;
// the result of the game lives in plane 0's spare byte).  Any batch size, no alignment requirement on the side arrays.
// The shape of both kernels (round 10; figures for k_step_c4std2 in profiles/r10a_c4_step_parts.txt):
//  - kExact (the grid covers the batch exactly): no test of i against n, so the wave asks for all its arguments in one
//    scalar clause and its first load waits for one scalar round trip, not two;
//  - the o plane (8 of a state's 18 bytes out) leaves right after placement, ahead of the line tests (the compiler
//    keeps the store there without being told: instruction 99 of 210; a scheduling barrier behind it measured
//    0.016 us slower, profiles/r10a_c4_step_dropped.txt);
//  - stores are non-temporal: the successor records are not read again by this launch, and written around the L2 they
//    neither displace the inputs still to be read nor wait for a write-back at the end of the kernel (measured in
//    round 3: 6.1-6.3 -> 5.0-5.1 us per launch at 2^20 states, 97-99 -> 89-91 us at 2^24; non-temporal LOADS as well: 6.8 us).
template <bool kExact>
__global__ void __launch_bounds__(kC4StepBlock)
k_step_c4std(const uint64_t* src, uint64_t* dst, int64_t n, const uint8_t* __restrict__ actions,  // src may BE dst
             uint8_t* __restrict__ mask_out, uint8_t* __restrict__ status) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kC4StepBlock + threadIdx.x;
  if constexpr (!kExact) {
    if (i >= n) return;
  }
  const C4Placed p = c4_place(src[i], src[n + i], actions[i]);
  __builtin_nontemporal_store((static_cast<uint64_t>(p.no_hi) << 32) | p.no_lo, dst + n + i);
  uint32_t nflags;
  const uint32_t r = c4_finish(p, nflags);
  __builtin_nontemporal_store((static_cast<uint64_t>(p.nx_hi | (nflags << 24)) << 32) | p.nx_lo, dst + i);
  __builtin_nontemporal_store(static_cast<uint8_t>(r), mask_out + i);
  __builtin_nontemporal_store(static_cast<uint8_t>(r >> 8), status + i);
}

// The same step with TWO consecutive states per thread (16-byte plane accesses, u16 side arrays) for even batches
// with 2-byte aligned side arrays — the headline configuration: 2^20 states are 8 192 wavefronts, ONE round of the
// chip's wave slots, so nothing of a launch overlaps a later round and the path from the first scalar load to the last
// store is what a launch costs beyond its bytes.  Both placements, the o plane's store, both finishes, the rest.
// Workgroups of ONE wavefront (round 10): 4.38 -> 4.07 us per launch at 2^20 states against workgroups of 128, 86.9 ->
// 86.2 us at 2^24 (profiles/r10a_c4_step_parts.txt, c3 / c4; workgroups of 256: 4.53 against 4.27 in the run of
// profiles/r10a_c4_step_dropped.txt) — a wavefront that need not start beside a second one starts sooner.
// Per lane of two states (hipcc -S, gfx950, exact form): 181 vector instructions, 14 of them 64-bit — 7 in the step (the
// columns' cells 2 shifts, the dropped stones 2 shifts, their tests 2 compares, the byte offset 1 shift) and 7 address
// adds — so 195 issue slots, 34 VGPRs; before round 10: 202, 35 (26 + 9), 237, 37.
constexpr int kC4PairBlock = 64;
template <bool kExact>
__global__ void __launch_bounds__(kC4PairBlock)
k_step_c4std2(const uint64_t* src, uint64_t* dst, int64_t n, const uint8_t* __restrict__ actions,  // src may BE dst
              uint8_t* __restrict__ mask_out, uint8_t* __restrict__ status) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kC4PairBlock + threadIdx.x) * 2;
  if constexpr (!kExact) {
    if (i >= n) return;
  }
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  typedef uint8_t u8x2 __attribute__((ext_vector_type(2)));
  const u64x2 xs = *reinterpret_cast<const u64x2*>(src + i), os = *reinterpret_cast<const u64x2*>(src + n + i);
  const u8x2 av = *reinterpret_cast<const u8x2*>(actions + i);
  const C4Placed p0 = c4_place(xs.x, os.x, av.x), p1 = c4_place(xs.y, os.y, av.y);
  u64x2 xo, oo;
  oo.x = (static_cast<uint64_t>(p0.no_hi) << 32) | p0.no_lo;
  oo.y = (static_cast<uint64_t>(p1.no_hi) << 32) | p1.no_lo;
  __builtin_nontemporal_store(oo, reinterpret_cast<u64x2*>(dst + n + i));
  uint32_t f0, f1;
  const uint32_t r0 = c4_finish(p0, f0), r1 = c4_finish(p1, f1);
  xo.x = (static_cast<uint64_t>(p0.nx_hi | (f0 << 24)) << 32) | p0.nx_lo;
  xo.y = (static_cast<uint64_t>(p1.nx_hi | (f1 << 24)) << 32) | p1.nx_lo;
  u8x2 mo, so;
  mo.x = static_cast<uint8_t>(r0); mo.y = static_cast<uint8_t>(r1);
  so.x = static_cast<uint8_t>(r0 >> 8); so.y = static_cast<uint8_t>(r1 >> 8);
  __builtin_nontemporal_store(xo, reinterpret_cast<u64x2*>(dst + i));
  __builtin_nontemporal_store(mo, reinterpret_cast<u8x2*>(mask_out + i));
  __builtin_nontemporal_store(so, reinterpret_cast<u8x2*>(status + i));
}

}  // namespace

extern "C" {

int osg_step(const osg_batch* src, osg_batch* dst, const uint8_t* d_actions, void* d_mask, uint8_t* d_status) {
  if (!same_game(dst, src) || dst->n != src->n) return set_error(OSG_ERR_INVALID, "osg_step: shape mismatch");
  if (src->spec.desc.num_distinct_actions > 255)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_step: action ids travel as one byte here (0xFF = skip); games with more than 255 "
                                          "actions (hex above 15 x 15) step through osg_apply / osg_env_step (32-bit actions)");
  osg_ctx* ctx = dst->ctx;
  const int cmb = src->spec.desc.compact_mask_bytes;
  const int W = src->spec.desc.mask_words;
  const int64_t n = src->n;
  // d_mask == NULL ("do not write the successor's mask"): hex only, where the mask is ~occupied of the successor record
  // (a board of up to 16 cells has a 1- or 2-byte compact mask; with no mask to write its format does not matter)
  if (!d_mask && !(src->spec.desc.game_kind == kHex && W == src->spec.hex_nw && W <= 4))
    return set_error(OSG_ERR_UNSUPPORTED, "osg_step: d_mask may be NULL only for hex boards of up to 128 cells (there the successor's "
                                          "mask is ~occupied of the record written); every other game's mask comes from the step itself");
  // the kernels that move several states per lane use 16-byte plane accesses: planes start 16-byte aligned when the
  // allocation does (hipMalloc: 256 B) and n x word size is a multiple of 16 — checked here, not assumed
  const bool planes16 = ((reinterpret_cast<uintptr_t>(src->words()) | reinterpret_cast<uintptr_t>(dst->words())) & 15u) == 0;
  if (planes16 && src->spec.desc.game_kind == kC4 && src->spec.c4_std && (n & 1) == 0 &&
      ((reinterpret_cast<uintptr_t>(d_actions) | reinterpret_cast<uintptr_t>(d_mask) | reinterpret_cast<uintptr_t>(d_status)) & 1u) == 0) {
    with_bool(n % (2 * kC4PairBlock) == 0, [&](auto exact) {   // (the grid covers the batch exactly: no bound test in the kernel)
      k_step_c4std2<decltype(exact)::value><<<dim3(static_cast<unsigned>((n / 2 + kC4PairBlock - 1) / kC4PairBlock)), dim3(kC4PairBlock), 0, ctx->stream>>>(
          static_cast<const uint64_t*>(src->words()), static_cast<uint64_t*>(dst->words()), n, d_actions,
          static_cast<uint8_t*>(d_mask), d_status);
      return OSG_OK;
    });
    OSG_HIP(hipGetLastError());
    return OSG_OK;
  }
  if (src->spec.desc.game_kind == kC4 && src->spec.c4_std) {  // odd batches / unaligned side arrays: one state per thread
    with_bool(n % kC4StepBlock == 0, [&](auto exact) {
      k_step_c4std<decltype(exact)::value><<<dim3(static_cast<unsigned>((n + kC4StepBlock - 1) / kC4StepBlock)), dim3(kC4StepBlock), 0, ctx->stream>>>(
          static_cast<const uint64_t*>(src->words()), static_cast<uint64_t*>(dst->words()), n, d_actions,
          static_cast<uint8_t*>(d_mask), d_status);
      return OSG_OK;
    });
    OSG_HIP(hipGetLastError());
    return OSG_OK;
  }
  const bool aligned2 = ((reinterpret_cast<uintptr_t>(d_actions) | reinterpret_cast<uintptr_t>(d_mask) |
                          reinterpret_cast<uintptr_t>(d_status)) & 1u) == 0;
  // (k_step_c4x2 writes ONE mask byte per state: boards of up to 8 columns.  A 64-bit board can have up to 32 — 2 x 19,
  // 1 x 32: a two- or four-byte mask —, which the generic kernel below writes in the format the description names)
  if (planes16 && src->spec.desc.game_kind == kC4 && !src->spec.c4_wide && (n & 1) == 0 && aligned2 && cmb == 1) {
    const int64_t pairs = n / 2;
    k_step_c4x2<C4><<<dim3(static_cast<unsigned>((pairs + kC4StepBlock - 1) / kC4StepBlock)), dim3(kC4StepBlock), 0, ctx->stream>>>(
        src->spec.c4, static_cast<const uint64_t*>(src->words()), static_cast<uint64_t*>(dst->words()), n, d_actions,
        static_cast<uint8_t*>(d_mask), d_status);
    OSG_HIP(hipGetLastError());
    return OSG_OK;
  }
  // one- and two-word states: V states per thread, 16-byte accesses (needs n % V == 0 and aligned side arrays)
  const uintptr_t side = reinterpret_cast<uintptr_t>(d_actions) | reinterpret_cast<uintptr_t>(d_mask) | reinterpret_cast<uintptr_t>(d_status);
  const int kind = src->spec.desc.game_kind;
  if (planes16 && kind == kTtt && (n & 3) == 0 && (side & 7u) == 0 && cmb == 2) {  // (8 states per thread measured slower)
    k_step_vec<Ttt, uint16_t, 4, 1><<<dim3(grid_for(n / 4)), dim3(kBlock), 0, ctx->stream>>>(
        src->spec.ttt, static_cast<const uint32_t*>(src->words()), static_cast<uint32_t*>(dst->words()), n, d_actions,
        static_cast<uint16_t*>(d_mask), d_status);
    OSG_HIP(hipGetLastError());
    return OSG_OK;
  }
  if (planes16 && kind == kKuhn && (n & 1) == 0 && (side & 1u) == 0 && cmb == 1) {
    k_step_vec<Kuhn, uint8_t, 2, 1><<<dim3(grid_for(n / 2)), dim3(kBlock), 0, ctx->stream>>>(
        src->spec.kuhn, static_cast<const uint64_t*>(src->words()), static_cast<uint64_t*>(dst->words()), n, d_actions,
        static_cast<uint8_t*>(d_mask), d_status);
    OSG_HIP(hipGetLastError());
    return OSG_OK;
  }
  // leduc_poker: its step is bound by the rules' arithmetic more than by the width of the plane accesses — two states
  // per thread pay off only once the batch is many rounds of wavefronts (2^24 states: 106.6 vs 114.1 us), smaller
  // batches run faster with one state per thread and twice the wavefronts (2^20 states: 9.6 vs 8.9 us;
  // tools/probe_states_per_thread.py, tools/probe_kernels.py)
  if (planes16 && kind == kLeduc && !src->spec.leduc_big && n >= (int64_t{1} << 22) && (n & 1) == 0 && (side & 1u) == 0 && cmb == 1) {
    k_step_vec<Leduc, uint8_t, 2, 2><<<dim3(grid_for(n / 2)), dim3(kBlock), 0, ctx->stream>>>(
        src->spec.leduc, static_cast<const uint64_t*>(src->words()), static_cast<uint64_t*>(dst->words()), n, d_actions,
        static_cast<uint8_t*>(d_mask), d_status);
    OSG_HIP(hipGetLastError());
    return OSG_OK;
  }
  // hex: V states per thread (16-byte plane accesses with V = 4); the mask rows are the [n, NW] u32 output
  if (kind == kHex && (cmb == 4 * W || !d_mask) && W == src->spec.hex_nw && W <= 4) {   // (the big boards: one state per thread, below)
    // OSG_HEX_STEP="<states per thread>:<non-temporal 0|1>" overrides the choice (a tuning knob; results do not depend on it)
    int v = 2, nt = n >= (int64_t{1} << 22) ? 1 : 0;
    if (const char* e = std::getenv("OSG_HEX_STEP")) {
      int ev = 0, ent = 0;
      if (std::sscanf(e, "%d:%d", &ev, &ent) == 2 && (ev == 1 || ev == 2)) { v = ev; nt = ent ? 1 : 0; }
    }
    while (v > 1 && ((n % v) != 0 || (side & static_cast<uintptr_t>(v - 1)) != 0 ||
                     (reinterpret_cast<uintptr_t>(d_mask) & static_cast<uintptr_t>(4 * v - 1)) != 0 || !planes16))
      v >>= 1;
    if (v > 1) {
      const auto* s32 = static_cast<const uint32_t*>(src->words());
      auto* d32 = static_cast<uint32_t*>(dst->words());
      auto* m32 = static_cast<uint32_t*>(d_mask);
      if (int rc = for_hex(src->spec, [&](auto nw, const auto& P) -> int {
            constexpr int NW = decltype(nw)::value;
            if constexpr (NW <= 4) {   // (the test above: W <= 4)
              return with_bool(src->spec.hex_fold, [&](auto fold) {
                return with_bool(nt != 0, [&](auto ntv) {
                  return with_bool(m32 != nullptr, [&](auto mask) {
                    k_step_hexvec<NW, 2, decltype(ntv)::value, decltype(mask)::value, decltype(fold)::value>
                        <<<dim3(grid_for(n / 2)), dim3(kBlock), 0, ctx->stream>>>(P, s32, d32, n, d_actions, m32, d_status);
                    return OSG_OK;
                  });
                });
              });
            }
            return OSG_OK;
          })) return rc;
      OSG_HIP(hipGetLastError());
      return OSG_OK;
    }
  }
  if (!d_mask)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_step: d_mask may be NULL only for hex boards of up to 128 cells stepped two states per "
                                          "thread (an even batch, 2-byte aligned side arrays): there the successor's mask is ~occupied "
                                          "of the record written; every other game's mask is computed by the step itself");
  const auto step = [&](auto m, int mask_stride) {   // m: one element of the compact mask
    using M = decltype(m);
    return for_game(src->spec, [&](auto g, const auto& P) {
      using G = typename decltype(g)::type;
      k_step<G, M><<<dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream>>>(P, static_cast<const typename G::word_t*>(src->words()),
          static_cast<typename G::word_t*>(dst->words()), n, d_actions,
          static_cast<M*>(d_mask), mask_stride, d_status);
      return OSG_OK;
    });
  };
  if (int rc = cmb == 1 ? step(uint8_t{}, 1) : cmb == 2 ? step(uint16_t{}, 1) : step(uint32_t{}, W)) return rc;
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}

}  // extern "C"
