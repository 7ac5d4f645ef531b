// Observation / information-state tensors of a batch (osg_observation).  File map: osg_batch_internal.h.
#include "osg_batch_internal.h"

namespace {

// Observation / information-state tensors: write-bound ([n, size] fp32, zero-filled
// then set like ContiguousAllocator / TensorView do, observer.h:174-185).  A row is cut
// into chunks of four floats; one lane produces one chunk — one state load, one cursor,
// four entries, one 16-byte store (the last chunk of a row may be shorter) — so lanes never
// straddle two states and the kernel has no divergent reloads.  Consecutive lanes write
// consecutive addresses (1 KiB per wave-instruction).
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));  // rows are only 4-byte aligned
// Tensor rows are written once and not read again by the kernel: non-temporal stores (see k_step_c4std) — where they
// measured faster (2^24 states, fraction of 8 TB/s, plain -> non-temporal): leduc [n, 16] 0.76 -> 0.89, [n, 30] 0.74 ->
// 0.83, kuhn [n, 7] 0.60 -> 0.67, [n, 11] 0.69 -> 0.76, hex(9) 0.67 -> 0.71; the tic_tac_toe rows keep plain stores
// (0.77 -> 0.70 with non-temporal ones), the connect_four planes take them from 2^22 states on (see the kernel).
OSG_D void store_row4(float4u* dst, const float4u& v) {  // 4-byte aligned rows
  __builtin_nontemporal_store(v, dst);
}
template <bool kNt = true>
OSG_D void store_row4(float4* dst, const float4& v) {  // 16-byte aligned spans
  if constexpr (!kNt) { *dst = v; return; }
  __builtin_nontemporal_store(v.x, &dst->x);
  __builtin_nontemporal_store(v.y, &dst->y);
  __builtin_nontemporal_store(v.z, &dst->z);
  __builtin_nontemporal_store(v.w, &dst->w);
}
template <class G, int F>  // F = floats per lane (a multiple of 4): 4 for short rows, 16 for long ones
__global__ void __launch_bounds__(kBlock)
k_observation(typename G::Params p, const typename G::word_t* base, int64_t n, int size, int seg_len, int chunks_per_seg,
              int player, int which, float* out) {
  // A row of `size` floats is a sequence of segments of `seg_len` floats (hex: one per tensor plane; other
  // games: the whole row); chunks never cross a segment, so a cursor never changes plane mid-chunk.
  // One 64-bit division per workgroup on wave-uniform values; lanes divide a small offset in 32 bits.
  // F == 16: a lane's four float4 pieces are 64 bytes apart from its neighbour's, so storing them directly
  // would make every store instruction hit 64 different cache lines with 16 bytes each.  Instead each
  // wavefront stages its 4 KiB through LDS and writes it back piece-major: instruction j stores pieces
  // 64 j ... 64 j + 63, i.e. whole consecutive chunks -> whole cache lines.
  __shared__ float4 s_tile[F >= 16 ? kBlock * (F / 4) : 1];
  __shared__ float* s_dst[F >= 16 ? kBlock : 1];
  __shared__ int s_count[F >= 16 ? kBlock : 1];
  const int chunks = (size / seg_len) * chunks_per_seg;  // per state
  const int64_t tb = static_cast<int64_t>(blockIdx.x) * kBlock;
  const int64_t ib = tb / chunks;
  const uint32_t local = static_cast<uint32_t>(tb - ib * chunks) + threadIdx.x;
  const uint32_t il = local / static_cast<uint32_t>(chunks);
  const int64_t i = ib + il;
  const bool live = i < n;
  int count = 0;
  float* dst = out;
  float4 q[F / 4];
#pragma unroll
  for (int g = 0; g < F / 4; ++g) q[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (live) {
    const uint32_t c_in_state = local - il * static_cast<uint32_t>(chunks);
    const uint32_t seg = c_in_state / static_cast<uint32_t>(chunks_per_seg);
    const int off = static_cast<int>(c_in_state - seg * chunks_per_seg) * F;  // offset inside the segment
    const int idx = static_cast<int>(seg) * seg_len + off;
    const typename G::State s = G::load(p, base, n, i);
    int pl = player;
    if (pl < 0) {
      pl = G::current_player(p, s);
      if (pl < 0) pl = 0;
    }
    typename G::ObsCursor cur;
    cur.init(p, s, pl, which, idx);
    count = seg_len - off;  // >= 1; only the last chunk of a segment has fewer than F
    if (count > F) count = F;
    dst = out + i * size + idx;
#pragma unroll
    for (int g = 0; g < F / 4; ++g) {
      if (4 * g >= count) break;
      float v[4];  // indexed by unrolled constants only: stays in registers
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (4 * g + k < count) ? cur.next(p, s, pl, which) : 0.0f;
      q[g] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  if (F == 4) {
    if (!live) return;
    if (count >= 4) {
      float4u w = {q[0].x, q[0].y, q[0].z, q[0].w};
      store_row4(reinterpret_cast<float4u*>(dst), w);
    } else {
      dst[0] = q[0].x;
      if (count > 1) dst[1] = q[0].y;
      if (count > 2) dst[2] = q[0].z;
    }
    return;
  }
  // ---- F >= 16: piece-major write-back through LDS (per wavefront; no workgroup barrier needed, every
  //      wave only reads what it wrote itself) ----
  const int lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63;
#pragma unroll
  for (int g = 0; g < F / 4; ++g) s_tile[(wave0 + lane) * (F / 4) + g] = q[g];
  s_dst[threadIdx.x] = dst;
  s_count[threadIdx.x] = live ? count : 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int j = 0; j < F / 4; ++j) {
    const int piece = j * 64 + lane;        // piece index inside the wave's tile
    const int src_lane = piece / (F / 4), part = piece % (F / 4);
    const float4 w4 = s_tile[(wave0 + src_lane) * (F / 4) + part];
    float* d = s_dst[wave0 + src_lane] + 4 * part;
    const int left = s_count[wave0 + src_lane] - 4 * part;
    if (left >= 4) {
      float4u w = {w4.x, w4.y, w4.z, w4.w};
      store_row4(reinterpret_cast<float4u*>(d), w);
    } else if (left > 0) {
      d[0] = w4.x;
      if (left > 1) d[1] = w4.y;
      if (left > 2) d[2] = w4.z;
    }
  }
}

// Short rows (tic_tac_toe 27 floats, kuhn_poker 7 / 11, leduc_poker 16 / 30, ...): ONE LANE PER STATE.  The lane
// loads its state once and walks the cursor over the whole row into the wavefront's LDS tile (row stride padded
// to an odd number of words: conflict-free); the 64 rows of a wavefront are one contiguous, 16-byte aligned span
// of the output (64 * size floats), which the wavefront then writes as aligned float4 — 1 KiB per store
// instruction instead of 64 scattered 12-28 byte pieces.  Needs a 16-byte aligned output.
constexpr int kRowsBlock = 256;
constexpr int kRowsMaxSize = 63;
// kR: states per lane.  A workgroup of the shortest rows (kuhn_poker: 4 bytes in, 28 out per state) carries 7 KiB; with
// eight of them per CU the bytes in flight (57 KiB per CU) do not cover bandwidth x latency of the memory system, so
// the launch is bound by how long a workgroup LIVES, not by what it moves.  kR consecutive blocks of 64 states per
// wavefront (all kR state loads issued before the first cursor step) put kR times the bytes behind every wavefront.
template <class G, int kR>
__global__ void __launch_bounds__(kRowsBlock)
k_observation_rows(typename G::Params p, const typename G::word_t* base, int64_t n, int size, int player, int which,
                   float* __restrict__ out) {
  extern __shared__ float s_rows[];  // [waves][kR * 64 * pad]
  const int pad = size | 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tile = s_rows + wave * (kR * 64) * pad;
  const int64_t i0 = (static_cast<int64_t>(blockIdx.x) * kRowsBlock + wave * 64) * kR;  // first state of this wavefront
  if (i0 >= n) return;
  typename G::State st[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int64_t i = i0 + r * 64 + lane;
    if (i < n) st[r] = G::load(p, base, n, i);
  }
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int64_t i = i0 + r * 64 + lane;
    if (i < n) {
      const typename G::State& s = st[r];
      int pl = player;
      if (pl < 0) {
        pl = G::current_player(p, s);
        if (pl < 0) pl = 0;
      }
      typename G::ObsCursor cur;
      cur.init(p, s, pl, which, 0);
      float* row = tile + (r * 64 + lane) * pad;
      for (int k = 0; k < size; ++k) row[k] = cur.next(p, s, pl, which);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int rows = static_cast<int>(n - i0 < 64 * kR ? n - i0 : 64 * kR);
  const int total = rows * size;                       // floats this wavefront writes
  float* dst = out + i0 * size;                        // 64 * kR * size * 4 bytes per wavefront: 16-byte aligned
  for (int j = 4 * lane; j < total; j += 256) {
    int r = j / size, k = j - r * size;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = (j + e < total) ? tile[r * pad + k] : 0.0f;
      if (++k == size) { k = 0; ++r; }
    }
    if (j + 4 <= total) {
      store_row4<!std::is_same<G, Ttt>::value>(reinterpret_cast<float4*>(dst + j), make_float4(v[0], v[1], v[2], v[3]));
    } else {
      for (int e = 0; e < 4 && j + e < total; ++e) dst[j + e] = v[e];
    }
  }
}

// connect_four 6x7 tensor pack, fallback for an output pointer that is only 4-byte aligned: one lane per
// BOARD ROW of the tensor (3 planes x 6 rows per state, 7 floats each).  The seven cells of a row sit at
// bit stride 7 in the column-major bitboard; one multiply gathers them (same identity as
// C4T::open_columns), then each float is a bit-field extract; stores are 16 + 12 bytes per lane.
typedef float float3u __attribute__((ext_vector_type(3), aligned(4)));
__global__ void __launch_bounds__(kBlock)
k_observation_c4std(C4Params p, const uint64_t* __restrict__ base, int64_t n, int player, float* __restrict__ out) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (row >= n * 18) return;
  const int64_t i = row / 18;
  const int rem = static_cast<int>(row - i * 18);
  const int plane = rem / 6, r = rem - plane * 6;
  const C4Std::State s = C4Std::unpack(base[i], base[n + i]);
  uint64_t first = s.x, second = s.o;
  if (p.ego) {  // PlayerRelative (connect_four.cc:299-310)
    int pl = player;
    if (pl < 0) {
      pl = C4Std::current_player(p, s);
      if (pl < 0) pl = 0;
    }
    first = pl == 0 ? s.o : s.x;
    second = pl == 0 ? s.x : s.o;
  }
  const uint64_t bits = plane == 0 ? first : (plane == 1 ? second : ~(s.x | s.o));
  const uint64_t stride7 = 1ull | (1ull << 7) | (1ull << 14) | (1ull << 21) | (1ull << 28) | (1ull << 35) | (1ull << 42);
  const uint64_t M = (1ull << 36) | (1ull << 30) | (1ull << 24) | (1ull << 18) | (1ull << 12) | (1ull << 6) | 1ull;
  const uint32_t g = static_cast<uint32_t>((((bits >> r) & stride7) * M) >> 36) & 0x7Fu;  // bit c = column c
  float v[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) v[c] = static_cast<float>((g >> c) & 1u);
  float* dst = out + row * 7;
  float4u lo = {v[0], v[1], v[2], v[3]};
  float3u hi = {v[4], v[5], v[6]};
  store_row4(reinterpret_cast<float4u*>(dst), lo);
  *reinterpret_cast<float3u*>(dst + 4) = hi;
}

// connect_four 6x7 fast path of the tensor pack: one lane per (state, PLANE), 6 rows x 7 floats = 168 bytes
// per lane, which amortises the index arithmetic and the state load over six times more output than a
// row per lane would (about 1.2 instructions per output byte instead of 5; 117 -> 94 us for [2^20, 126]).  A wavefront owns a contiguous, 16-byte
// aligned span of 64 x 42 floats; it is staged in LDS (8-byte writes at a 168-byte lane stride) and
// written back as aligned float4, one KiB per store instruction.  Needs a 16-byte aligned output.
constexpr int kC4ObsBlock = 128;
// kNt: non-temporal stores — slower while the tensor is small (2^20 states: 95.7 vs 90.8 us), faster once it is
// gigabytes (2^24 states, 8.5 GB: 1 395 vs 1 485 us); the launcher picks by size.
template <bool kNt>
__global__ void __launch_bounds__(kC4ObsBlock)
k_observation_c4std_planes(C4Params p, const uint64_t* __restrict__ base, int64_t n, int player, float* __restrict__ out) {
  __shared__ float2 s_stage[kC4ObsBlock * 21];
  const int64_t gl = static_cast<int64_t>(blockIdx.x) * kC4ObsBlock + threadIdx.x;
  const int64_t lanes = n * 3;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float2* w2 = s_stage + wave * (64 * 21);
  if (gl < lanes) {
    const int64_t i = gl / 3;
    const int plane = static_cast<int>(gl - i * 3);
    const C4Std::State s = C4Std::unpack(base[i], base[n + i]);
    uint64_t first = s.x, second = s.o;
    if (p.ego) {  // PlayerRelative (connect_four.cc:299-310)
      int pl = player;
      if (pl < 0) {
        pl = C4Std::current_player(p, s);
        if (pl < 0) pl = 0;
      }
      first = pl == 0 ? s.o : s.x;
      second = pl == 0 ? s.x : s.o;
    }
    const uint64_t bits = plane == 0 ? first : (plane == 1 ? second : ~(s.x | s.o));
    const uint64_t stride7 = 1ull | (1ull << 7) | (1ull << 14) | (1ull << 21) | (1ull << 28) | (1ull << 35) | (1ull << 42);
    const uint64_t M = (1ull << 36) | (1ull << 30) | (1ull << 24) | (1ull << 18) | (1ull << 12) | (1ull << 6) | 1ull;
    float v[42];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const uint32_t g = static_cast<uint32_t>((((bits >> r) & stride7) * M) >> 36);  // bit c = column c of row r
#pragma unroll
      for (int c = 0; c < 7; ++c) v[r * 7 + c] = static_cast<float>((g >> c) & 1u);
    }
#pragma unroll
    for (int j = 0; j < 21; ++j) w2[lane * 21 + j] = make_float2(v[2 * j], v[2 * j + 1]);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int64_t wave_lane0 = static_cast<int64_t>(blockIdx.x) * kC4ObsBlock + wave * 64;
  if (wave_lane0 >= lanes) return;
  const int64_t left = (lanes - wave_lane0) * 42;
  const int valid = left < 64 * 42 ? static_cast<int>(left) : 64 * 42;  // floats this wavefront owns
  float* gdst = out + wave_lane0 * 42;
  const float4* w4 = reinterpret_cast<const float4*>(w2);
  const float* w1 = reinterpret_cast<const float*>(w2);
#pragma unroll
  for (int j = 0; j < 11; ++j) {
    const int piece = lane + 64 * j;  // 672 float4 pieces
    if (piece * 4 + 4 <= valid) {
      store_row4<kNt>(reinterpret_cast<float4*>(gdst) + piece, w4[piece]);
    } else {
      for (int k = piece * 4; k < valid && k < piece * 4 + 4; ++k) gdst[k] = w1[k];
    }
  }
}

// hex 9-plane tensor: one lane per (state, plane).  The plane's membership mask is boolean algebra on the
// bitboards (HexT::plane_mask); the lane turns its `cells` bits into floats, stages them in LDS at a lane
// stride of `cells` words, and the wavefront's span — 64 x cells floats, contiguous and 16-byte aligned —
// goes out as aligned float4, one KiB per store instruction.  One wavefront per workgroup: the stage is
// 256 x cells bytes (20 KiB for 9 x 9), so seven wavefronts share a CU's LDS (157 us with two-wave groups,
// 148 us with one).  Needs a 16-byte aligned output.
constexpr int kHexObsBlock = 64;
template <class G>
__global__ void __launch_bounds__(kHexObsBlock)
k_observation_hex_planes(typename G::Params p, const typename G::word_t* base, int64_t n, int planes, float* __restrict__ out) {
  extern __shared__ float s_hex_stage[];
  const int cells = p.cells;
  const int64_t gl = static_cast<int64_t>(blockIdx.x) * kHexObsBlock + threadIdx.x;
  const int64_t lanes = n * planes;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* w = s_hex_stage + wave * 64 * cells;
  if (gl < lanes) {
    const int64_t i = gl / planes;
    const int plane = static_cast<int>(gl - i * planes);
    const typename G::State s = G::load(p, base, n, i);
    const typename G::Bits m = G::plane_mask(p, s, plane);
    float* mine = w + lane * cells;
    constexpr int kWords = static_cast<int>(sizeof(m.w) / sizeof(m.w[0]));
#pragma unroll
    for (int k = 0; k < kWords; ++k) {
      const int count = cells - 32 * k < 32 ? cells - 32 * k : 32;  // wave-uniform
      uint32_t bits = m.w[k];
#pragma unroll 8
      for (int b = 0; b < count; ++b) {
        mine[32 * k + b] = static_cast<float>(bits & 1u);
        bits >>= 1;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int64_t wave_lane0 = static_cast<int64_t>(blockIdx.x) * kHexObsBlock + wave * 64;
  if (wave_lane0 >= lanes) return;
  const int64_t left = (lanes - wave_lane0) * cells;
  const int span = 64 * cells;
  const int valid = left < span ? static_cast<int>(left) : span;  // floats this wavefront owns
  float* gdst = out + wave_lane0 * cells;
  const float4* w4 = reinterpret_cast<const float4*>(w);
  for (int piece = lane; piece * 4 < valid; piece += 64) {
    if (piece * 4 + 4 <= valid) {
      store_row4(reinterpret_cast<float4*>(gdst) + piece, w4[piece]);
    } else {
      for (int k = piece * 4; k < valid; ++k) gdst[k] = w[k];
    }
  }
}

// ---------------------------------------------------------------------------
// Tensor pack, "one aligned 16-byte piece per thread": thread t computes floats [4t, 4t + 4) of the flat
// [n, size] output and stores them once.  The store pattern is the one tools/fill_probe.hip measured as the
// write-only ceiling (0.86 of 8 TB/s: every wave-instruction covers one aligned KiB, consecutive waves
// consecutive KiB), where any form in which a wavefront owns a multi-KiB span of its own stays at 0.69-0.77
// (profiles/r03_fill_probe.log) — which is where the span-per-wavefront packers above sit.  The price is that a
// thread recomputes its position (state, offset) from the piece index and that the ~size / 4 threads of one state
// all need that state; what it takes to reach the ceiling (profiles/r04_obs_forms.log has every step):
//   * few instructions: at 0.85 a SIMD retires a 64-piece wavefront every ~150 ns, ~145 vector instructions — a
//     game's generic cursor per piece is far too slow (0.29-0.59), each game below has its own bit arithmetic;
//   * several pieces per thread with all loads issued first: a wavefront is load latency, then stores; one
//     piece per thread keeps too few bytes in flight (0.75), four reach 0.84, six / eight fall back (0.79);
//   * non-temporal stores: plain stores halve the rate (0.41-0.48) as soon as loads share the launch;
//   * whole aligned KiB per wave-instruction: spans that start at 16-byte but not 1 KiB boundaries cost 0.77 -> 0.55.
// Needs a 16-byte aligned output of fewer than 2^32 floats (the span-per-wavefront kernels serve the rest).
// ---------------------------------------------------------------------------
constexpr int kPieceBlock = 256;
// connect_four 6 x 7 in the piece form.  A piece is four consecutive cells in row-major order (row r, columns
// c .. c + 3, running on into the next row / plane / state); in the column-major bitboard (bit = 7 col + row) the cells
// of a row sit 7 bits apart, so ONE 64-bit shift per row brings a whole row's bits into a 32-bit window and each
// float is a bit-field extract: window 0 = the first cell's row from column c on, window 1 = the following row
// (of the same plane, the next plane, or plane 0 of the next state).  126 floats per row is even and a piece
// starts at a multiple of four, so floats 0 and 1 of a piece never leave the first state.
// What the form costs is instructions, not bytes: at 0.85 of 8 TB/s a SIMD retires a 64-piece wavefront every
// ~150 ns, i.e. ~145 vector instructions (the first version of this kernel had 127 + a 64-bit scalar division:
// 0.77).  Hence: 32-bit indices throughout (the launcher sends tensors of 2^32 floats or more elsewhere), the
// workgroup's first state by a 32-bit division by a constant, no unpacking of the result byte (no window ever
// reaches bits 49+ unmasked), and the four cells as bit-field extracts of ONE word U built from the two windows
// (float k = bit 7k of U).  kEgo: egocentric_obs_tensor (connect_four.cc:299-310), its own instantiation.
// kPer pieces per thread: piece j of a thread lies T = threads-of-the-launch pieces after piece j - 1 (every store
// instruction of the grid still covers consecutive KiB); all state loads are issued before the first float is formed.
template <bool kNt, bool kEgo, int kPer>
__global__ void __launch_bounds__(kPieceBlock)
k_observation_c4std_pieces(C4Params p, const uint64_t* __restrict__ base, uint32_t n, uint32_t total, int player,
                           float* __restrict__ out) {
  uint64_t A0[kPer], A1[kPer], B0[kPer], B1[kPer];
  uint32_t offs[kPer];
  bool live[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t wg = blockIdx.x + j * gridDim.x;       // < 2^22
    const uint32_t ib = (wg * 512u) / 63u;                // = 1024 wg / 126: first state the workgroup touches
    const uint32_t local = (wg * 1024u - ib * 126u) + 4u * threadIdx.x;   // < 126 + 1024
    const uint32_t il = (local * 1041u) >> 17;            // local / 126 for local < 2^13
    uint32_t i = ib + il;
    live[j] = i < n;
    if (!live[j]) i = n - 1;
    offs[j] = local - il * 126u;                          // even: floats off, off + 1 are in state i
    const uint32_t i1 = i + 1u < n ? i + 1u : i;
    A0[j] = base[i]; A1[j] = base[n + i]; B0[j] = base[i1];
    if (kEgo) B1[j] = base[n + i1];
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (!live[j]) continue;
    const uint32_t wg = blockIdx.x + j * gridDim.x;
    uint64_t a0 = A0[j], a1 = A1[j], b0 = B0[j];
    if (kEgo) {  // PlayerRelative (connect_four.cc:299-310)
      const C4Std::State sa = C4Std::unpack(a0, a1), sb = C4Std::unpack(b0, B1[j]);
      int pa = player, pb = player;
      if (player < 0) {
        pa = C4Std::current_player(p, sa); if (pa < 0) pa = 0;
        pb = C4Std::current_player(p, sb); if (pb < 0) pb = 0;
      }
      a0 = pa == 0 ? sa.o : sa.x;
      a1 = pa == 0 ? sa.x : sa.o;
      b0 = pb == 0 ? sb.o : sb.x;
    }
    const uint64_t a2 = ~(a0 | a1);
    const uint32_t off = offs[j];
    const uint32_t plane = (off >= 42u) + (off >= 84u);
    const uint32_t cell = off - __umul24(42u, plane);
    const uint32_t row = __umul24(cell, 37u) >> 8;         // cell / 7 for cell < 42
    const uint32_t col = cell - __umul24(7u, row);
    // window 0: the first cell's row from its column on (bit 7k = column col + k); window 1: the following row from
    // column 0 — of the same plane, of the next plane, or of plane 0 of the next state
    const uint64_t bits0 = plane == 0 ? a0 : (plane == 1 ? a1 : a2);
    const uint32_t w0 = static_cast<uint32_t>(bits0 >> (__umul24(7u, col) + row));
    const bool last_row = row == 5u;
    const uint32_t plane1 = plane + (last_row ? 1u : 0u);
    const uint64_t bits1 = plane1 == 0 ? a0 : (plane1 == 1 ? a1 : (plane1 == 2 ? a2 : b0));
    const uint32_t w1 = static_cast<uint32_t>(bits1 >> (last_row ? 0u : row + 1u));
    const uint32_t t7 = 49u - __umul24(7u, col);           // bits of window 0 that are cells of this row: 7 (7 - col)
    const uint32_t u = t7 >= 28u ? w0 : ((w0 & ((1u << t7) - 1u)) | (w1 << t7));
    const float4 v = make_float4(static_cast<float>(u & 1u), static_cast<float>((u >> 7) & 1u),
                                 static_cast<float>((u >> 14) & 1u), static_cast<float>((u >> 21) & 1u));
    const uint32_t f0 = wg * 1024u + 4u * threadIdx.x;
    float* dst = out + (static_cast<size_t>(wg) * 1024u) + 4u * threadIdx.x;   // scalar base + 32-bit lane offset
    if (f0 + 4u <= total) {
      store_row4<kNt>(reinterpret_cast<float4*>(dst), v);
    } else {  // the last piece of the tensor (126 n is even, not always a multiple of four).  Atomic stores: plain ones
      // are merged with the vector store above into a 12-byte + a 4-byte store on EVERY lane (seen in the ISA: 0.34)
      __hip_atomic_store(dst, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(dst + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The piece form for the other board tensors, written once.  The mapping is FLAT — thread t of workgroup w forms
// floats [1024 w + 4 t, + 4): every wave-instruction stores one whole, 1 KiB-aligned KiB; a first version that gave a
// workgroup whole rows (972 floats for tic_tac_toe: spans aligned to 16 bytes only) ran at 0.55 where this runs at
// the fill ceiling — so the workgroup's first state is a division of 1024 w by the row length: five scalar
// instructions with a host-made multiplier (FastDiv, libdivide's branch-free form), and the lane's row a
// multiply-shift the host has verified for its range.  Like the connect_four kernel above, every thread serves kPer
// spans, all state loads issued first.  F is the game's piece functor:
//   Words F::load(i)                           the raw state words a piece of state i may need
//   float4 F::piece(Words a, Words b, off)     floats off .. off + 3 of state a's row, running on into state b's
struct FastDiv {   // x / d for any 32-bit x: t = mulhi(x, m); q = (((x - t) >> 1) + t) >> s
  uint32_t m, s, d;
  OSG_HD uint32_t div(uint32_t x) const {
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t t = __umulhi(x, m);
#else
    const uint32_t t = static_cast<uint32_t>((static_cast<uint64_t>(x) * m) >> 32);
#endif
    return (((x - t) >> 1) + t) >> s;
  }
};
inline FastDiv make_fast_div(uint32_t d) {  // d >= 2
  FastDiv f;
  f.d = d;
  const uint32_t k = 31u - static_cast<uint32_t>(__builtin_clz(d));
  if ((d & (d - 1)) == 0) { f.m = 0; f.s = k - 1; return f; }   // 2^k: t = 0, q = (x >> 1) >> (k - 1)
  const uint64_t two = uint64_t{1} << (32 + k);
  uint64_t m = two / d;
  const uint64_t rem = two - m * d;
  m += m;
  const uint64_t twice = rem + rem;
  if (twice >= d) m += 1;
  f.m = static_cast<uint32_t>(m + 1);
  f.s = k;
  return f;
}
template <class F, bool kNt, int kPer>
__global__ void __launch_bounds__(kPieceBlock)
k_observation_row_pieces(F f, uint32_t n, FastDiv by_size, uint32_t lmagic, uint32_t lshift, uint32_t total,
                         float* __restrict__ out) {
  typename F::Words wa[kPer], wb[kPer];
  uint32_t offs[kPer];
  const uint32_t size = by_size.d;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t fb = (blockIdx.x + j * gridDim.x) * 1024u;        // first float of the span (scalar)
    const uint32_t ib = by_size.div(fb);
    const uint32_t local = (fb - ib * size) + 4u * threadIdx.x;      // < size + 1024
    const uint32_t il = (local * lmagic) >> lshift;                  // local / size
    uint32_t i = ib + il;
    offs[j] = local - il * size;
    if (i >= n) i = n - 1u;                                          // (a piece past the end: not stored)
    wa[j] = f.load(i);
    wb[j] = f.load(i + 1u < n ? i + 1u : i);
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t f0 = (blockIdx.x + j * gridDim.x) * 1024u + 4u * threadIdx.x;
    if (f0 >= total) continue;
    const float4 v = f.piece(wa[j], wb[j], offs[j]);
    float* dst = out + static_cast<size_t>(blockIdx.x + j * gridDim.x) * 1024u + 4u * threadIdx.x;
    if (f0 + 4u <= total) {
      store_row4<kNt>(reinterpret_cast<float4*>(dst), v);
    } else {  // the tensor's last piece (atomic stores: see k_observation_c4std_pieces)
      const uint32_t left = total - f0;
      __hip_atomic_store(dst, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (left > 1u) __hip_atomic_store(dst + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (left > 2u) __hip_atomic_store(dst + 2, v.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
// The same pieces with the rows' IMAGES staged in LDS: a span of 1024 floats belongs to 1024 / size + 2 states, and
// in the kernel above every piece rebuilds the images of its two states (leduc_poker's information row: 82 vector
// instructions per piece, the vector unit 84 % busy — profiles/r04_pmc_obs_rows_pieces.txt).  Here the workgroup's
// kSpans spans first get their states' images, one (span, state) per thread, then a piece is two LDS reads, a shift
// and four conversions.
template <class F, bool kNt, int kSpans>
__global__ void __launch_bounds__(kPieceBlock)
k_observation_row_pieces_lds(F f, uint32_t n, FastDiv by_size, uint32_t lmagic, uint32_t lshift, uint32_t cap, uint32_t cmagic,
                             uint32_t cshift, uint32_t total, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(8))) unsigned char s_raw[];
  typename F::Img* s_img = reinterpret_cast<typename F::Img*>(s_raw);   // [kSpans][cap]
  const uint32_t size = by_size.d;
  for (uint32_t flat = threadIdx.x; flat < kSpans * cap; flat += kPieceBlock) {
    const uint32_t j = (flat * cmagic) >> cshift, sl = flat - j * cap;                  // flat / cap
    const uint32_t fb = (blockIdx.x + j * gridDim.x) * 1024u;
    if (fb >= total) continue;
    uint32_t i = by_size.div(fb) + sl;
    if (i >= n) i = n - 1u;
    s_img[flat] = f.image(f.load(i));
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSpans; ++j) {
    const uint32_t fb = (blockIdx.x + j * gridDim.x) * 1024u;
    const uint32_t f0 = fb + 4u * threadIdx.x;
    if (f0 >= total) continue;
    const uint32_t ib = by_size.div(fb);
    const uint32_t local = (fb - ib * size) + 4u * threadIdx.x;      // < size + 1024
    const uint32_t il = (local * lmagic) >> lshift;                  // local / size
    const uint32_t off = local - il * size;
    const float4 v = f.piece_img(s_img[j * cap + il], s_img[j * cap + il + 1u], off);
    float* dst = out + static_cast<size_t>(blockIdx.x + j * gridDim.x) * 1024u + 4u * threadIdx.x;
    if (f0 + 4u <= total) {
      store_row4<kNt>(reinterpret_cast<float4*>(dst), v);
    } else {  // the tensor's last piece (atomic stores: see k_observation_c4std_pieces)
      const uint32_t left = total - f0;
      __hip_atomic_store(dst, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (left > 1u) __hip_atomic_store(dst + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (left > 2u) __hip_atomic_store(dst + 2, v.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
OSG_D float4 low_four_bits(uint32_t u) {
  return make_float4(static_cast<float>(u & 1u), static_cast<float>((u >> 1) & 1u), static_cast<float>((u >> 2) & 1u),
                     static_cast<float>((u >> 3) & 1u));
}
// tic_tac_toe (tic_tac_toe.cc:241-251): the row is a 27-bit image, plane 0 empty | plane 1 o | plane 2 x.
struct TttPieces {
  const uint32_t* base;
  using Words = uint32_t;
  OSG_D Words load(uint32_t i) const { return base[i]; }
  OSG_D static uint32_t image(uint32_t w) {
    const uint32_t x = w & 0x1FFu, o = (w >> 16) & 0x1FFu;
    return (~(x | o) & 0x1FFu) | (o << 9) | (x << 18);
  }
  OSG_D float4 piece(Words a, Words b, uint32_t off) const {  // off <= 26
    return low_four_bits((image(a) >> off) | (image(b) << (27u - off)));
  }
  using Img = uint32_t;
  OSG_D float4 piece_img(Img a, Img b, uint32_t off) const { return low_four_bits((a >> off) | (b << (27u - off))); }
};
// kuhn_poker, two players (KuhnObserver::WriteTensor, kuhn_poker.cc:72-107), in the piece form.  The round-3 rows
// kernel spends its whole launch issuing vector instructions (profiles/r04_pmc_k_observation_rows_kuhn_2p24.txt:
// SQ_ACTIVE_INST_VALU x 4 cycles / SIMD = the launch's duration): here a row is one small image —
//   observation  [player 2 | private card 3 | pot contribution 2]: seven 4-bit entries (the contributions are 1 .. 3)
//   information  [player 2 | private card 3 | betting 3 x 2]:      eleven 1-bit entries
// — two images per piece (its state and the next), one 64-bit shift, four field extracts.
template <int kWhich>
struct Kuhn2Pieces {
  const uint64_t* base;
  int player;
  using Words = uint64_t;
  static constexpr uint32_t kSize = kWhich == 0 ? 7u : 11u, kBits = kWhich == 0 ? 4u : 1u;
  OSG_D Words load(uint32_t i) const { return base[i]; }
  OSG_D uint64_t image(uint64_t h) const {
    const Kuhn::Params p{1, 2};
    const Kuhn::State s{h};
    int pl = player;
    if (pl < 0) {
      pl = Kuhn::current_player(p, s);
      if (pl < 0) pl = 0;
    }
    const uint32_t len = static_cast<uint32_t>(h & 31ull), bets = static_cast<uint32_t>(h >> 45);
    const uint32_t card = static_cast<uint32_t>(h >> (5 + 4 * pl)) & 15u;
    const bool dealt = len > static_cast<uint32_t>(pl);
    if (kWhich == 0) {
      const uint32_t c0 = 1u + (bets & 1u) + ((bets >> 2) & 1u), c1 = 1u + ((bets >> 1) & 1u);   // contribution(), P = 2
      uint32_t img = (1u << (4 * pl)) | (c0 << 20) | (c1 << 24);
      if (dealt) img |= 1u << (8 + 4 * card);
      return img;
    }
    uint32_t img = 1u << pl;
    if (dealt) img |= 1u << (2 + card);
    const uint32_t nact = len > 2u ? len - 2u : 0u;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j)
      if (j < nact) img |= 1u << (5u + 2u * j + ((bets >> j) & 1u));
    return img;
  }
  OSG_D float4 piece(Words a, Words b, uint32_t off) const {
    const uint64_t both = (image(a) | (image(b) << (kSize * kBits))) >> (kBits * off);
    const uint32_t u = static_cast<uint32_t>(both), m = (1u << kBits) - 1u;
    return make_float4(static_cast<float>(u & m), static_cast<float>((u >> kBits) & m),
                       static_cast<float>((u >> (2 * kBits)) & m), static_cast<float>((u >> (3 * kBits)) & m));
  }
};
// leduc_poker, two players (LeducObserver::WriteTensor, leduc_poker.cc:103-192), in the piece form, K = the number
// of card ranks the tensor distinguishes (6, or 3 with suit isomorphism):
//   observation  [player 2 | private K | public K | pot contribution 2]: 4-bit entries (contributions <= 13), <= 64 bits
//   information  [player 2 | private K | public K | betting 2 x 4 x 2]: 1-bit entries; a move's pair (call "10",
//                raise "01", fold "00") IS its 2-bit code in the record (1 call, 2 raise, 0 fold), so a round's
//                betting bits are its move sequence masked to its length.
template <int kWhich>
struct Leduc2Pieces {
  const uint64_t* base;
  uint32_t n;
  int player, K;
  Leduc::Params p;
  struct Words { uint64_t a, b; };
  static constexpr uint32_t kBits = kWhich == 0 ? 4u : 1u;
  OSG_D Words load(uint32_t i) const { return {base[i], base[n + i]}; }
  using Img = typename std::conditional<kWhich == 0, uint64_t, uint32_t>::type;   // information rows: 30 bits
  OSG_D Img image(const Words& w) const {
    // only the fields a row shows are taken out of the two packed words (Leduc::unpack's layout)
    const uint32_t ante_pk = static_cast<uint32_t>(w.a >> 42) & 0xFFFu, priv_pk = static_cast<uint32_t>(w.b >> 34) & 0xFFFu;
    const int pub = static_cast<int>((w.a >> 18) & 15ull) - 1;
    int pl = player;
    if (pl < 0) {
      pl = Leduc::current_player(p, Leduc::unpack(w.a, w.b));
      if (pl < 0) pl = 0;
    }
    const int pc = static_cast<int>((priv_pk >> (4 * pl)) & 15u) - 1;
    Img img = Img{1} << (kBits * pl);
    if (pc >= 0) img |= Img{1} << (kBits * (2 + pc));
    if (pub >= 0) img |= Img{1} << (kBits * (2 + K + pub));
    if (kWhich == 0) {
      img |= static_cast<Img>(ante_pk & 0xFFu) << (4 * (2 + 2 * K));   // ante[0] | ante[1] << 4: two entries
    } else {
      const uint32_t lo = static_cast<uint32_t>(w.b);
      const uint32_t len0 = lo & 7u, seq0 = (lo >> 3) & 0xFFu, len1 = (lo >> 17) & 7u, seq1 = (lo >> 20) & 0xFFu;
      const uint32_t r0 = seq0 & ((1u << (2 * len0)) - 1u), r1 = seq1 & ((1u << (2 * len1)) - 1u);
      img |= static_cast<Img>((r0 & 0xFFu) | ((r1 & 0xFFu) << 8)) << (2 + 2 * K);
    }
    return img;
  }
  OSG_D float4 piece(const Words& a, const Words& b, uint32_t off) const {
    const uint32_t size = kWhich == 0 ? 4u + 2u * K : 18u + 2u * K;
    Img both = image(a) >> (kBits * off);
    const uint32_t in_a = size - off;                        // entries of the piece that lie in a's row (>= 1)
    if (in_a < 4u) both |= image(b) << (kBits * in_a);
    const uint32_t u = static_cast<uint32_t>(both), m = (1u << kBits) - 1u;
    return make_float4(static_cast<float>(u & m), static_cast<float>((u >> kBits) & m),
                       static_cast<float>((u >> (2 * kBits)) & m), static_cast<float>((u >> (3 * kBits)) & m));
  }
  OSG_D float4 piece_img(Img ia, Img ib, uint32_t off) const {
    const uint32_t size = kWhich == 0 ? 4u + 2u * K : 18u + 2u * K;
    const uint32_t in_a = size - off;                        // entries of the piece that lie in a's row (>= 1)
    Img both = ia >> (kBits * off);
    both |= in_a < 4u ? ib << (kBits * in_a) : Img{0};
    const uint32_t u = static_cast<uint32_t>(both), m = (1u << kBits) - 1u;
    return make_float4(static_cast<float>(u & m), static_cast<float>((u >> kBits) & m),
                       static_cast<float>((u >> (2 * kBits)) & m), static_cast<float>((u >> (3 * kBits)) & m));
  }
};
// hex, the 9-plane tensor (hex.cc:379-398: plane = label + 4), in the piece form: a piece is four consecutive cells
// of one plane's membership mask (HexT::plane_mask: boolean algebra on the stone / edge-connection planes), running
// on into the next plane of the same state or plane 0 of the next state.  It needs nine words (three planes x {two
// words of the first mask — the four bits may straddle a word —, word 0 of the following mask}), each in another
// plane of the SoA image; as nine global loads per piece that is 0.35 of 8 TB/s (the texture path spends its cycles
// on load INSTRUCTIONS, not bytes).  So a workgroup owns spans of 4096 consecutive floats (16 KiB: four aligned KiB
// per wavefront); the 5-7 states a span belongs to are fetched ONCE into LDS, one word per thread (the only global
// loads), and the pieces read their nine words from there (same-address LDS reads within a wavefront: broadcasts).
constexpr int kHexLdsSpan = 4096;             // floats per workgroup
constexpr int kHexLdsMaxStates = 18;          // 4096 / (9 * 29 cells) + 2
// kSpans spans per workgroup (span j of workgroup w = span w + j * gridDim.x): all their states are fetched before the
// one barrier, so kSpans x 16 KiB of stores stand behind one load round trip.
template <int NW, bool kNt, int kSpans>
__global__ void __launch_bounds__(kPieceBlock)
k_observation_hex_pieces_lds(const uint32_t* __restrict__ base, uint32_t n, uint32_t cells, uint32_t cmagic, uint32_t cshift,
                             FastDiv by_size, uint32_t lmagic, uint32_t lshift, uint32_t total, float* __restrict__ out,
                             uint32_t last_word_mask) {   // (0x07FFFFFF where the planes' last words carry the meta bits)
  __shared__ uint32_t s_words[kSpans][kHexLdsMaxStates * 4 * NW];
  const uint32_t size = by_size.d;   // 9 cells
  uint32_t ias[kSpans];
#pragma unroll
  for (int j = 0; j < kSpans; ++j) {
    const uint32_t fb = (blockIdx.x + j * gridDim.x) * static_cast<uint32_t>(kHexLdsSpan);
    ias[j] = 0;
    if (fb >= total) continue;
    const uint32_t ia = by_size.div(fb);                               // first state of the span (scalar)
    ias[j] = ia;
    uint32_t last = fb + kHexLdsSpan - 1u;
    if (last >= total) last = total - 1u;
    const uint32_t count = by_size.div(last) - ia + 1u;                // states the span touches ...
    const uint32_t fetch = (count + 1u) * 4u * NW;                     // ... and one more (a piece's next mask), clamped
    if (threadIdx.x < fetch) {
      const uint32_t sl = threadIdx.x / (4u * NW), w = threadIdx.x - sl * 4u * NW;
      uint32_t i = ia + sl;
      if (i >= n) i = n - 1u;
      const uint32_t word = base[w * n + i];                           // plane-major SoA: word w of state i
      s_words[j][threadIdx.x] = (w % NW == NW - 1u) ? (word & last_word_mask) : word;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSpans; ++j) {
    const uint32_t span = blockIdx.x + j * gridDim.x;
    const uint32_t fb = span * static_cast<uint32_t>(kHexLdsSpan);
    if (fb >= total) break;
    const uint32_t rem = fb - ias[j] * size;
    const uint32_t* words = s_words[j];
#pragma unroll
    for (int r = 0; r < kHexLdsSpan / (4 * kPieceBlock); ++r) {
      const uint32_t p4 = 4u * (r * kPieceBlock + threadIdx.x);        // float inside the span
      const uint32_t f0 = fb + p4;
      if (f0 >= total) break;
      const uint32_t local = rem + p4;                                 // < size + 4096
      const uint32_t il = (local * lmagic) >> lshift;                  // local / size
      const uint32_t off = local - il * size;
      const uint32_t plane = (off * cmagic) >> cshift;                 // off / cells
      const uint32_t cell0 = off - plane * cells;
      const uint32_t k0 = cell0 >> 5, k1 = k0 + 1u < NW ? k0 + 1u : k0;
      const bool wrap = plane == 8u;                                   // the following mask: plane 0 of the next state
      const int l0 = static_cast<int>(plane) - 4, l1 = wrap ? -4 : l0 + 1;
      const uint32_t sa = il * 4u * NW, sb = wrap ? sa + 4u * NW : sa;
      // planes: 0 black, 1 white, 2 edge A, 3 edge B.  l == 0 (empty): X = black, Y = white.  else X = own, Y = ea, Z = eb
      const uint32_t px0 = (l0 >= 0 ? 0u : 1u) * NW, py0 = (l0 == 0 ? 1u : 2u) * NW;
      const uint32_t px1 = (l1 >= 0 ? 0u : 1u) * NW, py1 = (l1 == 0 ? 1u : 2u) * NW;
      uint32_t X[3], Y[3], Z[3];
      X[0] = words[sa + px0 + k0]; Y[0] = words[sa + py0 + k0]; Z[0] = words[sa + 3u * NW + k0];
      X[1] = words[sa + px0 + k1]; Y[1] = words[sa + py0 + k1]; Z[1] = words[sa + 3u * NW + k1];
      X[2] = words[sb + px1];      Y[2] = words[sb + py1];      Z[2] = words[sb + 3u * NW];
      uint32_t m[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int l = k < 2 ? l0 : l1;
        const int mag = l > 0 ? l : -l;                                 // 1 plain, 2 edge B only, 3 edge A only, 4 both
        const uint32_t fa = mag >= 3 ? 0u : ~0u, fb2 = (mag == 2 || mag == 4) ? 0u : ~0u;
        const uint32_t labelled = X[k] & (Y[k] ^ fa) & (Z[k] ^ fb2);
        m[k] = l == 0 ? ~(X[k] | Y[k]) : labelled;
      }
      const uint32_t second = k0 + 1u < NW ? m[1] : 0u;
      const uint32_t w0 = __funnelshift_r(m[0], second, cell0 & 31u);   // bit k = cell0 + k of mask 0
      const uint32_t t = cells - cell0;                                 // cells left in the plane (>= 1)
      const uint32_t u = t >= 4u ? w0 : ((w0 & ((1u << t) - 1u)) | (m[2] << t));
      const float4 v = low_four_bits(u);
      float* dst = out + static_cast<size_t>(span) * kHexLdsSpan + p4;
      if (f0 + 4u <= total) {
        store_row4<kNt>(reinterpret_cast<float4*>(dst), v);
      } else {
        const uint32_t left = total - f0;
        __hip_atomic_store(dst, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (left > 1u) __hip_atomic_store(dst + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (left > 2u) __hip_atomic_store(dst + 2, v.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}
// (x * magic) >> shift == x / d for every x < limit?  The host picks the pair with this check, so the kernels' lane
// arithmetic is a multiply and a shift whatever the row length.
inline bool find_div_magic(uint32_t d, uint32_t limit, uint32_t* magic, uint32_t* shift) {
  for (uint32_t s = 8; s <= 24; ++s) {
    const uint64_t m = ((uint64_t{1} << s) + d - 1) / d;
    if (m * (limit - 1) >= (uint64_t{1} << 32)) break;
    bool ok = true;
    for (uint32_t x = 0; x < limit && ok; ++x) ok = ((x * m) >> s) == x / d;
    if (ok) { *magic = static_cast<uint32_t>(m); *shift = s; return true; }
  }
  return false;
}

}  // namespace

extern "C" {

int osg_observation(const osg_batch* b, int player, int which, float* out, int on_host) {
  osg_ctx* ctx = b->ctx;
  const osg_game_desc& d = b->spec.desc;
  const int size = which == 0 ? d.obs_size : d.info_size;
  if (size <= 0) return set_error(OSG_ERR_INVALID, "this game provides no such tensor");
  if (player < -1 || player >= d.num_players)
    return set_error(OSG_ERR_INVALID, "player id out of range");  // SPIEL_CHECK_GE/LT, spiel.cc:914-915
  const int64_t total = b->n * size;
  float* d_out = out;
  if (on_host) {
    void* scratch;
    int rc = osg_ctx_scratch(ctx, sizeof(float) * total, &scratch);
    if (rc) return rc;
    d_out = static_cast<float*>(scratch);
  }
  // OSG_OBS_FORM=0: the span-per-wavefront kernels of round 3 (A/B: tools/probe_obs_forms.py); 1: the piece form
  // with plain stores; default 2: the piece form with non-temporal stores.
  static const int obs_form = std::getenv("OSG_OBS_FORM") ? std::atoi(std::getenv("OSG_OBS_FORM")) : 2;
  const bool aligned16 = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
  // (below ~2^24 floats the launch is a few hundred workgroups: the span kernels' finer grid fills the chip better —
  // [2^16, 126]: 7.4 vs 8.4 us, hex(9) [2^14, 729]: 11.9 vs 29.5 us; from [2^20, 27] on the piece form is ahead)
  const bool pieces = obs_form != 0 && aligned16 && total < (int64_t{1} << 32) && total >= (int64_t{1} << 24);
  const bool nt = obs_form != 1;
  // OSG_OBS_LDS=0: every piece builds its rows' images itself (A/B); 4 / 8: images staged in LDS, that many spans per
  // workgroup; default: 8 for tic_tac_toe (0.77 vs 0.70 with 4 and 0.75 without), 4 for leduc_poker (information rows 0.83
  // vs 0.78 with 8 and 0.80 without) — tools/probe_obs_lds.py
  static const int obs_lds_env = std::getenv("OSG_OBS_LDS") ? std::atoi(std::getenv("OSG_OBS_LDS")) : -1;
  const int obs_lds = obs_lds_env >= 0 ? obs_lds_env : (b->spec.desc.game_kind == kTtt ? 8 : 4);
  const unsigned piece_grid = static_cast<unsigned>(((total + 1023) / 1024 + 3) / 4);   // four 1 KiB-piece spans per workgroup
  // the piece form of a game whose rows come from a functor f, `spans` 1 KiB-piece spans per thread
  const auto row_pieces = [&](auto f, auto spans, unsigned grid) {
    uint32_t magic = 0, shift = 0;
    find_div_magic(static_cast<uint32_t>(size), static_cast<uint32_t>(size) + 1024u, &magic, &shift);
    return with_bool(nt, [&](auto ntv) {
      k_observation_row_pieces<decltype(f), decltype(ntv)::value, decltype(spans)::value><<<dim3(grid), dim3(kPieceBlock), 0, ctx->stream>>>(
          f, static_cast<uint32_t>(b->n), make_fast_div(static_cast<uint32_t>(size)), magic, shift, static_cast<uint32_t>(total), d_out);
      return OSG_OK;
    });
  };
  if (pieces && b->spec.desc.game_kind == kC4 && b->spec.c4_std) {
    with_bool(b->spec.c4.ego, [&](auto ego) {
      return with_bool(nt, [&](auto ntv) {
        k_observation_c4std_pieces<decltype(ntv)::value, decltype(ego)::value, 4><<<dim3(piece_grid), dim3(kPieceBlock), 0, ctx->stream>>>(
            b->spec.c4, static_cast<const uint64_t*>(b->words()), static_cast<uint32_t>(b->n), static_cast<uint32_t>(total), player, d_out);
        return OSG_OK;
      });
    });
  } else if (pieces && obs_lds && (b->spec.desc.game_kind == kTtt || (b->spec.desc.game_kind == kLeduc && d.num_players == 2))) {
    // the rows' images staged in LDS (k_observation_row_pieces_lds)
    uint32_t magic = 0, shift = 0, cmagic = 0, cshift = 0;
    const uint32_t cap = 1024u / static_cast<uint32_t>(size) + 3u;
    if (!find_div_magic(static_cast<uint32_t>(size), static_cast<uint32_t>(size) + 1024u, &magic, &shift) ||
        !find_div_magic(cap, 8u * cap, &cmagic, &cshift))
      return set_error(OSG_ERR_INVALID, "osg_observation: no multiply-shift pair for this row size");
    const FastDiv fd = make_fast_div(static_cast<uint32_t>(size));
    const uint32_t nn = static_cast<uint32_t>(b->n), tot = static_cast<uint32_t>(total);
    const auto rows_lds = [&](auto f) {   // f: the game's piece functor
      return with_int<8, 4>(obs_lds, [&](auto sp) {
        return with_bool(nt, [&](auto ntv) {
          constexpr int SP = decltype(sp)::value;
          const unsigned g = static_cast<unsigned>(((total + 1023) / 1024 + SP - 1) / SP);
          const size_t lds = sizeof(typename decltype(f)::Img) * SP * cap;
          k_observation_row_pieces_lds<decltype(f), decltype(ntv)::value, SP><<<dim3(g), dim3(kPieceBlock), lds, ctx->stream>>>(
              f, nn, fd, magic, shift, cap, cmagic, cshift, tot, d_out);
          return OSG_OK;
        });
      });
    };
    if (b->spec.desc.game_kind == kTtt) {
      rows_lds(TttPieces{static_cast<const uint32_t*>(b->words())});
    } else {
      const int K = b->spec.leduc.iso ? b->spec.leduc.cards / 2 : b->spec.leduc.cards;
      if (which == 0) rows_lds(Leduc2Pieces<0>{static_cast<const uint64_t*>(b->words()), nn, player, K, b->spec.leduc});
      else rows_lds(Leduc2Pieces<1>{static_cast<const uint64_t*>(b->words()), nn, player, K, b->spec.leduc});
    }
  } else if (pieces && b->spec.desc.game_kind == kTtt) {
    // eight spans per thread here (27-float rows: 0.74 with four, 0.76 with eight; the round-3 kernel: 0.69)
    row_pieces(TttPieces{static_cast<const uint32_t*>(b->words())}, std::integral_constant<int, 8>{}, (piece_grid + 1) / 2);
  } else if (pieces && b->spec.desc.game_kind == kKuhn && d.num_players == 2) {
    if (which == 0) row_pieces(Kuhn2Pieces<0>{static_cast<const uint64_t*>(b->words()), player}, std::integral_constant<int, 4>{}, piece_grid);
    else row_pieces(Kuhn2Pieces<1>{static_cast<const uint64_t*>(b->words()), player}, std::integral_constant<int, 4>{}, piece_grid);
  } else if (pieces && b->spec.desc.game_kind == kLeduc && d.num_players == 2) {
    const int K = b->spec.leduc.iso ? b->spec.leduc.cards / 2 : b->spec.leduc.cards;
    const uint32_t nn = static_cast<uint32_t>(b->n);
    if (which == 0) row_pieces(Leduc2Pieces<0>{static_cast<const uint64_t*>(b->words()), nn, player, K, b->spec.leduc}, std::integral_constant<int, 4>{}, piece_grid);
    else row_pieces(Leduc2Pieces<1>{static_cast<const uint64_t*>(b->words()), nn, player, K, b->spec.leduc}, std::integral_constant<int, 4>{}, piece_grid);
  } else if (pieces && b->spec.desc.game_kind == kHex && which == 0 && d.obs_shape[0] == 9 &&
             d.obs_shape[1] * d.obs_shape[2] >= 29) {   // (a span of 4096 floats then touches at most 18 states)
    const uint32_t cells = static_cast<uint32_t>(d.obs_shape[1] * d.obs_shape[2]);
    uint32_t cm = 0, cs = 0, lm = 0, ls = 0;
    if (!find_div_magic(cells, 9u * cells, &cm, &cs) || !find_div_magic(9u * cells, 9u * cells + kHexLdsSpan, &lm, &ls))
      return set_error(OSG_ERR_INVALID, "osg_observation: no multiply-shift pair for this hex board");
    const unsigned g = static_cast<unsigned>(((total + kHexLdsSpan - 1) / kHexLdsSpan + 3) / 4);
    for_hex(b->spec, [&](auto nw, const auto&) {
      return with_bool(nt, [&](auto ntv) {
        k_observation_hex_pieces_lds<decltype(nw)::value, decltype(ntv)::value, 4><<<dim3(g), dim3(kPieceBlock), 0, ctx->stream>>>(
            static_cast<const uint32_t*>(b->words()), static_cast<uint32_t>(b->n), cells, cm, cs, make_fast_div(9u * cells), lm, ls,
            static_cast<uint32_t>(total), d_out, b->spec.hex_fold ? 0x07FFFFFFu : 0xFFFFFFFFu);
        return OSG_OK;
      });
    });
  } else if (b->spec.desc.game_kind == kC4 && b->spec.c4_std) {
    if ((reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 && b->n >= (int64_t{1} << 22))
      k_observation_c4std_planes<true><<<dim3(static_cast<unsigned>((b->n * 3 + kC4ObsBlock - 1) / kC4ObsBlock)),
                                         dim3(kC4ObsBlock), 0, ctx->stream>>>(
          b->spec.c4, static_cast<const uint64_t*>(b->words()), b->n, player, d_out);
    else if ((reinterpret_cast<uintptr_t>(d_out) & 15u) == 0)
      k_observation_c4std_planes<false><<<dim3(static_cast<unsigned>((b->n * 3 + kC4ObsBlock - 1) / kC4ObsBlock)),
                                          dim3(kC4ObsBlock), 0, ctx->stream>>>(
          b->spec.c4, static_cast<const uint64_t*>(b->words()), b->n, player, d_out);
    else
      k_observation_c4std<<<dim3(grid_for(b->n * 18)), dim3(kBlock), 0, ctx->stream>>>(
          b->spec.c4, static_cast<const uint64_t*>(b->words()), b->n, player, d_out);
  } else if (b->spec.desc.game_kind == kHex && which == 0 && d.obs_shape[0] == 9 && b->spec.hex_nw <= 4 &&
             (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0) {   // (its LDS stage is 256 B per cell: the big boards go below)
    const size_t shmem = sizeof(float) * kHexObsBlock * static_cast<size_t>(d.obs_shape[1] * d.obs_shape[2]);
    const unsigned grid = static_cast<unsigned>((b->n * 9 + kHexObsBlock - 1) / kHexObsBlock);
    for_hex(b->spec, [&](auto nw, const auto& P) {
      if constexpr (decltype(nw)::value <= 4)
        k_observation_hex_planes<HexT<decltype(nw)::value>><<<dim3(grid), dim3(kHexObsBlock), shmem, ctx->stream>>>(
            P, static_cast<const uint32_t*>(b->words()), b->n, 9, d_out);
      return OSG_OK;
    });
  } else if (size <= kRowsMaxSize && b->spec.desc.game_kind != kHex && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0) {
    // short rows: one lane per state, LDS-staged aligned float4 stores
    // states per lane: two for the shortest rows (measured at 2^24 states, 1 / 2 / 4 per lane: kuhn [n, 7] 124.8 / 103.5 /
    // 104.1 us, [n, 11] 144.2 / 128.6 / 161.3; from 16 floats per row on one is best: leduc [n, 16] 193 / 198 / 274,
    // tic_tac_toe [n, 27] 338 / 445 / 678, leduc [n, 30] 352 / 499 / 921 — profiles/r03_obs_rows_per_lane.log)
    const int kr = size <= 12 ? 2 : 1;
    const size_t shmem = sizeof(float) * (kRowsBlock / 64) * 64 * kr * static_cast<size_t>(size | 1);
    const unsigned grid = static_cast<unsigned>((b->n + kRowsBlock * kr - 1) / (kRowsBlock * kr));
    if (int rc = with_int<2, 1>(kr, [&](auto krv) {
          return for_game(b->spec, [&](auto g, const auto& P) {
            using G = typename decltype(g)::type;
            k_observation_rows<G, decltype(krv)::value><<<dim3(grid), dim3(kRowsBlock), shmem, ctx->stream>>>(
                P, static_cast<const typename G::word_t*>(b->words()), b->n, size, player, which, d_out);
            return OSG_OK;
          });
        })) return rc;
  } else {
    // Segment = one tensor plane for hex's 9-plane layout (the cursor's mask is per plane), else the row.
    int seg_len = size;
    if (b->spec.desc.game_kind == kHex && d.obs_shape[0] == 9) seg_len = d.obs_shape[1] * d.obs_shape[2];
    const bool wide = size >= 64 || b->spec.desc.game_kind == kLeduc;  // 16+ floats per lane: long rows, or a
                                                                      // bit-packed state worth decoding once
    // (32 floats per lane was measured too: fewer, fuller chunks for hex(9) but 15 % slower — the
    // 28 KiB LDS tile per workgroup costs more occupancy than the fuller chunks give back.)
    const int F = wide ? 16 : 4;
    const int cps = (seg_len + F - 1) / F;
    const int64_t lanes = b->n * (size / seg_len) * cps;
    if (int rc = with_int<16, 4>(F, [&](auto ff) {
          return for_game(b->spec, [&](auto g, const auto& P) {
            using G = typename decltype(g)::type;
            k_observation<G, decltype(ff)::value><<<dim3(grid_for(lanes)), dim3(kBlock), 0, ctx->stream>>>(P,
                static_cast<const typename G::word_t*>(b->words()), b->n, size, seg_len,
                cps, player, which, d_out);
            return OSG_OK;
          });
        })) return rc;
  }
  OSG_HIP(hipGetLastError());
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(out, d_out, sizeof(float) * total, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return OSG_OK;
}

}  // extern "C"
