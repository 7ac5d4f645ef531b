// Where do the ~4.7 us of one k_step_c4std2 launch at 2^20 states go?  Stand-alone: the kernels below restate the
// launch shape of the headline kernel (workgroups of 128 as before round 10, or of 64 as since; two states per lane,
// 16-byte plane accesses, u16 side arrays, non-temporal stores; out of place) around the step bodies of osg_c4_step.h / step/osg_c4_step_split.h, and are timed
// as 2 000 back-to-back launches between one event pair after 200 warm-up launches, at 2^20 and 2^24 synthetic
// non-terminal positions, kRounds times round-robin so that every form meets the same drift of the clocks.
//   (a) an empty kernel                         -> launch floor
//   (b) the step's loads and stores, no rules   -> memory = (b) - (a)
//   (c) the full step                           -> vector residue = (c) - (b)
//   (d) the full step without the side arrays   -> side arrays = (c) - (d)
// (c) is timed in five forms, each adding one change to the one before, so that each change is judged on its own:
//   c0  c4_fused_step, early exit on i >= n before the pointers are fetched, all stores last (the form before r10)
//   c1  c0 with ONE scalar clause: no test of i against n (the grid covers the batch exactly), so every argument is
//       requested at the top of the wave
//   c2  c1 with the step on 32-bit halves (c4_place + c4_finish), all stores last
//   c3  c2 with the o plane stored between c4_place and c4_finish
//   c4  c3 in workgroups of 64 (one wavefront) instead of 128: k_step_c4std2 as it is now; a64 / b64 / d4 are (a), (b)
//       and (d) in that shape
// Every form's outputs are compared with c4_fused_step on the host at 2^20 states before anything is timed.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I open_spiel_amd/csrc tools/probe_c4_step_parts.hip -o tools/probe_c4_step_parts
//   tools/probe_c4_step_parts.sh      (builds where needed, runs under a time limit, keeps the table)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "step/osg_c4_step_split.h"

namespace {

constexpr int kWarm = 200, kTimed = 2000, kRounds = 5;
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef uint8_t u8x2 __attribute__((ext_vector_type(2)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  printf("%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } } while (0)

template <int kBlock>
__global__ void __launch_bounds__(kBlock)
k_empty(const uint64_t*, uint64_t*, int64_t, const uint8_t*, uint8_t*, uint8_t*) {}

// (b): every byte the step moves, none of its rules; mask and status come from the loaded bytes
template <int kBlock>
__global__ void __launch_bounds__(kBlock)
k_mem(const uint64_t* src, uint64_t* dst, int64_t n, const uint8_t* __restrict__ actions,
      uint8_t* __restrict__ mask_out, uint8_t* __restrict__ status) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * 2;
  if (i >= n) return;
  const u64x2 xs = *reinterpret_cast<const u64x2*>(src + i), os = *reinterpret_cast<const u64x2*>(src + n + i);
  const u8x2 av = *reinterpret_cast<const u8x2*>(actions + i);
  u8x2 mo, so;
  mo.x = static_cast<uint8_t>(xs.x) ^ av.x; mo.y = static_cast<uint8_t>(xs.y) ^ av.y;
  so.x = static_cast<uint8_t>(os.x) ^ av.x; so.y = static_cast<uint8_t>(os.y) ^ av.y;
  __builtin_nontemporal_store(xs, reinterpret_cast<u64x2*>(dst + i));
  __builtin_nontemporal_store(os, reinterpret_cast<u64x2*>(dst + n + i));
  __builtin_nontemporal_store(mo, reinterpret_cast<u8x2*>(mask_out + i));
  __builtin_nontemporal_store(so, reinterpret_cast<u8x2*>(status + i));
}

// (c) / (d).  kForm as listed above; kSide = false: no action load (the lane's index stands in), no mask / status store
// (a hash of their bytes is compared with a constant instead, so the rules are not optimised away).
template <int kForm, bool kSide, int kBlock>
__global__ void __launch_bounds__(kBlock)
k_step(const uint64_t* src, uint64_t* dst, int64_t n, const uint8_t* __restrict__ actions,
       uint8_t* __restrict__ mask_out, uint8_t* __restrict__ status) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * 2;
  if constexpr (kForm == 0) {
    if (i >= n) return;
  }   // (the other forms: the grid covers the batch exactly, as main() launches it — no test, so no wait for n)
  const u64x2 xs = *reinterpret_cast<const u64x2*>(src + i), os = *reinterpret_cast<const u64x2*>(src + n + i);
  u8x2 av;
  if constexpr (kSide) {
    av = *reinterpret_cast<const u8x2*>(actions + i);
  } else {
    av.x = static_cast<uint8_t>(threadIdx.x % 7u); av.y = static_cast<uint8_t>((threadIdx.x + 3u) % 7u);
  }
  u64x2 xo, oo;
  uint32_t r0, r1;
  if constexpr (kForm <= 1) {
    uint64_t x0 = xs.x, x1 = xs.y, o0 = os.x, o1 = os.y;
    r0 = osg::c4_fused_step(x0, o0, av.x); r1 = osg::c4_fused_step(x1, o1, av.y);
    xo.x = x0; xo.y = x1; oo.x = o0; oo.y = o1;
  } else {
    const osg::C4Placed p0 = osg::c4_place(xs.x, os.x, av.x), p1 = osg::c4_place(xs.y, os.y, av.y);
    oo.x = (static_cast<uint64_t>(p0.no_hi) << 32) | p0.no_lo;
    oo.y = (static_cast<uint64_t>(p1.no_hi) << 32) | p1.no_lo;
    if constexpr (kForm == 3) {
      __builtin_nontemporal_store(oo, reinterpret_cast<u64x2*>(dst + n + i));
    }
    uint32_t f0, f1;
    r0 = osg::c4_finish(p0, f0); r1 = osg::c4_finish(p1, f1);
    xo.x = (static_cast<uint64_t>(p0.nx_hi | (f0 << 24)) << 32) | p0.nx_lo;
    xo.y = (static_cast<uint64_t>(p1.nx_hi | (f1 << 24)) << 32) | p1.nx_lo;
  }
  if constexpr (!kSide) {
    if (r0 * 0x9E3779B1u + r1 == 0xDEADBEEFu) xo.x ^= 1ull << 63;   // keeps mask and status alive (three instructions)
  }
  __builtin_nontemporal_store(xo, reinterpret_cast<u64x2*>(dst + i));
  if constexpr (kForm != 3) __builtin_nontemporal_store(oo, reinterpret_cast<u64x2*>(dst + n + i));
  if constexpr (kSide) {
    u8x2 mo, so;
    mo.x = static_cast<uint8_t>(r0); mo.y = static_cast<uint8_t>(r1);
    so.x = static_cast<uint8_t>(r0 >> 8); so.y = static_cast<uint8_t>(r1 >> 8);
    __builtin_nontemporal_store(mo, reinterpret_cast<u8x2*>(mask_out + i));
    __builtin_nontemporal_store(so, reinterpret_cast<u8x2*>(status + i));
  }
}

typedef void (*kernel_t)(const uint64_t*, uint64_t*, int64_t, const uint8_t*, uint8_t*, uint8_t*);
struct Form { const char* name; kernel_t k; bool checked; int block; };
enum { kA, kB, kC0, kC1, kC2, kC3, kD0, kA64, kB64, kC4, kD4 };   // indices into kForms
const Form kForms[] = {
    {"a   empty", k_empty<128>, false, 128},
    {"b   loads + stores only", k_mem<128>, false, 128},
    {"c0  step, early exit, stores last", k_step<0, true, 128>, true, 128},
    {"c1  c0 + one scalar clause", k_step<1, true, 128>, true, 128},
    {"c2  c1 + 32-bit halves", k_step<2, true, 128>, true, 128},
    {"c3  c2 + o plane stored early", k_step<3, true, 128>, true, 128},
    {"d0  c0 without side arrays", k_step<0, false, 128>, false, 128},
    {"a64 empty, workgroups of 64", k_empty<64>, false, 64},
    {"b64 loads + stores, workgroups of 64", k_mem<64>, false, 64},
    {"c4  c3 in workgroups of 64", k_step<3, true, 64>, true, 64},
    {"d4  c4 without side arrays", k_step<3, false, 64>, false, 64},
};
constexpr int kNumForms = sizeof(kForms) / sizeof(kForms[0]);

struct Buffers { uint64_t *src, *dst; uint8_t *act, *mask, *status; };

double time_us(const Form& f, const Buffers& b, int64_t n, hipEvent_t e0, hipEvent_t e1) {
  const dim3 grid(static_cast<unsigned>(n / 2 / f.block)), block(f.block);   // exact: n / 2 is a multiple of 128
  for (int k = 0; k < kWarm; ++k) f.k<<<grid, block>>>(b.src, b.dst, n, b.act, b.mask, b.status);
  CHECK(hipEventRecord(e0));
  for (int k = 0; k < kTimed; ++k) f.k<<<grid, block>>>(b.src, b.dst, n, b.act, b.mask, b.status);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  CHECK(hipGetLastError());
  float ms = 0;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  return ms * 1e3 / kTimed;
}

}  // namespace

int main() {
  const int64_t n_max = int64_t{1} << 24;
  // synthetic non-terminal positions: 0 .. 35 random legal moves from the start, replayed if the game ends on the way
  const int kDistinct = 1 << 16;
  std::vector<uint64_t> px(kDistinct), po(kDistinct);
  std::vector<uint8_t> pa(kDistinct);
  uint64_t z = 0xC4;
  for (int s = 0; s < kDistinct; ++s) {
    for (;;) {
      uint64_t x = 0, o = 0;
      z = osg::mix64(z + 0x9E3779B97F4A7C15ULL);
      const int depth = static_cast<int>((z >> 33) % 36);
      bool over = false;
      uint32_t r = 0x7F;
      for (int t = 0; t < depth && !over; ++t) {
        z = osg::mix64(z + 0x9E3779B97F4A7C15ULL);
        uint32_t a = static_cast<uint32_t>(z % 7);
        while (!((r >> a) & 1u)) a = (a + 1) % 7;
        r = osg::c4_fused_step(x, o, a);
        over = ((r >> 8) & 0x80u) != 0;
      }
      if (over) continue;
      z = osg::mix64(z + 0x9E3779B97F4A7C15ULL);
      uint32_t a = static_cast<uint32_t>(z % 7);
      while (!((r >> a) & 1u)) a = (a + 1) % 7;
      px[s] = x; po[s] = o; pa[s] = static_cast<uint8_t>(a);
      break;
    }
  }
  std::vector<uint64_t> h_src(2 * n_max);
  std::vector<uint8_t> h_act(n_max);
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  printf("%s, %d CUs; %d timed launches after %d warm-up launches per figure, %d rounds round-robin; us per launch\n",
         prop.name, prop.multiProcessorCount, kTimed, kWarm, kRounds);
  Buffers b;
  CHECK(hipMalloc(&b.src, 2 * n_max * sizeof(uint64_t)));
  CHECK(hipMalloc(&b.dst, 2 * n_max * sizeof(uint64_t)));
  CHECK(hipMalloc(&b.act, n_max));
  CHECK(hipMalloc(&b.mask, n_max));
  CHECK(hipMalloc(&b.status, n_max));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const int64_t sizes[2] = {int64_t{1} << 20, int64_t{1} << 24};
  for (int64_t n : sizes) {
    for (int64_t i = 0; i < n; ++i) {   // plane-major: x plane, then o plane, n words each
      const int s = static_cast<int>(osg::mix64(static_cast<uint64_t>(i)) % kDistinct);
      h_src[i] = px[s]; h_src[n + i] = po[s]; h_act[i] = pa[s];
    }
    CHECK(hipMemcpy(b.src, h_src.data(), 2 * n * sizeof(uint64_t), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(b.act, h_act.data(), n, hipMemcpyHostToDevice));
    if (n == sizes[0]) {   // every form of (c) against the host's c4_fused_step, before anything is timed
      std::vector<uint64_t> want(2 * n), got(2 * n);
      std::vector<uint8_t> want_m(n), want_s(n), got_m(n), got_s(n);
      for (int64_t i = 0; i < n; ++i) {
        uint64_t x = h_src[i], o = h_src[n + i];
        const uint32_t r = osg::c4_fused_step(x, o, h_act[i]);
        want[i] = x; want[n + i] = o; want_m[i] = static_cast<uint8_t>(r); want_s[i] = static_cast<uint8_t>(r >> 8);
      }
      for (const Form& f : kForms) {
        if (!f.checked) continue;
        const dim3 grid(static_cast<unsigned>(n / 2 / f.block)), block(f.block);
        CHECK(hipMemset(b.dst, 0xEE, 2 * n * sizeof(uint64_t)));
        CHECK(hipMemset(b.mask, 0xEE, n));
        CHECK(hipMemset(b.status, 0xEE, n));
        f.k<<<grid, block>>>(b.src, b.dst, n, b.act, b.mask, b.status);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(got.data(), b.dst, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(got_m.data(), b.mask, n, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(got_s.data(), b.status, n, hipMemcpyDeviceToHost));
        if (got != want || got_m != want_m || got_s != want_s) { printf("%s: outputs differ from c4_fused_step\n", f.name); return 1; }
      }
      printf("outputs of c0-c4 at %lld states equal c4_fused_step on the host\n", static_cast<long long>(n));
    }
    std::vector<double> t[kNumForms];
    for (int round = 0; round < kRounds; ++round)
      for (int f = 0; f < kNumForms; ++f) t[f].push_back(time_us(kForms[f], b, n, e0, e1));
    double med[kNumForms];
    printf("\n%lld states (%.1f MB per launch with the side arrays)\n", static_cast<long long>(n), 35.0 * n / 1e6);
    printf("%-38s %9s %9s %9s   rounds\n", "form", "min", "median", "max");
    for (int f = 0; f < kNumForms; ++f) {
      std::vector<double> s = t[f];
      std::sort(s.begin(), s.end());
      med[f] = s[s.size() / 2];
      printf("%-38s %9.3f %9.3f %9.3f  ", kForms[f].name, s.front(), med[f], s.back());
      for (double v : t[f]) printf(" %.3f", v);
      printf("\n");
    }
    // paired: per round, each form of (c) minus c0 of the same round
    for (int f : {kC1, kC2, kC3, kC4}) {
      std::vector<double> d;
      for (int round = 0; round < kRounds; ++round) d.push_back(t[f][round] - t[kC0][round]);
      std::sort(d.begin(), d.end());
      printf("paired %-31s - c0: median %+.3f (range %+.3f .. %+.3f)\n", kForms[f].name, d[d.size() / 2], d.front(), d.back());
    }
    printf("parts by medians, before (a, b, c0, d0) | after (a64, b64, c4, d4):\n");
    printf("  launch floor   (a)       %7.3f | %7.3f\n", med[kA], med[kA64]);
    printf("  memory         (b) - (a) %7.3f | %7.3f\n", med[kB] - med[kA], med[kB64] - med[kA64]);
    printf("  vector residue (c) - (b) %7.3f | %7.3f\n", med[kC0] - med[kB], med[kC4] - med[kB64]);
    printf("  side arrays    (c) - (d) %7.3f | %7.3f\n", med[kC0] - med[kD0], med[kC4] - med[kD4]);
  }
  return 0;
}
