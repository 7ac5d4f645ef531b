// The fused learner of the policy-value MLP: VPNetModel::Learn (alpha_zero_torch vpnet.cc:223-287) — forward, the three
// losses of model.cc:338-376, backward and torch's Adam — for every update of a call in ONE launch.  The plan (R = 32,
// G, every LDS offset, the scratch, the bank arguments) is osg_vpnet_learn_plan.h; the forward's tile code is
// osg_vpnet_tile.h, shared with k_vpnet_forward.
//
// Per update, workgroup g of the group (8 wavefronts, 2 over the rows x 4 over the columns; rows [32 g, 32 g + 32))
//   forward   torso in place in the ONE activation buffer, every layer's output also to its slot of the scratch; the value
//             head's hidden layer from the accumulators to its slot and, reduced against the W -> 1 weights, to tanh;
//             the policy head's hidden layer over the torso, its logits, and per row (16 lanes) the masked
//             log-softmax: the loss term and dLoss/dlogit in place of the logit (exactly 0 at an illegal id, in a row
//             without a legal action and in a row past the batch);
//   backward  dW = dY^T X tile by tile (a wavefront holds one 16-column fragment of X, from LDS or streamed from the
//             scratch / the observations, against 8 output tiles at a time), finished in one pass over the 32 rows and
//             written to partial[g]; dX = dY W with W's rows through the panels, the output in the accumulators, then
//             through the ReLU's mask over dY.  Policy head first: its gradient into the torso goes to a slot; the
//             value head's is formed next and the two are added value + policy at the write-back;
//   -- barrier 1 --
//   step      its slice of the flat parameters: the G partials in ascending g, + weight_decay w on weights, torch's
//             Adam in place; the slice's sum of w^2 (before the step) to its loss words;
//   -- barrier 2 --   workgroup 0 then adds the G loss words in ascending g into d_loss[u].
// No floating-point atomics, one order per sum, beta^t by pow() of the step count: the bits depend on the inputs alone,
// not on the run or on how the updates are split into calls.  The barrier is k_deep_cfr_train_wide's: bounded by the
// wall clock, a workgroup that gives up raises the group's error word and a pinned host word.
#include "osg_cfr_internal.h"
#include "osg_vpnet_learn_plan.h"
#include "osg_vpnet_tile.h"

namespace {

using namespace osg_vpnet;

constexpr int kNc = 8;                                        // column tiles per wavefront (MR = 1)
constexpr unsigned long long kBarrierTicks = 400000000ull;   // 4 s of the 100 MHz wall clock

struct VlArgs {
  VpLearnPlan plan;
  int mask_words;
  int64_t U, step0;
  float *params, *m, *v;
  const float* obs;
  const int32_t* legal;
  const float* policy;
  const float* value;
  float* loss_out;
  unsigned int* bar;       // [0] arrivals, [1] a workgroup gave up (zeroed before the launch)
  float* partial;          // [G][partial_stride]
  float* saved;            // [G][slots][32 W16]
  unsigned int* host_err;
  double lr, beta1, beta2;
  float eps, wd;
};

// acc = dY W for this wavefront's column tiles: dY [32, out16] in LDS (row stride sdy), W [out, width] in global memory,
// KB of its rows per panel.  Ends with the workgroup met: nobody reads dY or a panel any more.
OSG_D void contract_rows(float* lds, const VpLearnPlan& L, const float* dy, int sdy, const float* w, int out, int mine, f4 (&acc)[kNc]) {
  const Lane ln = lane_of();
  const VpPlan& P = L.f;
  const int kb = L.kb, bs = L.bstride, wp = P.wp, W = P.width, stages = (out + kb - 1) / kb;
  float pre[kVpPanelRegs];
  const auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < kVpPanelRegs; ++q) {
      const int e = threadIdx.x + kVpThreads * q, row = e / wp, col = e % wp;
      pre[q] = row < kb && k0 + row < out && col < W ? w[static_cast<int64_t>(k0 + row) * W + col] : 0.0f;
    }
  };
  const auto store = [&](float* panel) {
#pragma unroll
    for (int q = 0; q < kVpPanelRegs; ++q) {
      const int e = threadIdx.x + kVpThreads * q, row = e / wp, col = e % wp;
      if (row < kb) panel[row * bs + col] = pre[q];
    }
  };
#pragma unroll
  for (int c = 0; c < kNc; ++c) acc[c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  fetch(0);
  store(lds + P.panel[0]);
  __syncthreads();
  for (int s = 0; s < stages; ++s) {
    if (s + 1 < stages) fetch((s + 1) * kb);
    const float* pan = lds + P.panel[s & 1] + ln.g * bs + ln.i;
    const float* x = dy + (ln.wr * kVpTile + ln.i) * sdy + s * kb + ln.g;
    for (int kk = 0; kk < kb; kk += 4) {
      const float fa = x[kk];
#pragma unroll
      for (int c = 0; c < kNc; ++c)
        if (c < mine) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, pan[kk * bs + (ln.wc + kVpWaveCols * c) * kVpTile], acc[c], 0, 0, 0);
    }
    if (s + 1 < stages) store(lds + P.panel[(s + 1) & 1]);
    __syncthreads();
  }
}

// dst[row][col] = (acc + add[row][col]) where mask[row][col] > 0, else 0 (add null: nothing to add); add has mask's stride.
OSG_D void write_masked(float* dst, int sd, const float* mask, int sm, const float* add, int mine, const f4 (&acc)[kNc]) {
  const Lane ln = lane_of();
#pragma unroll
  for (int c = 0; c < kNc; ++c)
    if (c < mine) {
      const int col = (ln.wc + kVpWaveCols * c) * kVpTile + ln.i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ln.wr * kVpTile + 4 * ln.g + r;
        const float v = add ? acc[c][r] + add[row * sm + col] : acc[c][r];
        dst[row * sd + col] = mask[row * sm + col] > 0.0f ? v : 0.0f;
      }
    }
}
OSG_D void write_plain(float* dst, int sd, int mine, const f4 (&acc)[kNc]) {
  const Lane ln = lane_of();
#pragma unroll
  for (int c = 0; c < kNc; ++c)
    if (c < mine) {
      const int col = (ln.wc + kVpWaveCols * c) * kVpTile + ln.i;
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(ln.wr * kVpTile + 4 * ln.g + r) * sd + col] = acc[c][r];
    }
}

// dW = dY^T X [out, in] and db = dY^T 1 over the workgroup's 32 rows to dst (weight, then bias): dY [32, out16] in LDS;
// X rows of stride sx, in LDS or global memory, zero at and past row xrows and column `in`.  Column tile nt of X on
// wavefront nt mod 8, its fragment in registers against 8 output tiles at a time; the four rows of a step four apart.
// (Out of line, as policy_top and adam_slice: inlined into the update loop they make its register allocation spill.)
__device__ __noinline__ void weight_gradient(float* dst, int out, int in, const float* dy, int sdy, const float* x, int sx, int xrows) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int nmt = (out + kVpTile - 1) / kVpTile, nnt = (in + kVpTile - 1) / kVpTile;
  for (int nt = wave; nt < nnt; nt += kVpThreads / 64) {
    const int col = nt * kVpTile + i;
    float xb[kVlRows / 4];
#pragma unroll
    for (int k = 0; k < kVlRows / 4; ++k) {
      const int row = (k / 4) * kVpTile + 4 * g + k % 4;
      xb[k] = col < in && row < xrows ? x[static_cast<int64_t>(row) * sx + col] : 0.0f;
    }
    for (int mt0 = 0; mt0 < nmt; mt0 += kNc) {
      f4 acc[kNc];
#pragma unroll
      for (int q = 0; q < kNc; ++q) acc[q] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < kVlRows / 4; ++k) {
        const float* a = dy + ((k / 4) * kVpTile + 4 * g + k % 4) * sdy + mt0 * kVpTile + i;
#pragma unroll
        for (int q = 0; q < kNc; ++q)
          if (mt0 + q < nmt) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q * kVpTile], xb[k], acc[q], 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < kNc; ++q)
        if (mt0 + q < nmt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = (mt0 + q) * kVpTile + 4 * g + r;
            if (o < out && col < in) dst[static_cast<int64_t>(o) * in + col] = acc[q][r];
          }
        }
    }
  }
  for (int o = threadIdx.x; o < out; o += kVpThreads) {
    float sum = 0.0f;
    for (int b = 0; b < kVlRows; ++b) sum = sum + dy[b * sdy + o];
    dst[static_cast<int64_t>(out) * in + o] = sum;
  }
}

// The policy loss and its gradient, 16 lanes per row (512 threads: one step): dLoss/dlogit in place of the logits,
// zeros in the padding; the row's -sum t log_softmax to its words.
__device__ __noinline__ void policy_top(float* lds, const VpLearnPlan& L, const VlArgs& a, int64_t u, int row0) {
  const VpPlan& P = L.f;
  const int i = threadIdx.x & 15, b = threadIdx.x >> 4, A = P.actions, at = row0 + b;
  const bool live = at < L.batch;
  const int64_t row = u * L.batch + (live ? at : 0);
  const int32_t* bits = a.legal + row * a.mask_words;
  const float* t = a.policy + row * A;
  float* z = lds + P.logits + b * P.logits_stride;
  float top = -INFINITY, mass = 0.0f, tsum = 0.0f;
  for (int x = i; x < A; x += 16)
    if (live && ((bits[x >> 5] >> (x & 31)) & 1) && z[x] > top) top = z[x];
  top = max16(top);
  for (int x = i; x < A; x += 16)
    if (live && ((bits[x >> 5] >> (x & 31)) & 1)) {
      mass = mass + expf(z[x] - top);
      tsum = tsum + t[x];
    }
  mass = sum16(mass);
  tsum = sum16(tsum);
  const bool any = live && mass > 0.0f;
  const float lse = any ? top + logf(mass) : 0.0f, inv = 1.0f / static_cast<float>(L.batch);
  float loss = 0.0f;
  for (int x = i; x < P.ap; x += 16) {
    float d = 0.0f;
    if (any && x < A && ((bits[x >> 5] >> (x & 31)) & 1)) {
      loss = loss - t[x] * (z[x] - lse);
      d = (expf(z[x] - top) / mass * tsum - t[x]) * inv;
    }
    z[x] = d;
  }
  loss = sum16(loss);
  if (i == 0) lds[L.row_words + b * kVlRowWords + 1] = loss;
}

// The group's barrier (k_deep_cfr_train_wide's).  False: a workgroup did not arrive within the bound, or another gave up.
OSG_D bool group_barrier(const VlArgs& a, unsigned int& epoch, int* s_ok) {
  ++epoch;
  __threadfence();   // this thread's stores are visible at agent scope, and drained, before the workgroup arrives
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(&a.bar[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned int want = epoch * static_cast<unsigned int>(a.plan.group);
    int ok = 1;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(&a.bar[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
      if (__hip_atomic_load(&a.bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u || wall_clock64() - t0 > kBarrierTicks) { ok = 0; break; }
      __builtin_amdgcn_s_sleep(1);
    }
    if (!ok) {
      __hip_atomic_store(&a.bar[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    *s_ok = ok;
  }
  __syncthreads();
  __threadfence();   // nothing below is served from a line cached before the others' stores
  return *s_ok != 0;
}

// Parameters [lo, hi) of the workgroup's slice: the G partials ascending, weight decay on weights, torch's Adam.
// Returns this thread's sum of w^2 over the weights it stepped (before the step).
OSG_D float adam_range(const VlArgs& a, int lo, int hi, bool weight, float step_size, float bc2_sqrt) {
  const VpLearnPlan& L = a.plan;
  const float beta1 = static_cast<float>(a.beta1), beta2 = static_cast<float>(a.beta2);
  float sq = 0.0f;
  for (int idx = lo + threadIdx.x; idx < hi; idx += kVpThreads) {
    float grad = a.partial[idx];
    for (int w = 1; w < L.group; ++w) grad = grad + a.partial[static_cast<size_t>(w) * L.partial_stride + idx];
    const float p = a.params[idx];
    if (weight) {
      grad = grad + a.wd * p;
      sq = sq + p * p;
    }
    const float m = beta1 * a.m[idx] + (1.0f - beta1) * grad;
    const float v = beta2 * a.v[idx] + (1.0f - beta2) * (grad * grad);
    a.m[idx] = m;
    a.v[idx] = v;
    a.params[idx] = p - step_size * (m / (sqrtf(v) / bc2_sqrt + a.eps));
  }
  return sq;
}
__device__ __noinline__ void adam_slice(float* lds, const VlArgs& a, int g, int64_t u, float* words) {
  const VpLearnPlan& L = a.plan;
  const VpPlan& P = L.f;
  const double t = static_cast<double>(a.step0 + u + 1);
  const float step_size = static_cast<float>(a.lr / (1.0 - pow(a.beta1, t))), bc2_sqrt = static_cast<float>(sqrt(1.0 - pow(a.beta2, t)));
  const int lo = g * L.slice, hi = lo + L.slice < P.param_count ? lo + L.slice : P.param_count;
  float sq = 0.0f;
  for (int k = 0; k <= P.depth + 4; ++k) {   // torso 0 .. depth, value 1, value 2, policy 1, policy 2
    const int h = k - P.depth;
    const int at = h <= 0 ? P.torso[k] : h == 1 ? P.v1 : h == 2 ? P.v2 : h == 3 ? P.p1 : P.p2;
    const int out = h == 2 ? 1 : h == 4 ? P.actions : P.width, in = k == 0 ? P.obs : P.width;
    const int w_end = at + out * in, b_end = w_end + out;
    sq = sq + adam_range(a, lo > at ? lo : at, hi < w_end ? hi : w_end, true, step_size, bc2_sqrt);
    adam_range(a, lo > w_end ? lo : w_end, hi < b_end ? hi : b_end, false, step_size, bc2_sqrt);
  }
  sq = osg_mfma::wave_sum(sq);
  if ((threadIdx.x & 63) == 0) lds[L.red + (threadIdx.x >> 6)] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.0f;
    for (int w = 0; w < kVpThreads / 64; ++w) sum = sum + lds[L.red + w];
    words[2] = sum;
  }
}

__global__ void __launch_bounds__(kVpThreads) k_vpnet_learn(const VlArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const VpLearnPlan& L = a.plan;
  const VpPlan& P = L.f;
  const Lane ln = lane_of();
  const int g = static_cast<int>(blockIdx.x), row0 = g * kVlRows, W = P.width, wp = P.wp, D = P.depth;
  const int wide = tiles_of(ln.wc, 0, wp / kVpTile, kNc), sa = P.act_stride, sz = P.logits_stride;
  float* act = lds + P.act;
  float* logits = lds + P.logits;
  float* rw = lds + L.row_words;
  int* s_ok = reinterpret_cast<int*>(lds + L.red + 15);
  float* mine = a.partial + static_cast<size_t>(g) * L.partial_stride;
  float* saved = a.saved + static_cast<size_t>(g) * L.slots * L.slot_floats;
  float* hv = saved + static_cast<size_t>(D + 1) * L.slot_floats;    // the value head's hidden layer
  float* dtp = saved + static_cast<size_t>(D + 2) * L.slot_floats;   // the policy head's gradient into the torso
  const float* torso_top = saved + static_cast<size_t>(D) * L.slot_floats;
  const int xrows = L.batch - row0 < kVlRows ? L.batch - row0 : kVlRows;
  unsigned int epoch = 0;
  for (int64_t u = 0; u < a.U; ++u) {
    float* words = mine + P.param_count + 4 * static_cast<int>(u & 1);
    VpArgs fa;
    fa.obs = a.obs + u * L.batch * P.obs;
    fa.n = L.batch;
    f4 acc[1][kNc];
    const float* wv2 = a.params + P.v2;
    const int narrow = tiles_of(ln.wc, 0, P.ap / kVpTile, kNc);
    // ---- forward: torso 0 .. D, the value head's hidden layer (D + 1), the policy head's (D + 2), the logits (D + 3) ----
    for (int l = 0; l <= D + 3; ++l) {
      const bool last = l == D + 3;
      const int off = l <= D ? P.torso[l] : l == D + 1 ? P.v1 : l == D + 2 ? P.p1 : P.p2;
      const int out = last ? P.actions : W, in = l == 0 ? P.obs : W, tiles = last ? narrow : wide;
      const float* w = a.params + off;
      const float* bias = w + out * in;
      clear(acc);
      if (l == 0) contract<1, kNc, true>(lds, P, fa, w, out, in, 0, tiles, row0, acc);
      else contract<1, kNc, false>(lds, P, fa, w, out, in, 0, tiles, row0, acc);
      if (l == D + 1) value_partials(lds + P.vpart, kVlRows, bias, wv2, W, wide, acc);
      if (l <= D + 1) write_back(saved + static_cast<size_t>(l) * L.slot_floats, wp, bias, W, 0, wide, true, acc);
      if (l != D + 1) write_back(last ? logits : act, last ? sz : sa, bias, out, 0, tiles, !last, acc);   // (the value head leaves the torso in place)
      __syncthreads();
      if (l == D + 1 && threadIdx.x < kVlRows) {
        const int b = threadIdx.x;
        const float* vp = lds + P.vpart + b;
        const float v = tanhf(((vp[0] + vp[kVlRows]) + (vp[2 * kVlRows] + vp[3 * kVlRows])) + wv2[W]);
        const bool live = row0 + b < L.batch;
        const float d = live ? v - a.value[u * L.batch + row0 + b] : 0.0f;
        rw[b * kVlRowWords] = 2.0f * d * (1.0f - v * v) / static_cast<float>(L.batch);
        rw[b * kVlRowWords + 2] = d * d;
      }
    }
    policy_top(lds, L, a, u, row0);
    __syncthreads();
    if (threadIdx.x < 64) {   // the workgroup's two loss sums: one 64-lane tree each
      const bool has = threadIdx.x < kVlRows;
      const float pl = osg_mfma::wave_sum(has ? rw[threadIdx.x * kVlRowWords + 1] : 0.0f);
      const float vl = osg_mfma::wave_sum(has ? rw[threadIdx.x * kVlRowWords + 2] : 0.0f);
      if (threadIdx.x == 0) { words[0] = pl; words[1] = vl; }
    }
    // ---- backward: logits (s = 0), policy hidden (1), value hidden (2), torso D .. 1 (3 ...), torso 0 (D + 3) ----
    for (int s = 0; s <= D + 3; ++s) {
      const int l = D + 3 - s;
      const bool top = s == 0, first = l == 0;
      if (s == 2) {   // the value head: dH = dy w2 through the mask; W -> 1's gradient on the way
        for (int x = threadIdx.x; x < kVlRows * wp; x += kVpThreads) {
          const int b = x / wp, c = x % wp;
          act[b * sa + c] = hv[x] > 0.0f ? rw[b * kVlRowWords] * wv2[c] : 0.0f;   // (hv is 0 past W)
        }
        for (int c = threadIdx.x; c <= W; c += kVpThreads) {
          float sum = 0.0f;
          for (int b = 0; b < kVlRows; ++b) sum = sum + rw[b * kVlRowWords] * (c < W ? hv[b * wp + c] : 1.0f);
          mine[P.v2 + c] = sum;
        }
        __syncthreads();
      }
      const int off = top ? P.p2 : s == 1 ? P.p1 : s == 2 ? P.v1 : P.torso[l];
      const float* dy = top ? logits : act;
      const int sdy = top ? sz : sa, out = top ? P.actions : W;
      // the layer's input: the policy hidden layer (still in LDS), the torso's top, the torso layer below, the observations
      const float* x = top ? act : s <= 2 ? torso_top : first ? fa.obs + static_cast<int64_t>(row0) * P.obs : saved + static_cast<size_t>(l - 1) * L.slot_floats;
      const int sx = top ? sa : first ? P.obs : wp;
      weight_gradient(mine + off, out, first ? P.obs : W, dy, sdy, x, sx, first ? xrows : kVlRows);
      if (first) break;
      __syncthreads();
      contract_rows(lds, L, dy, sdy, a.params + off, out, wide, acc[0]);
      if (s == 1) write_plain(dtp, wp, wide, acc[0]);                                  // the policy head's share of dT
      else write_masked(act, sa, x, sx, s == 2 ? dtp : nullptr, wide, acc[0]);         // (s == 2: value + policy)
      __syncthreads();
    }
    // ---- the step ----
    bool ok = group_barrier(a, epoch, s_ok);
    if (ok) {
      adam_slice(lds, a, g, u, words);
      ok = group_barrier(a, epoch, s_ok);
    }
    if (!ok) {   // a hung device: every workgroup leaves, the rest of the losses say so
      if (g == 0)
        for (int64_t k = 3 * u + threadIdx.x; k < 3 * a.U; k += kVpThreads) a.loss_out[k] = __builtin_nanf("");
      return;
    }
    if (g == 0 && threadIdx.x < 3) {
      float sum = 0.0f;
      for (int w = 0; w < L.group; ++w) sum = sum + a.partial[static_cast<size_t>(w) * L.partial_stride + P.param_count + 4 * static_cast<int>(u & 1) + threadIdx.x];
      a.loss_out[3 * u + threadIdx.x] = threadIdx.x == 2 ? a.wd * sum / 2.0f : sum / static_cast<float>(L.batch);
    }
  }
}

VpShape shape_of(int32_t obs_size, int32_t width, int32_t depth, int32_t actions) {
  VpShape s;
  s.obs = obs_size; s.width = width; s.depth = depth; s.actions = actions;
  return s;
}

}  // namespace

extern "C" int osg_vpnet_learn_plan(osg_ctx* ctx, int32_t obs_size, int32_t width, int32_t depth, int32_t actions, int32_t batch,
                                    int64_t* plan) {
  const std::string who = "osg_vpnet_learn_plan: ";
  if (!ctx || !plan) return set_error(OSG_ERR_INVALID, who + "bad argument");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  const VpLearnPlan L = plan_vpnet_learn(shape_of(obs_size, width, depth, actions), batch, limit);
  if (!L.ok) return set_error(OSG_ERR_UNSUPPORTED, who + L.why);
  plan[0] = L.f.rows; plan[1] = L.group; plan[2] = static_cast<int64_t>(L.f.lds_bytes); plan[3] = static_cast<int64_t>(L.scratch_bytes);
  plan[4] = L.f.param_count; plan[5] = 1; plan[6] = L.slots; plan[7] = L.slice;
  return OSG_OK;
}

extern "C" int osg_vpnet_learn(osg_ctx* ctx, const osg_vpnet_learn_job* job) {
  const std::string who = "osg_vpnet_learn: ";
  if (!ctx || !job) return set_error(OSG_ERR_INVALID, who + "bad argument");
  const osg_vpnet_learn_job& in = *job;
  if (in.updates < 0 || in.step0 < 0 || in.mask_words < 1 || !in.d_params || !in.d_adam_m || !in.d_adam_v || !in.d_obs || !in.d_legal_bits ||
      !in.d_policy || !in.d_value || !in.d_loss || !(in.beta1 >= 0.0 && in.beta1 < 1.0) || !(in.beta2 >= 0.0 && in.beta2 < 1.0) ||
      !(in.eps >= 0.0) || !(in.weight_decay >= 0.0))
    return set_error(OSG_ERR_INVALID, who + "bad argument");
  if (!ctx->h_learn_err) {
    OSG_HIP(ctx->h_learn_err.alloc(1));
    *ctx->h_learn_err.get() = 0u;
  }
  if (__atomic_exchange_n(ctx->h_learn_err.get(), 0u, __ATOMIC_RELAXED) != 0u)
    return set_error(OSG_ERR_HIP, who + "a group barrier timed out in an earlier launch (a hung or oversubscribed device); the losses it "
                                        "left are NaN and the parameters are not usable");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  if (ctx->num_cus == 0) {
    hipDeviceProp_t prop;
    OSG_HIP(hipGetDeviceProperties(&prop, ctx->device));
    ctx->num_cus = prop.multiProcessorCount;
  }
  VlArgs a;
  a.plan = plan_vpnet_learn(shape_of(in.obs_size, in.width, in.depth, in.actions), in.batch, limit);
  if (!a.plan.ok) return set_error(OSG_ERR_UNSUPPORTED, who + a.plan.why);
  if (in.actions > 32 * static_cast<int64_t>(in.mask_words)) return set_error(OSG_ERR_INVALID, who + "more actions than the legal mask has bits");
  if (a.plan.group > ctx->num_cus)
    return set_error(OSG_ERR_UNSUPPORTED, who + "the group needs more workgroups than the device's " + std::to_string(ctx->num_cus) +
                                              " compute units hold at once (one per unit)");
  if (in.updates == 0) return OSG_OK;
  a.plan.why = nullptr;
  a.mask_words = in.mask_words; a.U = in.updates; a.step0 = in.step0;
  a.params = in.d_params; a.m = in.d_adam_m; a.v = in.d_adam_v;
  a.obs = in.d_obs; a.legal = in.d_legal_bits; a.policy = in.d_policy; a.value = in.d_value; a.loss_out = in.d_loss;
  a.lr = in.learning_rate; a.beta1 = in.beta1; a.beta2 = in.beta2;
  a.eps = static_cast<float>(in.eps); a.wd = static_cast<float>(in.weight_decay);
  const void* kernel = reinterpret_cast<const void*>(&k_vpnet_learn);
  const size_t lds = a.plan.f.lds_bytes;
  if (lds > (32u << 10) && raise_lds_cap(kernel, static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(OSG_ERR_UNSUPPORTED, who + "the device does not grant " + std::to_string(lds) + " bytes of LDS to a workgroup");
  }
  hipStream_t st = ctx->stream;
  void* ptr = nullptr;
  if (int rc = osg_ctx_scratch(ctx, a.plan.scratch_bytes, &ptr)) return rc;
  unsigned char* base = static_cast<unsigned char*>(ptr);
  a.bar = reinterpret_cast<unsigned int*>(base);
  a.partial = reinterpret_cast<float*>(base + a.plan.scratch_partial);
  a.saved = reinterpret_cast<float*>(base + a.plan.scratch_saved);
  a.host_err = ctx->h_learn_err.get();
  OSG_HIP(hipMemsetAsync(base, 0, a.plan.scratch_partial, st));
  void* args[] = {&a};
  OSG_HIP(launch_grid_barrier_kernel(kernel, dim3(static_cast<unsigned>(a.plan.group)), dim3(kVpThreads), args, lds, st));
  return OSG_OK;
}
