// The fused policy-value MLP forward of the network-guided search: alpha_zero_torch's nn_model == "mlp" (model.cc:216-263,
// 318-336, 391-396) for n states in one launch, writing the prior [n, A] f64 and the value [n, 2] f64 = {v, -v} that
// osg_mcts_tree_advance reads (vpevaluator.cc:73-85).  The plan — R rows per workgroup, the wavefronts' register
// blocking, the panel depth, every LDS offset and its bank argument — is osg_vpnet_plan.h; this file follows it.
//
// A workgroup (8 wavefronts, 2 over the rows x 4 over the columns) carries rows [R b, R (b + 1)) through every layer:
//   torso 0     the observation tile streams from global memory in chunks of KC columns (zeros past O and past row n)
//               beside the weight panels of the same columns; the layer's output stays in the accumulators;
//   in place    the workgroup meets, and bias + ReLU on the accumulators overwrite the ONE activation buffer; the next
//               layer contracts over it while its weights stream through the two panel buffers (fetch panel s + 1 into
//               registers, matrix instructions on panel s, registers into the other buffer, one __syncthreads);
//   value head  its hidden layer is reduced against the W -> 1 weights on the accumulators (lane, 16-lane tree, the four
//               column wavefronts ascending), then tanh; the torso is still in LDS for
//   policy head whose hidden layer then overwrites the torso; W -> A runs in passes of 64 NC columns into the logits;
//   softmax     16 lanes per row over the legal actions only: max, then sum of exp in one order, f64 at the store; an
//               illegal action gets exactly 0 and a row without a legal action an all-zero prior.
// fp32 in, fp32 accumulate (v_mfma_f32_16x16x4_f32); no atomics; a row's bits depend on that row and the parameters.
#include <cmath>

#include "osg_internal.h"
#include "osg_mfma_tile.h"
#include "osg_vpnet_plan.h"

namespace {

using namespace osg;
using namespace osg_vpnet;
using osg_mfma::f4;
using osg_mfma::sum16;

struct VpArgs {
  VpPlan plan;
  const float* params;
  const float* obs;
  const int32_t* legal;
  int mask_words;
  int64_t n;
  double* prior;
  double* value;
};

// Where a lane of wavefront (wr, wc) stands: lane 16 g + i.
struct Lane {
  int wr, wc, i, g;
};
OSG_D Lane lane_of() {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  return Lane{wave / kVpWaveCols, wave % kVpWaveCols, lane & 15, lane >> 4};
}
// The column tiles wc, wc + 4, ... of a pass that starts at tile0 and ends before `tiles`: how many wavefront wc has.
OSG_D int tiles_of(int wc, int tile0, int tiles, int nc) {
  const int here = tiles - tile0 < kVpWaveCols * nc ? tiles - tile0 : kVpWaveCols * nc;
  return here > wc ? (here - wc + kVpWaveCols - 1) / kVpWaveCols : 0;
}

template <int MR, int NC>
OSG_D void clear(f4 (&acc)[MR][NC]) {
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[m][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
}

// Columns [k0, k0 + KC) of the weight rows a pass needs (output rows 16 tile0 ...; zeros past `out` and past `in`) into
// the thread's registers — KC consecutive threads read KC consecutive words of a row — and from there into a panel.
OSG_D void panel_fetch(float (&pre)[kVpPanelRegs], const VpPlan& P, const float* w, int out, int in, int tile0, int pass_rows, int k0) {
  const int kc = P.kc;
#pragma unroll
  for (int q = 0; q < kVpPanelRegs; ++q) {
    const int e = threadIdx.x + kVpThreads * q, row = e / kc, col = e % kc;
    const int o = tile0 * kVpTile + row;
    pre[q] = row < pass_rows && o < out && k0 + col < in ? w[static_cast<int64_t>(o) * in + k0 + col] : 0.0f;
  }
}
OSG_D void panel_store(const float (&pre)[kVpPanelRegs], float* panel, const VpPlan& P, int pass_rows) {
  const int kc = P.kc;
#pragma unroll
  for (int q = 0; q < kVpPanelRegs; ++q) {
    const int e = threadIdx.x + kVpThreads * q, row = e / kc, col = e % kc;
    if (row < pass_rows) panel[row * kc + (col ^ vp_swizzle(kc, row))] = pre[q];
  }
}
// The same for the observation tile: rows row0 ... of d_obs, columns [k0, k0 + KC).
OSG_D void obs_fetch(float (&pre)[kVpObsRegs], const VpPlan& P, const VpArgs& a, int64_t row0, int k0) {
  const int kc = P.kc;
#pragma unroll
  for (int q = 0; q < kVpObsRegs; ++q) {
    const int e = threadIdx.x + kVpThreads * q, row = e / kc, col = e % kc;
    const int64_t at = row0 + row;
    pre[q] = row < P.rows && at < a.n && k0 + col < P.obs ? a.obs[at * P.obs + k0 + col] : 0.0f;
  }
}
OSG_D void obs_store(const float (&pre)[kVpObsRegs], float* stage, const VpPlan& P) {
  const int kc = P.kc;
#pragma unroll
  for (int q = 0; q < kVpObsRegs; ++q) {
    const int e = threadIdx.x + kVpThreads * q, row = e / kc, col = e % kc;
    if (row < P.rows) stage[row * kc + (col ^ vp_swizzle(kc, row))] = pre[q];
  }
}

// acc += X W^T for one pass of a layer: X the workgroup's rows ([R, in]: the activation buffer, or with kObs the
// observation rows from global memory), W [out, in] in global memory, the pass's column tiles tile0 ... (this
// wavefront has `mine` of them).  Ends with the workgroup met: nobody reads X or a panel any more.
template <int MR, int NC, bool kObs>
OSG_D void contract(float* lds, const VpPlan& P, const VpArgs& a, const float* w, int out, int in, int tile0, int mine, int64_t row0,
                    f4 (&acc)[MR][NC]) {
  const Lane L = lane_of();
  const int kc = P.kc, stages = (in + kc - 1) / kc;
  const int left = (out + kVpTile - 1) / kVpTile * kVpTile - tile0 * kVpTile;
  const int pass_rows = left < P.panel_rows ? left : P.panel_rows;
  const int swz = vp_swizzle(kc, L.i);
  float pre[kVpPanelRegs];
  float xpre[kVpObsRegs];
  panel_fetch(pre, P, w, out, in, tile0, pass_rows, 0);
  if (kObs) obs_fetch(xpre, P, a, row0, 0);
  panel_store(pre, lds + P.panel[0], P, pass_rows);
  if (kObs) obs_store(xpre, lds + P.xstage[0], P);
  __syncthreads();
  for (int s = 0; s < stages; ++s) {
    if (s + 1 < stages) {
      panel_fetch(pre, P, w, out, in, tile0, pass_rows, (s + 1) * kc);
      if (kObs) obs_fetch(xpre, P, a, row0, (s + 1) * kc);
    }
    const float* pan = lds + P.panel[s & 1] + L.i * kc + L.g;
    const float* x = kObs ? lds + P.xstage[s & 1] + L.i * kc + L.g : lds + P.act + L.i * P.act_stride + s * kc + L.g;
    const int sx = kObs ? kc : P.act_stride;
    for (int kk = 0; kk < kc; kk += 4) {
      const int kx = kObs ? kk ^ swz : kk;
      float fa[MR], fb[NC];
#pragma unroll
      for (int m = 0; m < MR; ++m) fa[m] = x[(L.wr + kVpWaveRows * m) * kVpTile * sx + kx];
#pragma unroll
      for (int c = 0; c < NC; ++c) fb[c] = c < mine ? pan[(L.wc + kVpWaveCols * c) * kVpTile * kc + (kk ^ swz)] : 0.0f;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < mine) {
#pragma unroll
          for (int m = 0; m < MR; ++m) acc[m][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[m], fb[c], acc[m][c], 0, 0, 0);
        }
    }
    if (s + 1 < stages) {
      panel_store(pre, lds + P.panel[(s + 1) & 1], P, pass_rows);
      if (kObs) obs_store(xpre, lds + P.xstage[(s + 1) & 1], P);
    }
    __syncthreads();
  }
}

// dst[row][col] = acc + bias (ReLU where asked) for the pass's tiles; columns past `out` get bias 0: with the zero
// weight rows of the panels they hold exact zeros, which the next contraction's padded columns rely on.
template <int MR, int NC>
OSG_D void write_back(float* dst, int sd, const float* bias, int out, int tile0, int mine, bool relu, const f4 (&acc)[MR][NC]) {
  const Lane L = lane_of();
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < mine) {
      const int col = (tile0 + L.wc + kVpWaveCols * c) * kVpTile + L.i;
      const float b = col < out ? bias[col] : 0.0f;
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[m][c][r] + b;
          if (relu) v = v > 0.0f ? v : 0.0f;
          dst[((L.wr + kVpWaveRows * m) * kVpTile + 4 * L.g + r) * sd + col] = v;
        }
    }
}

// The value head's W -> 1 layer on the accumulators of its hidden layer: this wavefront's columns of every row, its
// tiles ascending, then one tree over the 16 lanes of a row; column wavefront wc's sum of row b goes to vpart[wc][b].
template <int MR, int NC>
OSG_D void value_partials(float* vpart, int rows, const float* bias, const float* w2, int width, int mine, const f4 (&acc)[MR][NC]) {
  const Lane L = lane_of();
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float part = 0.0f;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < mine) {
          const int col = (L.wc + kVpWaveCols * c) * kVpTile + L.i;
          if (col < width) {
            const float h = acc[m][c][r] + bias[col];
            part = part + (h > 0.0f ? h : 0.0f) * w2[col];
          }
        }
      part = sum16(part);
      if (L.i == 0) vpart[L.wc * rows + (L.wr + kVpWaveRows * m) * kVpTile + 4 * L.g + r] = part;
    }
}

OSG_D float max16(float v) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const float o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}

// The masked softmax of the logits and the two stores: 16 lanes per row, lane i on actions i, i + 16, ...
OSG_D void softmax_and_store(const float* lds, const VpPlan& P, const VpArgs& a, int64_t row0) {
  const int i = threadIdx.x & 15, A = P.actions;
  for (int b = threadIdx.x >> 4; b < P.rows; b += kVpThreads / 16) {
    const int64_t at = row0 + b;
    const bool live = at < a.n;
    const int32_t* bits = a.legal + (live ? at : 0) * a.mask_words;
    const float* z = lds + P.logits + b * P.logits_stride;
    float top = -INFINITY;
    for (int x = i; x < A; x += 16)
      if (live && ((bits[x >> 5] >> (x & 31)) & 1) && z[x] > top) top = z[x];
    top = max16(top);
    float mass = 0.0f;
    for (int x = i; x < A; x += 16)
      if (live && ((bits[x >> 5] >> (x & 31)) & 1)) mass = mass + expf(z[x] - top);
    mass = sum16(mass);
    if (live) {
      for (int x = i; x < A; x += 16) {
        const bool legal = (bits[x >> 5] >> (x & 31)) & 1;
        a.prior[at * A + x] = legal ? static_cast<double>(expf(z[x] - top) / mass) : 0.0;
      }
      if (i == 0) {
        const double v = static_cast<double>(lds[P.vals + b]);
        a.value[2 * at] = v;
        a.value[2 * at + 1] = -v;
      }
    }
  }
}

template <int MR, int NC>
__global__ void __launch_bounds__(kVpThreads) k_vpnet_forward(const VpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const VpPlan& P = a.plan;
  const Lane L = lane_of();
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * P.rows;
  const int W = P.width, wide = tiles_of(L.wc, 0, P.wp / kVpTile, NC);
  float* act = lds + P.act;
  f4 acc[MR][NC];
  clear(acc);
  contract<MR, NC, true>(lds, P, a, a.params + P.torso[0], W, P.obs, 0, wide, row0, acc);
  write_back(act, P.act_stride, a.params + P.torso[0] + W * P.obs, W, 0, wide, true, acc);
  __syncthreads();
  // the torso's other layers, then the value head's hidden layer (l == depth + 1) and the policy head's (depth + 2)
  for (int l = 1; l <= P.depth + 2; ++l) {
    const float* w = a.params + (l <= P.depth ? P.torso[l] : l == P.depth + 1 ? P.v1 : P.p1);
    clear(acc);
    contract<MR, NC, false>(lds, P, a, w, W, W, 0, wide, row0, acc);
    if (l == P.depth + 1) {
      const float* w2 = a.params + P.v2;
      value_partials(lds + P.vpart, P.rows, w + W * W, w2, W, wide, acc);
      __syncthreads();
      if (threadIdx.x < P.rows) {
        const float* vp = lds + P.vpart + threadIdx.x;
        lds[P.vals + threadIdx.x] = tanhf(((vp[0] + vp[P.rows]) + (vp[2 * P.rows] + vp[3 * P.rows])) + w2[W]);
      }
    } else {
      write_back(act, P.act_stride, w + W * W, W, 0, wide, true, acc);
      __syncthreads();
    }
  }
  const float* wp2 = a.params + P.p2;
  for (int tile0 = 0; tile0 < P.ap / kVpTile; tile0 += kVpWaveCols * NC) {
    const int mine = tiles_of(L.wc, tile0, P.ap / kVpTile, NC);
    clear(acc);
    contract<MR, NC, false>(lds, P, a, wp2, P.actions, W, tile0, mine, row0, acc);
    write_back(lds + P.logits, P.logits_stride, wp2 + P.actions * W, P.actions, tile0, mine, false, acc);
  }
  __syncthreads();
  softmax_and_store(lds, P, a, row0);
}

VpShape shape_of(int32_t obs_size, int32_t width, int32_t depth, int32_t actions) {
  VpShape s;
  s.obs = obs_size; s.width = width; s.depth = depth; s.actions = actions;
  return s;
}

}  // namespace

extern "C" int osg_vpnet_plan(osg_ctx* ctx, int32_t obs_size, int32_t width, int32_t depth, int32_t actions, int64_t* plan) {
  const std::string who = "osg_vpnet_plan: ";
  if (!ctx || !plan) return set_error(OSG_ERR_INVALID, who + "bad argument");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  const VpPlan p = plan_vpnet(shape_of(obs_size, width, depth, actions), limit);
  if (!p.ok) return set_error(OSG_ERR_UNSUPPORTED, who + p.why);
  plan[0] = p.rows; plan[1] = p.kc; plan[2] = static_cast<int64_t>(p.lds_bytes); plan[3] = p.param_count;
  plan[4] = p.mr; plan[5] = p.nc; plan[6] = p.panel_rows; plan[7] = p.act_stride;
  return OSG_OK;
}

extern "C" int osg_vpnet_forward(osg_ctx* ctx, int32_t obs_size, int32_t width, int32_t depth, int32_t actions, const float* d_params,
                                 const float* d_obs, const int32_t* d_legal_bits, int32_t mask_words, int64_t n, double* d_prior,
                                 double* d_value) {
  const std::string who = "osg_vpnet_forward: ";
  if (!ctx || !d_params || !d_obs || !d_legal_bits || !d_prior || !d_value || n < 1 || mask_words < 1)
    return set_error(OSG_ERR_INVALID, who + "bad argument");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  VpArgs a;
  a.plan = plan_vpnet(shape_of(obs_size, width, depth, actions), limit);
  if (!a.plan.ok) return set_error(OSG_ERR_UNSUPPORTED, who + a.plan.why);
  if (actions > 32 * static_cast<int64_t>(mask_words)) return set_error(OSG_ERR_INVALID, who + "more actions than the legal mask has bits");
  const int64_t blocks = (n + a.plan.rows - 1) / a.plan.rows;
  if (blocks >= (int64_t{1} << 31)) return set_error(OSG_ERR_UNSUPPORTED, who + "2^31 workgroups or more");
  a.plan.why = nullptr;
  a.params = d_params; a.obs = d_obs; a.legal = d_legal_bits; a.mask_words = mask_words; a.n = n;
  a.prior = d_prior; a.value = d_value;
  void (*kernel)(const VpArgs) = a.plan.mr == 4 ? &k_vpnet_forward<4, 4> : a.plan.mr == 2 ? &k_vpnet_forward<2, 8> : &k_vpnet_forward<1, 8>;
  const size_t lds = a.plan.lds_bytes;
  if (lds > (32u << 10) && raise_lds_cap(reinterpret_cast<const void*>(kernel), static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(OSG_ERR_UNSUPPORTED, who + "the device does not grant " + std::to_string(lds) + " bytes of LDS to a workgroup");
  }
  kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(kVpThreads), lds, ctx->stream>>>(a);
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}
