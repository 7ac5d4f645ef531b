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
#include "osg_vpnet_tile.h"

namespace {

using namespace osg;
using namespace osg_vpnet;

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
