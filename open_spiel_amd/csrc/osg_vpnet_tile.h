// What the policy-value kernels share (k_vpnet_forward, osg_vpnet.hip; k_vpnet_learn, osg_vpnet_learn.hip): the lane's
// place in the 2 x 4 wavefront grid, the panel and observation fetches, the register-blocked contraction acc += X W^T on
// v_mfma_f32_16x16x4_f32, the accumulators' write-back and the value head's W -> 1 reduction.  The layouts and their bank
// arguments are osg_vpnet_plan.h.
#pragma once
#include <cmath>

#include "osg_internal.h"
#include "osg_mfma_tile.h"
#include "osg_vpnet_plan.h"

namespace osg_vpnet {

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

}  // namespace osg_vpnet
