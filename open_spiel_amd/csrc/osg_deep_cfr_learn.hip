// The fused learner of Deep CFR (open_spiel/python/pytorch/deep_cfr.py:343-420 _learn_advantage_network and
// _learn_strategy_network, both with Adam): every update a call of DeepCFRSolver._train makes, in one launch.
//
// A job is one network of deep_cfr.MLP — Linear + ReLU per hidden layer, LayerNorm, Linear, and for the policy network a
// softmax over all action ids — and its U sequential Adam updates.  The updates are a chain, so ONE workgroup
// (8 wavefronts) runs one job from its first update to its last with the parameters in LDS (osg_adam_plan.h has the
// layout, the strides, which reads may collide on banks and what the planner chooses); jobs of a call run side by side.
//
// What differs from k_mlp_train (osg_mlp_train.hip) is the batch: up to 1024 rows, walked in tiles of T rows.  Per
// tile, ascending: gather the rows and their tensors, forward, loss and top gradient, backward.  Nothing is stepped
// meanwhile — the weights do not move between tiles, so dH reads the weights (or their transposed copies) as they
// are — and the gradient of every [out, in] tile stays in the accumulator registers of the wavefront that owns it
// (own_grad): the matrix instruction adds each 16-row chunk of each batch tile onto it.  The LayerNorm gradients are
// sums of one thread per column.  After the last tile's backward the owners step their parameters (Adam, torch's
// defaults) straight from the accumulators, with the moments in LDS or, where they do not fit, in the job's global
// buffers; then the transposed copies are refreshed.
//
// Contractions (v_mfma_f32_16x16x4_f32, osg_mfma_tile.h), per tile of T rows:
//   forward  Y = X W^T + b      [T, out] tiles over the wavefronts; contraction over `in`
//   dH = dY W                   the same split; contraction over `out`, B from the transposed copy (or from W, colliding)
//   dW += dY^T X, db += dY^T 1  the [out, in] tiles over the wavefronts; contraction over the tile's rows
// Every sum has one order: the instruction's and the k loop's, tiles ascending, 16-lane shuffle trees for the
// LayerNorm statistics, rows ascending for its gradients, a lane-strided sum and one 64-lane tree for the loss.  No
// atomics: a job's bits depend on its own inputs only (and on T, which the planner derives from the shape and the limit).
#include "osg_adam_plan.h"
#include "osg_cfr_internal.h"
#include "osg_mfma_tile.h"

using namespace osg_adam;
using namespace osg_mfma;   // f4, mma_rows, mma_cols, wave_sum

namespace {

struct AdamJob {   // one job as the kernel sees it (device pointers)
  AdamLayout lay;
  int kind, S, A;
  int64_t U, I, rows;
  float *params, *m, *v;
  const float* tensors;
  const int32_t* info;        // the reservoir's columns
  const int32_t* iter;
  const float* vals;          // [rows, A]
  const int64_t* slots;
  float* loss_out;
  double lr, beta1, beta2, pow1, pow2;   // pow: beta ^ (updates already made)
  float eps, ln_eps;
};

typedef f4 Grads[kAdamMaxOwn];   // a wavefront's gradient tiles: tile t = wave + 8 s in accumulator s

// The flat parameters (network.parameters() order) into the padded LDS layout, zeros in the padding; the moments flat.
OSG_D void load_params(float* lds, const AdamLayout& L, const AdamJob& j) {
  for (int l = 0; l < L.n_linear; ++l) {
    const int sw = L.w_stride[l], in = L.in[l], out = L.out[l];
    const float* w = j.params + L.param_off[l];
    for (int x = threadIdx.x; x < L.out_pad[l] * sw; x += kAdamThreads) {
      const int o = x / sw, c = x % sw;
      lds[L.w[l] + x] = o < out && c < in ? w[o * in + c] : 0.0f;
    }
    for (int o = threadIdx.x; o < L.out_pad[l]; o += kAdamThreads) lds[L.b[l] + o] = o < out ? w[out * in + o] : 0.0f;
  }
  for (int c = threadIdx.x; c < L.ln_pad; c += kAdamThreads) {
    lds[L.gamma + c] = c < L.ln_width ? j.params[L.ln_off + c] : 0.0f;
    lds[L.beta + c] = c < L.ln_width ? j.params[L.ln_off + L.ln_width + c] : 0.0f;
  }
  if (L.moments_resident)
    for (int x = threadIdx.x; x < L.param_count; x += kAdamThreads) {
      lds[L.mom_m + x] = j.m[x];
      lds[L.mom_v + x] = j.v[x];
    }
}
OSG_D void store_params(const float* lds, const AdamLayout& L, const AdamJob& j) {
  for (int l = 0; l < L.n_linear; ++l) {
    const int sw = L.w_stride[l], in = L.in[l], out = L.out[l];
    float* w = j.params + L.param_off[l];
    for (int x = threadIdx.x; x < out * in; x += kAdamThreads) w[x] = lds[L.w[l] + (x / in) * sw + x % in];
    for (int o = threadIdx.x; o < out; o += kAdamThreads) w[out * in + o] = lds[L.b[l] + o];
  }
  for (int c = threadIdx.x; c < L.ln_width; c += kAdamThreads) {
    j.params[L.ln_off + c] = lds[L.gamma + c];
    j.params[L.ln_off + L.ln_width + c] = lds[L.beta + c];
  }
  if (L.moments_resident)
    for (int x = threadIdx.x; x < L.param_count; x += kAdamThreads) {
      j.m[x] = lds[L.mom_m + x];
      j.v[x] = lds[L.mom_v + x];
    }
}
OSG_D void refresh_transposed(float* lds, const AdamLayout& L, int l) {
  const int sw = L.w_stride[l], swt = L.wt_stride[l], op = L.out_pad[l];
  for (int x = threadIdx.x; x < L.in_pad[l] * op; x += kAdamThreads) {
    const int c = x / op, o = x % op;
    lds[L.wt[l] + c * swt + o] = lds[L.w[l] + o * sw + c];
  }
}

// Tile k of update u: its rows' words and X [T, S16] (a row past the batch or naming something out of range: zeros,
// infostate -1; the latter also raises the update's flag).
OSG_D void fetch_tile(float* lds, const AdamLayout& L, const AdamJob& j, int64_t u, int k) {
  int* rows = reinterpret_cast<int*>(lds + L.rows);
  const int b = threadIdx.x;
  if (b < L.tile) {
    const int at = k * L.tile + b;
    int info = -1, slot = 0;
    float it = 0.0f;
    bool bad = false;
    if (at < L.batch) {
      const int64_t s = j.slots[u * L.batch + at];
      bad = s < 0 || s >= j.rows;
      if (!bad) {
        info = j.info[s];
        bad = info < 0 || info >= j.I;
      }
      if (bad) info = -1;
      else { slot = static_cast<int>(s); it = static_cast<float>(j.iter[s]); }
    }
    rows[b * kAdamRowWords] = info;
    rows[b * kAdamRowWords + 1] = slot;
    lds[L.rows + b * kAdamRowWords + 2] = it;
    lds[L.rows + b * kAdamRowWords + 3] = 0.0f;
    if (bad) lds[L.reduce] = 1.0f;   // (every writer writes the same word)
  }
  __syncthreads();
  const int sp = L.in_pad[0], sx = L.act_stride[0];
  for (int x = threadIdx.x; x < L.tile * sp; x += kAdamThreads) {
    const int r = x / sp, c = x % sp;
    const int i = rows[r * kAdamRowWords];
    lds[L.act[0] + r * sx + c] = i >= 0 && c < j.S ? j.tensors[static_cast<int64_t>(i) * j.S + c] : 0.0f;
  }
  __syncthreads();
}

// Layer l on the tile: act[l] -> act[l + 1] with ReLU, or for the last layer N -> Z.
OSG_D void forward_linear(float* lds, const AdamLayout& L, int l) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const bool top = l + 1 == L.n_linear;
  const float* x = lds + (top ? L.n : L.act[l]);
  float* y = lds + (top ? L.z : L.act[l + 1]);
  const int sx = L.act_stride[l], sy = top ? L.z_stride : L.act_stride[l + 1], sw = L.w_stride[l];
  const int nrt = L.tile / kAdamTile, tiles = nrt * (L.out_pad[l] / kAdamTile);
  for (int t = wave; t < tiles; t += kAdamWaves) {
    const int rt = t % nrt, ct = t / nrt;
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    acc = mma_rows(x + rt * kAdamTile * sx, sx, lds + L.w[l] + ct * kAdamTile * sw, sw, L.in_pad[l], acc);
    const float bias = lds[L.b[l] + ct * kAdamTile + i];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[r] + bias;
      if (!top) v = v > 0.0f ? v : 0.0f;
      y[(rt * kAdamTile + 4 * g + r) * sy + ct * kAdamTile + i] = v;
    }
  }
  __syncthreads();
}

// nn.LayerNorm (biased variance) on the last hidden activation H: N = gamma x^ + beta; a row's mean and 1 / std go to its
// words.  16 lanes per row, the four rows of a step four apart.
OSG_D void layer_norm_forward(float* lds, const AdamLayout& L, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int last = L.n_linear - 1, s = L.n_stride;
  const float width = static_cast<float>(L.ln_width);
  for (int chunk = wave; chunk < L.tile / kAdamTile; chunk += kAdamWaves)
    for (int t = 0; t < 4; ++t) {
      const int row = chunk * kAdamTile + t + 4 * g;
      const float* h = lds + L.act[last] + row * s;
      float sum = 0.0f, sq = 0.0f;
      for (int c = i; c < L.ln_pad; c += 16) sum = sum + h[c];      // (the padding holds zeros)
      const float mean = sum16(sum) / width;
      for (int c = i; c < L.ln_width; c += 16) sq = sq + (h[c] - mean) * (h[c] - mean);
      const float rstd = 1.0f / sqrtf(sum16(sq) / width + eps);
      for (int c = i; c < L.ln_pad; c += 16) lds[L.n + row * s + c] = lds[L.gamma + c] * ((h[c] - mean) * rstd) + lds[L.beta + c];
      if (i == 0) {
        lds[L.rows + row * kAdamRowWords + 4] = mean;
        lds[L.rows + row * kAdamRowWords + 5] = rstd;
      }
    }
  __syncthreads();
}

// The loss of every row of the tile and dLoss/dZ in place of Z (zeros in the padding and in rows that do not count);
// returns the tile's sum of it_b (y - t)^2 (the same on every thread).
OSG_D float top_gradient(float* lds, const AdamLayout& L, const AdamJob& j) {
  const int* rows = reinterpret_cast<const int*>(lds + L.rows);
  const int b = threadIdx.x, ap = L.out_pad[L.n_linear - 1];
  const float inv = 1.0f / static_cast<float>(L.batch * j.A);
  if (b < L.tile) {
    float* z = lds + L.z + b * L.z_stride;
    float loss = 0.0f;
    if (rows[b * kAdamRowWords] < 0) {
      for (int a = 0; a < ap; ++a) z[a] = 0.0f;
    } else {
      const float it = lds[L.rows + b * kAdamRowWords + 2];
      const float* t = j.vals + static_cast<int64_t>(rows[b * kAdamRowWords + 1]) * j.A;
      float top = 0.0f, mass = 1.0f, dot = 0.0f;
      if (j.kind == 1) {   // y = softmax(z) over all action ids
        top = z[0];
        for (int a = 1; a < j.A; ++a) top = z[a] > top ? z[a] : top;
        mass = 0.0f;
        for (int a = 0; a < j.A; ++a) mass = mass + expf(z[a] - top);
      }
      for (int a = 0; a < j.A; ++a) {
        const float y = j.kind == 1 ? expf(z[a] - top) / mass : z[a];
        const float d = y - t[a];
        loss = loss + it * (d * d);
        dot = dot + (2.0f * it * d * inv) * y;
      }
      for (int a = 0; a < ap; ++a) {
        float grad = 0.0f;
        if (a < j.A) {
          const float y = j.kind == 1 ? expf(z[a] - top) / mass : z[a];
          const float dy = 2.0f * it * (y - t[a]) * inv;
          grad = j.kind == 1 ? y * (dy - dot) : dy;
        }
        z[a] = grad;
      }
    }
    lds[L.rows + b * kAdamRowWords + 3] = loss;
  }
  __syncthreads();
  float v = 0.0f;   // (every wavefront adds the same rows in the same order: no broadcast)
  for (int r = threadIdx.x & 63; r < L.tile; r += 64) v = v + lds[L.rows + r * kAdamRowWords + 3];
  return wave_sum(v);
}

// The wavefront's index as a scalar the compiler takes for new at every call: which tiles a wavefront owns, and where
// they lie, is then worked out in scalar registers where it is used, not kept in vector registers per accumulator from
// the kernel's start to its end (that cost 12 registers per accumulator, and scratch).
OSG_D int own_wave() {
  int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  asm volatile("" : "+s"(wave));
  return wave;
}

// dW_l += dY^T X and db_l += dY^T 1 on the tile's rows, each gradient tile on its owner's accumulator.
OSG_D void own_grad(Grads& grads, const AdamLayout& L, int l, const float* dy, int sdy, const float* x, int sx) {
  const int wave = own_wave();
  const int nmt = L.out_pad[l] / kAdamTile, nnt = L.in_pad[l] / kAdamTile, first = L.tile_off[l], count = L.tile_off[l + 1] - first;
#pragma unroll
  for (int s = 0; s < kAdamMaxOwn; ++s) {
    const int t = wave + kAdamWaves * s - first;
    if (t >= 0 && t < count) {
      const int mt = t % nmt, nt = t / nmt;   // (column tile nnt: the bias)
      grads[s] = mma_cols(dy + mt * kAdamTile, sdy, nt < nnt ? x + nt * kAdamTile : nullptr, sx, L.tile, grads[s]);
    }
  }
}

// dst = dY W_l on the tile (masked: only where dst, the ReLU's output, is positive).
OSG_D void input_gradient(float* lds, const AdamLayout& L, int l, const float* dy, int sdy, float* dst, int sd, bool masked) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int nrt = L.tile / kAdamTile, nnt = L.in_pad[l] / kAdamTile;
  for (int t = wave; t < nrt * nnt; t += kAdamWaves) {
    const int rt = t % nrt, ct = t / nrt;
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (L.wt_resident) acc = mma_rows(dy + rt * kAdamTile * sdy, sdy, lds + L.wt[l] + ct * kAdamTile * L.wt_stride[l], L.wt_stride[l], L.out_pad[l], acc);
    else acc = mma_mixed(dy + rt * kAdamTile * sdy, sdy, lds + L.w[l] + ct * kAdamTile, L.w_stride[l], L.out_pad[l], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* h = dst + (rt * kAdamTile + 4 * g + r) * sd + ct * kAdamTile + i;
      *h = !masked || *h > 0.0f ? acc[r] : 0.0f;
    }
  }
  __syncthreads();
}

// LayerNorm backward on the tile, dN in the N buffer: thread c adds the column's d gamma (thread ln_pad + c: d beta)
// onto ln_grad, rows ascending; then dH = (gamma dN - mean(gamma dN) - x^ mean(gamma dN x^)) / std, through the
// ReLU's mask, in place of H.
OSG_D void layer_norm_backward(float* lds, const AdamLayout& L, float& ln_grad) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int last = L.n_linear - 1, s = L.n_stride;
  const float width = static_cast<float>(L.ln_width);
  if (static_cast<int>(threadIdx.x) < 2 * L.ln_pad) {
    const int c = threadIdx.x % L.ln_pad;
    const bool bias = static_cast<int>(threadIdx.x) >= L.ln_pad;
    for (int b = 0; b < L.tile; ++b) {
      const float dn = lds[L.n + b * s + c];
      const float xh = (lds[L.act[last] + b * s + c] - lds[L.rows + b * kAdamRowWords + 4]) * lds[L.rows + b * kAdamRowWords + 5];
      ln_grad = ln_grad + (bias ? dn : dn * xh);
    }
  }
  __syncthreads();
  for (int chunk = wave; chunk < L.tile / kAdamTile; chunk += kAdamWaves)
    for (int t = 0; t < 4; ++t) {
      const int row = chunk * kAdamTile + t + 4 * g;
      float* h = lds + L.act[last] + row * s;
      const float* dn = lds + L.n + row * s;
      const float mean = lds[L.rows + row * kAdamRowWords + 4], rstd = lds[L.rows + row * kAdamRowWords + 5];
      float s1 = 0.0f, s2 = 0.0f;
      for (int c = i; c < L.ln_pad; c += 16) {   // (gamma's padding holds zeros)
        const float a = lds[L.gamma + c] * dn[c];
        s1 = s1 + a;
        s2 = s2 + a * ((h[c] - mean) * rstd);
      }
      s1 = sum16(s1) / width;
      s2 = sum16(s2) / width;
      for (int c = i; c < L.ln_pad; c += 16) {
        const float a = lds[L.gamma + c] * dn[c], xh = (h[c] - mean) * rstd;
        h[c] = c < L.ln_width && h[c] > 0.0f ? (a - s1 - xh * s2) * rstd : 0.0f;
      }
    }
  __syncthreads();
}

struct AdamStep { float beta1, beta2, eps, step_size, bc2_sqrt; };

// One parameter's Adam step (torch's defaults): idx is its place in the flat buffers.
OSG_D void adam_one(float* lds, const AdamLayout& L, const AdamJob& j, const AdamStep& a, float* p, int idx, float grad) {
  float* pm = L.moments_resident ? lds + L.mom_m + idx : j.m + idx;
  float* pv = L.moments_resident ? lds + L.mom_v + idx : j.v + idx;
  const float m = a.beta1 * *pm + (1.0f - a.beta1) * grad;
  const float v = a.beta2 * *pv + (1.0f - a.beta2) * (grad * grad);
  *pm = m;
  *pv = v;
  *p = *p - a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}

// After the last tile: every owner steps its tiles' parameters from its accumulators and clears them.
OSG_D void adam_step(Grads& grads, float& ln_grad, float* lds, const AdamLayout& L, const AdamJob& j, const AdamStep& a) {
  const int wave = own_wave(), lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int s = 0; s < kAdamMaxOwn; ++s) {
    const int t = wave + kAdamWaves * s;
    if (t < L.tile_off[L.n_linear]) {
      int l = 0;
      while (t >= L.tile_off[l + 1]) ++l;
      const int nmt = L.out_pad[l] / kAdamTile, nnt = L.in_pad[l] / kAdamTile, in = L.in[l], out = L.out[l];
      const int mt = (t - L.tile_off[l]) % nmt, nt = (t - L.tile_off[l]) / nmt, c = nt * kAdamTile + i;
      const bool bias = nt == nnt;   // (every column of a bias tile holds the same sums: column 0 steps)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = mt * kAdamTile + 4 * g + r;
        if (o < out && (bias ? i == 0 : c < in))
          adam_one(lds, L, j, a, lds + (bias ? L.b[l] + o : L.w[l] + o * L.w_stride[l] + c),
                   L.param_off[l] + (bias ? out * in + o : o * in + c), grads[s][r]);
      }
    }
    grads[s] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const int c = threadIdx.x % L.ln_pad;
  if (static_cast<int>(threadIdx.x) < 2 * L.ln_pad && c < L.ln_width) {
    const bool bias = static_cast<int>(threadIdx.x) >= L.ln_pad;
    adam_one(lds, L, j, a, lds + (bias ? L.beta : L.gamma) + c, L.ln_off + (bias ? L.ln_width : 0) + c, ln_grad);
  }
  ln_grad = 0.0f;
  __syncthreads();
}

__global__ void __launch_bounds__(kAdamThreads) k_deep_cfr_train(const AdamJob* __restrict__ jobs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const AdamJob& j = jobs[blockIdx.x];
  const AdamLayout& L = j.lay;
  const int last = L.n_linear - 1;
  load_params(lds, L, j);
  __syncthreads();
  if (L.wt_resident)
    for (int l = 1; l <= last; ++l) refresh_transposed(lds, L, l);
  Grads grads;
#pragma unroll
  for (int s = 0; s < kAdamMaxOwn; ++s) grads[s] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  float ln_grad = 0.0f;
  double pow1 = j.pow1, pow2 = j.pow2;
  for (int64_t u = 0; u < j.U; ++u) {
    if (threadIdx.x == 0) lds[L.reduce] = 0.0f;
    __syncthreads();
    float loss = 0.0f;
    for (int k = 0; k < L.n_tiles; ++k) {
      fetch_tile(lds, L, j, u, k);
      for (int l = 0; l < last; ++l) forward_linear(lds, L, l);
      layer_norm_forward(lds, L, j.ln_eps);
      forward_linear(lds, L, last);
      loss = loss + top_gradient(lds, L, j);
      // (no parameter moves below: the accumulators take the gradients, the activations turn into theirs)
      own_grad(grads, L, last, lds + L.z, L.z_stride, lds + L.n, L.n_stride);
      __syncthreads();
      input_gradient(lds, L, last, lds + L.z, L.z_stride, lds + L.n, L.n_stride, false);
      layer_norm_backward(lds, L, ln_grad);
      for (int l = last - 1; l >= 0; --l) {
        own_grad(grads, L, l, lds + L.act[l + 1], L.act_stride[l + 1], lds + L.act[l], L.act_stride[l]);
        __syncthreads();
        if (l > 0) input_gradient(lds, L, l, lds + L.act[l + 1], L.act_stride[l + 1], lds + L.act[l], L.act_stride[l], true);
      }
    }
    pow1 *= j.beta1;
    pow2 *= j.beta2;
    const AdamStep a{static_cast<float>(j.beta1), static_cast<float>(j.beta2), j.eps, static_cast<float>(j.lr / (1.0 - pow1)),
                     static_cast<float>(sqrt(1.0 - pow2))};
    adam_step(grads, ln_grad, lds, L, j, a);
    if (L.wt_resident) {
      for (int l = 1; l <= last; ++l) refresh_transposed(lds, L, l);
      __syncthreads();
    }
    if (threadIdx.x == 0) j.loss_out[u] = lds[L.reduce] != 0.0f ? __builtin_nanf("") : loss / static_cast<float>(L.batch * j.A);
  }
  store_params(lds, L, j);
}

}  // namespace

extern "C" int osg_deep_cfr_learn_plan(osg_ctx* ctx, int32_t n_linear, const int32_t* widths, int32_t batch, int32_t* plan) {
  const std::string who = "osg_deep_cfr_learn_plan: ";
  if (!ctx || !widths || !plan) return set_error(OSG_ERR_INVALID, who + "bad argument");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  AdamShape shape;
  shape.n_linear = n_linear;
  if (n_linear >= 1 && n_linear <= kAdamMaxLinear)
    for (int l = 0; l <= n_linear; ++l) shape.widths[l] = widths[l];
  shape.batch = batch;
  const AdamLayout lay = plan_adam(shape, limit);
  if (!lay.ok) return set_error(OSG_ERR_UNSUPPORTED, who + lay.why);
  plan[0] = lay.tile; plan[1] = lay.n_tiles; plan[2] = lay.wt_resident; plan[3] = lay.moments_resident;
  plan[4] = static_cast<int32_t>(lay.lds_bytes); plan[5] = lay.param_count;
  return OSG_OK;
}

extern "C" int osg_deep_cfr_learn(osg_ctx* ctx, const osg_deep_cfr_learn_job* jobs, int64_t n_jobs) {
  const std::string who = "osg_deep_cfr_learn: ";
  if (!ctx || !jobs || n_jobs < 1 || n_jobs > 65535) return set_error(OSG_ERR_INVALID, who + "bad argument");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  std::vector<AdamJob> dev(static_cast<size_t>(n_jobs));
  size_t lds = 0;
  for (int64_t k = 0; k < n_jobs; ++k) {
    const osg_deep_cfr_learn_job& in = jobs[k];
    AdamJob& j = dev[static_cast<size_t>(k)];
    if ((in.kind != 0 && in.kind != 1) || in.updates < 0 || in.infostates < 1 || in.step0 < 0 || !in.d_params || !in.d_adam_m || !in.d_adam_v ||
        !in.d_tensors || !in.reservoir || !in.d_slots || !in.d_loss || !(in.beta1 >= 0.0 && in.beta1 < 1.0) ||
        !(in.beta2 >= 0.0 && in.beta2 < 1.0) || !(in.eps >= 0.0) || !(in.ln_eps >= 0.0))
      return set_error(OSG_ERR_INVALID, who + "bad argument in job " + std::to_string(k));
    if (in.infostates >= (int64_t{1} << 31)) return set_error(OSG_ERR_UNSUPPORTED, who + "2^31 infostates or more");
    AdamShape shape;
    shape.n_linear = in.n_linear;
    if (in.n_linear >= 1 && in.n_linear <= kAdamMaxLinear)
      for (int l = 0; l <= in.n_linear; ++l) shape.widths[l] = in.widths[l];
    shape.batch = in.batch;
    j.lay = plan_adam(shape, limit);
    if (!j.lay.ok) return set_error(OSG_ERR_UNSUPPORTED, who + j.lay.why + " (job " + std::to_string(k) + ")");
    j.lay.why = nullptr;
    j.kind = in.kind; j.S = in.widths[0]; j.A = in.widths[in.n_linear];
    j.U = in.updates; j.I = in.infostates;
    j.params = in.d_params; j.m = in.d_adam_m; j.v = in.d_adam_v; j.tensors = in.d_tensors;
    j.slots = in.d_slots; j.loss_out = in.d_loss;
    const ReservoirView v = reservoir_view(in.reservoir);
    if (v.ctx != ctx || v.A != j.A) return set_error(OSG_ERR_INVALID, who + "a reservoir of another row width or context");
    if (v.size >= (int64_t{1} << 31)) return set_error(OSG_ERR_UNSUPPORTED, who + "2^31 buffer rows or more");
    if (in.batch > v.size) return set_error(OSG_ERR_INVALID, who + "a batch larger than the buffer's rows");
    j.rows = v.size; j.info = v.info; j.iter = v.iter; j.vals = v.vals;
    j.lr = in.learning_rate; j.beta1 = in.beta1; j.beta2 = in.beta2;
    j.pow1 = std::pow(in.beta1, static_cast<double>(in.step0)); j.pow2 = std::pow(in.beta2, static_cast<double>(in.step0));
    j.eps = static_cast<float>(in.eps); j.ln_eps = static_cast<float>(in.ln_eps);
    lds = std::max(lds, j.lay.lds_bytes);
  }
  const void* kernel = reinterpret_cast<const void*>(&k_deep_cfr_train);
  if (lds > (32u << 10) && raise_lds_cap(kernel, static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(OSG_ERR_UNSUPPORTED, who + "the device does not grant " + std::to_string(lds) + " bytes of LDS to a workgroup");
  }
  hipStream_t st = ctx->stream;
  void* ptr = nullptr;
  if (int rc = osg_ctx_scratch(ctx, sizeof(AdamJob) * dev.size(), &ptr)) return rc;
  OSG_HIP(hipMemcpyAsync(ptr, dev.data(), sizeof(AdamJob) * dev.size(), hipMemcpyHostToDevice, st));   // (small: staged before it returns)
  k_deep_cfr_train<<<dim3(static_cast<unsigned>(n_jobs)), dim3(kAdamThreads), lds, st>>>(static_cast<const AdamJob*>(ptr));
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}
