// The WIDE form of Deep CFR's fused learner: the networks one workgroup cannot hold ((256, 256), the solver's default
// policy network, up to hidden widths of 512).  Same job, same arithmetic and same formulas as k_deep_cfr_train
// (osg_deep_cfr_learn.hip); what differs is who does the work.
//
// A job is a GROUP of G workgroups (osg_adam_wide_plan.h: R, G, the LDS layout, the scratch), data-parallel over the
// batch.  Per update, workgroup g of the group
//   1. gathers its R rows and their tensors into LDS, and keeps every activation of those rows there;
//   2. forward, LayerNorm, loss and top gradient, backward — as the narrow form, but the WEIGHTS stay in global memory
//      (L2) and come through LDS in double-buffered panels of 16 output rows: the threads request panel s + 1 into
//      registers, the wavefronts run v_mfma_f32_16x16x4_f32 on panel s, then the registers go to the other buffer.
//      Forward contracts over a panel's columns; dH = dY W contracts over its 16 rows (the same panel, no transposed
//      copy), k-chunk-major so that at most 8 output tiles per wavefront are open at a time;
//   3. finishes every gradient tile dW = dY^T X in one pass over its rows (16-row chunks ascending) and writes it
//      straight to partial[g][param] in the job's scratch — nothing is kept in accumulators across tiles; likewise
//      the LayerNorm gradients (one thread per column, rows ascending), its loss sum and its out-of-range flag;
//   -- barrier 1 (the job's group only) --
//   4. owns a contiguous slice of the flat parameters: adds the G partials of each in ascending workgroup order and
//      takes torch's Adam step on it (m and v in place in global memory); workgroup 0 adds the loss partials, again
//      ascending, into d_loss[u];
//   -- barrier 2 --
// No floating-point atomics and one order per sum: a job's bits depend on its own inputs (and on R and G, which the
// planner derives from the shape and the LDS limit alone), not on the other jobs, the run, or the split into calls
// (beta^t is pow() of the step count, not a running product).
//
// The barrier: every thread's stores are made visible at agent scope (__threadfence) and drained, the workgroup
// meets, ONE lane adds to the job's counter and polls it, bounded by the 100 MHz wall clock as k_cfr_split's.  A
// workgroup that gives up raises the job's error word (the others leave when they see it), workgroup 0 fills the job's
// remaining d_loss with NaN, and a pinned host word makes the next osg_deep_cfr_learn_wide call return OSG_ERR_HIP.
// The launch goes through launch_grid_barrier_kernel and is refused unless every workgroup of every job can be
// resident (one per CU).
#include "osg_adam_wide_plan.h"
#include "osg_cfr_internal.h"
#include "osg_mfma_tile.h"

using namespace osg_adam_wide;
using namespace osg_mfma;   // f4, mma_rows, mma_cols, mma_mixed, sum16, wave_sum

namespace {

constexpr int kPanelRegs = kWideTile * kWidePanelCols / kWideThreads;   // 8 floats of a panel per thread
constexpr int kOpenTiles = kWideMaxRows / kWideTile * (kWidePanelCols / kWideTile) / kWideWaves;   // 8: dH tiles of a k-chunk per wavefront
constexpr unsigned long long kBarrierTicks = 400000000ull;   // 4 s of the 100 MHz wall clock

struct WideJob {   // one job as the kernel sees it (device pointers)
  WideLayout lay;
  int kind, S, A, first_block;   // workgroups first_block .. first_block + G - 1 of the launch
  int64_t U, I, rows, step0;
  float *params, *m, *v;
  const float* tensors;
  const int32_t* info;        // the reservoir's columns
  const int32_t* iter;
  const float* vals;          // [rows, A]
  const int64_t* slots;
  float* loss_out;
  unsigned int* bar;          // [0] arrivals, [1] a workgroup gave up (zeroed by the launch's memset)
  float* partial;             // [G][partial_stride]: flat gradient, loss sum, out-of-range flag
  double lr, beta1, beta2;
  float eps, ln_eps;
};

// Rows [row0, row0 + R) of update u: their words and X [R, S16] (a row past the batch: zeros, infostate -1; one naming
// something out of range: the same, and the update's flag); and the LayerNorm weights of this update.
OSG_D void fetch_rows(float* lds, const WideLayout& L, const WideJob& j, int64_t u, int row0) {
  int* rows = reinterpret_cast<int*>(lds + L.row_words);
  const int b = threadIdx.x;
  if (b < L.rows) {
    const int at = row0 + b;
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
    rows[b * kWideRowWords] = info;
    rows[b * kWideRowWords + 1] = slot;
    lds[L.row_words + b * kWideRowWords + 2] = it;
    lds[L.row_words + b * kWideRowWords + 3] = 0.0f;
    if (bad) lds[L.flags] = 1.0f;   // (every writer writes the same word)
  }
  for (int c = threadIdx.x; c < L.ln_pad; c += kWideThreads) {
    lds[L.gamma + c] = c < L.ln_width ? j.params[L.ln_off + c] : 0.0f;
    lds[L.beta + c] = c < L.ln_width ? j.params[L.ln_off + L.ln_width + c] : 0.0f;
  }
  __syncthreads();
  const int sp = L.in_pad[0], sx = L.act_stride[0];
  for (int x = threadIdx.x; x < L.rows * sp; x += kWideThreads) {
    const int r = x / sp, c = x % sp;
    const int i = rows[r * kWideRowWords];
    lds[L.act[0] + r * sx + c] = i >= 0 && c < j.S ? j.tensors[static_cast<int64_t>(i) * j.S + c] : 0.0f;
  }
  __syncthreads();
}

// Panel (ct, kc) of layer l — output rows 16 ct ..., input columns panel_cols kc ... — from global memory into the
// thread's registers (32 threads per row, consecutive words; zeros past the layer's real rows and columns), and from
// there into a panel buffer.
OSG_D void panel_fetch(float (&pre)[kPanelRegs], const WideLayout& L, const WideJob& j, int l, int ct, int kc) {
  const int r = threadIdx.x >> 5, x0 = threadIdx.x & 31;
  const int o = ct * kWideTile + r, in = L.in[l], c0 = kc * L.panel_cols;
  const float* w = j.params + L.param_off[l] + static_cast<int64_t>(o) * in + c0;
  const int left = o < L.out[l] ? (in - c0 < L.panel_cols ? in - c0 : L.panel_cols) : 0;
#pragma unroll
  for (int q = 0; q < kPanelRegs; ++q) pre[q] = x0 + 32 * q < left ? w[x0 + 32 * q] : 0.0f;
}
OSG_D void panel_store(const float (&pre)[kPanelRegs], float* panel, const WideLayout& L) {
  const int r = threadIdx.x >> 5, x0 = threadIdx.x & 31;
#pragma unroll
  for (int q = 0; q < kPanelRegs; ++q)
    if (x0 + 32 * q < L.panel_cols) panel[r * L.panel_stride + x0 + 32 * q] = pre[q];
}

// Layer l on the workgroup's rows: act[l] -> act[l + 1] with ReLU, or for the last layer N -> Z.  Stages (ct, kc),
// ct-major: wavefront w < R / 16 holds the accumulator of rows 16 w ... for output tile ct over its k-chunks.
OSG_D void forward_linear(float* lds, const WideLayout& L, const WideJob& j, int l) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const bool top = l + 1 == L.n_linear;
  const float* x = lds + (top ? L.n : L.act[l]);
  float* y = lds + (top ? L.z : L.act[l + 1]);
  const int sx = L.act_stride[l], sy = top ? L.z_stride : L.act_stride[l + 1], ps = L.panel_stride;
  const int nrt = L.rows / kWideTile, nkc = (L.in_pad[l] + L.panel_cols - 1) / L.panel_cols, stages = L.out_pad[l] / kWideTile * nkc;
  const float* bias = j.params + L.param_off[l] + L.out[l] * L.in[l];
  float pre[kPanelRegs];
  panel_fetch(pre, L, j, l, 0, 0);
  panel_store(pre, lds + L.panel[0], L);
  __syncthreads();
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int s = 0; s < stages; ++s) {
    const int ct = s / nkc, kc = s % nkc;
    if (s + 1 < stages) panel_fetch(pre, L, j, l, (s + 1) / nkc, (s + 1) % nkc);
    if (wave < nrt) {
      const int k0 = kc * L.panel_cols, K = L.in_pad[l] - k0 < L.panel_cols ? L.in_pad[l] - k0 : L.panel_cols;
      acc = mma_rows(x + wave * kWideTile * sx + k0, sx, lds + L.panel[s & 1], ps, K, acc);
      if (kc == nkc - 1) {
        const int o = ct * kWideTile + i;
        const float b = o < L.out[l] ? bias[o] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[r] + b;
          if (!top) v = v > 0.0f ? v : 0.0f;
          y[(wave * kWideTile + 4 * g + r) * sy + o] = v;
        }
        acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
    if (s + 1 < stages) panel_store(pre, lds + L.panel[(s + 1) & 1], L);
    __syncthreads();
  }
}

// dst = dY W_l on the workgroup's rows (masked: only where dst, the ReLU's output, is positive).  Stages (kc, ct),
// kc-major: the [R, cols of the k-chunk] output tiles are open on the wavefronts (tile t on wavefront t mod 8) while
// the panels of every ct add onto them, ct ascending.
OSG_D void input_gradient(float* lds, const WideLayout& L, const WideJob& j, int l, const float* dy, int sdy, float* dst, int sd, bool masked) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int nrt = L.rows / kWideTile, nct = L.out_pad[l] / kWideTile, ps = L.panel_stride;
  const int nkc = (L.in_pad[l] + L.panel_cols - 1) / L.panel_cols, stages = nkc * nct;
  float pre[kPanelRegs];
  panel_fetch(pre, L, j, l, 0, 0);
  panel_store(pre, lds + L.panel[0], L);
  __syncthreads();
  f4 acc[kOpenTiles];
#pragma unroll
  for (int q = 0; q < kOpenTiles; ++q) acc[q] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int s = 0; s < stages; ++s) {
    const int kc = s / nct, ct = s % nct;
    if (s + 1 < stages) panel_fetch(pre, L, j, l, (s + 1) % nct, (s + 1) / nct);
    const int k0 = kc * L.panel_cols, cols = L.in_pad[l] - k0 < L.panel_cols ? L.in_pad[l] - k0 : L.panel_cols;
    const int tiles = nrt * (cols / kWideTile);
    const float* panel = lds + L.panel[s & 1];
#pragma unroll
    for (int q = 0; q < kOpenTiles; ++q) {
      const int t = wave + kWideWaves * q;
      if (t < tiles) {
        const int rt = t % nrt, nt = t / nrt;
        acc[q] = mma_mixed(dy + rt * kWideTile * sdy + ct * kWideTile, sdy, panel + nt * kWideTile, ps, kWideTile, acc[q]);
        if (ct == nct - 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* h = dst + (rt * kWideTile + 4 * g + r) * sd + k0 + nt * kWideTile + i;
            *h = !masked || *h > 0.0f ? acc[q][r] : 0.0f;
          }
          acc[q] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        }
      }
    }
    if (s + 1 < stages) panel_store(pre, lds + L.panel[(s + 1) & 1], L);
    __syncthreads();
  }
}

// nn.LayerNorm (biased variance) on the last hidden activation H: N = gamma x^ + beta; a row's mean and 1 / std go to its
// words.  16 lanes per row, the four rows of a step four apart.
OSG_D void layer_norm_forward(float* lds, const WideLayout& L, float eps) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int last = L.n_linear - 1, s = L.n_stride;
  const float width = static_cast<float>(L.ln_width);
  for (int chunk = wave; chunk < L.rows / kWideTile; chunk += kWideWaves)
    for (int t = 0; t < 4; ++t) {
      const int row = chunk * kWideTile + t + 4 * g;
      const float* h = lds + L.act[last] + row * s;
      float sum = 0.0f, sq = 0.0f;
      for (int c = i; c < L.ln_pad; c += 16) sum = sum + h[c];      // (the padding holds zeros)
      const float mean = sum16(sum) / width;
      for (int c = i; c < L.ln_width; c += 16) sq = sq + (h[c] - mean) * (h[c] - mean);
      const float rstd = 1.0f / sqrtf(sum16(sq) / width + eps);
      for (int c = i; c < L.ln_pad; c += 16) lds[L.n + row * s + c] = lds[L.gamma + c] * ((h[c] - mean) * rstd) + lds[L.beta + c];
      if (i == 0) {
        lds[L.row_words + row * kWideRowWords + 4] = mean;
        lds[L.row_words + row * kWideRowWords + 5] = rstd;
      }
    }
  __syncthreads();
}

// The loss of every row and dLoss/dZ in place of Z (zeros in the padding and in rows that do not count); the
// workgroup's sum of it_b (y - t)^2 and its out-of-range flag go to its partials.
OSG_D void top_gradient(float* lds, const WideLayout& L, const WideJob& j, float* mine) {
  const int* rows = reinterpret_cast<const int*>(lds + L.row_words);
  const int b = threadIdx.x, ap = L.out_pad[L.n_linear - 1];
  const float inv = 1.0f / static_cast<float>(L.batch * j.A);
  if (b < L.rows) {
    float* z = lds + L.z + b * L.z_stride;
    float loss = 0.0f;
    if (rows[b * kWideRowWords] < 0) {
      for (int a = 0; a < ap; ++a) z[a] = 0.0f;
    } else {
      const float it = lds[L.row_words + b * kWideRowWords + 2];
      const float* t = j.vals + static_cast<int64_t>(rows[b * kWideRowWords + 1]) * j.A;
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
    lds[L.row_words + b * kWideRowWords + 3] = loss;
  }
  __syncthreads();
  if (threadIdx.x < 64) {   // a lane-strided sum and one 64-lane tree
    float v = 0.0f;
    for (int r = threadIdx.x; r < L.rows; r += 64) v = v + lds[L.row_words + r * kWideRowWords + 3];
    v = wave_sum(v);
    if (threadIdx.x == 0) {
      mine[L.param_count] = v;
      mine[L.param_count + 1] = lds[L.flags];
    }
  }
}

// dW_l = dY^T X and db_l = dY^T 1 over the workgroup's rows, tile by tile (tile t on wavefront t mod 8), each finished
// in one pass and written to the workgroup's partials.
OSG_D void weight_gradient(const WideLayout& L, int l, const float* dy, int sdy, const float* x, int sx, float* mine) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int nmt = L.out_pad[l] / kWideTile, nnt = L.in_pad[l] / kWideTile, in = L.in[l], out = L.out[l];
  float* w = mine + L.param_off[l];
  for (int t = wave; t < nmt * (nnt + 1); t += kWideWaves) {
    const int mt = t % nmt, nt = t / nmt, c = nt * kWideTile + i;   // (column tile nnt: the bias)
    const f4 acc = mma_cols(dy + mt * kWideTile, sdy, nt < nnt ? x + nt * kWideTile : nullptr, sx, L.rows, f4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = mt * kWideTile + 4 * g + r;
      if (o < out) {
        if (nt == nnt) { if (i == 0) w[out * in + o] = acc[r]; }   // (every column of a bias tile holds the same sums)
        else if (c < in) w[o * in + c] = acc[r];
      }
    }
  }
}

// LayerNorm backward, dN in the N buffer: the columns' d gamma and d beta over the workgroup's rows, ascending, to its
// partials; then dH = (gamma dN - mean(gamma dN) - x^ mean(gamma dN x^)) / std, through the ReLU's mask, in place of H.
OSG_D void layer_norm_backward(float* lds, const WideLayout& L, float* mine) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int last = L.n_linear - 1, s = L.n_stride;
  const float width = static_cast<float>(L.ln_width);
  for (int x = threadIdx.x; x < 2 * L.ln_pad; x += kWideThreads) {
    const int c = x % L.ln_pad;
    const bool bias = x >= L.ln_pad;
    float sum = 0.0f;
    for (int b = 0; b < L.rows; ++b) {
      const float dn = lds[L.n + b * s + c];
      const float xh = (lds[L.act[last] + b * s + c] - lds[L.row_words + b * kWideRowWords + 4]) * lds[L.row_words + b * kWideRowWords + 5];
      sum = sum + (bias ? dn : dn * xh);
    }
    if (c < L.ln_width) mine[L.ln_off + (bias ? L.ln_width : 0) + c] = sum;
  }
  __syncthreads();
  for (int chunk = wave; chunk < L.rows / kWideTile; chunk += kWideWaves)
    for (int t = 0; t < 4; ++t) {
      const int row = chunk * kWideTile + t + 4 * g;
      float* h = lds + L.act[last] + row * s;
      const float* dn = lds + L.n + row * s;
      const float mean = lds[L.row_words + row * kWideRowWords + 4], rstd = lds[L.row_words + row * kWideRowWords + 5];
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

// The group's barrier.  False: a workgroup of the job did not arrive within the bound (or another gave up): leave.
OSG_D bool group_barrier(const WideJob& j, unsigned int& epoch, int* s_ok, unsigned int* host_err) {
  ++epoch;
  __threadfence();   // this thread's stores are visible at agent scope, and drained, before the workgroup arrives
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(&j.bar[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned int want = epoch * static_cast<unsigned int>(j.lay.group);
    int ok = 1;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(&j.bar[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
      if (__hip_atomic_load(&j.bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u || wall_clock64() - t0 > kBarrierTicks) { ok = 0; break; }
      __builtin_amdgcn_s_sleep(1);
    }
    if (!ok) {
      __hip_atomic_store(&j.bar[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    *s_ok = ok;
  }
  __syncthreads();
  __threadfence();   // nothing below is served from a line cached before the others' stores
  return *s_ok != 0;
}

// The workgroup's slice of the flat parameters: the G partials of each in ascending workgroup order, then torch's Adam.
OSG_D void adam_slice(const WideLayout& L, const WideJob& j, int g, int64_t u) {
  const double t = static_cast<double>(j.step0 + u + 1);
  const float beta1 = static_cast<float>(j.beta1), beta2 = static_cast<float>(j.beta2);
  const float step_size = static_cast<float>(j.lr / (1.0 - pow(j.beta1, t))), bc2_sqrt = static_cast<float>(sqrt(1.0 - pow(j.beta2, t)));
  const int lo = g * L.slice, hi = lo + L.slice < L.param_count ? lo + L.slice : L.param_count;
  for (int idx = lo + threadIdx.x; idx < hi; idx += kWideThreads) {
    float grad = j.partial[idx];
    for (int w = 1; w < L.group; ++w) grad = grad + j.partial[static_cast<size_t>(w) * L.partial_stride + idx];
    const float m = beta1 * j.m[idx] + (1.0f - beta1) * grad;
    const float v = beta2 * j.v[idx] + (1.0f - beta2) * (grad * grad);
    j.m[idx] = m;
    j.v[idx] = v;
    j.params[idx] = j.params[idx] - step_size * (m / (sqrtf(v) / bc2_sqrt + j.eps));
  }
  if (g == 0 && threadIdx.x == 0) {
    float loss = 0.0f;
    bool bad = false;
    for (int w = 0; w < L.group; ++w) {
      loss = loss + j.partial[static_cast<size_t>(w) * L.partial_stride + L.param_count];
      bad = bad || j.partial[static_cast<size_t>(w) * L.partial_stride + L.param_count + 1] != 0.0f;
    }
    j.loss_out[u] = bad ? __builtin_nanf("") : loss / static_cast<float>(L.batch * j.A);
  }
}

__global__ void __launch_bounds__(kWideThreads) k_deep_cfr_train_wide(const WideJob* __restrict__ jobs, const int32_t* __restrict__ block_job,
                                                                      unsigned int* host_err) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const WideJob& j = jobs[block_job[blockIdx.x]];
  const WideLayout& L = j.lay;
  int* s_ok = reinterpret_cast<int*>(lds + L.flags + 1);   // (the planner's limit is the whole of a workgroup's LDS: no static word)
  const int last = L.n_linear - 1, g = static_cast<int>(blockIdx.x) - j.first_block;
  float* mine = j.partial + static_cast<size_t>(g) * L.partial_stride;
  unsigned int epoch = 0;
  for (int64_t u = 0; u < j.U; ++u) {
    if (threadIdx.x == 0) lds[L.flags] = 0.0f;
    __syncthreads();
    fetch_rows(lds, L, j, u, g * L.rows);
    for (int l = 0; l < last; ++l) forward_linear(lds, L, j, l);
    layer_norm_forward(lds, L, j.ln_eps);
    forward_linear(lds, L, j, last);
    top_gradient(lds, L, j, mine);
    // (no parameter moves before the barrier: the activations turn into their gradients, the tiles go to the partials)
    weight_gradient(L, last, lds + L.z, L.z_stride, lds + L.n, L.n_stride, mine);
    __syncthreads();
    input_gradient(lds, L, j, last, lds + L.z, L.z_stride, lds + L.n, L.n_stride, false);
    layer_norm_backward(lds, L, mine);
    for (int l = last - 1; l >= 0; --l) {
      weight_gradient(L, l, lds + L.act[l + 1], L.act_stride[l + 1], lds + L.act[l], L.act_stride[l], mine);
      __syncthreads();
      if (l > 0) input_gradient(lds, L, j, l, lds + L.act[l + 1], L.act_stride[l + 1], lds + L.act[l], L.act_stride[l], true);
    }
    bool ok = group_barrier(j, epoch, s_ok, host_err);
    if (ok) {
      adam_slice(L, j, g, u);
      ok = group_barrier(j, epoch, s_ok, host_err);
    }
    if (!ok) {   // a hung device: every workgroup of the job leaves, the rest of its losses say so
      if (g == 0)
        for (int64_t k = u + threadIdx.x; k < j.U; k += kWideThreads) j.loss_out[k] = __builtin_nanf("");
      return;
    }
  }
}

WideShape shape_of(int32_t n_linear, const int32_t* widths, int32_t batch) {
  WideShape shape;
  shape.n_linear = n_linear;
  if (n_linear >= 1 && n_linear <= kWideMaxLinear)
    for (int l = 0; l <= n_linear; ++l) shape.widths[l] = widths[l];
  shape.batch = batch;
  return shape;
}

}  // namespace

extern "C" int osg_deep_cfr_learn_wide_plan(osg_ctx* ctx, int32_t n_linear, const int32_t* widths, int32_t batch, int64_t* plan) {
  const std::string who = "osg_deep_cfr_learn_wide_plan: ";
  if (!ctx || !widths || !plan) return set_error(OSG_ERR_INVALID, who + "bad argument");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  const WideLayout lay = plan_adam_wide(shape_of(n_linear, widths, batch), limit);
  if (!lay.ok) return set_error(OSG_ERR_UNSUPPORTED, who + lay.why);
  plan[0] = lay.rows; plan[1] = lay.group; plan[2] = static_cast<int64_t>(lay.lds_bytes);
  plan[3] = static_cast<int64_t>(lay.scratch_bytes); plan[4] = lay.param_count;
  return OSG_OK;
}

extern "C" int osg_deep_cfr_learn_wide(osg_ctx* ctx, const osg_deep_cfr_learn_job* jobs, int64_t n_jobs) {
  const std::string who = "osg_deep_cfr_learn_wide: ";
  if (!ctx || !jobs || n_jobs < 1 || n_jobs > 65535) return set_error(OSG_ERR_INVALID, who + "bad argument");
  if (!ctx->h_learn_err) {
    OSG_HIP(ctx->h_learn_err.alloc(1));
    *ctx->h_learn_err.get() = 0u;
  }
  if (__atomic_exchange_n(ctx->h_learn_err.get(), 0u, __ATOMIC_RELAXED) != 0u)
    return set_error(OSG_ERR_HIP, who + "a group barrier timed out in an earlier launch (a hung or oversubscribed device); the losses of the "
                                        "jobs it left are NaN and their parameters are not usable");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  if (ctx->num_cus == 0) {
    hipDeviceProp_t prop;
    OSG_HIP(hipGetDeviceProperties(&prop, ctx->device));
    ctx->num_cus = prop.multiProcessorCount;
  }
  std::vector<WideJob> dev(static_cast<size_t>(n_jobs));
  std::vector<int32_t> block_job;
  std::vector<size_t> partial_at(static_cast<size_t>(n_jobs));   // where a job's partials start, in floats
  size_t lds = 0, partial_floats = 0;
  for (int64_t k = 0; k < n_jobs; ++k) {
    const osg_deep_cfr_learn_job& in = jobs[k];
    WideJob& j = dev[static_cast<size_t>(k)];
    if ((in.kind != 0 && in.kind != 1) || in.updates < 0 || in.infostates < 1 || in.step0 < 0 || !in.d_params || !in.d_adam_m || !in.d_adam_v ||
        !in.d_tensors || !in.reservoir || !in.d_slots || !in.d_loss || !(in.beta1 >= 0.0 && in.beta1 < 1.0) ||
        !(in.beta2 >= 0.0 && in.beta2 < 1.0) || !(in.eps >= 0.0) || !(in.ln_eps >= 0.0))
      return set_error(OSG_ERR_INVALID, who + "bad argument in job " + std::to_string(k));
    if (in.infostates >= (int64_t{1} << 31)) return set_error(OSG_ERR_UNSUPPORTED, who + "2^31 infostates or more");
    j.lay = plan_adam_wide(shape_of(in.n_linear, in.widths, in.batch), limit);
    if (!j.lay.ok) return set_error(OSG_ERR_UNSUPPORTED, who + j.lay.why + " (job " + std::to_string(k) + ")");
    j.lay.why = nullptr;
    j.kind = in.kind; j.S = in.widths[0]; j.A = in.widths[in.n_linear];
    j.U = in.updates; j.I = in.infostates; j.step0 = in.step0;
    j.params = in.d_params; j.m = in.d_adam_m; j.v = in.d_adam_v; j.tensors = in.d_tensors;
    j.slots = in.d_slots; j.loss_out = in.d_loss;
    const ReservoirView v = reservoir_view(in.reservoir);
    if (v.ctx != ctx || v.A != j.A) return set_error(OSG_ERR_INVALID, who + "a reservoir of another row width or context");
    if (v.size >= (int64_t{1} << 31)) return set_error(OSG_ERR_UNSUPPORTED, who + "2^31 buffer rows or more");
    if (in.batch > v.size) return set_error(OSG_ERR_INVALID, who + "a batch larger than the buffer's rows");
    j.rows = v.size; j.info = v.info; j.iter = v.iter; j.vals = v.vals;
    j.lr = in.learning_rate; j.beta1 = in.beta1; j.beta2 = in.beta2;
    j.eps = static_cast<float>(in.eps); j.ln_eps = static_cast<float>(in.ln_eps);
    j.first_block = static_cast<int>(block_job.size());
    partial_at[static_cast<size_t>(k)] = partial_floats;
    partial_floats += static_cast<size_t>(j.lay.group) * j.lay.partial_stride;
    block_job.insert(block_job.end(), static_cast<size_t>(j.lay.group), static_cast<int32_t>(k));
    lds = std::max(lds, j.lay.lds_bytes);
    if (static_cast<int64_t>(block_job.size()) > ctx->num_cus)
      return set_error(OSG_ERR_UNSUPPORTED, who + "the jobs' groups need more workgroups than the device's " + std::to_string(ctx->num_cus) +
                                                " compute units hold at once (one per unit): make fewer jobs per call");
  }
  const void* kernel = reinterpret_cast<const void*>(&k_deep_cfr_train_wide);
  if (lds > (32u << 10) && raise_lds_cap(kernel, static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(OSG_ERR_UNSUPPORTED, who + "the device does not grant " + std::to_string(lds) + " bytes of LDS to a workgroup");
  }
  // scratch: [counters of every job | partials of every job | jobs | block -> job]
  const size_t o_partial = align_up(sizeof(unsigned int) * kWideBarrierWords * dev.size());
  const size_t o_jobs = o_partial + align_up(sizeof(float) * partial_floats);
  const size_t o_map = o_jobs + align_up(sizeof(WideJob) * dev.size());
  hipStream_t st = ctx->stream;
  void* ptr = nullptr;
  if (int rc = osg_ctx_scratch(ctx, o_map + sizeof(int32_t) * block_job.size(), &ptr)) return rc;
  unsigned char* base = static_cast<unsigned char*>(ptr);
  for (size_t k = 0; k < dev.size(); ++k) {
    dev[k].bar = reinterpret_cast<unsigned int*>(base) + kWideBarrierWords * k;
    dev[k].partial = reinterpret_cast<float*>(base + o_partial) + partial_at[k];
  }
  OSG_HIP(hipMemsetAsync(base, 0, o_partial, st));
  OSG_HIP(hipMemcpyAsync(base + o_jobs, dev.data(), sizeof(WideJob) * dev.size(), hipMemcpyHostToDevice, st));   // (small: staged before it returns)
  OSG_HIP(hipMemcpyAsync(base + o_map, block_job.data(), sizeof(int32_t) * block_job.size(), hipMemcpyHostToDevice, st));
  const WideJob* d_jobs = reinterpret_cast<const WideJob*>(base + o_jobs);
  const int32_t* d_map = reinterpret_cast<const int32_t*>(base + o_map);
  unsigned int* host_err = ctx->h_learn_err.get();
  void* args[] = {&d_jobs, &d_map, &host_err};
  OSG_HIP(launch_grid_barrier_kernel(kernel, dim3(static_cast<unsigned>(block_job.size())), dim3(kWideThreads), args, lds, st));
  return OSG_OK;
}
