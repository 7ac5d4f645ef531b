// The fused learner of NFSP and DQN (open_spiel/python/pytorch/dqn.py:501-569 DQN.learn, nfsp.py:364-409 NFSP._learn,
// both with SGD): every update a chunk of self-play owes, in one launch.
//
// A job is one network — Linear + ReLU per hidden layer, then Linear — and its U sequential updates.  The updates of
// one network are a chain: update u + 1 reads the weights update u wrote.  So ONE workgroup (8 wavefronts) runs one job
// from its first update to its last with the weights, the biases, the batch's inputs and every activation in LDS
// (osg_mlp_plan.h has the layout, the strides and why no operand read collides on banks); global memory is read for the
// parameters once, for the batch rows (gathered here from the ring / reservoir and the infostate tensors) once per
// update, and written for the parameters once and for one loss per update.  All jobs of a call run side by side.
//
// The contractions are v_mfma_f32_16x16x4_f32: fp32 in, fp32 accumulate.  With lane l = 16 g + i of a wavefront the
// instruction takes A[i][g] and B[g][i] and leaves D[4 g + r][i] in register r of the accumulator.
//   forward  Y = X W^T + b      tiles of [B, out] over the wavefronts, batch rows first; contraction over `in`
//   dH = dY W                   the same split; contraction over `out`, the B operand from the transposed copy Wt
//   dW = dY^T X, db = dY^T 1    the OUTPUT tiles [out, in] over the wavefronts; contraction over the batch
// Every sum has one order — the instruction's, the k loop's, and fixed trees over lanes and wavefronts for the loss and
// the gradient norm — and there is no atomic, so a job's bits depend on nothing but its own inputs.
//
// Two orderings.  (1) dH of layer l reads the OLD W_l: the layer's SGD step rewrites W_l, dH reads Wt_l, and Wt_l is
// refreshed from W_l after dH.  (2) Clipping by the global norm: a first backward pass only adds up the squares (and
// turns the activations into gradients on its way down), the forward pass is run again — nothing has moved — and the
// second backward pass steps with the clip coefficient.
#include "osg_cfr_internal.h"
#include "osg_mfma_tile.h"
#include "osg_mlp_plan.h"

using namespace osg_mlp;
using namespace osg_mfma;   // f4, mma_rows, mma_cols, wave_sum

namespace {

constexpr int kWaves = kMlpThreads / 64;

struct MlpJob {   // one job as the kernel sees it (device pointers)
  MlpLayout lay;
  int kind, loss, S, A;
  int64_t U, I, rows;
  float* params;
  const float* target;
  const float* tensors;
  const uint8_t* mask;
  const int32_t* info;        // ring and reservoir
  const int32_t* action;      // ring
  const int32_t* next;
  const float* reward;
  const uint8_t* final_;
  const float* probs;         // reservoir [rows, A]
  const int64_t* slots;
  float* loss_out;
  float lr, discount, beta, clip;
};

struct Net { const int* w; const int* b; };   // offsets of one network's layers in LDS (arrays of the job's layout)

// The flat parameters (nn.Linear layout) into the padded LDS layout, zeros in the padding.
OSG_D void load_params(float* lds, const MlpLayout& L, const Net& n, const float* __restrict__ src) {
  for (int l = 0; l < L.n_linear; ++l) {
    const int sw = L.w_stride[l], in = L.in[l], out = L.out[l];
    const float* w = src + L.param_off[l];
    for (int x = threadIdx.x; x < L.out_pad[l] * sw; x += kMlpThreads) {
      const int o = x / sw, c = x % sw;
      lds[n.w[l] + x] = o < out && c < in ? w[o * in + c] : 0.0f;
    }
    for (int o = threadIdx.x; o < L.out_pad[l]; o += kMlpThreads) lds[n.b[l] + o] = o < out ? w[out * in + o] : 0.0f;
  }
}
OSG_D void store_params(const float* lds, const MlpLayout& L, const Net& n, float* __restrict__ dst) {
  for (int l = 0; l < L.n_linear; ++l) {
    const int sw = L.w_stride[l], in = L.in[l], out = L.out[l];
    float* w = dst + L.param_off[l];
    for (int x = threadIdx.x; x < out * in; x += kMlpThreads) w[x] = lds[n.w[l] + (x / in) * sw + x % in];
    for (int o = threadIdx.x; o < out; o += kMlpThreads) w[out * in + o] = lds[n.b[l] + o];
  }
}
OSG_D void refresh_transposed(float* lds, const MlpLayout& L, const Net& n, int l) {
  const int sw = L.w_stride[l], swt = L.wt_stride[l], op = L.out_pad[l];
  for (int x = threadIdx.x; x < L.in_pad[l] * op; x += kMlpThreads) {
    const int c = x / op, o = x % op;
    lds[L.wt[l] + c * swt + o] = lds[n.w[l] + o * sw + c];
  }
}

// X [B16, S16]: row b is the tensor of infostate rows[b][which] (below 0: zeros).
OSG_D void gather_inputs(float* lds, const MlpLayout& L, const MlpJob& j, int which) {
  const int sp = L.in_pad[0], sx = L.act_stride[0];
  const int* rows = reinterpret_cast<const int*>(lds + L.rows);
  for (int x = threadIdx.x; x < L.batch_pad * sp; x += kMlpThreads) {
    const int b = x / sp, c = x % sp;
    const int i = rows[b * kMlpRowWords + which];
    lds[L.act[0] + b * sx + c] = i >= 0 && c < j.S ? j.tensors[static_cast<int64_t>(i) * j.S + c] : 0.0f;
  }
}

// X -> Y through every layer of network n; the hidden activations stay in their buffers.
OSG_D void forward(float* lds, const MlpLayout& L, const Net& n) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int nrt = L.batch_pad / kMlpTile;
  for (int l = 0; l < L.n_linear; ++l) {
    const float* x = lds + L.act[l];
    float* y = lds + L.act[l + 1];
    const int sx = L.act_stride[l], sy = L.act_stride[l + 1], sw = L.w_stride[l];
    const bool relu = l + 1 < L.n_linear;
    const int tiles = nrt * (L.out_pad[l] / kMlpTile);
    for (int t = wave; t < tiles; t += kWaves) {
      const int rt = t % nrt, ct = t / nrt;
      f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      acc = mma_rows(x + rt * kMlpTile * sx, sx, lds + n.w[l] + ct * kMlpTile * sw, sw, L.in_pad[l], acc);
      const float bias = lds[n.b[l] + ct * kMlpTile + i];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[r] + bias;
        if (relu) v = v > 0.0f ? v : 0.0f;
        y[(rt * kMlpTile + 4 * g + r) * sy + ct * kMlpTile + i] = v;
      }
    }
    __syncthreads();
  }
}

// From dY in the Y buffer down to the first layer.  apply: every layer steps by lr * scale * gradient; else nothing
// moves and the return value is the sum of the squares of every gradient (the same on every thread).
OSG_D float backward(float* lds, const MlpLayout& L, const Net& n, bool apply, float lr, float scale) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int nrt = L.batch_pad / kMlpTile;
  float sq = 0.0f;
  for (int l = L.n_linear - 1; l >= 0; --l) {
    float* x = lds + L.act[l];
    const float* dy = lds + L.act[l + 1];
    const int sx = L.act_stride[l], sdy = L.act_stride[l + 1], sw = L.w_stride[l];
    const int nmt = L.out_pad[l] / kMlpTile, nnt = L.in_pad[l] / kMlpTile;
    for (int t = wave; t < nmt * (nnt + 1); t += kWaves) {   // (column tile nnt: the bias)
      const int mt = t % nmt, nt = t / nmt;
      f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      acc = mma_cols(dy + mt * kMlpTile, sdy, nt < nnt ? x + nt * kMlpTile : nullptr, sx, L.batch_pad, acc);
      if (nt == nnt && i != 0) continue;   // every column of the bias tile holds the same sums
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = mt * kMlpTile + 4 * g + r;
        float* p = nt < nnt ? lds + n.w[l] + o * sw + nt * kMlpTile + i : lds + n.b[l] + o;
        if (apply) *p = *p - lr * (acc[r] * scale);
        else sq = sq + acc[r] * acc[r];
      }
    }
    __syncthreads();
    if (l == 0) break;
    const int swt = L.wt_stride[l];
    for (int t = wave; t < nrt * nnt; t += kWaves) {
      const int rt = t % nrt, ct = t / nrt;
      f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      acc = mma_rows(dy + rt * kMlpTile * sdy, sdy, lds + L.wt[l] + ct * kMlpTile * swt, swt, L.out_pad[l], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* h = x + (rt * kMlpTile + 4 * g + r) * sx + ct * kMlpTile + i;
        *h = *h > 0.0f ? acc[r] : 0.0f;
      }
    }
    __syncthreads();
    if (apply) refresh_transposed(lds, L, n, l);
  }
  if (apply) return 0.0f;
  float* red = lds + L.reduce;
  sq = wave_sum(sq);
  if (lane == 0) red[wave] = sq;
  __syncthreads();
  float total = 0.0f;
  for (int w = 0; w < kWaves; ++w) total = total + red[w];
  __syncthreads();
  return total;
}

// The batch's rows into LDS; returns whether any row named something out of range (such a row counts as zeros).
OSG_D bool fetch_rows(float* lds, const MlpLayout& L, const MlpJob& j, int64_t u) {
  int* rows = reinterpret_cast<int*>(lds + L.rows);
  const int b = threadIdx.x;
  bool bad = false;
  if (b == 0) lds[L.reduce + kMlpReduceWords - 1] = 0.0f;
  __syncthreads();
  if (b < L.batch_pad) {
    int info = -1, second = -1, act = 0;
    float reward = 0.0f;
    if (b < L.batch) {
      const int64_t slot = j.slots[u * L.batch + b];
      if (slot < 0 || slot >= j.rows) {
        bad = true;
      } else if (j.kind == 0) {
        info = j.info[slot]; act = j.action[slot]; reward = j.reward[slot];
        const bool last = j.final_[slot] != 0;
        second = last ? -1 : j.next[slot];
        bad = info < 0 || info >= j.I || act < 0 || act >= j.A || (!last && (second < 0 || second >= j.I));
      } else {
        info = j.info[slot];
        second = static_cast<int>(slot);
        bad = info < 0 || info >= j.I;
      }
      if (bad) { info = -1; second = -1; act = 0; reward = 0.0f; }
    }
    rows[b * kMlpRowWords] = info;
    rows[b * kMlpRowWords + 1] = second;
    rows[b * kMlpRowWords + 2] = act;
    lds[L.rows + b * kMlpRowWords + 3] = reward;   // (then the row's target, then its loss)
  }
  if (bad) lds[L.reduce + kMlpReduceWords - 1] = 1.0f;   // (every writer writes the same word)
  __syncthreads();
  return lds[L.reduce + kMlpReduceWords - 1] != 0.0f;
}

// DQN: the targets from the target network's outputs on the next infostates (in the Y buffer).
OSG_D void dqn_targets(float* lds, const MlpLayout& L, const MlpJob& j) {
  const int* rows = reinterpret_cast<const int*>(lds + L.rows);
  const int b = threadIdx.x, sy = L.act_stride[L.n_linear];
  if (b < L.batch) {
    const int next = rows[b * kMlpRowWords + 1];
    float target = lds[L.rows + b * kMlpRowWords + 3];
    if (next >= 0) {
      float best = -3.402823466e+38f;
      for (int a = 0; a < j.A; ++a) {
        const float q = lds[L.act[L.n_linear] + b * sy + a];
        if (j.mask[static_cast<int64_t>(next) * j.A + a] && q > best) best = q;
      }
      target = target + j.discount * best;
    }
    lds[L.rows + b * kMlpRowWords + 3] = target;
  }
  __syncthreads();
}

// The loss of every row and dLoss/dY in place of Y (zeros in the padding); returns the batch's mean loss.
OSG_D float top_gradient(float* lds, const MlpLayout& L, const MlpJob& j) {
  const int* rows = reinterpret_cast<const int*>(lds + L.rows);
  const int b = threadIdx.x, sy = L.act_stride[L.n_linear], ap = L.out_pad[L.n_linear - 1];
  const float inv_b = 1.0f / static_cast<float>(L.batch);
  if (b < L.batch_pad) {
    float* y = lds + L.act[L.n_linear] + b * sy;
    const int info = rows[b * kMlpRowWords];
    float loss = 0.0f;
    if (info < 0) {
      for (int a = 0; a < ap; ++a) y[a] = 0.0f;
    } else if (j.kind == 0) {
      const int act = rows[b * kMlpRowWords + 2];
      const float d = y[act] - lds[L.rows + b * kMlpRowWords + 3];
      float grad;
      if (j.loss == 0) {
        loss = d * d;
        grad = 2.0f * d;
      } else {
        const float ad = fabsf(d);
        if (ad < j.beta) { loss = 0.5f * d * d / j.beta; grad = d / j.beta; }
        else { loss = ad - 0.5f * j.beta; grad = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }
      }
      for (int a = 0; a < ap; ++a) y[a] = a == act ? grad * inv_b : 0.0f;
    } else {
      const uint8_t* legal = j.mask + static_cast<int64_t>(info) * j.A;
      const float* probs = j.probs + static_cast<int64_t>(rows[b * kMlpRowWords + 1]) * j.A;
      float top = -3.402823466e+38f, z = 0.0f, mass = 0.0f;
      for (int a = 0; a < j.A; ++a)
        if (legal[a] && y[a] > top) top = y[a];
      for (int a = 0; a < j.A; ++a)
        if (legal[a]) { z = z + expf(y[a] - top); mass = mass + probs[a]; }
      const float lse = logf(z);
      for (int a = 0; a < ap; ++a) {
        float grad = 0.0f;
        if (a < j.A && legal[a]) {
          const float shifted = y[a] - top;
          loss = loss - probs[a] * (shifted - lse);
          grad = (expf(shifted) / z * mass - probs[a]) * inv_b;
        }
        y[a] = grad;
      }
    }
    lds[L.rows + b * kMlpRowWords + 3] = loss;
  }
  __syncthreads();
  float v = 0.0f;   // (every wavefront adds the same rows in the same order: no broadcast)
  for (int r = threadIdx.x & 63; r < L.batch_pad; r += 64) v = v + lds[L.rows + r * kMlpRowWords + 3];
  return wave_sum(v) * inv_b;
}

__global__ void __launch_bounds__(kMlpThreads) k_mlp_train(const MlpJob* __restrict__ jobs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const MlpJob& j = jobs[blockIdx.x];
  const MlpLayout& L = j.lay;
  const Net online{L.w, L.b}, frozen{L.tw, L.tb};
  load_params(lds, L, online, j.params);
  if (j.kind == 0) load_params(lds, L, frozen, j.target);
  __syncthreads();
  for (int l = 1; l < L.n_linear; ++l) refresh_transposed(lds, L, online, l);
  __syncthreads();
  for (int64_t u = 0; u < j.U; ++u) {
    const bool bad = fetch_rows(lds, L, j, u);
    if (j.kind == 0) {
      gather_inputs(lds, L, j, 1);
      __syncthreads();
      forward(lds, L, frozen);
      dqn_targets(lds, L, j);
    }
    gather_inputs(lds, L, j, 0);
    __syncthreads();
    forward(lds, L, online);
    const float loss = top_gradient(lds, L, j);
    float scale = 1.0f;
    if (j.kind == 1 && j.clip > 0.0f) {
      const float norm = sqrtf(backward(lds, L, online, false, 0.0f, 1.0f));
      const float coef = j.clip / (norm + 1e-6f);
      scale = coef < 1.0f ? coef : 1.0f;
      forward(lds, L, online);
      (void)top_gradient(lds, L, j);
    }
    (void)backward(lds, L, online, true, j.lr, scale);
    __syncthreads();
    if (threadIdx.x == 0) j.loss_out[u] = bad ? __builtin_nanf("") : loss;
  }
  store_params(lds, L, online, j.params);
}

}  // namespace

extern "C" int osg_nfsp_learn(osg_ctx* ctx, const osg_nfsp_learn_job* jobs, int64_t n_jobs) {
  const std::string who = "osg_nfsp_learn: ";
  if (!ctx || !jobs || n_jobs < 1 || n_jobs > 65535) return set_error(OSG_ERR_INVALID, who + "bad argument");
  size_t limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &limit)) return rc;
  std::vector<MlpJob> dev(static_cast<size_t>(n_jobs));
  size_t lds = 0;
  for (int64_t k = 0; k < n_jobs; ++k) {
    const osg_nfsp_learn_job& in = jobs[k];
    MlpJob& j = dev[static_cast<size_t>(k)];
    if ((in.kind != 0 && in.kind != 1) || in.updates < 0 || in.infostates < 1 || !in.d_params || !in.d_tensors || !in.d_legal_mask ||
        !in.d_slots || !in.d_loss || (in.kind == 0 && (!in.ring || !in.d_target_params || (in.loss != 0 && in.loss != 1))) ||
        (in.kind == 1 && !in.reservoir))
      return set_error(OSG_ERR_INVALID, who + "bad argument in job " + std::to_string(k));
    if (in.infostates >= (int64_t{1} << 31)) return set_error(OSG_ERR_UNSUPPORTED, who + "2^31 infostates or more");
    MlpShape shape;
    shape.n_linear = in.n_linear;
    if (in.n_linear >= 1 && in.n_linear <= kMlpMaxLinear)
      for (int l = 0; l <= in.n_linear; ++l) shape.widths[l] = in.widths[l];
    shape.batch = in.batch;
    shape.dqn = in.kind == 0;
    j.lay = plan_mlp(shape, limit);
    if (!j.lay.ok) return set_error(OSG_ERR_UNSUPPORTED, who + j.lay.why + " (job " + std::to_string(k) + ")");
    j.lay.why = nullptr;
    j.kind = in.kind; j.loss = in.loss; j.S = in.widths[0]; j.A = in.widths[in.n_linear];
    j.U = in.updates; j.I = in.infostates;
    j.params = in.d_params; j.target = in.d_target_params; j.tensors = in.d_tensors; j.mask = in.d_legal_mask;
    j.slots = in.d_slots; j.loss_out = in.d_loss;
    j.info = nullptr; j.action = nullptr; j.next = nullptr; j.reward = nullptr; j.final_ = nullptr; j.probs = nullptr;
    if (in.kind == 0) {
      const RingView v = ring_view(in.ring);
      if (v.ctx != ctx) return set_error(OSG_ERR_INVALID, who + "a ring of another context");
      j.rows = v.size; j.info = v.info; j.action = v.action; j.next = v.next; j.reward = v.reward; j.final_ = v.final_;
    } else {
      const ReservoirView v = reservoir_view(in.reservoir);
      if (v.ctx != ctx || v.A != j.A) return set_error(OSG_ERR_INVALID, who + "a reservoir of another row width or context");
      j.rows = v.size; j.info = v.info; j.probs = v.vals;
    }
    if (in.batch > j.rows) return set_error(OSG_ERR_INVALID, who + "a batch larger than the buffer's rows");
    j.lr = static_cast<float>(in.learning_rate); j.discount = static_cast<float>(in.discount);
    j.beta = static_cast<float>(in.huber_beta); j.clip = static_cast<float>(in.clip);
    lds = std::max(lds, j.lay.lds_bytes);
  }
  const void* kernel = reinterpret_cast<const void*>(&k_mlp_train);
  if (lds > (32u << 10) && raise_lds_cap(kernel, static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(OSG_ERR_UNSUPPORTED, who + "the device does not grant " + std::to_string(lds) + " bytes of LDS to a workgroup");
  }
  hipStream_t st = ctx->stream;
  void* ptr = nullptr;
  if (int rc = osg_ctx_scratch(ctx, sizeof(MlpJob) * dev.size(), &ptr)) return rc;
  OSG_HIP(hipMemcpyAsync(ptr, dev.data(), sizeof(MlpJob) * dev.size(), hipMemcpyHostToDevice, st));   // (small: staged before it returns)
  k_mlp_train<<<dim3(static_cast<unsigned>(n_jobs)), dim3(kMlpThreads), lds, st>>>(static_cast<const MlpJob*>(ptr));
  OSG_HIP(hipGetLastError());
  return OSG_OK;
}
