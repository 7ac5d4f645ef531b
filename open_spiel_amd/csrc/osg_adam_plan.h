// The fused Deep CFR learner's LDS layout (k_deep_cfr_train, osg_deep_cfr_learn.hip), worked out on the host: plain
// C++, no device call, no environment switch.  tests/native/adam_plan_host_test.cpp includes this header alone.
//
// One workgroup trains one network of deep_cfr.MLP — Linear + ReLU per hidden layer, LayerNorm, Linear — for U
// sequential Adam updates.  The parameters stay in LDS for the whole call; the batch of B rows (up to 1024) does not
// fit and is walked in tiles of T rows, T the largest of 128 / 64 / 32 / 16 that fits (heights of which the half still
// covers the batch are skipped).  Only one tile has its inputs and activations in LDS.
//
//   padding   as osg_mlp_plan.h: every feature width and T are padded to the 16 of v_mfma_f32_16x16x4_f32 inside LDS
//             only; padded weights, biases, LayerNorm weights and inputs are exact zeros and stay so (they are never
//             stepped), so padded activations and their gradients are exact zeros too.
//   stride    a row of `width` padded floats has stride width + 4, which is 4 mod 16.  With lane l = 16 g + i,
//             row-wise operands (element (row i, column k0 + g)) and batch-wise operands (element (row t + 4 g,
//             column c0 + i) of a 16-row chunk: rows four apart) name 64 different banks; the argument is
//             osg_mlp_plan.h's.  The LayerNorm row passes take the batch-wise form as well: lane 16 g + i works on row
//             t + 4 g of a chunk and reads its columns i, i + 16, ...; its statistics are 16-lane shuffle trees.  The
//             column pass of the LayerNorm gradients (thread c reads column c of row after row) reads consecutive
//             words, and the row's two statistics as a broadcast.
//   gradients live in REGISTERS, not in LDS: the [out, in] tiles (and one bias tile per 16 outputs) of all layers are
//             numbered through (tile_off) and tile t belongs to wavefront t mod 8, which keeps its accumulator from
//             the batch's first tile to its last — the instruction adds every 16-row chunk onto it, tiles ascending —
//             and steps the parameter from it.  At most kAdamMaxOwn tiles per wavefront are served.  The LayerNorm
//             gradients are per-column sums of thread c (weight) and thread ln_pad + c (bias), rows ascending.
//   Wt        the transposed weights of every layer but the first ([in, out], for dH = dY W), if there is room.  Without
//             them the B operand of that product is read batch-wise from W with its four rows ADJACENT (the
//             contraction index is shared with dY, read row-wise): g * stride + i lands in windows 4 apart, up to
//             four lanes to a bank.  That read is allowed to collide.  So are the transposed refresh (column reads,
//             once per layer and update) and the Adam step's moment reads when the moments are resident: they are
//             stored flat, unpadded, in network.parameters() order — the layout of the global buffers — and a lane's
//             word there is o * in + c.
//   moments   Adam's m and v, param_count floats each, resident if there is room; else the thread that steps a
//             parameter reads and writes them in the job's global buffers, once per update, same operations.
//   choice    tile height first, then (Wt, moments) in the order (yes, yes), (yes, no), (no, yes), (no, no): a pure
//             function of the shape and the limit, since a job's bits may depend on the tile height.
//   buffers   [W_l, b_l]; LayerNorm weight and bias; [Wt_l, l >= 1]; [m, v]; X [T, S16 + 4]; H_l [T, width16 + 4] per
//             hidden layer; N [T, width16 + 4] (LayerNorm's output, then its gradient); Z [T, A16 + 4] (the output,
//             then its gradient); kAdamRowWords words per row (infostate, slot, iteration, loss, mean, 1 / std);
//             16 words of flags.
#pragma once
#include <cstddef>
#include <cstdint>

namespace osg_adam {

constexpr int kAdamTile = 16;
constexpr int kAdamMaxLinear = 3;      // linear layers: 1 or 2 hidden layers and the output layer
constexpr int kAdamMaxWidth = 128;     // hidden widths
constexpr int kAdamMaxInputs = 256;    // S
constexpr int kAdamMaxActions = 16;    // A
constexpr int kAdamMaxBatch = 1024;    // B: the batched draw's limit
constexpr int kAdamMaxRows = 128;      // the tallest tile
constexpr int kAdamThreads = 512;      // 8 wavefronts
constexpr int kAdamWaves = kAdamThreads / 64;
constexpr int kAdamMaxOwn = 20;        // gradient tiles per wavefront (80 accumulator registers)
constexpr int kAdamRowWords = 8;       // per tile row: infostate, slot, iteration, loss, mean, 1 / std, 2 spare
constexpr int kAdamReduceWords = 16;

inline int adam_pad(int n) { return (n + kAdamTile - 1) / kAdamTile * kAdamTile; }
inline int adam_stride(int n) { return adam_pad(n) + 4; }

struct AdamShape {
  int n_linear = 0;                    // 2 or 3
  int widths[kAdamMaxLinear + 1] = {0, 0, 0, 0};   // S, hidden ..., A
  int batch = 0;
};

// Offsets in floats from the start of the dynamic LDS.
struct AdamLayout {
  bool ok = false;
  const char* why = nullptr;
  int n_linear = 0, batch = 0, tile = 0, n_tiles = 0;
  bool wt_resident = false, moments_resident = false;
  int in[kAdamMaxLinear] = {0, 0, 0}, out[kAdamMaxLinear] = {0, 0, 0};
  int in_pad[kAdamMaxLinear] = {0, 0, 0}, out_pad[kAdamMaxLinear] = {0, 0, 0};
  int w_stride[kAdamMaxLinear] = {0, 0, 0};    // of W_l [out_pad, in_pad + 4]
  int wt_stride[kAdamMaxLinear] = {0, 0, 0};   // of Wt_l [in_pad, out_pad + 4], l >= 1
  int w[kAdamMaxLinear] = {0, 0, 0}, b[kAdamMaxLinear] = {0, 0, 0}, wt[kAdamMaxLinear] = {0, 0, 0};
  int ln_width = 0, ln_pad = 0, gamma = 0, beta = 0;
  int act[kAdamMaxLinear] = {0, 0, 0};         // X, H_0, H_1: layer l's input (l below the last)
  int act_stride[kAdamMaxLinear] = {0, 0, 0};
  int n = 0, n_stride = 0, z = 0, z_stride = 0;
  int mom_m = 0, mom_v = 0, rows = 0, reduce = 0;
  int tile_off[kAdamMaxLinear + 1] = {0, 0, 0, 0};   // layer l's gradient tiles are tile_off[l] .. tile_off[l + 1] - 1
  int param_off[kAdamMaxLinear] = {0, 0, 0};   // of layer l's weight in the flat parameter buffer (its bias follows)
  int ln_off = 0, param_count = 0;             // of the LayerNorm weight (its bias follows)
  size_t lds_bytes = 0;
};

inline AdamLayout plan_adam(const AdamShape& s, size_t lds_limit_bytes) {
  AdamLayout p;
  const auto refuse = [&p](const char* why) { p.ok = false; p.why = why; return p; };
  if (s.n_linear < 2 || s.n_linear > kAdamMaxLinear) return refuse("one or two hidden layers are served");
  if (s.batch < 1 || s.batch > kAdamMaxBatch) return refuse("a batch of 1 to 1024 rows is served");
  if (s.widths[0] < 1 || s.widths[0] > kAdamMaxInputs) return refuse("1 to 256 inputs are served");
  if (s.widths[s.n_linear] < 1 || s.widths[s.n_linear] > kAdamMaxActions) return refuse("1 to 16 outputs are served");
  for (int l = 1; l < s.n_linear; ++l)
    if (s.widths[l] < 1 || s.widths[l] > kAdamMaxWidth) return refuse("hidden widths of 1 to 128 are served");
  const int last = s.n_linear - 1;
  p.n_linear = s.n_linear; p.batch = s.batch;
  p.ln_width = s.widths[last]; p.ln_pad = adam_pad(p.ln_width);
  for (int l = 0; l < s.n_linear; ++l) {
    p.in[l] = s.widths[l]; p.out[l] = s.widths[l + 1];
    p.in_pad[l] = adam_pad(p.in[l]); p.out_pad[l] = adam_pad(p.out[l]);
    p.w_stride[l] = adam_stride(p.in[l]);
    if (l) p.wt_stride[l] = adam_stride(p.out[l]);
    if (l == last) { p.ln_off = p.param_count; p.param_count += 2 * p.ln_width; }
    p.param_off[l] = p.param_count;
    p.param_count += p.out[l] * p.in[l] + p.out[l];
    p.tile_off[l + 1] = p.tile_off[l] + p.out_pad[l] / kAdamTile * (p.in_pad[l] / kAdamTile + 1);
  }
  if (p.tile_off[s.n_linear] > kAdamMaxOwn * kAdamWaves) return refuse("the network has more gradient tiles than the wavefronts' registers hold");
  size_t at = 0;
  const auto take = [&at](size_t floats) { const size_t o = at; at += (floats + 3) / 4 * 4; return static_cast<int>(o); };
  const auto lay = [&](int tile, bool wt, bool moments) {
    at = 0;
    for (int l = 0; l < s.n_linear; ++l) {
      p.w[l] = take(static_cast<size_t>(p.out_pad[l]) * p.w_stride[l]);
      p.b[l] = take(p.out_pad[l]);
    }
    p.gamma = take(p.ln_pad); p.beta = take(p.ln_pad);
    for (int l = 1; l < s.n_linear; ++l) p.wt[l] = wt ? take(static_cast<size_t>(p.in_pad[l]) * p.wt_stride[l]) : 0;
    p.mom_m = moments ? take(p.param_count) : 0;
    p.mom_v = moments ? take(p.param_count) : 0;
    for (int l = 0; l < s.n_linear; ++l) {
      p.act_stride[l] = adam_stride(p.in[l]);
      p.act[l] = take(static_cast<size_t>(tile) * p.act_stride[l]);
    }
    p.n_stride = p.act_stride[last];
    p.n = take(static_cast<size_t>(tile) * p.n_stride);
    p.z_stride = adam_stride(p.out[last]);
    p.z = take(static_cast<size_t>(tile) * p.z_stride);
    p.rows = take(static_cast<size_t>(kAdamRowWords) * tile);
    p.reduce = take(kAdamReduceWords);
    p.tile = tile; p.n_tiles = (s.batch + tile - 1) / tile;
    p.wt_resident = wt; p.moments_resident = moments;
    p.lds_bytes = at * sizeof(float);
    return p.lds_bytes <= lds_limit_bytes;
  };
  for (int tile = kAdamMaxRows; tile >= kAdamTile; tile /= 2) {
    if (tile > kAdamTile && tile / 2 >= s.batch) continue;   // the half covers the batch as well
    for (int form = 0; form < 4; ++form)
      if (lay(tile, form < 2, form % 2 == 0)) { p.ok = true; return p; }
  }
  return refuse("the network and one 16-row tile of its batch do not fit a workgroup's LDS");
}

}  // namespace osg_adam
