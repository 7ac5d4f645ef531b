// The WIDE form of the fused Deep CFR learner (k_deep_cfr_train_wide, osg_deep_cfr_learn_wide.hip), planned on the
// host: plain C++, no device call, no environment switch.  tests/native/adam_wide_plan_host_test.cpp includes this
// header alone.
//
// The narrow form (osg_adam_plan.h) keeps a network in one workgroup's LDS and registers, which ends at hidden widths
// of 128.  Here a GROUP of G workgroups trains one network, data-parallel over the batch: workgroup g owns rows
// [g R, min((g + 1) R, B)) of every update's batch, and the weights stay in global memory (L2).
//
//   R, G      R is the largest multiple of 16, at most kWideMaxRows and at most the padded batch, whose layout fits the
//             LDS limit; G = ceil(B / R) (at most 64, since R >= 16 and B <= 1024).  Both are a pure function of
//             (widths, batch, limit): a job's bits depend on G, so neither the device's CU count nor the other jobs of
//             a launch may move them.
//   rows      the R rows' inputs X, every hidden activation H_l, LayerNorm's output N (then its gradient) and the
//             output Z (then its gradient) stay in LDS for the whole update, with the narrow form's strides: a row of
//             `width` padded floats has stride width16 + 4, which is 4 mod 16, and the bank argument of osg_mlp_plan.h
//             holds for the row-wise and the batch-wise operand reads alike.  kWideRowWords words per row (infostate,
//             slot, iteration, loss, mean, 1 / std).
//   panels    a weight matrix is streamed through LDS in panels of 16 output rows by at most kWidePanelCols input
//             columns ([16, cols16 + 4]), two buffers: one feeds the matrix instruction while the other is filled.
//             Forward reads a panel row-wise (contraction over its columns); dH = dY W reads the SAME panel with its
//             rows as the contraction (the four rows of a step adjacent: that read collides on banks, as the narrow
//             form's does without its transposed copy).  No transposed copy exists in this form.
//   scratch   per job, in global memory: kWideBarrierWords counter words, then partial[G][partial_stride] floats —
//             workgroup g's gradient of every flat parameter, then its loss sum and its out-of-range flag.
//   slices    after the first barrier workgroup g owns parameters [g slice, min((g + 1) slice, P)): it adds the G
//             partials of each in ascending workgroup order and takes the Adam step.
#pragma once
#include <cstddef>
#include <cstdint>

namespace osg_adam_wide {

constexpr int kWideTile = 16;
constexpr int kWideMaxLinear = 3;       // linear layers: 1 or 2 hidden layers and the output layer
constexpr int kWideMaxWidth = 512;      // hidden widths
constexpr int kWideMaxInputs = 256;     // S
constexpr int kWideMaxActions = 16;     // A
constexpr int kWideMaxBatch = 1024;     // B: the batched draw's limit
constexpr int kWideMaxRows = 64;        // R: at most four 16-row chunks per workgroup
constexpr int kWideMaxGroup = 64;       // G
constexpr int kWidePanelCols = 256;     // input columns of a panel (8 per thread)
constexpr int kWideThreads = 512;       // 8 wavefronts
constexpr int kWideWaves = kWideThreads / 64;
constexpr int kWideRowWords = 8;        // per row: infostate, slot, iteration, loss, mean, 1 / std, 2 spare
constexpr int kWideFlagWords = 16;
constexpr int kWideBarrierWords = 64;   // per job: [0] arrivals, [1] a workgroup gave up; 256 bytes

inline int wide_pad(int n) { return (n + kWideTile - 1) / kWideTile * kWideTile; }
inline int wide_stride(int n) { return wide_pad(n) + 4; }

struct WideShape {
  int n_linear = 0;                     // 2 or 3
  int widths[kWideMaxLinear + 1] = {0, 0, 0, 0};   // S, hidden ..., A
  int batch = 0;
};

// Offsets in floats from the start of the dynamic LDS.
struct WideLayout {
  bool ok = false;
  const char* why = nullptr;
  int n_linear = 0, batch = 0, rows = 0, group = 0;      // rows: R, group: G
  int in[kWideMaxLinear] = {0, 0, 0}, out[kWideMaxLinear] = {0, 0, 0};
  int in_pad[kWideMaxLinear] = {0, 0, 0}, out_pad[kWideMaxLinear] = {0, 0, 0};
  int act[kWideMaxLinear] = {0, 0, 0};          // X, H_0, H_1: layer l's input (l below the last)
  int act_stride[kWideMaxLinear] = {0, 0, 0};
  int n = 0, n_stride = 0, z = 0, z_stride = 0;
  int ln_width = 0, ln_pad = 0, gamma = 0, beta = 0;
  int panel[2] = {0, 0}, panel_cols = 0, panel_stride = 0;
  int row_words = 0, flags = 0;
  int param_off[kWideMaxLinear] = {0, 0, 0};    // of layer l's weight in the flat parameter buffer (its bias follows)
  int ln_off = 0, param_count = 0;              // of the LayerNorm weight (its bias follows)
  int partial_stride = 0, slice = 0;            // floats per workgroup in scratch; parameters per workgroup's Adam slice
  size_t lds_bytes = 0, scratch_bytes = 0;
};

inline WideLayout plan_adam_wide(const WideShape& s, size_t lds_limit_bytes) {
  WideLayout p;
  const auto refuse = [&p](const char* why) { p.ok = false; p.why = why; return p; };
  if (s.n_linear < 2 || s.n_linear > kWideMaxLinear) return refuse("one or two hidden layers are served");
  if (s.batch < 1 || s.batch > kWideMaxBatch) return refuse("a batch of 1 to 1024 rows is served");
  if (s.widths[0] < 1 || s.widths[0] > kWideMaxInputs) return refuse("1 to 256 inputs are served");
  if (s.widths[s.n_linear] < 1 || s.widths[s.n_linear] > kWideMaxActions) return refuse("1 to 16 outputs are served");
  for (int l = 1; l < s.n_linear; ++l)
    if (s.widths[l] < 1 || s.widths[l] > kWideMaxWidth) return refuse("hidden widths of 1 to 512 are served");
  const int last = s.n_linear - 1;
  p.n_linear = s.n_linear; p.batch = s.batch;
  p.ln_width = s.widths[last]; p.ln_pad = wide_pad(p.ln_width);
  int widest = 0;
  for (int l = 0; l < s.n_linear; ++l) {
    p.in[l] = s.widths[l]; p.out[l] = s.widths[l + 1];
    p.in_pad[l] = wide_pad(p.in[l]); p.out_pad[l] = wide_pad(p.out[l]);
    if (l == last) { p.ln_off = p.param_count; p.param_count += 2 * p.ln_width; }
    p.param_off[l] = p.param_count;
    p.param_count += p.out[l] * p.in[l] + p.out[l];
    widest = p.in_pad[l] > widest ? p.in_pad[l] : widest;
  }
  p.panel_cols = widest < kWidePanelCols ? widest : kWidePanelCols;
  p.panel_stride = p.panel_cols + 4;
  p.partial_stride = (p.param_count + 2 + 3) / 4 * 4;
  size_t at = 0;
  const auto take = [&at](size_t floats) { const size_t o = at; at += (floats + 3) / 4 * 4; return static_cast<int>(o); };
  const auto lay = [&](int rows) {
    at = 0;
    p.gamma = take(p.ln_pad); p.beta = take(p.ln_pad);
    for (int b = 0; b < 2; ++b) p.panel[b] = take(static_cast<size_t>(kWideTile) * p.panel_stride);
    for (int l = 0; l < s.n_linear; ++l) {
      p.act_stride[l] = wide_stride(p.in[l]);
      p.act[l] = take(static_cast<size_t>(rows) * p.act_stride[l]);
    }
    p.n_stride = p.act_stride[last];
    p.n = take(static_cast<size_t>(rows) * p.n_stride);
    p.z_stride = wide_stride(p.out[last]);
    p.z = take(static_cast<size_t>(rows) * p.z_stride);
    p.row_words = take(static_cast<size_t>(kWideRowWords) * rows);
    p.flags = take(kWideFlagWords);
    p.rows = rows;
    p.lds_bytes = at * sizeof(float);
    return p.lds_bytes <= lds_limit_bytes;
  };
  const int need = wide_pad(s.batch);
  for (int rows = need < kWideMaxRows ? need : kWideMaxRows; rows >= kWideTile; rows -= kWideTile)
    if (lay(rows)) {
      p.group = (s.batch + rows - 1) / rows;
      p.slice = (p.param_count + p.group - 1) / p.group;
      p.scratch_bytes = (kWideBarrierWords * sizeof(unsigned int) + static_cast<size_t>(p.group) * p.partial_stride * sizeof(float) + 255) / 256 * 256;
      p.ok = true;
      return p;
    }
  return refuse("sixteen rows of the network's activations and two weight panels do not fit a workgroup's LDS");
}

}  // namespace osg_adam_wide
