// The fused NFSP / DQN learner's LDS layout (k_mlp_train, osg_mlp_train.hip), worked out on the host: plain C++, no
// device call, no environment switch.  tests/native/mlp_plan_host_test.cpp includes this header alone.
//
// One workgroup trains one multi-layer perceptron (Linear + ReLU per hidden layer, then Linear; nn.Linear layout) for U
// sequential updates with everything in LDS.  Sizes: S inputs, hidden widths, A outputs, B rows per batch.
//
//   padding   every feature width (S, hidden, A) and B are padded to the 16 of the fp32 matrix tile
//             (v_mfma_f32_16x16x4_f32) inside LDS only; padded weights, biases, inputs and batch rows are exact zeros
//             and stay so (a padded weight's gradient is a sum of products with a zero factor).
//   stride    a row of `width` padded floats is stored with stride width + 4.  width is a multiple of 16, so the stride
//             is 4 mod 16.  The LDS has 64 banks of 4 bytes; a 32-bit read of a wavefront is served in one pass when
//             the 64 lanes name 64 different banks.  Lane l = 16 g + i (g 0..3, i 0..15) reads
//               row-wise operands (forward's A and B, dH's A and B):  element (row i, column k0 + g)
//                 bank (i * stride + g) mod 64 = (4 i (4 q + 1) + g) mod 64: the 16 multiples of 4 are distinct since
//                 4 q + 1 is odd, and g fills the gaps: 64 different banks;
//               batch-wise operands (the weight gradient's A and B, contracting over the batch): element
//                 (row t + 4 g, column c0 + i) of a 16-row chunk — the four rows one instruction contracts are taken
//                 4 apart, not adjacent — bank (4 g * stride + i) mod 64 = (16 g (4 q + 1) + i) mod 64: four disjoint
//                 windows of 16: 64 different banks.
//             The tile's write-back (lane holds rows 4 g + r, column i) has the second form.  Only the transposed copy's
//             refresh (below) reads columns with conflicts; it moves out * in floats once per layer and update.
//   Wt        every layer but the first also keeps its weights transposed ([in, out]): dH = dY W contracts over `out`,
//             and with W alone its B operand would be read batch-wise from a matrix whose A-side partner (dY) is read
//             row-wise — no single stride serves both.  The copy also IS the old weight: the layer's SGD step rewrites
//             W, dH reads Wt, and Wt is refreshed from W afterwards.
//   buffers   [W_l, b_l]; [Wt_l, l >= 1]; DQN: [target W_l, b_l]; X [B16, S16 + 4]; H_l [B16, width16 + 4] per hidden
//             layer; Y [B16, A16 + 4]; four words per row (kMlpRowWords); 16 words of reductions.
#pragma once
#include <cstddef>
#include <cstdint>

namespace osg_mlp {

constexpr int kMlpTile = 16;
constexpr int kMlpMaxLinear = 3;       // linear layers: 1 or 2 hidden layers and the output layer
constexpr int kMlpMaxWidth = 128;      // hidden widths
constexpr int kMlpMaxInputs = 256;     // S
constexpr int kMlpMaxActions = 16;     // A
constexpr int kMlpMaxBatch = 128;      // B
constexpr int kMlpThreads = 512;       // 8 wavefronts: one 16-row tile each at B = 128
constexpr int kMlpRowWords = 4;        // per batch row: infostate, next infostate (or slot), action, reward -> target -> loss
constexpr int kMlpReduceWords = 16;

inline int mlp_pad(int n) { return (n + kMlpTile - 1) / kMlpTile * kMlpTile; }
inline int mlp_stride(int n) { return mlp_pad(n) + 4; }

struct MlpShape {
  int n_linear = 0;                    // 2 or 3
  int widths[kMlpMaxLinear + 1] = {0, 0, 0, 0};   // S, hidden ..., A
  int batch = 0;
  bool dqn = false;                    // a frozen target network sits in LDS too
};

// Offsets in floats from the start of the dynamic LDS.
struct MlpLayout {
  bool ok = false;
  const char* why = nullptr;
  int n_linear = 0, batch = 0, batch_pad = 0;
  int in[kMlpMaxLinear] = {0, 0, 0}, out[kMlpMaxLinear] = {0, 0, 0};
  int in_pad[kMlpMaxLinear] = {0, 0, 0}, out_pad[kMlpMaxLinear] = {0, 0, 0};
  int w_stride[kMlpMaxLinear] = {0, 0, 0};     // of W_l [out_pad, in_pad + 4]
  int wt_stride[kMlpMaxLinear] = {0, 0, 0};    // of Wt_l [in_pad, out_pad + 4], l >= 1
  int act_stride[kMlpMaxLinear + 1] = {0, 0, 0, 0};   // of X, H_0 .., Y
  int w[kMlpMaxLinear] = {0, 0, 0}, b[kMlpMaxLinear] = {0, 0, 0}, wt[kMlpMaxLinear] = {0, 0, 0};
  int tw[kMlpMaxLinear] = {0, 0, 0}, tb[kMlpMaxLinear] = {0, 0, 0};   // the target network's (DQN)
  int act[kMlpMaxLinear + 1] = {0, 0, 0, 0};   // X, H_0 .., Y
  int rows = 0, reduce = 0;
  int param_off[kMlpMaxLinear] = {0, 0, 0};    // of layer l's weight in the flat parameter buffer (its bias follows)
  int param_count = 0;
  size_t lds_bytes = 0;
};

inline MlpLayout plan_mlp(const MlpShape& s, size_t lds_limit_bytes) {
  MlpLayout p;
  const auto refuse = [&p](const char* why) { p.ok = false; p.why = why; return p; };
  if (s.n_linear < 2 || s.n_linear > kMlpMaxLinear) return refuse("one or two hidden layers are served");
  if (s.batch < 1 || s.batch > kMlpMaxBatch) return refuse("a batch of 1 to 128 rows is served");
  if (s.widths[0] < 1 || s.widths[0] > kMlpMaxInputs) return refuse("1 to 256 inputs are served");
  if (s.widths[s.n_linear] < 1 || s.widths[s.n_linear] > kMlpMaxActions) return refuse("1 to 16 outputs are served");
  for (int l = 1; l < s.n_linear; ++l)
    if (s.widths[l] < 1 || s.widths[l] > kMlpMaxWidth) return refuse("hidden widths of 1 to 128 are served");
  p.n_linear = s.n_linear; p.batch = s.batch; p.batch_pad = mlp_pad(s.batch);
  size_t at = 0;
  const auto take = [&at](size_t floats) { const size_t o = at; at += (floats + 3) / 4 * 4; return static_cast<int>(o); };
  for (int l = 0; l < s.n_linear; ++l) {
    p.in[l] = s.widths[l]; p.out[l] = s.widths[l + 1];
    p.in_pad[l] = mlp_pad(p.in[l]); p.out_pad[l] = mlp_pad(p.out[l]);
    p.w_stride[l] = mlp_stride(p.in[l]);
    p.param_off[l] = p.param_count;
    p.param_count += p.out[l] * p.in[l] + p.out[l];
    p.w[l] = take(static_cast<size_t>(p.out_pad[l]) * p.w_stride[l]);
    p.b[l] = take(p.out_pad[l]);
  }
  for (int l = 1; l < s.n_linear; ++l) {
    p.wt_stride[l] = mlp_stride(p.out[l]);
    p.wt[l] = take(static_cast<size_t>(p.in_pad[l]) * p.wt_stride[l]);
  }
  if (s.dqn)
    for (int l = 0; l < s.n_linear; ++l) {
      p.tw[l] = take(static_cast<size_t>(p.out_pad[l]) * p.w_stride[l]);
      p.tb[l] = take(p.out_pad[l]);
    }
  for (int l = 0; l <= s.n_linear; ++l) {
    p.act_stride[l] = mlp_stride(s.widths[l]);
    p.act[l] = take(static_cast<size_t>(p.batch_pad) * p.act_stride[l]);
  }
  p.rows = take(static_cast<size_t>(kMlpRowWords) * p.batch_pad);
  p.reduce = take(kMlpReduceWords);
  p.lds_bytes = at * sizeof(float);
  if (p.lds_bytes > lds_limit_bytes) return refuse("the network, its batch and activations do not fit a workgroup's LDS");
  p.ok = true;
  return p;
}

}  // namespace osg_mlp
