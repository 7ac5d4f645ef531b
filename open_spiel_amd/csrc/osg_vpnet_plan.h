// The fused policy-value MLP forward (k_vpnet_forward, osg_vpnet.hip), planned on the host: plain C++, no device call,
// no environment switch.  tests/native/vpnet_plan_host_test.cpp includes this header alone.
//
// The network is alpha_zero_torch's nn_model == "mlp": Linear(O, W) + ReLU, depth x (Linear(W, W) + ReLU), a value head
// Linear(W, W) + ReLU, Linear(W, 1), tanh and a policy head Linear(W, W) + ReLU, Linear(W, A), softmax over the legal
// actions.  A workgroup of 8 wavefronts owns R rows and carries them through every layer.
//
//   in place  ONE activation buffer [R, W16 + 4].  A layer's whole output [R, W16] stays in the accumulators of the
//             wavefronts until its contraction has ended; then the workgroup meets and the accumulators (bias, ReLU)
//             overwrite the layer's input.  Ping-pong buffers would halve R at the same LDS; every workgroup re-reads
//             all parameters, so the weight traffic of a launch is parameters x ceil(n / R): in place halves it.
//   blocking  the wavefronts form a 2 x 4 grid over the output: wavefront (wr, wc) holds row tiles wr + 2 m (m < MR,
//             R = 32 MR) and column tiles wc + 4 c (c < NC) of 16 x 16, MR NC <= 16 tiles = 64 accumulator registers.
//             (MR, NC) is (4, 4) for W16 <= 256 (R = 128) and (2, 8) or (1, 8) otherwise (R = 64, 32).  A k-step of 4
//             reads MR + NC operand fragments of 256 bytes per wavefront for MR NC instructions: 128 bytes of LDS per
//             v_mfma_f32_16x16x4_f32 at (4, 4), 160 at (2, 8), 288 at (1, 8).  The four SIMDs of a CU retire one such
//             instruction per 8 clocks together, so the operands ask for 16, 20 and 36 bytes per clock of the 128 the
//             LDS delivers.  (One tile per wavefront, as in the learners, asks for 64.)
//   panels    the weights stay in global memory (L2) and come through LDS in double-buffered panels of KC input columns
//             by all output rows a pass needs (at most 64 NC): the threads request panel s + 1 into registers, the
//             wavefronts run the matrix instruction on panel s, then the registers go to the other buffer; one
//             __syncthreads per panel.  Straight into the B operand would make every wavefront of a column fetch the
//             same words again (twice here) with 16-byte pieces of 16 rows per request; through LDS a weight is
//             requested once per workgroup.  KC is the largest of 16, 8, 4 that fits beside the largest R.
//   layer 0   contracts over O: the observation tile comes from global memory in the same K-chunks [R, KC], zeros past
//             O and past row n, into two stage buffers that ALIAS the activation buffer (dead until layer 0 has ended).
//   heads     the value head's hidden layer never reaches LDS: its W -> 1 layer is a reduction over the accumulators
//             (lane, 16-lane tree, then the four column wavefronts in ascending order through `vpart`).  The policy
//             head's hidden layer then overwrites the torso; its W -> A layer runs in passes of 64 NC columns into
//             `logits` [R, A16 + 4].  The two heads' first layers are NOT one [2 W, W] contraction: that doubles the
//             accumulators a wavefront holds, which is what bounds R.
//   strides   LDS has 64 banks of 4 bytes.  Lane 16 g + i reads operand element (row i, column k + g).  Activation and
//             logit rows have a stride s that is 4 mod 16: bank (i s + g) mod 64 = (4 i (4 q + 1) + g) mod 64, the 16
//             multiples of 4 are distinct since 4 q + 1 is odd, and g fills the gaps: 64 different banks.  The
//             accumulators' write-back (row 4 g + r, column i) lands in bank (16 g (4 q + 1) + i) mod 64: four windows
//             of 16.  Panels and observation stages are not padded (at W = 256, R = 128 the padding of a KC = 8 panel
//             is what would not fit): their stride is KC and column c of row r sits at c ^ vp_swizzle(KC, r), which
//             moves whole groups of 4 columns.  With G = KC / 4 groups, rows i and i + 16 / G, ... share their banks
//             unswizzled; the swizzle 4 ((i G / 16) mod G) sends them to the G different groups: 64 different banks.
#pragma once
#include <cstddef>
#include <cstdint>

namespace osg_vpnet {

constexpr int kVpTile = 16;
constexpr int kVpThreads = 512;        // 8 wavefronts: 2 over the rows x 4 over the columns
constexpr int kVpWaveRows = 2, kVpWaveCols = 4;
constexpr int kVpMaxObs = 2048;        // O
constexpr int kVpMaxWidth = 512;       // W
constexpr int kVpMaxDepth = 8;         // nn_depth
constexpr int kVpMaxActions = 384;     // A
constexpr int kVpPanelRegs = 8;        // floats of a weight panel per thread
constexpr int kVpObsRegs = 4;          // floats of an observation chunk per thread

inline int vp_pad(int n) { return (n + kVpTile - 1) / kVpTile * kVpTile; }
// (constexpr: the kernel calls it too)
constexpr int vp_swizzle(int kc, int row) { return 4 * ((row % kVpTile) * (kc / 4) / kVpTile); }

struct VpShape {
  int obs = 0, width = 0, depth = 0, actions = 0;
};

// Offsets in floats from the start of the dynamic LDS; param offsets in floats from the start of the flat parameters.
struct VpPlan {
  bool ok = false;
  const char* why = nullptr;
  int obs = 0, width = 0, depth = 0, actions = 0;
  int wp = 0, ap = 0;                    // W and A padded to 16
  int rows = 0, mr = 0, nc = 0;          // R = 32 MR; NC column tiles per wavefront and pass
  int kc = 0, panel_stride = 0, panel_rows = 0;
  int act = 0, act_stride = 0;
  int logits = 0, logits_stride = 0;
  int panel[2] = {0, 0};
  int xstage[2] = {0, 0};                // inside act
  int vpart = 0, vals = 0;               // [4][R] partial value sums; [R] values
  int torso[kVpMaxDepth + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // weight of torso layer l (its bias follows)
  int v1 = 0, v2 = 0, p1 = 0, p2 = 0;    // the heads' weights (each followed by its bias)
  int param_count = 0;
  size_t lds_bytes = 0;
};

// Where every Linear of a plan whose shape is set starts in the flat parameters (osg_vpnet_learn_plan.h calls it too).
inline void vp_param_offsets(VpPlan& p) {
  const int W = p.width;
  int at_param = 0;
  const auto linear = [&at_param](int out, int in) { const int o = at_param; at_param += out * in + out; return o; };
  p.torso[0] = linear(W, p.obs);
  for (int l = 1; l <= p.depth; ++l) p.torso[l] = linear(W, W);
  p.v1 = linear(W, W); p.v2 = linear(1, W); p.p1 = linear(W, W); p.p2 = linear(p.actions, W);
  p.param_count = at_param;
}

inline VpPlan plan_vpnet(const VpShape& s, size_t lds_limit_bytes) {
  VpPlan p;
  const auto refuse = [&p](const char* why) { p.ok = false; p.why = why; return p; };
  if (s.obs < 1 || s.obs > kVpMaxObs) return refuse("observations of 1 to 2048 floats are served");
  if (s.width < 1 || s.width > kVpMaxWidth) return refuse("an nn_width of 1 to 512 is served");
  if (s.depth < 0 || s.depth > kVpMaxDepth) return refuse("an nn_depth of 0 to 8 is served");
  if (s.actions < 1 || s.actions > kVpMaxActions) return refuse("1 to 384 actions are served");
  p.obs = s.obs; p.width = s.width; p.depth = s.depth; p.actions = s.actions;
  p.wp = vp_pad(s.width); p.ap = vp_pad(s.actions);
  vp_param_offsets(p);
  p.act_stride = p.wp + 4;
  p.logits_stride = p.ap + 4;
  size_t at = 0;
  const auto take = [&at](size_t floats) { const size_t o = at; at += (floats + 3) / 4 * 4; return static_cast<int>(o); };
  const int widest = p.wp > p.ap ? p.wp : p.ap;
  for (int mr = 4; mr >= 1; mr /= 2) {
    const int nc = mr == 4 ? 4 : 8, rows = 32 * mr;
    if (p.wp > kVpWaveCols * nc * kVpTile) continue;   // the layer's output does not fit the accumulators
    const int panel_rows = widest < kVpWaveCols * nc * kVpTile ? widest : kVpWaveCols * nc * kVpTile;
    for (int kc = 16; kc >= 4; kc /= 2) {
      const int ps = kc;
      if (2 * ps > p.act_stride) continue;                                  // the observation stages live in act
      if (panel_rows * kc > kVpPanelRegs * kVpThreads || rows * kc > kVpObsRegs * kVpThreads) continue;
      at = 0;
      p.act = take(static_cast<size_t>(rows) * p.act_stride);
      p.logits = take(static_cast<size_t>(rows) * p.logits_stride);
      for (int b = 0; b < 2; ++b) p.panel[b] = take(static_cast<size_t>(panel_rows) * ps);
      p.vpart = take(static_cast<size_t>(kVpWaveCols) * rows);
      p.vals = take(rows);
      if (at * sizeof(float) > lds_limit_bytes) continue;
      p.xstage[0] = p.act; p.xstage[1] = p.act + rows * ps;
      p.rows = rows; p.mr = mr; p.nc = nc; p.kc = kc; p.panel_stride = ps; p.panel_rows = panel_rows;
      p.lds_bytes = at * sizeof(float);
      p.ok = true;
      return p;
    }
  }
  return refuse("32 rows of the network's activations and logits and two weight panels do not fit a workgroup's LDS");
}

}  // namespace osg_vpnet
