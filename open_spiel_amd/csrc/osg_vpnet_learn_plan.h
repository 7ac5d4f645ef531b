// The fused learner of the policy-value MLP (k_vpnet_learn, osg_vpnet_learn.hip), planned on the host: plain C++, no
// device call, no environment switch.  tests/native/vpnet_learn_plan_host_test.cpp includes this header alone.
//
// A GROUP of G workgroups of 8 wavefronts trains one network, data-parallel over the batch (the wide Deep CFR learner's
// split, osg_adam_wide_plan.h): workgroup g owns rows [g R, (g + 1) R) of every update's batch, writes its gradient of
// every parameter to partial[g], the group meets, workgroup g adds the G partials of its slice in ascending order and
// takes the Adam step, and the group meets again.
//
//   R, G      R = 32 for every shape: the wavefront grid of osg_vpnet_plan.h (2 over the rows x 4 over the columns) at
//             MR = 1, NC = 8.  A group is at most 32 workgroups of a device with 256 compute units, so an update takes
//             as long as ONE workgroup takes, and that falls with R until the grid has no rows left to give up; the
//             weights a workgroup streams per update do not depend on R.  G = ceil(B / 32), a pure function of the batch.
//   forward   as k_vpnet_forward: ONE activation buffer [32, W16 + 4] that every layer overwrites in place, the weights
//             through two panel buffers of KC input columns by all the output rows (KC the largest of 16, 8, 4 with
//             rows KC <= 4096, the threads' fetch registers).
//   saved     backward needs every torso output and the value head's hidden layer.  NONE of them stays in LDS: with the
//             widest network (W = 512: 66 KB per buffer, 32 KB of panels, 17 KB of logits) a second buffer does not fit
//             the 160 KB, and one placement for every shape keeps one order of every sum.  Each is written once on the
//             way forward to the workgroup's slots [depth + 3][32, W16] of the job's scratch in global memory (L2: 64 KB a
//             slot at W = 512) and read on the way back: as the batch-side operand of dW = dY^T X, which streams X from
//             there exactly as layer 0 streams the observations, and as the ReLU's mask.  The policy head's hidden
//             layer is the exception: it is still in the activation buffer when its gradient is formed.
//   backward  the activation buffer holds dY of the layer at hand.  dX = dY W contracts over W's ROWS: the weights come
//             through the same two panel buffers as KB whole rows of W ([KB, W16], KB = 16 where 16 W16 <= 4096, the
//             threads' fetch registers, else 8), read in the other orientation — no transposed copy anywhere.  The output [32, W16]
//             stays in the accumulators, then overwrites the buffer through the mask.
//   strides   activation and logit rows: 4 mod 16, the argument of osg_vpnet_plan.h (operand element (row i, column
//             k + g) of lane 16 g + i: 64 banks) — it also serves dY as the A operand of dX.  A backward panel's rows
//             have a stride that is 16 mod 64: lane 16 g + i reads (row k + g, column c + i), bank (16 (k + g) + c + i)
//             mod 64: four windows of 16, 64 different banks.  dW reads dY batch-wise, four rows of a step four apart
//             (osg_mlp_plan.h's argument: 16 g (4 q + 1) + i).
//   scratch   [64 counter words | partial [G][partial_stride] | saved [G][depth + 3][32 W16]], partial_stride =
//             parameters + 8 loss words (policy sum, value sum, sum of w^2 of the slice; twice, by the update's parity)
//             padded to 4.
//   slices    workgroup g owns parameters [g slice, min((g + 1) slice, P)), slice = ceil(P / G).
#pragma once
#include "osg_vpnet_plan.h"

namespace osg_vpnet {

constexpr int kVlRows = 32;             // R
constexpr int kVlMaxBatch = 1024;
constexpr int kVlBarrierWords = 64;     // [0] arrivals, [1] a workgroup gave up; 256 bytes
constexpr int kVlLossWords = 8;         // per workgroup after its partial gradient: {policy, value, w^2, spare} x parity
constexpr int kVlRowWords = 4;          // per row in LDS: dLoss/dy of the value head, policy loss term, value loss term, spare

struct VpLearnPlan {
  bool ok = false;
  const char* why = nullptr;
  VpPlan f;                              // the forward's fields at R = 32: the shared tile code reads them
  int batch = 0, group = 0;              // B, G
  int kb = 0, bstride = 0;               // backward panels: KB rows of W, row stride
  int row_words = 0, red = 0;            // [R][kVlRowWords]; [16] reduction and flag words
  int slots = 0, slot_floats = 0;        // saved activations per workgroup: torso 0 .. depth, value hidden, the policy head's dT
  int partial_stride = 0, slice = 0;
  size_t scratch_partial = 0, scratch_saved = 0, scratch_bytes = 0;   // byte offsets of the two regions; the total
};

inline VpLearnPlan plan_vpnet_learn(const VpShape& s, int batch, size_t lds_limit_bytes) {
  VpLearnPlan L;
  VpPlan& p = L.f;
  const auto refuse = [&L](const char* why) { L.ok = false; L.why = why; return L; };
  if (s.obs < 1 || s.obs > kVpMaxObs) return refuse("observations of 1 to 2048 floats are served");
  if (s.width < 1 || s.width > kVpMaxWidth) return refuse("an nn_width of 1 to 512 is served");
  if (s.depth < 0 || s.depth > kVpMaxDepth) return refuse("an nn_depth of 0 to 8 is served");
  if (s.actions < 1 || s.actions > kVpMaxActions) return refuse("1 to 384 actions are served");
  if (batch < 1 || batch > kVlMaxBatch) return refuse("a batch of 1 to 1024 rows is served");
  p.obs = s.obs; p.width = s.width; p.depth = s.depth; p.actions = s.actions;
  p.wp = vp_pad(s.width); p.ap = vp_pad(s.actions);
  vp_param_offsets(p);
  p.rows = kVlRows; p.mr = 1; p.nc = 8;
  p.act_stride = p.wp + 4;
  p.logits_stride = p.ap + 4;
  const int widest = p.wp > p.ap ? p.wp : p.ap;
  p.panel_rows = widest;                 // (at most 512 = 64 NC: one pass per layer)
  L.batch = batch;
  L.group = (batch + kVlRows - 1) / kVlRows;
  L.kb = p.wp * 16 <= kVpPanelRegs * kVpThreads ? 16 : 8;   // divides 16: a contraction never runs past the padded rows
  L.bstride = p.wp + (16 + 64 - p.wp % 64) % 64;
  L.slots = s.depth + 3;
  L.slot_floats = kVlRows * p.wp;
  L.partial_stride = (p.param_count + kVlLossWords + 3) / 4 * 4;
  L.slice = (p.param_count + L.group - 1) / L.group;
  L.scratch_partial = kVlBarrierWords * sizeof(unsigned int);
  L.scratch_saved = (L.scratch_partial + static_cast<size_t>(L.group) * L.partial_stride * sizeof(float) + 255) / 256 * 256;
  L.scratch_bytes = (L.scratch_saved + static_cast<size_t>(L.group) * L.slots * L.slot_floats * sizeof(float) + 255) / 256 * 256;
  size_t at = 0;
  const auto take = [&at](size_t floats) { const size_t o = at; at += (floats + 3) / 4 * 4; return static_cast<int>(o); };
  for (int kc = 16; kc >= 4; kc /= 2) {
    if (2 * kc > p.act_stride) continue;                                     // the observation stages live in act
    if (p.panel_rows * kc > kVpPanelRegs * kVpThreads) continue;
    const size_t forward = static_cast<size_t>(p.panel_rows) * kc, backward = static_cast<size_t>(L.kb) * L.bstride;
    at = 0;
    p.act = take(static_cast<size_t>(kVlRows) * p.act_stride);
    p.logits = take(static_cast<size_t>(kVlRows) * p.logits_stride);
    for (int b = 0; b < 2; ++b) p.panel[b] = take(forward > backward ? forward : backward);
    p.vpart = take(static_cast<size_t>(kVpWaveCols) * kVlRows);
    p.vals = take(kVlRows);
    L.row_words = take(static_cast<size_t>(kVlRows) * kVlRowWords);
    L.red = take(16);
    if (at * sizeof(float) > lds_limit_bytes) continue;
    p.xstage[0] = p.act; p.xstage[1] = p.act + kVlRows * kc;
    p.kc = kc; p.panel_stride = kc;
    p.lds_bytes = at * sizeof(float);
    p.ok = L.ok = true;
    return L;
  }
  return refuse("32 rows of the network's activations and logits and two weight panels do not fit a workgroup's LDS");
}

}  // namespace osg_vpnet
