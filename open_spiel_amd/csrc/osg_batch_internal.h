// Shared declarations of the batch translation units: the batched State kernels for the five games and the C-ABI
// around them, one unit per kernel family.
//
//   osg_context.hip      (no kernels)                               osg_ctx_*, osg_ctx_scratch, ctx_grow, ctx_retain / ctx_release
//   osg_batch.hip        k_init, k_copy16, k_gather, k_legal_mask,  osg_batch_*, osg_copy_bytes, osg_legal_mask, osg_apply,
//                        k_apply, k_status, k_chance_probs,         osg_status_query, osg_chance_probs
//                        k_set_cells
//   osg_step.hip         k_step, k_step_vec, k_step_hexvec,         osg_step (the fused step)
//                        k_step_c4x2, k_step_c4std, k_step_c4std2
//   osg_observation.hip  k_observation*, the piece functors         osg_observation (observation / information-state tensors)
//   osg_playout.hip      k_random_steps, k_fold_counters, k_synth,  osg_random_steps, osg_synth_batch, osg_rollout
//                        k_rollout, k_rollout_fold, k_rollout_hexfill
//   osg_env_step.hip     k_env_step, k_env_step_x2,                 osg_env_step, osg_env_step_compact
//                        k_env_step_compact, k_env_step_compact_x2
//
// Every kernel is launched from the unit that defines it.  Here is only what more than one unit needs; the context and
// the batch themselves (struct osg_ctx, struct osg_batch, for_game) are in osg_internal.h.
//
// Data layout in HBM: struct-of-arrays.  A batch of n states of a game with W
// words per state is ONE allocation of W planes of n elements (u32 or u64);
// lane i of a wavefront touches element i of every plane, so each plane access
// is a fully coalesced 256-512 B transaction per wave.  All kernels are
// HBM-bound byte/integer work: no MFMA, no LDS needed for the pure step path
// (the state lives in VGPRs between load and store).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <type_traits>

#include "osg_internal.h"

using namespace osg;

namespace {

constexpr int kBlock = 256;  // 4 wavefronts
inline int grid_for(int64_t n) { return static_cast<int>((n + kBlock - 1) / kBlock); }

// The partial counter slots of k_random_steps (osg_playout.hip); the context allocates them behind its illegal-apply
// counter (osg_context.hip).
constexpr int kCounterSlots = 64;

inline bool same_game(const osg_batch* a, const osg_batch* b) {
  return strcmp(a->spec.desc.canonical, b->spec.desc.canonical) == 0 &&
         a->spec.desc.state_words == b->spec.desc.state_words;
}

}  // namespace

namespace osg {
// Reads and clears the context's counter of illegal applies (osg_context.hip): into *h_illegal, or, without one, as
// OSG_ERR_ILLEGAL when it is not zero.
int check_illegal(osg_ctx* ctx, int64_t* h_illegal);
}  // namespace osg
