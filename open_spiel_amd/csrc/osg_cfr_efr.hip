// Extensive-form regret minimization on the flattened tree (EFRSolver, open_spiel/python/algorithms/efr.py; Morrill et
// al. 2021).  The current policy lives in the `cur` table, the reach-weighted cumulative policy in `cum` (so every
// accessor and the evaluation read them as they read CFR's), the regret table is not touched: the regrets are per
// (infostate, deviation) and live in EfrPlan::state with the carried y values.  One iteration (osg_efr.h has the
// arithmetic of every item and states every sum's order):
//   values    a lane per history of one tree level, deepest level first: every player's return under the current policy
//   reach     a lane per member history: its reaches from the root path, whether the reference's walk enters it
//   cumulate  a lane per infostate: the cumulative policy, and whether any member was entered
//   regrets   a lane per (infostate, deviation): k_efr_regrets adds the members' terms to R
//   policy    a lane per infostate of one own-decision depth, shallowest first: y by swap key, regret matching with the
//             small SVD, a row per member history and the infostate's row (k_efr_policy)
// Levels form: a launch per phase, tree level and depth (any tree: 3-player leduc).  Resident form (k_efr_resident): ONE
// launch runs all iterations of a call in one workgroup, a workgroup barrier where the levels form has a launch
// boundary; the tables stay in global memory (one workgroup's traffic sits in L2).  Both forms run the same functions on
// the same values, an item's sums in the same order: bit-identical tables.  No floating-point atomics.
#include "osg_cfr_internal.h"

namespace {

constexpr int kEfrThreads = 256;
constexpr int kEfrResidentThreads = 1024;
constexpr int kEfrResidentMaxHistories = 4096;   // above: the levels form.  Measured (profiles/efr_probe.txt): one workgroup wins
                                                   // on kuhn_poker (58 histories) by 1.2x to 1.7x and loses on leduc_poker (9 457) by 1.1x to 1.35x

__global__ void __launch_bounds__(kEfrThreads) k_efr_values(EfrTree t, EfrState s, int level) {
  const int h = t.level_off[level] + blockIdx.x * blockDim.x + threadIdx.x;
  if (h < t.level_off[level + 1]) efr_value_item(t, s, h);
}

__global__ void __launch_bounds__(kEfrThreads) k_efr_reach(EfrTree t, EfrState s) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < t.M) efr_reach_item(t, s, m);
}

__global__ void __launch_bounds__(kEfrThreads) k_efr_cumulate(EfrTree t, EfrState s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < t.I) efr_cumulate_item(t, s, i);
}

__global__ void __launch_bounds__(kEfrThreads) k_efr_regrets(EfrTree t, EfrState s) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k < t.Dtot) efr_regret_item(t, s, k);
}

__global__ void __launch_bounds__(kEfrThreads) k_efr_policy(EfrTree t, EfrState s, int depth) {
  const int k = t.depth_off[depth] + blockIdx.x * blockDim.x + threadIdx.x;
  if (k < t.depth_off[depth + 1]) efr_policy_item(t, s, t.depth_info[k]);
}

__global__ void __launch_bounds__(kEfrResidentThreads) k_efr_resident(EfrTree t, EfrState s, int iters) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int it = 0; it < iters; ++it) {
    for (int l = t.D - 1; l >= 0; --l) {
      for (int h = t.level_off[l] + tid; h < t.level_off[l + 1]; h += nt) efr_value_item(t, s, h);
      __syncthreads();
    }
    for (int m = tid; m < t.M; m += nt) efr_reach_item(t, s, m);
    __syncthreads();
    for (int i = tid; i < t.I; i += nt) efr_cumulate_item(t, s, i);
    for (int64_t k = tid; k < t.Dtot; k += nt) efr_regret_item(t, s, k);
    __syncthreads();
    for (int d = 0; d < t.ND; ++d) {
      for (int k = t.depth_off[d] + tid; k < t.depth_off[d + 1]; k += nt) efr_policy_item(t, s, t.depth_info[k]);
      __syncthreads();
    }
  }
}

unsigned efr_blocks(int64_t n) { return static_cast<unsigned>((std::max<int64_t>(n, 1) + kEfrThreads - 1) / kEfrThreads); }

EfrTree efr_tree(const osg_cfr* s) {
  const EfrPlan& p = s->efr;
  EfrTree t;
  t.H = s->H; t.I = s->I; t.A = s->A; t.P = s->P; t.D = s->D; t.M = static_cast<int>(s->mem.size());
  t.L = p.tables.L; t.ND = p.tables.ND; t.external_only = efr_external_only(p.tables.type) ? 1 : 0;
  t.Dtot = static_cast<int64_t>(p.tables.dev_info.size());
  t.level_off = s->d_level_off; t.first_child = s->d_first_child; t.kind = s->d_kind; t.nchild = s->d_nchild;
  t.actor = s->d_actor; t.info = s->d_info; t.edge_prob = s->d_edge_prob; t.term_ret = s->d_term_ret;
  t.mem_off = s->d_mem_off; t.mem = s->d_mem; t.nact = s->d_nact; t.info_player = s->d_info_player;
  t.path_off = s->d_path_off; t.path = s->d_path;
  t.dev_off = p.dev_off; t.dev_info = p.dev_info; t.dev_desc = p.dev_desc; t.dev_cols = p.dev_cols;
  t.nkeys = p.nkeys; t.key_desc = p.key_desc; t.own_len = p.own_len; t.own_info = p.own_info; t.mown = p.mown;
  t.depth_off = p.depth_off; t.depth_info = p.depth_info;
  return t;
}

EfrState efr_state(const osg_cfr* s) {
  const EfrPlan& p = s->efr;
  const size_t M = s->mem.size();
  EfrState st;
  st.pol = s->cur(); st.cum = s->cum();
  st.R = p.state; st.y = p.state + p.tables.dev_info.size();
  st.value = s->d_value;
  st.mcf = p.work; st.mown = p.work + M; st.mpol = p.work + 2 * M;
  st.live = p.flags; st.visited = p.flags + M;
  return st;
}

// What every EFR entry point needs of the solver.
int efr_refusal(const osg_cfr* s, const char* who) {
  const std::string w = who;
  if (s->cfg.solver != 0) return set_error(OSG_ERR_INVALID, w + ": needs a CFRSolverBase table (solver 0), not an MCCFR solver");
  if (s->dcfr) return set_error(OSG_ERR_INVALID, w + ": EFR has no discounting, this solver discounts (osg_cfr_set_discounting)");
  if (mmd_mode(s)) return set_error(OSG_ERR_INVALID, w + ": the solver is in mirror-descent mode (osg_mmd_set_params)");
  if (s->B > 1) return set_error(OSG_ERR_UNSUPPORTED, w + ": one solver per object (replicas > 1 are not served)");
  if (!s->path_kernel || s->P > kEfrMaxPlayers) return set_error(OSG_ERR_UNSUPPORTED, w + ": the tree's root paths are not indexable");
  // leduc_poker(action_mapping=True): "fold" where there is nothing to call is "call" and leads to the same information
  // state, so an information state has no single own history for a deviation to remember, and the reference's run cannot
  // be pinned (the regrets between the two tied moves are rounding noise that its max(0, R) then decides on)
  if (s->spec.desc.game_kind == kLeduc && s->spec.leduc.mapping)
    return set_error(OSG_ERR_UNSUPPORTED, w + ": leduc_poker with action_mapping=True gives an information state several own histories (fold "
                                              "and call lead to the same one); EFR serves action_mapping=False");
  if (s->A > kEfrMaxA) return set_error(OSG_ERR_UNSUPPORTED, w + ": a policy row wider than " + std::to_string(kEfrMaxA) + " actions");
  return cfr_sub_error(s);
}

bool efr_takes_the_resident_form(const osg_cfr* s) {
  return s->efr.form == 1 || (s->efr.form == 0 && s->H <= kEfrResidentMaxHistories);
}

int efr_zero_state(osg_cfr* s) {
  hipStream_t st = s->ctx->stream;
  OSG_HIP(hipMemsetAsync(s->efr.state, 0, sizeof(double) * s->efr.state_doubles(s->I), st));
  OSG_HIP(hipStreamSynchronize(st));
  return OSG_OK;
}

}  // namespace

namespace osg_cfr_impl {

bool efr_mode(const osg_cfr* s) { return s->efr.active; }

int efr_after_reset(osg_cfr* s) { return efr_zero_state(s); }

}  // namespace osg_cfr_impl

extern "C" {

int osg_efr_set_deviations(osg_cfr* s, int type, int form) {
  if (!s) return set_error(OSG_ERR_INVALID, "osg_efr_set_deviations: null argument");
  if (int rc = efr_refusal(s, "osg_efr_set_deviations")) return rc;
  if (type < 0 || type >= kEfrTypes) return set_error(OSG_ERR_INVALID, "osg_efr_set_deviations: no deviation set " + std::to_string(type));
  if (form < 0 || form > 2) return set_error(OSG_ERR_INVALID, "osg_efr_set_deviations: form must be 0 (by tree size), 1 (resident) or 2 (levels)");
  EfrHostTree ht;
  ht.H = s->H; ht.I = s->I; ht.A = s->A;
  ht.parent = s->parent.data(); ht.kind = s->kind.data(); ht.actor = s->actor.data(); ht.info = s->info.data();
  ht.aidx = s->aidx.data(); ht.mem_off = s->mem_off.data(); ht.mem = s->mem.data(); ht.mem_index = s->mem_index.data();
  ht.nact = s->nact.data(); ht.legal = s->legal.data(); ht.info_player = s->info_player.data();
  EfrTables built;
  const std::string why = efr_build_tables(ht, type, &built);
  if (!why.empty()) return set_error(OSG_ERR_UNSUPPORTED, "osg_efr_set_deviations: " + why);
  hipStream_t st = s->ctx->stream;
  OSG_HIP(hipStreamSynchronize(st));   // (an earlier launch may still read the tables this call replaces)
  EfrPlan& p = s->efr;
  p.active = false;
  p.tables = std::move(built);
  p.form = form;
  const EfrTables& T = p.tables;
  int rc;
  if ((rc = upload(T.dev_off, p.dev_off, st)) || (rc = upload(T.dev_info, p.dev_info, st)) || (rc = upload(T.dev_desc, p.dev_desc, st)) ||
      (rc = upload(T.dev_cols, p.dev_cols, st)) || (rc = upload(T.nkeys, p.nkeys, st)) || (rc = upload(T.key_desc, p.key_desc, st)) ||
      (rc = upload(T.own_len, p.own_len, st)) || (rc = upload(T.own_info, p.own_info, st)) || (rc = upload(T.mown, p.mown, st)) ||
      (rc = upload(T.depth_off, p.depth_off, st)) || (rc = upload(T.depth_info, p.depth_info, st)))
    return rc;
  const size_t M = s->mem.size();
  OSG_HIP(p.state.alloc(p.state_doubles(s->I)));
  OSG_HIP(p.work.alloc(2 * M + M * s->A));
  OSG_HIP(p.flags.alloc(M + s->I));
  OSG_HIP(hipMemsetAsync(p.work, 0, sizeof(double) * (2 * M + M * s->A), st));
  OSG_HIP(hipMemsetAsync(p.flags, 0, sizeof(int32_t) * (M + s->I), st));
  OSG_HIP(hipStreamSynchronize(st));
  if ((rc = osg_cfr_reset(s))) return rc;   // uniform policy, empty cumulative policy
  if ((rc = efr_zero_state(s))) return rc;
  s->iteration = 0;
  p.active = true;
  return OSG_OK;
}

int osg_efr_iterate(osg_cfr* s, int iters) {
  if (!s || iters < 0) return set_error(OSG_ERR_INVALID, "osg_efr_iterate: bad argument");
  if (int rc = efr_refusal(s, "osg_efr_iterate")) return rc;
  if (!efr_mode(s)) return set_error(OSG_ERR_INVALID, "osg_efr_iterate: no deviation set yet (osg_efr_set_deviations comes first)");
  if (iters == 0) return OSG_OK;
  hipStream_t st = s->ctx->stream;
  const EfrTree t = efr_tree(s);
  const EfrState es = efr_state(s);
  if (efr_takes_the_resident_form(s)) {
    k_efr_resident<<<dim3(1), dim3(kEfrResidentThreads), 0, st>>>(t, es, iters);
    OSG_HIP(hipGetLastError());
    s->iteration += iters;
    s->last_kernel = "k_efr_resident";
    return OSG_OK;
  }
  const EfrTables& T = s->efr.tables;
  for (int it = 0; it < iters; ++it) {
    for (int l = s->D - 1; l >= 0; --l)
      k_efr_values<<<dim3(efr_blocks(s->level_off[l + 1] - s->level_off[l])), dim3(kEfrThreads), 0, st>>>(t, es, l);
    k_efr_reach<<<dim3(efr_blocks(t.M)), dim3(kEfrThreads), 0, st>>>(t, es);
    k_efr_cumulate<<<dim3(efr_blocks(t.I)), dim3(kEfrThreads), 0, st>>>(t, es);
    k_efr_regrets<<<dim3(efr_blocks(t.Dtot)), dim3(kEfrThreads), 0, st>>>(t, es);
    for (int d = 0; d < T.ND; ++d)
      k_efr_policy<<<dim3(efr_blocks(T.depth_off[d + 1] - T.depth_off[d])), dim3(kEfrThreads), 0, st>>>(t, es, d);
    ++s->iteration;
  }
  OSG_HIP(hipGetLastError());
  s->last_kernel = "k_efr";
  return OSG_OK;
}

int osg_efr_sizes(const osg_cfr* s, int64_t* out) {
  if (!s || !out) return set_error(OSG_ERR_INVALID, "osg_efr_sizes: null argument");
  if (!efr_mode(s)) return set_error(OSG_ERR_INVALID, "osg_efr_sizes: no deviation set yet (osg_efr_set_deviations comes first)");
  const EfrTables& T = s->efr.tables;
  out[0] = static_cast<int64_t>(T.dev_info.size());
  out[1] = T.max_per_info;
  out[2] = T.L;
  out[3] = static_cast<int64_t>(s->efr.state_doubles(s->I));
  out[4] = T.ND;
  return OSG_OK;
}

int osg_efr_deviations(const osg_cfr* s, int32_t* dev_off, int8_t* target, int8_t* source, int8_t* weights_none, int8_t* weights,
                       int8_t* memory, int32_t* y_slot, int32_t* cells) {
  if (!s) return set_error(OSG_ERR_INVALID, "osg_efr_deviations: null argument");
  if (!efr_mode(s)) return set_error(OSG_ERR_INVALID, "osg_efr_deviations: no deviation set yet (osg_efr_set_deviations comes first)");
  const EfrTables& T = s->efr.tables;
  const size_t D = T.dev_info.size(), L = static_cast<size_t>(T.L);
  if (dev_off) std::copy(T.dev_off.begin(), T.dev_off.end(), dev_off);
  for (size_t k = 0; k < D; ++k) {
    const int desc = T.dev_desc[k];
    if (target) target[k] = static_cast<int8_t>(desc & 0xF);
    if (source) source[k] = static_cast<int8_t>(((desc >> 4) & 0xF) - 1);
    if (weights_none) weights_none[k] = T.dev_none[k];
    if (y_slot) y_slot[k] = (desc >> 8) & 0xFF;
    for (size_t j = 0; j < L; ++j) {
      if (weights) weights[k * L + j] = T.dev_weight[k * L + j];
      if (memory) memory[k * L + j] = T.dev_memory[k * L + j];
      if (!cells) continue;
      const unsigned col = (T.dev_cols[k] >> (4 * j)) & 0xF;
      const bool remembered = ((desc >> (16 + j)) & 1) != 0;
      cells[k * L + j] = !remembered ? -1 : (col == kEfrZeroCol ? -2 : T.own_info[static_cast<size_t>(T.dev_info[k]) * L + j] * s->A + static_cast<int>(col));
    }
  }
  return OSG_OK;
}

int osg_efr_regrets(osg_cfr* s, double* h_state) {
  if (!s || !h_state) return set_error(OSG_ERR_INVALID, "osg_efr_regrets: null argument");
  if (!efr_mode(s)) return set_error(OSG_ERR_INVALID, "osg_efr_regrets: no deviation set yet (osg_efr_set_deviations comes first)");
  hipStream_t st = s->ctx->stream;
  OSG_HIP(hipMemcpyAsync(h_state, s->efr.state, sizeof(double) * s->efr.state_doubles(s->I), hipMemcpyDeviceToHost, st));
  OSG_HIP(hipStreamSynchronize(st));
  return OSG_OK;
}

int osg_efr_upload_regrets(osg_cfr* s, const double* h_state) {
  if (!s || !h_state) return set_error(OSG_ERR_INVALID, "osg_efr_upload_regrets: null argument");
  if (!efr_mode(s)) return set_error(OSG_ERR_INVALID, "osg_efr_upload_regrets: no deviation set yet (osg_efr_set_deviations comes first)");
  hipStream_t st = s->ctx->stream;
  OSG_HIP(hipMemcpyAsync(s->efr.state, h_state, sizeof(double) * s->efr.state_doubles(s->I), hipMemcpyHostToDevice, st));
  OSG_HIP(hipStreamSynchronize(st));
  return OSG_OK;
}

}  // extern "C"
