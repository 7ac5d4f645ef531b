// Magnetic mirror descent on the flattened tree (MMDDilatedEnt, open_spiel/python/algorithms/mmd_dilated.py:132-366;
// Sokota et al. 2023).  The behavioural policy pi lives in the `cur` table, the average sequences avg_x in the `cum`
// table (row-normalised they are the average policy, which is what osg_cfr_tables / osg_cfr_evaluate_policy make of a
// cumulative-policy table), the regret table is not touched.  One update_sequences():
//   level   a lane per infostate of one infostate level, deepest level first: the payoff gradient of its cells (each cell's
//           terminals in history-index order), the entropy gradient, the finished children's terms, the row's softmax
//           (osg_mmd.h: mmd_infostate).  It reads the OLD sequence values x and writes the new pi row.
//   commit  a lane per infostate: x of the new pi, then avg_x (mmd_sequence_row, mmd_average).
// General form (k_mmd; any two-player tree whose infostates sit on one level each): one launch of k_mmd_level per
// infostate level and one of k_mmd_commit per iteration, after one k_mmd_sequences per call (x is a function of pi, so
// a checkpoint is pi, avg_x and the counter).  Resident form (k_mmd_small): ONE launch runs all iterations of a call,
// one workgroup per replica with pi, x, avg_x and the children's terms in LDS and a workgroup barrier where the
// general form has a launch boundary; the static tree arrays are read-only and stay in L2.  Both forms run the same
// functions on the same values in the same order: bit-identical tables.  No floating-point atomics anywhere.
#include "osg_cfr_internal.h"
#include "osg_mmd.h"

namespace osg_cfr_impl {

struct MmdState {
  std::vector<int32_t> lvl_off, lvl_info, own_off, own, child_off, child, term_off, term_opp;
  std::vector<double> term_cu;
  int L = 0, max_level = 0;
  double max_abs_payoff = 0.0;
  DeviceArray<int32_t> d_lvl_off, d_lvl_info, d_own_off, d_own, d_child_off, d_child, d_term_off, d_term_opp;
  DeviceArray<double> d_term_cu;
  DeviceArray<double> d_work;   // x [IA] | dot [I] | neg_ent [I] | pi_br [IA] | x_br [IA] | part_a [IA + 1] | part_b [IA + 1] | dgf [I] | dgf_br [I] | gap [1]
  DeviceArray<double> d_par;    // [B, 2] alpha, stepsize of every replica
  std::vector<double> par;    // the same on the host
  bool active = false;        // osg_mmd_set_params was accepted: the solver is in MMD mode
};

}  // namespace osg_cfr_impl

// (here, where MmdState is complete, for the unique_ptr that holds it)
osg_cfr::osg_cfr() = default;
osg_cfr::~osg_cfr() = default;

namespace {

constexpr int kMmdThreads = 256;
// Dynamic LDS of k_mmd_small.  A CU has 160 KiB and one workgroup may take all of it; 128 KiB leaves the rest to whatever
// else is resident.  kuhn_poker asks for 0.8 KiB (many workgroups per CU: the replicas), leduc_poker for 80.4 KiB.
constexpr size_t kMmdLdsLimit = 128 * 1024;

struct MmdWork {
  double *x, *dot, *neg_ent, *pi_br, *x_br, *part_a, *part_b, *dgf, *dgf_br, *gap;
};
MmdWork mmd_work(double* base, int I, int A) {
  const size_t IA = static_cast<size_t>(I) * A;
  MmdWork w;
  w.x = base; w.dot = w.x + IA; w.neg_ent = w.dot + I; w.pi_br = w.neg_ent + I; w.x_br = w.pi_br + IA;
  w.part_a = w.x_br + IA; w.part_b = w.part_a + IA + 1; w.dgf = w.part_b + IA + 1; w.dgf_br = w.dgf + I; w.gap = w.dgf_br + I;
  return w;
}
size_t mmd_work_doubles(int I, int A) { return 5 * static_cast<size_t>(I) * A + 4 * static_cast<size_t>(I) + 3; }

// x [I, A] of the policy table pi
__global__ void __launch_bounds__(kMmdThreads) k_mmd_sequences(MmdTree t, const double* __restrict__ pi, double* __restrict__ x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < t.I) mmd_sequence_row(t, i, pi, x);
}

// The start state of every replica (mmd_dilated.py:174-175): avg_x = x of its current-policy table.  blockIdx.x = replica.
__global__ void __launch_bounds__(kMmdThreads) k_mmd_start(MmdTree t, double* tables, size_t replica_stride) {
  const int i = blockIdx.y * blockDim.x + threadIdx.x;
  if (i >= t.I) return;
  double* cum = tables + blockIdx.x * replica_stride + static_cast<size_t>(t.I) * t.A;   // regrets | cum | cur | ...
  for (int a = t.nact[i]; a < t.A; ++a) cum[i * t.A + a] = 0.0;
  mmd_sequence_row(t, i, cum + static_cast<size_t>(t.I) * t.A, cum);
}

// the infostates of level l
__global__ void __launch_bounds__(kMmdThreads)
k_mmd_level(MmdTree t, int l, const double* __restrict__ x, const double* __restrict__ par, double* pi, double* dot, double* neg_ent) {
  const int k = t.lvl_off[l] + blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= t.lvl_off[l + 1]) return;
  mmd_infostate(t, t.lvl_info[k], x, par[1], par[0], false, pi, dot, neg_ent);
}

__global__ void __launch_bounds__(kMmdThreads)
k_mmd_commit(MmdTree t, const double* __restrict__ pi, double* __restrict__ x, double* __restrict__ avg, double k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.I) return;
  mmd_sequence_row(t, i, pi, x);
  for (int a = 0; a < t.nact[i]; ++a) avg[i * t.A + a] = mmd_average(avg[i * t.A + a], x[i * t.A + a], k);
}

// All iterations of a call in one launch: workgroup b advances replica b with its own (alpha, stepsize).
// Dynamic LDS: pi [IA] | x [IA] | avg_x [IA] | dot [I] | neg_ent [I].
__global__ void __launch_bounds__(1024)
k_mmd_small(MmdTree t, double* tables, size_t replica_stride, const double* __restrict__ par, int iteration0, int iters) {
  extern __shared__ __attribute__((aligned(16))) double mmd_smem[];
  const int IA = t.I * t.A;
  double* pi = mmd_smem;
  double* x = pi + IA;
  double* avg = x + IA;
  double* dot = avg + IA;
  double* neg_ent = dot + t.I;
  double* cum_global = tables + blockIdx.x * replica_stride + IA;   // regrets | cum | cur | ...
  double* cur_global = cum_global + IA;
  const double alpha = par[2 * blockIdx.x], eta = par[2 * blockIdx.x + 1];
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int c = tid; c < IA; c += nt) {
    pi[c] = cur_global[c];
    avg[c] = cum_global[c];
    x[c] = 0.0;
  }
  __syncthreads();
  for (int i = tid; i < t.I; i += nt) mmd_sequence_row(t, i, pi, x);
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    for (int l = 0; l < t.L; ++l) {
      for (int k = t.lvl_off[l] + tid; k < t.lvl_off[l + 1]; k += nt) mmd_infostate(t, t.lvl_info[k], x, eta, alpha, false, pi, dot, neg_ent);
      __syncthreads();
    }
    const double k = static_cast<double>(iteration0 + it + 2);   // iteration_count starts at 1 and is raised first
    for (int i = tid; i < t.I; i += nt) {
      mmd_sequence_row(t, i, pi, x);
      for (int a = 0; a < t.nact[i]; ++a) avg[i * t.A + a] = mmd_average(avg[i * t.A + a], x[i * t.A + a], k);
    }
    __syncthreads();
  }
  for (int c = tid; c < IA; c += nt) {
    cur_global[c] = pi[c];
    cum_global[c] = avg[c];
  }
}

// get_gap() (mmd_dilated.py:325-359) of the policy table pi by one workgroup, scratch in global memory.
__global__ void __launch_bounds__(kMmdThreads)
k_mmd_gap(MmdTree t, const int8_t* __restrict__ player, const double* __restrict__ pi, MmdWork w, double alpha) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int IA = t.I * t.A;
  for (int i = tid; i < t.I; i += nt) mmd_sequence_row(t, i, pi, w.x);
  __syncthreads();
  for (int l = 0; l < t.L; ++l) {
    for (int k = t.lvl_off[l] + tid; k < t.lvl_off[l + 1]; k += nt) mmd_infostate(t, t.lvl_info[k], w.x, 0.0, alpha, true, w.pi_br, w.dot, w.neg_ent);
    __syncthreads();
  }
  for (int i = tid; i < t.I; i += nt) mmd_sequence_row(t, i, w.pi_br, w.x_br);
  __syncthreads();
  for (int i = tid; i < t.I; i += nt) {
    w.dgf[i] = mmd_dgf_term(t, i, w.x);
    w.dgf_br[i] = mmd_dgf_term(t, i, w.x_br);
    for (int a = 0; a < t.A; ++a) {
      const int cell = i * t.A + a;
      const bool mine = player[i] == 0 && a < t.nact[i];
      w.part_a[cell] = mine ? mmd_bilinear_cell(t, cell, w.x[cell], w.x_br) : 0.0;
      w.part_b[cell] = mine ? mmd_bilinear_cell(t, cell, w.x_br[cell], w.x) : 0.0;
    }
  }
  if (tid == 0) {
    w.part_a[IA] = mmd_bilinear_cell(t, IA, 1.0, w.x_br);
    w.part_b[IA] = mmd_bilinear_cell(t, IA, 1.0, w.x);
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0, d[2] = {0.0, 0.0}, d_br[2] = {0.0, 0.0};
    for (int c = 0; c <= IA; ++c) {
      a = a + w.part_a[c];
      b = b + w.part_b[c];
    }
    for (int i = 0; i < t.I; ++i) {
      d[player[i]] = d[player[i]] + w.dgf[i];
      d_br[player[i]] = d_br[player[i]] + w.dgf_br[i];
    }
    *w.gap = mmd_gap(a, b, d, d_br, alpha);
  }
}

// The per-sequence terminal lists, the infostate children, the own-decision chains and the infostate levels, from what
// build_tree keeps.  Once per solver, at the first MMD call.
int mmd_build(osg_cfr* s) {
  if (s->mmd) return OSG_OK;
  auto built = std::make_unique<MmdState>();
  MmdState* m = built.get();
  const int I = s->I, A = s->A, IA = I * A;
  std::vector<int32_t> parent_cell(I, -1);
  m->own_off.push_back(0);
  for (int i = 0; i < I; ++i) {
    const int mem = s->mem_off[i];
    for (int e = s->path_off[mem]; e < s->path_off[mem + 1]; ++e) {
      const int code = s->path[e];
      if (((code >> 23) & 1) || ((code >> 24) & 0xF) != s->info_player[i]) continue;
      m->own.push_back(code & 0x7FFFFF);
    }
    m->own_off.push_back(static_cast<int32_t>(m->own.size()));
    if (m->own_off[i + 1] > m->own_off[i]) parent_cell[i] = m->own.back();
  }
  std::vector<std::vector<int32_t>> kids(IA);
  for (int i = 0; i < I; ++i)
    if (parent_cell[i] >= 0) kids[parent_cell[i]].push_back(i);
  m->child_off.push_back(0);
  for (int c = 0; c < IA; ++c) {
    m->child.insert(m->child.end(), kids[c].begin(), kids[c].end());
    m->child_off.push_back(static_cast<int32_t>(m->child.size()));
  }
  std::vector<int32_t> levels(s->info_level.begin(), s->info_level.end());
  std::sort(levels.begin(), levels.end());
  levels.erase(std::unique(levels.begin(), levels.end()), levels.end());
  m->lvl_off.push_back(0);
  for (auto l = levels.rbegin(); l != levels.rend(); ++l) {   // deepest first
    for (int i = 0; i < I; ++i)
      if (s->info_level[i] == *l) m->lvl_info.push_back(i);
    m->max_level = std::max(m->max_level, static_cast<int>(m->lvl_info.size()) - m->lvl_off.back());
    m->lvl_off.push_back(static_cast<int32_t>(m->lvl_info.size()));
  }
  m->L = static_cast<int>(levels.size());
  // every terminal history, ascending: both players' last sequences and chance(z), multiplied root to leaf as
  // sequence_form_utils.py:160 does (prob * chance_reach)
  struct Term { int32_t bucket[2]; double cu[2]; };
  std::vector<Term> terms;
  std::map<std::pair<int32_t, int32_t>, double> payoff;
  std::vector<int32_t> up;
  for (int h = 0; h < s->H; ++h) {
    if (s->kind[h] != kTerminalNode) continue;
    up.clear();
    for (int32_t v = h; s->parent[v] >= 0; v = s->parent[v]) up.push_back(v);
    Term t{{IA, IA + 1}, {0.0, 0.0}};
    double chance = 1.0;
    for (auto v = up.rbegin(); v != up.rend(); ++v) {
      const int32_t par = s->parent[*v];
      if (s->kind[par] == kChanceNode) chance = s->edge_prob[*v] * chance;
      else t.bucket[s->actor[par]] = s->info[par] * A + s->aidx[*v];
    }
    for (int p = 0; p < 2; ++p) t.cu[p] = s->term_ret[static_cast<size_t>(h) * s->P + p] * chance;
    payoff[{t.bucket[0], t.bucket[1]}] += t.cu[0];
    terms.push_back(t);
  }
  for (const auto& kv : payoff) m->max_abs_payoff = std::max(m->max_abs_payoff, std::fabs(kv.second));
  std::vector<int32_t> count(IA + 3, 0);
  for (const Term& t : terms)
    for (int p = 0; p < 2; ++p) ++count[t.bucket[p] + 1];
  m->term_off.assign(IA + 3, 0);
  for (int c = 0; c < IA + 2; ++c) m->term_off[c + 1] = m->term_off[c] + count[c + 1];
  m->term_opp.resize(2 * terms.size());
  m->term_cu.resize(2 * terms.size());
  std::vector<int32_t> fill(m->term_off.begin(), m->term_off.end() - 1);
  for (const Term& t : terms)
    for (int p = 0; p < 2; ++p) {
      const int at = fill[t.bucket[p]]++;
      m->term_opp[at] = t.bucket[1 - p] >= IA ? -1 : t.bucket[1 - p];
      m->term_cu[at] = t.cu[p];
    }
  hipStream_t st = s->ctx->stream;
  int rc;
  if ((rc = upload(m->lvl_off, m->d_lvl_off, st)) || (rc = upload(m->lvl_info, m->d_lvl_info, st)) ||
      (rc = upload(m->own_off, m->d_own_off, st)) || (rc = upload(m->own, m->d_own, st)) ||
      (rc = upload(m->child_off, m->d_child_off, st)) || (rc = upload(m->child, m->d_child, st)) ||
      (rc = upload(m->term_off, m->d_term_off, st)) || (rc = upload(m->term_opp, m->d_term_opp, st)) ||
      (rc = upload(m->term_cu, m->d_term_cu, st)))
    return rc;
  OSG_HIP(m->d_work.alloc(mmd_work_doubles(I, A)));
  OSG_HIP(m->d_par.alloc(2 * static_cast<size_t>(s->B)));
  OSG_HIP(hipMemsetAsync(m->d_work, 0, sizeof(double) * mmd_work_doubles(I, A), st));   // (the padding cells stay 0)
  OSG_HIP(hipStreamSynchronize(st));
  s->mmd = std::move(built);   // (whole, or not there: a failed build leaves nothing behind)
  return OSG_OK;
}

MmdTree mmd_tree(const osg_cfr* s) {
  const MmdState* m = s->mmd.get();
  MmdTree t;
  t.I = s->I; t.A = s->A; t.L = m->L;
  t.nact = s->d_nact; t.lvl_off = m->d_lvl_off; t.lvl_info = m->d_lvl_info; t.own_off = m->d_own_off; t.own = m->d_own;
  t.child_off = m->d_child_off; t.child = m->d_child; t.term_off = m->d_term_off; t.term_opp = m->d_term_opp; t.term_cu = m->d_term_cu;
  return t;
}

size_t mmd_small_lds_bytes(const osg_cfr* s) { return sizeof(double) * (3 * static_cast<size_t>(s->I) * s->A + 2 * static_cast<size_t>(s->I)); }
bool mmd_takes_the_resident_form(const osg_cfr* s) { return s->cfg.kernel == OSG_CFR_KERNEL_AUTO && mmd_small_lds_bytes(s) <= kMmdLdsLimit; }

// What every MMD entry point needs of the solver, whatever its mode.
int mmd_refusal(const osg_cfr* s, const char* who) {
  const std::string w = who;
  if (s->cfg.solver != 0) return set_error(OSG_ERR_INVALID, w + ": needs a CFRSolverBase table (solver 0), not an MCCFR solver");
  if (s->dcfr) return set_error(OSG_ERR_INVALID, w + ": mirror descent has no discounting, this solver discounts (osg_cfr_set_discounting)");
  if (s->P != 2) return set_error(OSG_ERR_UNSUPPORTED, w + ": two-player zero-sum games only, this game has " + std::to_string(s->P) + " players");
  // leduc_poker(action_mapping=True): "fold" where there is nothing to call is "call", both lead to the same information
  // state of the player who chose, so an information state has several parent sequences and the game has no sequence
  // form (the reference's mmd_dilated.py ends in log(0) = NaN there)
  if (s->spec.desc.game_kind == kLeduc && s->spec.leduc.mapping)
    return set_error(OSG_ERR_UNSUPPORTED, w + ": leduc_poker with action_mapping=True has no sequence form (fold and call lead to the same "
                                              "information state); mirror descent serves action_mapping=False");
  if (!s->eval_ok) return set_error(OSG_ERR_UNSUPPORTED, w + ": an information state spans several tree levels");
  if (s->A > kMmdMaxRow) return set_error(OSG_ERR_UNSUPPORTED, w + ": a policy row wider than " + std::to_string(kMmdMaxRow) + " actions");
  if (s->B > 1 && !mmd_takes_the_resident_form(s))
    return set_error(OSG_ERR_UNSUPPORTED, w + ": replicas > 1 need the resident form (k_mmd_small), and only the general form serves this solver");
  return cfr_sub_error(s);
}

unsigned mmd_blocks(int n) { return static_cast<unsigned>((std::max(n, 1) + kMmdThreads - 1) / kMmdThreads); }

int mmd_start_average(osg_cfr* s) {
  hipStream_t st = s->ctx->stream;
  k_mmd_start<<<dim3(static_cast<unsigned>(s->B), mmd_blocks(s->I)), dim3(kMmdThreads), 0, st>>>(mmd_tree(s), s->replica_base(0), s->replica_stride());
  OSG_HIP(hipGetLastError());
  OSG_HIP(hipStreamSynchronize(st));
  return OSG_OK;
}

}  // namespace

namespace osg_cfr_impl {

bool mmd_mode(const osg_cfr* s) { return s->mmd && s->mmd->active; }

int mmd_after_reset(osg_cfr* s) { return mmd_start_average(s); }

}  // namespace osg_cfr_impl

extern "C" {

int osg_mmd_default_stepsize(osg_cfr* s, double alpha, double* out) {
  if (!s || !out) return set_error(OSG_ERR_INVALID, "osg_mmd_default_stepsize: null argument");
  if (int rc = mmd_refusal(s, "osg_mmd_default_stepsize")) return rc;
  if (!std::isfinite(alpha) || alpha < 0.0) return set_error(OSG_ERR_INVALID, "osg_mmd_default_stepsize: alpha must be finite and >= 0");
  if (int rc = mmd_build(s)) return rc;
  *out = mmd_default_stepsize(alpha, s->mmd->max_abs_payoff);
  return OSG_OK;
}

int osg_mmd_set_params(osg_cfr* s, int n, const double* alpha, const double* stepsize) {
  if (!s || !alpha || !stepsize) return set_error(OSG_ERR_INVALID, "osg_mmd_set_params: null argument");
  if (int rc = mmd_refusal(s, "osg_mmd_set_params")) return rc;
  if (n != s->B)
    return set_error(OSG_ERR_INVALID, "osg_mmd_set_params: " + std::to_string(n) + " parameter pairs for " + std::to_string(s->B) + " replicas");
  for (int r = 0; r < n; ++r) {
    if (!std::isfinite(alpha[r]) || alpha[r] < 0.0)
      return set_error(OSG_ERR_INVALID, "osg_mmd_set_params: alpha must be finite and >= 0 (replica " + std::to_string(r) + ")");
    if (!std::isfinite(stepsize[r]) || stepsize[r] < 0.0)
      return set_error(OSG_ERR_INVALID, "osg_mmd_set_params: the stepsize must be finite and >= 0 (replica " + std::to_string(r) + ")");
  }
  if (int rc = mmd_build(s)) return rc;
  MmdState* m = s->mmd.get();
  hipStream_t st = s->ctx->stream;
  OSG_HIP(hipStreamSynchronize(st));   // (an earlier launch may still read d_par)
  m->par.resize(2 * static_cast<size_t>(n));
  for (int r = 0; r < n; ++r) {
    m->par[2 * r] = alpha[r];
    m->par[2 * r + 1] = stepsize[r];
  }
  OSG_HIP(hipMemcpyAsync(m->d_par, m->par.data(), sizeof(double) * m->par.size(), hipMemcpyHostToDevice, st));
  OSG_HIP(hipStreamSynchronize(st));
  if (!m->active) {
    if (int rc = mmd_start_average(s)) return rc;
    s->iteration = 0;
    m->active = true;
  }
  return OSG_OK;
}

int osg_mmd_iterate(osg_cfr* s, int iters) {
  if (!s || iters < 0) return set_error(OSG_ERR_INVALID, "osg_mmd_iterate: bad argument");
  if (int rc = mmd_refusal(s, "osg_mmd_iterate")) return rc;
  if (!mmd_mode(s)) return set_error(OSG_ERR_INVALID, "osg_mmd_iterate: no parameters yet (osg_mmd_set_params comes first)");
  if (iters == 0) return OSG_OK;
  const MmdState* m = s->mmd.get();
  hipStream_t st = s->ctx->stream;
  const MmdTree t = mmd_tree(s);
  if (mmd_takes_the_resident_form(s)) {
    const size_t lds = mmd_small_lds_bytes(s);
    if (raise_lds_cap(reinterpret_cast<const void*>(&k_mmd_small), static_cast<int>(lds)) != hipSuccess) {
      (void)hipGetLastError();
      return set_error(OSG_ERR_HIP, "osg_mmd_iterate: the resident kernel's LDS request was refused");
    }
    const int threads = std::max(64, std::min(((m->max_level + 63) / 64) * 64, 1024));
    k_mmd_small<<<dim3(static_cast<unsigned>(s->B)), dim3(threads), lds, st>>>(t, s->replica_base(0), s->replica_stride(), m->d_par,
                                                                               s->iteration, iters);
    OSG_HIP(hipGetLastError());
    s->iteration += iters;
    s->last_kernel = "k_mmd_small";
    return OSG_OK;
  }
  const MmdWork w = mmd_work(m->d_work, s->I, s->A);
  k_mmd_sequences<<<dim3(mmd_blocks(s->I)), dim3(kMmdThreads), 0, st>>>(t, s->cur(), w.x);
  for (int it = 0; it < iters; ++it) {
    for (int l = 0; l < m->L; ++l)
      k_mmd_level<<<dim3(mmd_blocks(m->lvl_off[l + 1] - m->lvl_off[l])), dim3(kMmdThreads), 0, st>>>(t, l, w.x, m->d_par, s->cur(), w.dot, w.neg_ent);
    ++s->iteration;
    k_mmd_commit<<<dim3(mmd_blocks(s->I)), dim3(kMmdThreads), 0, st>>>(t, s->cur(), w.x, s->cum(), static_cast<double>(s->iteration + 1));
  }
  OSG_HIP(hipGetLastError());
  s->last_kernel = "k_mmd";
  return OSG_OK;
}

int osg_mmd_gap(osg_cfr* s, double* out) {
  if (!s || !out) return set_error(OSG_ERR_INVALID, "osg_mmd_gap: null argument");
  if (int rc = mmd_refusal(s, "osg_mmd_gap")) return rc;
  if (!mmd_mode(s)) return set_error(OSG_ERR_INVALID, "osg_mmd_gap: no parameters yet (osg_mmd_set_params comes first)");
  const MmdState* m = s->mmd.get();
  const double alpha = m->par[2 * static_cast<size_t>(s->selected)];
  if (!(alpha > 0.0)) return set_error(OSG_ERR_INVALID, "osg_mmd_gap: the gap cannot be computed for alpha = 0 (mmd_dilated.py:333)");
  hipStream_t st = s->ctx->stream;
  const MmdWork w = mmd_work(m->d_work, s->I, s->A);
  k_mmd_gap<<<dim3(1), dim3(kMmdThreads), 0, st>>>(mmd_tree(s), s->d_info_player, s->cur(), w, alpha);
  OSG_HIP(hipGetLastError());
  OSG_HIP(hipMemcpyAsync(out, w.gap, sizeof(double), hipMemcpyDeviceToHost, st));
  OSG_HIP(hipStreamSynchronize(st));
  return OSG_OK;
}

int osg_mmd_sequences(osg_cfr* s, int which, double* h_x) {
  if (!s || !h_x || which < 0 || which > 1) return set_error(OSG_ERR_INVALID, "osg_mmd_sequences: bad argument");
  if (int rc = mmd_refusal(s, "osg_mmd_sequences")) return rc;
  if (!mmd_mode(s)) return set_error(OSG_ERR_INVALID, "osg_mmd_sequences: no parameters yet (osg_mmd_set_params comes first)");
  hipStream_t st = s->ctx->stream;
  const size_t bytes = sizeof(double) * s->I * s->A;
  const double* src = s->cum();
  if (which == 0) {
    const MmdWork w = mmd_work(s->mmd->d_work, s->I, s->A);
    k_mmd_sequences<<<dim3(mmd_blocks(s->I)), dim3(kMmdThreads), 0, st>>>(mmd_tree(s), s->cur(), w.x);
    OSG_HIP(hipGetLastError());
    src = w.x;
  }
  OSG_HIP(hipMemcpyAsync(h_x, src, bytes, hipMemcpyDeviceToHost, st));
  OSG_HIP(hipStreamSynchronize(st));
  return OSG_OK;
}

}  // extern "C"
