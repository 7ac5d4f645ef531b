// Extensive-form fictitious play on the flattened tree (XFPSolver, open_spiel/python/algorithms/fictitious_play.py:115-240;
// Heinrich, Lanctot and Silver 2015, Algorithm 1).  The average policy lives in the `cur` table.  One iteration:
//   every player's best response to the average policy (the evaluation's kernels: they leave the chosen action index
//   of every infostate in `best` on the device),
//   reach    a thread per infostate: the two own-player reach products of its first member history (osg_xfp.h),
//   update   a thread per infostate: the closed-form mixing of its row (osg_xfp.h).
// Every reach is formed from the old table before the first row is stored: a launch boundary in the general form
// (k_xfp_reach, k_xfp_update; any tree the evaluation serves), a workgroup barrier in the fused one (k_xfp_small: ONE
// workgroup runs all iterations of a call in one launch, with the tree, the policy and the scratch of the best response
// in LDS; trees that k_policy_eval evaluates and that fit).  Both forms run the same functions on the same values in the same
// order: bit-identical tables.
#include "osg_cfr_internal.h"
#include "osg_xfp.h"

namespace {

constexpr int kXfpThreads = 256;
constexpr size_t kXfpLdsLimit = 64 * 1024;   // dynamic LDS of k_xfp_small; larger tables take the general form
constexpr int kXfpItersPerLaunch = 4096;     // alphas handed to one launch of k_xfp_small

// reach: [2, I] — avg_reach, then br_reach
__global__ void __launch_bounds__(kXfpThreads)
k_xfp_reach(Tree t, const int32_t* __restrict__ path_off, const int32_t* __restrict__ path, const double* __restrict__ pol,
            const int32_t* __restrict__ best, double* __restrict__ reach) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.I) return;
  const int m = t.mem_off[i];   // the first member history in the reference's visiting order
  const XfpReach r = xfp_reach(path, path_off[m], path_off[m + 1], t.info_player[i], t.A, pol, best);
  reach[i] = r.avg;
  reach[t.I + i] = r.br;
}

__global__ void __launch_bounds__(kXfpThreads)
k_xfp_update(Tree t, double* __restrict__ pol, const int32_t* __restrict__ best, const double* __restrict__ reach, double alpha) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.I) return;
  xfp_update_row(pol + static_cast<size_t>(i) * t.A, t.nact[i], best[i], alpha, XfpReach{reach[i], reach[t.I + i]});
}

// What k_xfp_small keeps in LDS: the policy, the scratch of the best response, the reaches, and every array of the tree
// the iteration reads.  The host asks the same function for the size (base == nullptr).
struct XfpResident {
  double *pol, *brv, *cf, *reach, *edge_prob, *term_ret;
  int32_t *best, *level_off, *mem, *mem_off, *nact, *first_child, *info, *path_off, *path, *info_level;
  int8_t *actor, *info_player;
  uint8_t *kind, *nchild;
};
struct XfpCarve {   // hands out 8-byte aligned pieces of a buffer; without a buffer it only counts
  char* base;
  size_t used;
  template <class T>
  OSG_HD T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += (n * sizeof(T) + 7) & ~static_cast<size_t>(7);
    return p;
  }
};
OSG_HD size_t xfp_resident(char* base, int H, int I, int A, int P, int D, int M, int n_path, XfpResident* r) {
  XfpCarve c{base, 0};
  const size_t h = static_cast<size_t>(H), i = static_cast<size_t>(I), m = static_cast<size_t>(M);
  r->pol = c.take<double>(i * A);
  r->brv = c.take<double>(h);
  r->cf = c.take<double>(m);
  r->reach = c.take<double>(2 * i);
  r->edge_prob = c.take<double>(h);
  r->term_ret = c.take<double>(h * P);
  r->best = c.take<int32_t>(i);
  r->level_off = c.take<int32_t>(static_cast<size_t>(D) + 1);
  r->mem = c.take<int32_t>(m);
  r->mem_off = c.take<int32_t>(i + 1);
  r->nact = c.take<int32_t>(i);
  r->first_child = c.take<int32_t>(h);
  r->info = c.take<int32_t>(h);
  r->path_off = c.take<int32_t>(m + 1);
  r->path = c.take<int32_t>(static_cast<size_t>(n_path));
  r->info_level = c.take<int32_t>(i);
  r->actor = c.take<int8_t>(h);
  r->info_player = c.take<int8_t>(i);
  r->kind = c.take<uint8_t>(h);
  r->nchild = c.take<uint8_t>(h);
  return c.used;
}
template <class T>
OSG_D void xfp_stage(T* dst, const T* __restrict__ src, int n) {
  for (int k = threadIdx.x; k < n; k += blockDim.x) dst[k] = src[k];
}

// All iterations of a call in one launch by one workgroup, everything an iteration touches resident in LDS.
__global__ void __launch_bounds__(1024)
k_xfp_small(Tree t, EvalArrays ea, int n_path, double* pol_global, int32_t* best_global, const double* __restrict__ alphas, int iters) {
  extern __shared__ __attribute__((aligned(16))) double xfp_smem[];
  XfpResident r;
  xfp_resident(reinterpret_cast<char*>(xfp_smem), t.H, t.I, t.A, t.P, t.D, ea.M, n_path, &r);
  const int IA = t.I * t.A;
  const int tid = threadIdx.x, nt = blockDim.x;
  xfp_stage(r.pol, pol_global, IA);
  xfp_stage(r.edge_prob, t.edge_prob, t.H);
  xfp_stage(r.term_ret, t.term_ret, t.H * t.P);
  xfp_stage(r.level_off, t.level_off, t.D + 1);
  xfp_stage(r.mem, t.mem, ea.M);
  xfp_stage(r.mem_off, t.mem_off, t.I + 1);
  xfp_stage(r.nact, t.nact, t.I);
  xfp_stage(r.first_child, t.first_child, t.H);
  xfp_stage(r.info, t.info, t.H);
  xfp_stage(r.path_off, ea.path_off, ea.M + 1);
  xfp_stage(r.path, ea.path, n_path);
  xfp_stage(r.info_level, ea.info_level, t.I);
  xfp_stage(r.actor, t.actor, t.H);
  xfp_stage(r.info_player, t.info_player, t.I);
  xfp_stage(r.kind, t.kind, t.H);
  xfp_stage(r.nchild, t.nchild, t.H);
  t.edge_prob = r.edge_prob; t.term_ret = r.term_ret; t.level_off = r.level_off; t.mem = r.mem; t.mem_off = r.mem_off;
  t.nact = r.nact; t.first_child = r.first_child; t.info = r.info; t.actor = r.actor; t.info_player = r.info_player;
  t.kind = r.kind; t.nchild = r.nchild;
  ea.path_off = r.path_off; ea.path = r.path; ea.info_level = r.info_level;
  ea.brv = r.brv; ea.cf = r.cf; ea.best = r.best;
  double* pol = r.pol;
  double* reach = r.reach;
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    policy_eval_best_responses(t, ea, pol);   // (ends with a barrier)
    for (int i = tid; i < t.I; i += nt) {
      const int m = t.mem_off[i];
      const XfpReach x = xfp_reach(ea.path, ea.path_off[m], ea.path_off[m + 1], t.info_player[i], t.A, pol, ea.best);
      reach[i] = x.avg;
      reach[t.I + i] = x.br;
    }
    __syncthreads();
    const double alpha = alphas[it];
    for (int i = tid; i < t.I; i += nt)
      xfp_update_row(pol + i * t.A, t.nact[i], ea.best[i], alpha, XfpReach{reach[i], reach[t.I + i]});
    __syncthreads();
  }
  xfp_stage(pol_global, pol, IA);
  xfp_stage(best_global, ea.best, t.I);
}

size_t xfp_small_lds_bytes(const osg_cfr* s) {
  XfpResident r;
  return xfp_resident(nullptr, s->H, s->I, s->A, s->P, s->D, static_cast<int>(s->mem.size()), static_cast<int>(s->path.size()), &r);
}

// The fused form takes what k_policy_eval would evaluate (no jobs, not the grid) when the resident arrays fit.
bool xfp_takes_the_fused_form(const osg_cfr* s) {
  return s->cfg.kernel == OSG_CFR_KERNEL_AUTO && eval_form(s) == EvalForm::kOneWorkgroup && xfp_small_lds_bytes(s) <= kXfpLdsLimit;
}

// Every player's best response to `cur`, left in d_best, by the form osg_cfr_cfg.kernel asks for.
int xfp_respond_to_current(osg_cfr* s, const EvalArrays& ea) {
  return launch_policy_eval(s, eval_form_for_kernel_option(s), ea, s->cur(), false, nullptr, true);
}

const char* xfp_general_name(const osg_cfr* s) {   // (of the form xfp_respond_to_current just took)
  switch (s->last_eval_form) {
    case EvalForm::kJobs: return "k_xfp<k_eval_jobs>";
    case EvalForm::kGrid: return "k_xfp<k_geval>";
    case EvalForm::kGridPersist: return "k_xfp<k_geval_persist>";
    default: return "k_xfp<k_policy_eval>";
  }
}

void launch_reach(const osg_cfr* s, double* reach) {
  const unsigned blocks = static_cast<unsigned>((s->I + kXfpThreads - 1) / kXfpThreads);
  k_xfp_reach<<<dim3(blocks), dim3(kXfpThreads), 0, s->ctx->stream>>>(s->tree(), s->d_path_off, s->d_path, s->cur(), s->eval.best, reach);
}
void launch_update(const osg_cfr* s, const double* reach, double alpha) {
  const unsigned blocks = static_cast<unsigned>((s->I + kXfpThreads - 1) / kXfpThreads);
  k_xfp_update<<<dim3(blocks), dim3(kXfpThreads), 0, s->ctx->stream>>>(s->tree(), s->cur(), s->eval.best, reach, alpha);
}

// What every entry point refuses, and the [2, I] reach scratch (borrowed from d_reach) of those it serves.
int xfp_refusal(const osg_cfr* s, const char* who, double** reach) {
  const std::string w = who;
  if (s->cfg.solver != 0) return set_error(OSG_ERR_INVALID, w + ": needs a CFRSolverBase table (solver 0), not an MCCFR solver");
  if (s->B != 1) return set_error(OSG_ERR_UNSUPPORTED, w + ": one solver per object (replicas > 1)");
  if (s->dcfr) return set_error(OSG_ERR_INVALID, w + ": fictitious play has no discounting, this solver discounts (osg_cfr_set_discounting)");
  if (!s->eval_ok) return set_error(OSG_ERR_UNSUPPORTED, w + ": an information state spans several tree levels");
  if (int rc = xfp_reach_in_reach(s, w, reach)) return rc;
  return cfr_sub_error(s);
}

// The caller's best responses: checked on the host, then in d_best.
int xfp_upload_best(osg_cfr* s, const int32_t* h_best_index, const char* who) {
  for (int i = 0; i < s->I; ++i)
    if (h_best_index[i] < 0 || h_best_index[i] >= s->nact[i])
      return set_error(OSG_ERR_INVALID, std::string(who) + ": best-response index out of range at information state " +
                                            std::to_string(i) + " (" + std::to_string(h_best_index[i]) + ", legal actions " +
                                            std::to_string(s->nact[i]) + ")");
  hipStream_t st = s->ctx->stream;
  OSG_HIP(hipMemcpyAsync(s->eval.best, h_best_index, sizeof(int32_t) * s->I, hipMemcpyHostToDevice, st));
  OSG_HIP(hipStreamSynchronize(st));   // (the caller's array may be pageable and die with the call)
  return OSG_OK;
}

}  // namespace

extern "C" {

int osg_xfp_iterate(osg_cfr* s, int iters) {
  if (!s || iters < 0) return set_error(OSG_ERR_INVALID, "osg_xfp_iterate: bad argument");
  if (mmd_mode(s)) return set_error(OSG_ERR_INVALID, "osg_xfp_iterate: the solver is in mirror-descent mode (osg_mmd_set_params); fictitious play would overwrite its policy table");
  double* reach = nullptr;
  if (int rc = xfp_refusal(s, "osg_xfp_iterate", &reach)) return rc;
  if (iters == 0) return OSG_OK;
  hipStream_t st = s->ctx->stream;
  EvalArrays ea = eval_arrays_of(s);
  if (xfp_takes_the_fused_form(s)) {
    const size_t lds = xfp_small_lds_bytes(s);
    if (raise_lds_cap(reinterpret_cast<const void*>(&k_xfp_small), static_cast<int>(lds)) != hipSuccess) {
      (void)hipGetLastError();
      return set_error(OSG_ERR_HIP, "osg_xfp_iterate: the fused kernel's LDS request was refused");
    }
    for (int done = 0; done < iters; done += kXfpItersPerLaunch) {
      const int n = std::min(kXfpItersPerLaunch, iters - done);
      // (the stream may still be reading h_iter_table / d_iter_table for the previous launch)
      OSG_HIP(hipStreamSynchronize(st));
      OSG_HIP(s->d_iter_table.ensure(kXfpItersPerLaunch));
      s->h_iter_table.resize(n);
      for (int k = 0; k < n; ++k) s->h_iter_table[k] = xfp_alpha(s->iteration + k + 1);
      OSG_HIP(hipMemcpyAsync(s->d_iter_table, s->h_iter_table.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
      k_xfp_small<<<dim3(1), dim3(level_threads(s)), lds, st>>>(s->tree(), ea, static_cast<int>(s->path.size()), s->cur(), s->eval.best,
                                                                    s->d_iter_table, n);
      OSG_HIP(hipGetLastError());
      s->iteration += n;
    }
    s->last_kernel = "k_xfp_small";
    return OSG_OK;
  }
  for (int it = 0; it < iters; ++it) {
    if (int rc = xfp_respond_to_current(s, ea)) return rc;
    launch_reach(s, reach);
    ++s->iteration;
    launch_update(s, reach, xfp_alpha(s->iteration));
  }
  OSG_HIP(hipGetLastError());
  s->last_kernel = xfp_general_name(s);
  return OSG_OK;
}

int osg_xfp_update(osg_cfr* s, const int32_t* h_best_index) {
  if (!s || !h_best_index) return set_error(OSG_ERR_INVALID, "osg_xfp_update: null argument");
  double* reach = nullptr;
  if (int rc = xfp_refusal(s, "osg_xfp_update", &reach)) return rc;
  if (int rc = xfp_upload_best(s, h_best_index, "osg_xfp_update")) return rc;
  launch_reach(s, reach);
  ++s->iteration;
  launch_update(s, reach, xfp_alpha(s->iteration));
  OSG_HIP(hipGetLastError());
  s->last_kernel = "k_xfp_update";
  return OSG_OK;
}

int osg_xfp_reaches(osg_cfr* s, const int32_t* h_best_index, double* h_avg_reach, double* h_br_reach) {
  if (!s || !h_avg_reach || !h_br_reach) return set_error(OSG_ERR_INVALID, "osg_xfp_reaches: null argument");
  double* reach = nullptr;
  if (int rc = xfp_refusal(s, "osg_xfp_reaches", &reach)) return rc;
  hipStream_t st = s->ctx->stream;
  if (h_best_index) {
    if (int rc = xfp_upload_best(s, h_best_index, "osg_xfp_reaches")) return rc;
  } else {
    if (int rc = xfp_respond_to_current(s, eval_arrays_of(s))) return rc;
  }
  launch_reach(s, reach);
  OSG_HIP(hipGetLastError());
  OSG_HIP(hipMemcpyAsync(h_avg_reach, reach, sizeof(double) * s->I, hipMemcpyDeviceToHost, st));
  OSG_HIP(hipMemcpyAsync(h_br_reach, reach + s->I, sizeof(double) * s->I, hipMemcpyDeviceToHost, st));
  OSG_HIP(hipStreamSynchronize(st));
  return OSG_OK;
}

}  // extern "C"
