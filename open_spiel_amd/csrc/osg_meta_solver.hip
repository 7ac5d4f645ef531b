// PSRO's meta-strategy solvers on the device: projected replicator dynamics and regret matching on a batch of
// normal-form meta-games (projected_replicator_dynamics.py, regret_matching.py, nfg_utils.py of
// open_spiel/python/algorithms); the arithmetic and the one order of every sum are osg_meta_solver.h's.
//   k_meta_solve   one workgroup per problem, one wavefront per player, lane a = own action a; every iteration of the
//                  call in one launch.  The strategies live in LDS twice over (the previous step's and the one being
//                  written), so ONE workgroup barrier per iteration orders the players; regrets, the average's running
//                  sum and everything a player's step passes between its lanes (the ascending sums, the ranks of the
//                  sort, the sorted values, the bisection's bits) stay in registers and go through lane reads and
//                  ballots: lane a holds element a, and a sum over a wavefront is the header's ascending loop fed by
//                  one lane read per index (the index is wave-uniform: v_readlane, no trip through LDS), not a tree.
//   two forms      <true>: the P tensors are staged in LDS once, each transposed so that the player's OWN action is the
//                  fastest index (lane a reads word a of a row: no bank conflict); <false>: they are read from global
//                  memory where they lie.  Both evaluate meta_value with a different MetaView over the same cells in
//                  the same order, so their results are bit-identical.
// A problem's result depends on its tensors, its cfg and its initial strategies alone: nothing is shared between
// workgroups.
#include "osg_internal.h"
#include "osg_meta_solver.h"

#include <cmath>

namespace {

using namespace osg;

constexpr int64_t kMetaMaxProblems = int64_t{1} << 20;          // per call
constexpr size_t kMetaMaxTensorBytes = size_t{1} << 32;         // n_problems * P * cells * 8 per call
constexpr int kMetaMaxIterations = 100000000;                   // per problem: one launch runs them all
constexpr size_t kMetaLdsReserve = 1024;                       // kept free of the workgroup's limit

struct MetaCall {
  int P, SK;                       // players; sum of K
  int K[kMetaMaxPlayers], off[kMetaMaxPlayers];
  int64_t cells;                   // K_0 * .. * K_{P-1}
  MetaView view[kMetaMaxPlayers];  // of the form launched
  const double* tensors;           // [n, P, cells]
  const osg_meta_cfg* cfgs;        // [n] on the device, or null: `cfg` for every problem
  osg_meta_cfg cfg;
  const double* initial;           // [n, SK] or null
  double* average;                 // [n, SK]
  double* last;                    // [n, SK] or null
};

// x of lane `lane`, which is the same in every lane of the wavefront (a loop counter, a ballot's bit): two lane reads
// through the scalar unit instead of a shuffle through LDS.
__device__ __forceinline__ double lane_read(double x, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
  return __hiloint2double(hi, lo);
}

// sum_j x_j over the wavefront's first n lanes: from 0.0, ascending, in every lane.
__device__ __forceinline__ double wave_ascending_sum(double x, int n) {
  double sum = 0.0;
  for (int j = 0; j < n; ++j) sum = meta_sum_step(sum, lane_read(x, j));
  return sum;
}

// meta_prd_step with element a in lane a (inactive lanes carry s = v = 0.0 and take part in every shuffle).
__device__ __forceinline__ double wave_prd_step(double v, double s, int n, int a, bool active, double dt, double gamma, bool use_approx) {
  const double avg = wave_ascending_sum(meta_return_term(v, s), n);
  const double u = meta_prd_update(s, v, avg, dt);
  if (use_approx) {
    const double c = meta_clamp(u, gamma);
    return c / wave_ascending_sum(c, n);
  }
  int rank = 0;   // meta_rank_desc
  for (int j = 0; j < n; ++j) rank += meta_before(lane_read(u, j), j, u, a) ? 1 : 0;
  double cumsum = 0.0, my_sorted = 0.0, my_cumsum = 0.0;
  for (int i = 0; i < n; ++i) {   // meta_simplex_projection's loop: position i of the sorted order
    const unsigned long long holder = __ballot(active && rank == i);
    const double x = lane_read(u, holder ? __ffsll(static_cast<long long>(holder)) - 1 : 0);
    cumsum = i == 0 ? x : meta_sum_step(cumsum, x);
    if (a == i) { my_sorted = x; my_cumsum = cumsum; }
  }
  const double my_tmp = meta_u_tmp(my_cumsum, n, a, gamma);
  const unsigned long long below = __ballot(active && meta_rho_test(my_sorted, my_tmp, gamma));
  const double shift = lane_read(my_tmp, meta_rho_index(meta_bisect_left(below, n), n));
  return meta_project(u, shift, gamma);
}

// meta_rm_step with element a in lane a.
__device__ __forceinline__ double wave_rm_step(double v, double s, int n, double gamma, double* regret) {
  const double avg = wave_ascending_sum(meta_return_term(v, s), n);
  *regret = meta_rm_regret(*regret, v, avg);
  const double positive = meta_rm_positive(*regret);
  return meta_rm_strategy(positive, wave_ascending_sum(positive, n), n, gamma);
}

template <bool kResident>
__global__ void __launch_bounds__(64 * kMetaMaxPlayers) k_meta_solve(MetaCall c) {
  extern __shared__ double meta_lds[];   // strategies [2][SK]; kResident: the tensors [P][cells], transposed
  const int tid = threadIdx.x, a = tid & 63;
  const int p = __builtin_amdgcn_readfirstlane(tid >> 6);   // the wavefront's player, known uniform (64 * P threads: p < P)
  const int64_t b = blockIdx.x;
  const osg_meta_cfg cfg = c.cfgs ? c.cfgs[b] : c.cfg;
  int n = 0, off = 0;
#pragma unroll
  for (int q = 0; q < kMetaMaxPlayers; ++q) {
    if (q == p) { n = c.K[q]; off = c.off[q]; }
  }
  const bool active = a < n;
  double s_cur = 0.0;
  if (active) {
    s_cur = c.initial ? c.initial[b * c.SK + off + a] : 1.0 / static_cast<double>(n);
    meta_lds[off + a] = s_cur;
  }
  const double* problem = c.tensors + b * c.P * c.cells;
  if (kResident) {
    double* staged = meta_lds + 2 * c.SK;
    for (int64_t x = tid; x < c.cells; x += blockDim.x) {
      int idx[kMetaMaxPlayers];
      int64_t r = x;
#pragma unroll
      for (int q = kMetaMaxPlayers - 1; q >= 0; --q) {
        idx[q] = 0;
        if (q < c.P) { idx[q] = static_cast<int>(r % c.K[q]); r /= c.K[q]; }
      }
#pragma unroll
      for (int q = 0; q < kMetaMaxPlayers; ++q) {
        if (q < c.P) staged[q * c.cells + meta_cell_at(c.view[q], q, idx)] = problem[q * c.cells + x];
      }
    }
  }
  __syncthreads();
  const MetaView w = c.view[p];   // (p is uniform: scalar loads from the kernel's arguments)
  const double* tensor = (kResident ? meta_lds + 2 * c.SK : problem) + p * c.cells;
  const int64_t count = meta_average_count(cfg.iterations, cfg.window);
  const int64_t first = static_cast<int64_t>(cfg.iterations) + 1 - count;   // the oldest entry the average counts
  double sum = 0.0, regret = kMetaInitialRegret;
  if (first == 0) sum = meta_sum_step(sum, s_cur);
  for (int t = 1; t <= cfg.iterations; ++t) {
    const double* s_old = meta_lds + ((t - 1) & 1) * c.SK;
    double* s_next = meta_lds + (t & 1) * c.SK;
    const double v = active ? meta_value(w, tensor, s_old, a) : 0.0;
    const double s_new = cfg.method == kMetaPrd ? wave_prd_step(v, s_cur, n, a, active, cfg.dt, cfg.gamma, cfg.use_approx != 0)
                                                : wave_rm_step(v, s_cur, n, cfg.gamma, &regret);
    s_cur = active ? s_new : 0.0;
    if (active) {
      s_next[off + a] = s_cur;
      if (t >= first) sum = meta_sum_step(sum, s_cur);
    }
    __syncthreads();   // the one barrier of an iteration: every player's new strategy is written, every old one read
  }
  if (active) {
    c.average[b * c.SK + off + a] = meta_average(sum, count);
    if (c.last) c.last[b * c.SK + off + a] = s_cur;
  }
}

}  // namespace

extern "C" {

int osg_meta_solve(osg_ctx* ctx, int n_players, const int32_t* shape, int64_t n_problems, const double* tensors,
                   const osg_meta_cfg* cfgs, int64_t n_cfgs, const double* initial, double* average, double* last, int on_host) {
  const std::string who = "osg_meta_solve";
  if (!ctx || !shape || !cfgs || !average) return set_error(OSG_ERR_INVALID, who + ": null argument");
  if (n_problems < 0) return set_error(OSG_ERR_INVALID, who + ": n_problems is negative");
  if (n_cfgs != 1 && n_cfgs != n_problems) return set_error(OSG_ERR_INVALID, who + ": n_cfgs must be 1 or n_problems");
  for (int64_t k = 0; k < (n_problems == 0 ? 0 : n_cfgs); ++k) {
    const osg_meta_cfg& g = cfgs[k];
    if (g.method != kMetaPrd && g.method != kMetaRm) return set_error(OSG_ERR_INVALID, who + ": method must be 0 (projected replicator dynamics) or 1 (regret matching)");
    if (g.iterations < 0) return set_error(OSG_ERR_INVALID, who + ": iterations is negative");
    if (g.iterations > kMetaMaxIterations)
      return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(g.iterations) + " iterations exceed the limit of " +
                                                std::to_string(kMetaMaxIterations) + " per call");
    if (g.window < 0) return set_error(OSG_ERR_INVALID, who + ": window is negative");
    if (g.form < 0 || g.form > 2) return set_error(OSG_ERR_INVALID, who + ": form must be 0 (by size), 1 (LDS) or 2 (global memory)");
    if (g.form != cfgs[0].form) return set_error(OSG_ERR_INVALID, who + ": the cfgs of one call must name one form");
    if (!std::isfinite(g.gamma) || (g.method == kMetaPrd && !std::isfinite(g.dt))) return set_error(OSG_ERR_INVALID, who + ": dt or gamma is not finite");
  }
  if (n_players < kMetaMinPlayers || n_players > kMetaMaxPlayers)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(n_players) + " players (served: 2 to 5)");
  MetaCall c{};
  c.P = n_players;
  c.cells = 1;
  for (int p = 0; p < n_players; ++p) {
    if (shape[p] < 1 || shape[p] > kMetaMaxActions)
      return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(shape[p]) + " policies of player " + std::to_string(p) + " (served: 1 to 64)");
    c.K[p] = shape[p];
    c.off[p] = c.SK;
    c.SK += shape[p];
    c.cells *= shape[p];
  }
  if (c.cells > kMetaMaxCells)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(c.cells) + " cells per tensor exceed the limit of " + std::to_string(kMetaMaxCells));
  if (n_problems > kMetaMaxProblems)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(n_problems) + " problems exceed the limit of " + std::to_string(kMetaMaxProblems) + " per call");
  const size_t per_problem = static_cast<size_t>(c.P) * c.cells;
  if (n_problems > 0 && per_problem > kMetaMaxTensorBytes / sizeof(double) / static_cast<size_t>(n_problems))
    return set_error(OSG_ERR_UNSUPPORTED, who + ": the tensors exceed the limit of " + std::to_string(kMetaMaxTensorBytes) + " bytes per call");
  if (n_problems == 0) return OSG_OK;
  if (!tensors) return set_error(OSG_ERR_INVALID, who + ": null tensors");
  // The form: the tensors stay in LDS where they fit the workgroup's limit beside the two strategy buffers.
  size_t lds_limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &lds_limit)) return rc;
  const size_t vectors = sizeof(double) * 2 * c.SK, resident_bytes = vectors + sizeof(double) * per_problem;
  const bool fits = resident_bytes + kMetaLdsReserve <= lds_limit;
  if (cfgs[0].form == 1 && !fits)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": form 1 needs " + std::to_string(resident_bytes) + " bytes of LDS, the workgroup's limit is " +
                                              std::to_string(lds_limit));
  const bool resident = cfgs[0].form == 1 || (cfgs[0].form == 0 && fits);
  for (int p = 0; p < c.P; ++p) c.view[p] = meta_view(c.P, c.K, c.off, p, resident);

  hipStream_t st = ctx->stream;
  const size_t n = static_cast<size_t>(n_problems), out_doubles = n * c.SK, tensor_doubles = n * per_problem;
  // Scratch: the cfgs where every problem has its own, and with on_host the inputs and outputs.
  const size_t o_cfg = 0, o_tensors = align_up(n_cfgs > 1 ? sizeof(osg_meta_cfg) * n : 0);
  const size_t o_initial = o_tensors + (on_host ? align_up(sizeof(double) * tensor_doubles) : 0);
  const size_t o_average = o_initial + (on_host && initial ? align_up(sizeof(double) * out_doubles) : 0);
  const size_t o_last = o_average + (on_host ? align_up(sizeof(double) * out_doubles) : 0);
  const size_t scratch_bytes = o_last + (on_host && last ? align_up(sizeof(double) * out_doubles) : 0);
  unsigned char* scratch = nullptr;
  if (scratch_bytes) {
    void* ptr = nullptr;
    if (int rc = osg_ctx_scratch(ctx, scratch_bytes, &ptr)) return rc;
    scratch = static_cast<unsigned char*>(ptr);
  }
  c.cfg = cfgs[0];
  if (n_cfgs > 1) {
    OSG_HIP(hipMemcpyAsync(scratch + o_cfg, cfgs, sizeof(osg_meta_cfg) * n, hipMemcpyHostToDevice, st));
    if (!on_host) OSG_HIP(hipStreamSynchronize(st));   // the caller's array may die when the call returns
    c.cfgs = reinterpret_cast<const osg_meta_cfg*>(scratch + o_cfg);
  }
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(scratch + o_tensors, tensors, sizeof(double) * tensor_doubles, hipMemcpyHostToDevice, st));
    if (initial) OSG_HIP(hipMemcpyAsync(scratch + o_initial, initial, sizeof(double) * out_doubles, hipMemcpyHostToDevice, st));
    c.tensors = reinterpret_cast<const double*>(scratch + o_tensors);
    c.initial = initial ? reinterpret_cast<const double*>(scratch + o_initial) : nullptr;
    c.average = reinterpret_cast<double*>(scratch + o_average);
    c.last = last ? reinterpret_cast<double*>(scratch + o_last) : nullptr;
  } else {
    c.tensors = tensors; c.initial = initial; c.average = average; c.last = last;
  }
  const size_t lds = resident ? resident_bytes : vectors;
  const void* kernel = resident ? reinterpret_cast<const void*>(&k_meta_solve<true>) : reinterpret_cast<const void*>(&k_meta_solve<false>);
  if (lds > (32u << 10) && raise_lds_cap(kernel, static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(OSG_ERR_UNSUPPORTED, who + ": the device does not grant " + std::to_string(lds) + " bytes of LDS to a workgroup");
  }
  const dim3 grid(static_cast<unsigned>(n)), block(64 * c.P);
  if (resident) k_meta_solve<true><<<grid, block, lds, st>>>(c);
  else k_meta_solve<false><<<grid, block, lds, st>>>(c);
  OSG_HIP(hipGetLastError());
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(average, c.average, sizeof(double) * out_doubles, hipMemcpyDeviceToHost, st));
    if (last) OSG_HIP(hipMemcpyAsync(last, c.last, sizeof(double) * out_doubles, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipStreamSynchronize(st));
  }
  return OSG_OK;
}

}  // extern "C"
