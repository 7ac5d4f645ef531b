// Alpha-rank on the device: the Markov chain over the pure profiles of a batch of normal-form meta-games, its stationary
// distribution by Grassmann-Taksar-Heyman elimination, the sweep over the infinite-alpha noise and the marginals
// (open_spiel/python/egt/alpharank.py, psro_v2/utils.py); the arithmetic and the one order of every sum are
// osg_alpharank.h's.
//   k_alpharank_solve   one workgroup per (problem, epsilon of the chunk).  It zeroes the matrix, writes the off-diagonal
//                       entries (one lane per state and move), and eliminates with ONE barrier per pivot: every wavefront
//                       forms the pivot row's sum s itself (lane partials, then six exchange steps: ar_lane_sum's order),
//                       then takes rows i = wave, wave + W, .. of the trailing block, its lanes along the columns; the
//                       quotient a[i][k] / s is uniform in a wavefront and stored by its lane 0.  The back-substitution
//                       pushes x[i] * a[i][i+1 ..] into the x above it, one barrier per i: every x[k] is a plain sum
//                       over i ascending.  <true>: the matrix in LDS beside x; <false>: in the call's workspace (rows
//                       padded to 128 bytes), x in LDS.  The same operations on the same elements either way, and
//                       whatever the number of wavefronts: bit-identical results.
//   k_alpharank_stop    one workgroup per problem: walks the chunk's epsilons in order, applies the stop rule to
//                       neighbouring pairs (the last pi of the previous chunk is kept), and on a stop, a status 1 or the
//                       end of max_iters writes pi, the marginals, eps_used, iterations and status, marks the problem
//                       done and counts it (an integer atomic; there are no floating-point atomics here).
// The host launches chunk after chunk until every problem is done; it reads the count once per chunk.
#include "osg_internal.h"
#include "osg_alpharank.h"

#include <cmath>

namespace {

using namespace osg;

constexpr int64_t kArMaxProblems = int64_t{1} << 16;          // per call
constexpr size_t kArWorkspaceBudget = size_t{1} << 30;         // the chunk's solutions and, in the global form, matrices
constexpr int kArDefaultChunk = 8, kArMaxChunk = 64;
constexpr size_t kArLdsReserve = 1024;                        // kept free of the workgroup's limit
constexpr int kArStopThreads = 256;
constexpr int kArMaxSweepSteps = 4096;                        // 0.5 * 2^-t is 0 from t = 1075 on

struct ArCall {
  ArShape sh;
  int64_t lda;                      // doubles between two rows of the matrix
  int chunk, t0;                    // this launch solves the sweep's steps t0 .. t0 + chunk - 1
  const double* tensors;            // [B, cells]
  const osg_alpharank_cfg* cfgs;    // [B] on the device, or null: `cfg` for every problem
  osg_alpharank_cfg cfg;
  double* matrices;                 // global form: [B * chunk, n * lda]
  double* slots;                    // [B * chunk, n]: the pi of every (problem, step of the chunk)
  int32_t* slot_status;             // [B * chunk]
  double* prev;                     // [B, n]: the pi of step t0 - 1
  int32_t* done;                    // [B]
  int32_t* n_done;                  // [1]
  double* pi;                       // [B, n]
  double* marginals;                // [B, SK] or null
  double* eps_used;                 // [B] or null
  int32_t* iterations;              // [B] or null
  int32_t* status;                  // [B]
};

__device__ __forceinline__ double wave_tree(double part) {   // ar_tree with partial l in lane l; every lane gets the sum
#pragma unroll
  for (int mask = 1; mask < kArLanes; mask <<= 1) part = part + __shfl_xor(part, mask, kArLanes);
  return part;
}
__device__ __forceinline__ double wave_lane_sum(const double* v, int count, int lane) {   // ar_lane_sum
  double part = 0.0;
  for (int j = lane; j < count; j += kArLanes) part = part + v[j];
  return wave_tree(part);
}

template <bool kLds>
__global__ void __launch_bounds__(1024) k_alpharank_solve(ArCall c) {
  extern __shared__ double ar_lds[];   // x [n]; kLds: the matrix [n, lda]
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, W = T >> 6;
  const int64_t slot = blockIdx.x, b = slot / c.chunk;
  const int t = c.t0 + static_cast<int>(slot % c.chunk);
  if (c.done[b]) return;
  const osg_alpharank_cfg cfg = c.cfgs ? c.cfgs[b] : c.cfg;
  if (cfg.mode == kArSweep ? t >= cfg.max_iters : t != 0) return;
  const double eps = cfg.mode == kArSweep ? ar_eps_at(ar_sweep_start(cfg.eps), t) : cfg.eps;
  const int n = c.sh.n;
  const int64_t lda = c.lda;
  double* x = ar_lds;
  double* a = kLds ? ar_lds + n : c.matrices + slot * (static_cast<int64_t>(n) * lda);
  const double* tensors = c.tensors + b * c.sh.cells;

  for (int64_t e = tid; e < n * lda; e += T) a[e] = 0.0;
  __syncthreads();
  const int64_t pairs = static_cast<int64_t>(n) * c.sh.moves;
  for (int64_t e = tid; e < pairs; e += T) {
    const int row = static_cast<int>(e / c.sh.moves), mv = static_cast<int>(e % c.sh.moves);
    int col;
    const double value = ar_entry(c.sh, tensors, row, mv, cfg.mode, eps, cfg.alpha, cfg.m, &col);
    a[row * lda + col] = value;
  }
  __syncthreads();

  int status = kArOk;
  for (int k = n - 1; k >= 1; --k) {
    const double* rk = a + k * lda;
    const double s = wave_lane_sum(rk, k, lane);   // the same value in every wavefront
    if (!ar_pivot_ok(s)) { status = kArReducible; break; }
    for (int i = wave; i < k; i += W) {
      double* ri = a + i * lda;
      const double q = ri[k] / s;
      for (int j = lane; j < k; j += kArLanes) ri[j] = ar_madd(ri[j], q, rk[j]);
      if (lane == 0) ri[k] = q;
    }
    __syncthreads();   // the one barrier of a pivot
  }
  double* out = c.slots + slot * n;
  if (status == kArOk) {
    for (int i = tid; i < n; i += T) x[i] = i == 0 ? 1.0 : 0.0;
    __syncthreads();
    for (int i = 0; i + 1 < n; ++i) {
      const double xi = x[i];
      const double* ri = a + i * lda;
      for (int k = i + 1 + tid; k < n; k += T) x[k] = ar_madd(x[k], xi, ri[k]);
      __syncthreads();
    }
    const double total = wave_lane_sum(x, n, lane);
    if (!ar_is_finite(total)) status = kArReducible;
    else for (int i = tid; i < n; i += T) out[i] = x[i] / total;
  }
  if (status != kArOk)
    for (int i = tid; i < n; i += T) out[i] = ar_nan();
  if (tid == 0) c.slot_status[slot] = status;
}

__global__ void __launch_bounds__(kArStopThreads) k_alpharank_stop(ArCall c) {
  const int tid = threadIdx.x, n = c.sh.n;
  const int64_t b = blockIdx.x;
  if (c.done[b]) return;
  const osg_alpharank_cfg cfg = c.cfgs ? c.cfgs[b] : c.cfg;
  const double* slots = c.slots + b * c.chunk * n;
  const double eps0 = ar_sweep_start(cfg.eps);
  int status = -1, at = 0, t = c.t0;
  for (int cc = 0; cc < c.chunk && status < 0; ++cc) {
    at = cc;
    t = c.t0 + cc;
    if (cfg.mode != kArSweep) { status = c.slot_status[b * c.chunk + cc]; break; }
    if (t >= cfg.max_iters) { status = kArNoStop; at = -1; break; }
    if (c.slot_status[b * c.chunk + cc] != kArOk) { status = kArReducible; break; }
    if (t > cfg.min_iters) {
      const double* now = slots + static_cast<int64_t>(cc) * n;
      const double* before = cc == 0 ? c.prev + b * n : now - n;
      int close = 1;
      for (int i = tid; i < n; i += kArStopThreads) close &= ar_close(now[i], before[i]) ? 1 : 0;
      if (__syncthreads_and(close)) { status = kArOk; break; }
    }
    if (t + 1 >= cfg.max_iters) { status = kArNoStop; break; }
  }
  if (status < 0) {   // the sweep goes on: keep the chunk's last pi
    const double* last = slots + static_cast<int64_t>(c.chunk - 1) * n;
    for (int i = tid; i < n; i += kArStopThreads) c.prev[b * n + i] = last[i];
    return;
  }
  const double* result = at >= 0 ? slots + static_cast<int64_t>(at) * n : nullptr;
  const bool good = status == kArOk;
  for (int i = tid; i < n; i += kArStopThreads) c.pi[b * n + i] = good ? result[i] : ar_nan();
  if (c.marginals)
    for (int x = tid; x < c.sh.SK; x += kArStopThreads) c.marginals[b * c.sh.SK + x] = good ? ar_marginal(c.sh, result, x) : ar_nan();
  if (tid == 0) {
    if (c.eps_used) c.eps_used[b] = cfg.mode == kArSweep ? ar_eps_at(eps0, t) : cfg.mode == kArInfinite ? cfg.eps : 0.0;
    if (c.iterations) c.iterations[b] = cfg.mode == kArSweep ? t : 0;
    c.status[b] = status;
    c.done[b] = 1;
    atomicAdd(c.n_done, 1);
  }
}

}  // namespace

extern "C" {

int osg_alpharank(osg_ctx* ctx, int n_players, const int32_t* shape, int64_t n_problems, const double* tensors,
                  const osg_alpharank_cfg* cfgs, int64_t n_cfgs, double* pi, double* marginals, double* eps_used,
                  int32_t* iterations, int32_t* status, int on_host) {
  const std::string who = "osg_alpharank";
  if (!ctx || !shape || !cfgs || !pi || !status) return set_error(OSG_ERR_INVALID, who + ": null argument");
  if (n_problems < 0) return set_error(OSG_ERR_INVALID, who + ": n_problems is negative");
  if (n_cfgs != 1 && n_cfgs != n_problems) return set_error(OSG_ERR_INVALID, who + ": n_cfgs must be 1 or n_problems");
  bool sweeps = false;
  for (int64_t k = 0; k < (n_problems == 0 ? 0 : n_cfgs); ++k) {
    const osg_alpharank_cfg& g = cfgs[k];
    if (g.mode < kArFinite || g.mode > kArSweep) return set_error(OSG_ERR_INVALID, who + ": mode must be 0 (finite alpha), 1 (infinite alpha) or 2 (sweep)");
    if (g.mode == kArFinite && g.m < 1) return set_error(OSG_ERR_INVALID, who + ": m must be at least 1");
    if (g.mode == kArFinite && !std::isfinite(g.alpha)) return set_error(OSG_ERR_INVALID, who + ": alpha is not finite");
    if (g.mode != kArFinite && !(std::isfinite(g.eps) && g.eps >= 0.0)) return set_error(OSG_ERR_INVALID, who + ": eps is negative or not finite");
    if (g.mode == kArInfinite && g.eps == 0.0) return set_error(OSG_ERR_INVALID, who + ": mode 1 needs an eps above 0");
    if (g.mode == kArSweep && (g.min_iters < 0 || g.max_iters < 1)) return set_error(OSG_ERR_INVALID, who + ": min_iters < 0 or max_iters < 1");
    if (g.mode == kArSweep && g.max_iters > kArMaxSweepSteps)
      return set_error(OSG_ERR_UNSUPPORTED, who + ": max_iters exceeds " + std::to_string(kArMaxSweepSteps) + " (epsilon is 0 long before)");
    if (g.form < 0 || g.form > 2) return set_error(OSG_ERR_INVALID, who + ": form must be 0 (by size), 1 (LDS) or 2 (global memory)");
    if (g.chunk < 0) return set_error(OSG_ERR_INVALID, who + ": chunk is negative");
    if (g.form != cfgs[0].form || g.chunk != cfgs[0].chunk) return set_error(OSG_ERR_INVALID, who + ": the cfgs of one call must name one form and one chunk");
    sweeps |= g.mode == kArSweep;
  }
  if (n_players < 1 || n_players > kArMaxPlayers)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(n_players) + " players (served: 1 to 5)");
  const int dims = n_players == 1 ? 2 : n_players;
  int64_t profiles = 1;
  for (int p = 0; p < dims; ++p) {
    if (shape[p] < 1) return set_error(OSG_ERR_INVALID, who + ": a size below 1");
    if (shape[p] > kArMaxProfiles) return set_error(OSG_ERR_UNSUPPORTED, who + ": more than " + std::to_string(kArMaxProfiles) + " profiles");
    profiles *= shape[p];
    if (n_players > 1 && profiles > kArMaxProfiles)
      return set_error(OSG_ERR_UNSUPPORTED, who + ": more than " + std::to_string(kArMaxProfiles) + " profiles");
  }
  if (n_players == 1 && shape[0] != shape[1]) return set_error(OSG_ERR_INVALID, who + ": the table of a single population must be square");
  if (n_problems > kArMaxProblems)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(n_problems) + " problems exceed the limit of " + std::to_string(kArMaxProblems) + " per call");
  if (cfgs[0].chunk > kArMaxChunk && n_problems > 0)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": chunk exceeds " + std::to_string(kArMaxChunk));

  ArCall c{};
  c.sh = ar_shape(n_players, shape);
  const int n = c.sh.n;
  size_t lds_limit = 0;
  if (int rc = workgroup_lds_limit(ctx->device, &lds_limit)) return rc;
  const size_t vector_bytes = sizeof(double) * n, resident_bytes = vector_bytes + sizeof(double) * n * n;
  const bool fits = resident_bytes + kArLdsReserve <= lds_limit;
  const int form = n_problems > 0 ? cfgs[0].form : 0;
  if (form == 1 && !fits)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": form 1 needs " + std::to_string(resident_bytes) + " bytes of LDS, the workgroup's limit is " +
                                              std::to_string(lds_limit));
  const bool resident = form == 1 || (form == 0 && fits);
  c.lda = resident ? n : (static_cast<int64_t>(n) + 15) & ~int64_t{15};
  if (n_problems == 0) return OSG_OK;
  // The chunk: the cfg's, or the default halved while the chunk's solutions and matrices exceed the budget.
  const size_t B = static_cast<size_t>(n_problems);
  const size_t per_slot = sizeof(double) * n + (resident ? 0 : sizeof(double) * n * c.lda);
  int chunk = !sweeps ? 1 : cfgs[0].chunk ? cfgs[0].chunk : kArDefaultChunk;
  if (sweeps && cfgs[0].chunk == 0)
    while (chunk > 1 && per_slot * chunk > kArWorkspaceBudget / B) chunk >>= 1;
  if (per_slot * chunk > kArWorkspaceBudget / B)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(n_problems) + " problems of " + std::to_string(n) + " profiles with " +
                                              std::to_string(chunk) + " epsilons per launch exceed the workspace budget of " +
                                              std::to_string(kArWorkspaceBudget) + " bytes");
  if (!tensors) return set_error(OSG_ERR_INVALID, who + ": null tensors");
  c.chunk = chunk;

  hipStream_t st = ctx->stream;
  const size_t slots = B * chunk, tensor_doubles = B * static_cast<size_t>(c.sh.cells);
  size_t at = 0;
  auto take = [&at](size_t bytes) { const size_t o = at; at += align_up(bytes); return o; };
  const size_t o_cfg = take(n_cfgs > 1 ? sizeof(osg_alpharank_cfg) * B : 0);
  const size_t o_done = take(sizeof(int32_t) * (B + 1));           // done [B], then the count
  const size_t o_slot_status = take(sizeof(int32_t) * slots);
  const size_t o_prev = take(sizeof(double) * B * n);
  const size_t o_slots = take(sizeof(double) * slots * n);
  const size_t o_matrices = take(resident ? 0 : sizeof(double) * slots * n * c.lda);
  const size_t o_tensors = take(on_host ? sizeof(double) * tensor_doubles : 0);
  const size_t o_pi = take(on_host ? sizeof(double) * B * n : 0);
  const size_t o_marginals = take(on_host && marginals ? sizeof(double) * B * c.sh.SK : 0);
  const size_t o_eps = take(on_host && eps_used ? sizeof(double) * B : 0);
  const size_t o_iterations = take(on_host && iterations ? sizeof(int32_t) * B : 0);
  const size_t o_status = take(on_host ? sizeof(int32_t) * B : 0);
  void* ptr = nullptr;
  if (int rc = osg_ctx_scratch(ctx, at, &ptr)) return rc;
  unsigned char* scratch = static_cast<unsigned char*>(ptr);
  c.cfg = cfgs[0];
  if (n_cfgs > 1) {
    OSG_HIP(hipMemcpyAsync(scratch + o_cfg, cfgs, sizeof(osg_alpharank_cfg) * B, hipMemcpyHostToDevice, st));
    c.cfgs = reinterpret_cast<const osg_alpharank_cfg*>(scratch + o_cfg);
  }
  c.done = reinterpret_cast<int32_t*>(scratch + o_done);
  c.n_done = c.done + B;
  c.slot_status = reinterpret_cast<int32_t*>(scratch + o_slot_status);
  c.prev = reinterpret_cast<double*>(scratch + o_prev);
  c.slots = reinterpret_cast<double*>(scratch + o_slots);
  c.matrices = resident ? nullptr : reinterpret_cast<double*>(scratch + o_matrices);
  OSG_HIP(hipMemsetAsync(c.done, 0, sizeof(int32_t) * (B + 1), st));
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(scratch + o_tensors, tensors, sizeof(double) * tensor_doubles, hipMemcpyHostToDevice, st));
    c.tensors = reinterpret_cast<const double*>(scratch + o_tensors);
    c.pi = reinterpret_cast<double*>(scratch + o_pi);
    c.marginals = marginals ? reinterpret_cast<double*>(scratch + o_marginals) : nullptr;
    c.eps_used = eps_used ? reinterpret_cast<double*>(scratch + o_eps) : nullptr;
    c.iterations = iterations ? reinterpret_cast<int32_t*>(scratch + o_iterations) : nullptr;
    c.status = reinterpret_cast<int32_t*>(scratch + o_status);
  } else {
    c.tensors = tensors; c.pi = pi; c.marginals = marginals; c.eps_used = eps_used; c.iterations = iterations; c.status = status;
  }
  const size_t lds = resident ? resident_bytes : vector_bytes;
  const void* kernel = resident ? reinterpret_cast<const void*>(&k_alpharank_solve<true>) : reinterpret_cast<const void*>(&k_alpharank_solve<false>);
  if (lds > (32u << 10) && raise_lds_cap(kernel, static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(OSG_ERR_UNSUPPORTED, who + ": the device does not grant " + std::to_string(lds) + " bytes of LDS to a workgroup");
  }
  int waves = (n + 15) / 16;
  waves = waves < 1 ? 1 : waves > 16 ? 16 : waves;
  const dim3 grid(static_cast<unsigned>(slots)), block(64 * waves);
  int max_steps = 1;
  for (int64_t k = 0; k < n_cfgs; ++k)
    if (cfgs[k].mode == kArSweep && cfgs[k].max_iters > max_steps) max_steps = cfgs[k].max_iters;
  int32_t n_done = 0;
  for (c.t0 = 0; c.t0 < max_steps + chunk; c.t0 += chunk) {
    if (resident) k_alpharank_solve<true><<<grid, block, lds, st>>>(c);
    else k_alpharank_solve<false><<<grid, block, lds, st>>>(c);
    OSG_HIP(hipGetLastError());
    k_alpharank_stop<<<dim3(static_cast<unsigned>(B)), dim3(kArStopThreads), 0, st>>>(c);
    OSG_HIP(hipGetLastError());
    if (!sweeps) break;   // modes 0 and 1 are done after the first launch: nothing to wait for
    OSG_HIP(hipMemcpyAsync(&n_done, c.n_done, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    OSG_HIP(hipStreamSynchronize(st));
    if (n_done == static_cast<int32_t>(B)) break;
  }
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(pi, c.pi, sizeof(double) * B * n, hipMemcpyDeviceToHost, st));
    if (marginals) OSG_HIP(hipMemcpyAsync(marginals, c.marginals, sizeof(double) * B * c.sh.SK, hipMemcpyDeviceToHost, st));
    if (eps_used) OSG_HIP(hipMemcpyAsync(eps_used, c.eps_used, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    if (iterations) OSG_HIP(hipMemcpyAsync(iterations, c.iterations, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipMemcpyAsync(status, c.status, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipStreamSynchronize(st));
  } else if (n_cfgs > 1 && !sweeps) {
    OSG_HIP(hipStreamSynchronize(st));   // the caller's cfg array may die when the call returns
  }
  return OSG_OK;
}

}  // extern "C"
