// The exact Nash meta-solver on the device: a batch of two-player zero-sum matrix games, each solved as a linear
// program by a primal simplex with Bland's rule on the condensed tableau (psro_v2's "nash": lp_solver.
// solve_zero_sum_matrix_game); the arithmetic and the one order of every operation are osg_nash_lp.h's.
//   k_nash_lp   one workgroup of 256 threads (four wavefronts) per problem.  The tableau [m + 1, n + 1] and the row and
//               column labels live in LDS for the whole solve; global memory is read once (the matrix) and written once
//               (x, y, v, the pivot count, the status).
//     stride    ld = (n + 1) | 1 doubles (nl_stride), i.e. ODD: lane i of the pivot column's read is at double
//               i * ld + c, so lanes 0 .. 31 (a 64-bit LDS read serves 32 lanes per pass) fall into 32 different pairs
//               of the 64 banks (2 * ld * i mod 64 takes every even value once when ld is odd); the row-major update
//               has lane j at double i * ld + j: consecutive, free of conflicts with any stride.
//     select    EVERY wavefront selects the pivot itself, from the same LDS words and so with the same result: lane j
//               holds column j's reduced cost and label, lane i row i's entry of the entering column, right-hand side
//               and label (m, n <= 64).  The candidates are a ballot; the smallest label among them is found by seven
//               more ballots, one per bit of a label from the top (labels are distinct and below 128); the minimum
//               ratio by six exchange steps (a minimum does not depend on their order).  Nothing goes through global
//               memory, and no wavefront has to be told the choice.
//     update    the pivot row (scaled, lane j: column j, lane 0 also column 64) and the pivot column (lane i: row i; row
//               m's entry in a scalar) are in registers before the first write.  Wavefront w then rewrites rows w,
//               w + 4, ..: one LDS read and one write per element, the row's entry of the pivot column by a lane read.
//     barriers  TWO per pivot: one after every wavefront has read what it selects and updates from (before the first
//               write), one after the last write (before the next selection).  Five more per problem, outside the loop.
// A problem's bits depend on its matrix alone: nothing is shared between workgroups, and no operation's order depends
// on the grid.  No floating-point atomics.
#include "osg_internal.h"
#include "osg_nash_lp.h"

#include <cmath>

namespace {

using namespace osg;

constexpr int64_t kNlMaxProblems = int64_t{1} << 20;   // per call
constexpr int kNlThreads = 256, kNlWaves = kNlThreads / 64;

struct NlCall {
  int m, n, ld;
  const double* matrices;   // [B, m, n]
  double* x;                // [B, m]
  double* y;                // [B, n]
  double* value;            // [B]
  int32_t* pivots;          // [B] or null
  int32_t* status;          // [B]
};

// Doubles of LDS: the tableau, then two vectors of 64 (the minimum and maximum of the wavefronts first, x' and y' at
// the end), then the labels (2 * 64 ints).
__host__ __device__ inline size_t nl_lds_doubles(int m, int ld) { return static_cast<size_t>(m + 1) * ld + 2 * kNlMaxSide + kNlMaxSide; }

// x of lane `lane`, which is the same in every lane of the wavefront: two lane reads through the scalar unit.
__device__ __forceinline__ double lane_read(double x, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
  return __hiloint2double(hi, lo);
}

// Of the lanes in `members` (not empty) the one whose label is smallest; labels are distinct and below 128.
__device__ __forceinline__ int lowest_label(unsigned long long members, int label, int lane) {
#pragma unroll
  for (int bit = 6; bit >= 0; --bit) {
    const unsigned long long clear = __ballot(((members >> lane) & 1) && !((label >> bit) & 1));
    if (clear) members = clear;
  }
  return __ffsll(static_cast<long long>(members)) - 1;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
    const double other = __shfl_xor(v, mask, 64);
    v = other < v ? other : v;
  }
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
    const double other = __shfl_xor(v, mask, 64);
    v = other > v ? other : v;
  }
  return v;
}

// nl_sum over element k in lane k, k < count; the same value in every lane.
__device__ __forceinline__ double wave_nl_sum(double v, int count) {
  double sum = 0.0, err = 0.0;
  for (int k = 0; k < count; ++k) nl_sum_step(&sum, &err, lane_read(v, k));
  return sum + err;
}

__global__ void __launch_bounds__(kNlThreads) k_nash_lp(NlCall c) {
  extern __shared__ double nl_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = c.m, n = c.n, ld = c.ld;
  const int64_t b = blockIdx.x;
  double* t = nl_lds;
  double* yv = t + (m + 1) * ld;   // [64]; before the solve: the wavefronts' minima [4] and maxima [4]
  double* xv = yv + kNlMaxSide;    // [64]
  int* col_label = reinterpret_cast<int*>(xv + kNlMaxSide);   // [64]
  int* row_label = col_label + kNlMaxSide;                    // [64]
  const double* a = c.matrices + b * (static_cast<int64_t>(m) * n);

  // ---- the matrix: finite?  its minimum and maximum; the tableau ----
  double lo = INFINITY, hi = -INFINITY;
  int bad = 0;
  for (int e = tid; e < m * n; e += kNlThreads) {
    const double v = a[e];
    bad |= nl_is_finite(v) ? 0 : 1;
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
    t[(e / n) * ld + e % n] = v;   // (normalised below by the thread that wrote it)
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane == 0) { yv[wave] = lo; yv[kNlWaves + wave] = hi; }
  if (__syncthreads_or(bad)) {
    for (int i = tid; i < m; i += kNlThreads) c.x[b * m + i] = nl_nan();
    for (int j = tid; j < n; j += kNlThreads) c.y[b * n + j] = nl_nan();
    if (tid == 0) {
      c.value[b] = nl_nan();
      if (c.pivots) c.pivots[b] = 0;
      c.status[b] = kNlNotFinite;
    }
    return;
  }
#pragma unroll
  for (int w = 0; w < kNlWaves; ++w) {
    lo = yv[w] < lo ? yv[w] : lo;
    hi = yv[kNlWaves + w] > hi ? yv[kNlWaves + w] : hi;
  }
  double pre, base, span;
  nl_range(lo, hi, &pre, &base, &span);
  for (int e = tid; e < m * n; e += kNlThreads) {
    double* cell = t + (e / n) * ld + e % n;
    *cell = nl_normalise(*cell * pre, base, span);
  }
  for (int i = tid; i < m; i += kNlThreads) { t[i * ld + n] = 1.0; row_label[i] = n + i; }
  for (int j = tid; j < n; j += kNlThreads) { t[m * ld + j] = -1.0; col_label[j] = j; }
  if (tid == 0) t[m * ld + n] = 0.0;
  __syncthreads();

  // ---- the pivots ----
  const bool is_col = lane < n, is_row = lane < m, in_row = lane <= n;   // (in_row: a tableau row's columns 0 .. n)
  const bool tail = n == kNlMaxSide && lane == 0;                          // lane 0 also keeps column 64
  int status = kNlOk, done = 0;
  for (;;) {
    const double cost = is_col ? t[m * ld + lane] : 0.0;
    const int my_col_label = is_col ? col_label[lane] : 0;
    const unsigned long long entering = __ballot(is_col && nl_enters(cost));
    if (!entering) break;   // optimal (the same in every wavefront: they read the same words)
    if (done == kNlMaxPivots) { status = kNlNoOptimum; break; }
    const int pc = lowest_label(entering, my_col_label, lane);
    const double column = is_row ? t[lane * ld + pc] : 0.0, rhs = is_row ? t[lane * ld + n] : 0.0;
    const int my_row_label = is_row ? row_label[lane] : 0;
    const bool candidate = is_row && nl_pivotable(column);
    if (!__ballot(candidate)) { status = kNlNoOptimum; break; }
    const double ratio = candidate ? nl_ratio(rhs, column) : INFINITY;
    const double best = wave_min(ratio);
    const unsigned long long ties = __ballot(candidate && nl_ties(ratio, best));
    if (!ties) { status = kNlNoOptimum; break; }   // (a ratio that overflowed: inf - inf is no tie)
    const int pr = lowest_label(ties, my_row_label, lane);
    const double p = lane_read(column, pr);
    const double bottom = t[m * ld + pc];   // row m's entry of the pivot column
    const double scaled = in_row ? nl_scaled(t[pr * ld + lane], p) : 0.0;
    const double scaled_tail = tail ? nl_scaled(t[pr * ld + kNlMaxSide], p) : 0.0;
    const int entering_label = __builtin_amdgcn_readlane(my_col_label, pc), leaving_label = __builtin_amdgcn_readlane(my_row_label, pr);
    __syncthreads();   // barrier 1 of 2: every wavefront holds the pivot row and column; now the tableau may change
    for (int i = wave; i <= m; i += kNlWaves) {
      double* row = t + i * ld;
      if (i == pr) {
        if (in_row) row[lane] = lane == pc ? nl_inverse(p) : scaled;
        if (tail) row[kNlMaxSide] = scaled_tail;
        continue;
      }
      const double ci = i < m ? lane_read(column, i) : bottom;
      if (in_row) row[lane] = lane == pc ? nl_column(ci, p) : nl_update(row[lane], ci, scaled);
      if (tail) row[kNlMaxSide] = nl_update(row[kNlMaxSide], ci, scaled_tail);
    }
    if (tid == 0) { col_label[pc] = leaving_label; row_label[pr] = entering_label; }
    ++done;
    __syncthreads();   // barrier 2 of 2: the tableau and the labels of the next selection are written
  }

  // ---- the read-out ----
  if (status != kNlOk) {
    for (int i = tid; i < m; i += kNlThreads) c.x[b * m + i] = nl_nan();
    for (int j = tid; j < n; j += kNlThreads) c.y[b * n + j] = nl_nan();
    if (tid == 0) {
      c.value[b] = nl_nan();
      if (c.pivots) c.pivots[b] = done;
      c.status[b] = status;
    }
    return;
  }
  if (tid < kNlMaxSide) { yv[tid] = 0.0; xv[tid] = 0.0; }
  __syncthreads();
  if (tid < m && row_label[tid] < n) yv[row_label[tid]] = nl_clamp(t[tid * ld + n]);
  if (tid < n && col_label[tid] >= n) xv[col_label[tid] - n] = nl_clamp(t[m * ld + tid]);
  __syncthreads();
  if (wave == 0) {
    const double mine = yv[lane];
    const double total = wave_nl_sum(mine, n);
    if (lane < n) c.y[b * n + lane] = mine / total;
    if (lane == 0) {
      c.value[b] = nl_value(total, span, base) / pre;
      if (c.pivots) c.pivots[b] = done;
      c.status[b] = kNlOk;
    }
  } else if (wave == 1) {
    const double mine = xv[lane];
    const double total = wave_nl_sum(mine, m);
    if (lane < m) c.x[b * m + lane] = mine / total;
  }
}

}  // namespace

extern "C" {

int osg_nash_lp(osg_ctx* ctx, int rows, int cols, int64_t n_problems, const double* matrices, double* row_strategy,
                double* col_strategy, double* value, int32_t* pivots, int32_t* status, int on_host) {
  const std::string who = "osg_nash_lp";
  if (!ctx) return set_error(OSG_ERR_INVALID, who + ": null context");
  if (n_problems < 0) return set_error(OSG_ERR_INVALID, who + ": n_problems is negative");
  if (rows < 1 || rows > kNlMaxSide || cols < 1 || cols > kNlMaxSide)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": a matrix of " + std::to_string(rows) + " rows and " + std::to_string(cols) +
                                              " columns (served: 1 to 64 of each)");
  if (n_problems > kNlMaxProblems)
    return set_error(OSG_ERR_UNSUPPORTED, who + ": " + std::to_string(n_problems) + " problems exceed the limit of " + std::to_string(kNlMaxProblems) + " per call");
  if (n_problems == 0) return OSG_OK;
  if (!matrices || !row_strategy || !col_strategy || !value || !status) return set_error(OSG_ERR_INVALID, who + ": null argument");

  NlCall c{};
  c.m = rows;
  c.n = cols;
  c.ld = nl_stride(cols);
  hipStream_t st = ctx->stream;
  const size_t B = static_cast<size_t>(n_problems), cells = static_cast<size_t>(rows) * cols;
  if (on_host) {
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at += align_up(bytes); return o; };
    const size_t o_matrices = take(sizeof(double) * B * cells), o_x = take(sizeof(double) * B * rows), o_y = take(sizeof(double) * B * cols);
    const size_t o_value = take(sizeof(double) * B), o_pivots = take(sizeof(int32_t) * B), o_status = take(sizeof(int32_t) * B);
    void* ptr = nullptr;
    if (int rc = osg_ctx_scratch(ctx, at, &ptr)) return rc;
    unsigned char* scratch = static_cast<unsigned char*>(ptr);
    OSG_HIP(hipMemcpyAsync(scratch + o_matrices, matrices, sizeof(double) * B * cells, hipMemcpyHostToDevice, st));
    c.matrices = reinterpret_cast<const double*>(scratch + o_matrices);
    c.x = reinterpret_cast<double*>(scratch + o_x);
    c.y = reinterpret_cast<double*>(scratch + o_y);
    c.value = reinterpret_cast<double*>(scratch + o_value);
    c.pivots = pivots ? reinterpret_cast<int32_t*>(scratch + o_pivots) : nullptr;
    c.status = reinterpret_cast<int32_t*>(scratch + o_status);
  } else {
    c.matrices = matrices; c.x = row_strategy; c.y = col_strategy; c.value = value; c.pivots = pivots; c.status = status;
  }
  const size_t lds = sizeof(double) * nl_lds_doubles(rows, c.ld);
  if (lds > (32u << 10) && raise_lds_cap(reinterpret_cast<const void*>(&k_nash_lp), static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(OSG_ERR_UNSUPPORTED, who + ": the device does not grant " + std::to_string(lds) + " bytes of LDS to a workgroup");
  }
  k_nash_lp<<<dim3(static_cast<unsigned>(B)), dim3(kNlThreads), lds, st>>>(c);
  OSG_HIP(hipGetLastError());
  if (on_host) {
    OSG_HIP(hipMemcpyAsync(row_strategy, c.x, sizeof(double) * B * rows, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipMemcpyAsync(col_strategy, c.y, sizeof(double) * B * cols, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipMemcpyAsync(value, c.value, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    if (pivots) OSG_HIP(hipMemcpyAsync(pivots, c.pivots, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipMemcpyAsync(status, c.status, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    OSG_HIP(hipStreamSynchronize(st));
  }
  return OSG_OK;
}

}  // extern "C"
