// Per-infostate action values and reaches of a policy on the flattened tree (TreeWalkCalculator, action_value.py:87-216;
// Calculator, action_value_vs_best_response.py:63-156): the arithmetic is osg_action_values.h's, here in two forms.
//   k_qvalues_small   ONE workgroup, one launch, a barrier between the phases: trees the one-workgroup evaluation serves.
//                     sigma, the members' reach products and the [H, P] values sit in LDS where they fit 150 KiB,
//                     else in the evaluation's scratch in memory.
//   k_qvalues         (k_qv_sigma, k_qv_reach, k_qv_values per tree level, k_qv_infostates) full-grid launches, the
//                     stream order is the barrier, like k_geval_*; one WAVEFRONT per infostate adds its members' terms
//                     in member order from the lanes' registers (k_geval_best's pattern).
// Phases: sigma (the evaluated policy, the best responder's rows replaced by the indicator of its action); the P + 1
// reach products of every member history from its root path; the values bottom-up; every infostate's sums.  No
// floating-point atomics; both forms run the same functions on the same values in the same order: the same bits.
#include "osg_cfr_internal.h"
#include "osg_action_values.h"

namespace {

constexpr int kQvThreads = 256;
constexpr size_t kQvLdsLimit = 150 * 1024;   // the budget k_eval_jobs allows itself

struct QvCall {
  const double* src;        // [I, A] the cumulative table (mode 0) or a policy (mode 1)
  int mode;
  int responder;            // -1: nobody
  double brv;               // the responder's best-response value (the evaluation's)
  const int32_t* best;      // [I] the evaluation's argmax (read at the responder's rows only)
  const int32_t* path_off;  // [M + 1]
  const int32_t* path;
  int M;
  double* sigma;            // [I, A] scratch
  double* rm;               // [M, P + 1] scratch
  double* value;            // [H, P] scratch
  double* root;             // [P] then the best-response value
  int32_t* best_out;        // [I]
  QvTables out;
};

OSG_D void qv_sigma_of(const Tree& t, const QvCall& c, int i, double* sigma) {
  const bool own = c.responder >= 0 && t.info_player[i] == c.responder;
  const int best = own ? c.best[i] : -1;
  qv_sigma_row(c.src + static_cast<size_t>(i) * t.A, sigma + static_cast<size_t>(i) * t.A, t.nact[i], t.A, c.mode, best);
  c.best_out[i] = best;
}
OSG_D void qv_values_of(const Tree& t, const QvCall& c, int h, const double* sigma, double* value) {
  const int P = t.P, k = t.kind[h];
  if (k == kTerminalNode) {
    for (int q = 0; q < P; ++q) value[static_cast<size_t>(h) * P + q] = t.term_ret[static_cast<size_t>(h) * P + q];
    return;
  }
  const int fc = t.first_child[h], nc = t.nchild[h];
  const double* prob = k == kChanceNode ? t.edge_prob + fc : sigma + static_cast<size_t>(t.info[h]) * t.A;
  for (int q = 0; q < P; ++q) value[static_cast<size_t>(h) * P + q] = qv_node_value(prob, value, fc, nc, P, q);
}

__global__ void __launch_bounds__(kQvThreads) k_qv_sigma(Tree t, QvCall c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) c.root[t.P] = c.brv;
  if (i >= t.I) return;
  qv_sigma_of(t, c, i, c.sigma);
}
__global__ void __launch_bounds__(kQvThreads) k_qv_reach(Tree t, QvCall c) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= c.M) return;
  qv_member_reach(c.path, c.path_off[m], c.path_off[m + 1], t.P, c.sigma, t.edge_prob, c.rm + static_cast<size_t>(m) * (t.P + 1));
}
__global__ void __launch_bounds__(kQvThreads) k_qv_values(Tree t, QvCall c, int l) {
  const int h = t.level_off[l] + blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= t.level_off[l + 1]) return;
  qv_values_of(t, c, h, c.sigma, c.value);
  if (h == 0)
    for (int q = 0; q < t.P; ++q) c.root[q] = c.value[q];
}
// One WAVEFRONT per infostate: the lanes take 64 members at a time, every lane forms its member's term, and the terms
// are added IN MEMBER ORDER from the lanes' registers (readlane with a uniform index): qv_infostate's sums, bit for bit.
__global__ void __launch_bounds__(kQvThreads) k_qv_infostates(Tree t, QvCall c) {
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (i >= t.I) return;   // (wave-uniform)
  const int P = t.P, A = t.A, p = t.info_player[i], n = t.nact[i];
  const int m0 = t.mem_off[i], cnt = t.mem_off[i + 1] - m0;
  const QvTables& o = c.out;
  auto member = [&](int c0) {   // the lane's member of the chunk that starts at c0 (lanes past the end: zeros, never added)
    QvMember x{0.0, 0.0, 0.0, 0.0};
    if (c0 + lane < cnt) x = qv_member(c.rm + static_cast<size_t>(m0 + c0 + lane) * (P + 1), P, p);
    return x;
  };
  const QvMember first = member(0);
  double reach = 0.0, cf = 0.0, chance = 0.0;
  for (int c0 = 0; c0 < cnt; c0 += 64) {
    const int here = cnt - c0 < 64 ? cnt - c0 : 64;
    const QvMember x = c0 == 0 ? first : member(c0);
    const double cft = qv_cf_reach_term(x);
    for (int j = 0; j < here; ++j) cf += readlane_f64(cft, j);
    for (int j = 0; j < here; ++j) reach += readlane_f64(x.reach, j);
    for (int j = 0; j < here; ++j) chance += readlane_f64(x.chance, j);
  }
  if (lane == 0) {
    o.reach[i] = reach;
    o.cf_reach[i] = cf;
    o.chance_reach[i] = chance;
    o.player_reach[i] = cnt > 0 ? c.rm[static_cast<size_t>(m0 + cnt - 1) * (P + 1) + p] : 0.0;   // the last member's (qv_infostate)
  }
  for (int a = 0; a < A; ++a) {
    double cfq = 0.0, own = 0.0;
    for (int q = 0; q < P; ++q) {
      double w = 0.0;
      if (a < n)
        for (int c0 = 0; c0 < cnt; c0 += 64) {
          const int here = cnt - c0 < 64 ? cnt - c0 : 64;
          const QvMember x = c0 == 0 ? first : member(c0);
          double term = 0.0, cterm = 0.0;
          if (lane < here) {
            const double v = c.value[static_cast<size_t>(t.first_child[t.mem[m0 + c0 + lane]] + a) * P + q];
            term = qv_weighted_term(v, x);
            cterm = qv_cf_value_term(v, x);
          }
          for (int j = 0; j < here; ++j) w += readlane_f64(term, j);
          if (q == p)
            for (int j = 0; j < here; ++j) cfq += readlane_f64(cterm, j);
        }
      if (lane == 0) o.weighted[(static_cast<size_t>(i) * A + a) * P + q] = w;
      if (q == p) own = w;
    }
    if (lane == 0) {
      o.q[static_cast<size_t>(i) * A + a] = a < n ? qv_action_value(own, reach) : 0.0;
      o.cf_q[static_cast<size_t>(i) * A + a] = cfq;
    }
  }
}

// The resident form: the same phases by ONE workgroup.  in_lds: sigma, rm and value are carved from dynamic LDS.
__global__ void __launch_bounds__(1024) k_qvalues_small(Tree t, QvCall c, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) double qv_smem[];
  const int P = t.P;
  const int tid = threadIdx.x, nt = blockDim.x;
  double* sigma = in_lds ? qv_smem : c.sigma;
  double* rm = in_lds ? sigma + static_cast<size_t>(t.I) * t.A : c.rm;
  double* value = in_lds ? rm + static_cast<size_t>(c.M) * (P + 1) : c.value;
  for (int i = tid; i < t.I; i += nt) qv_sigma_of(t, c, i, sigma);
  __syncthreads();
  for (int m = tid; m < c.M; m += nt)
    qv_member_reach(c.path, c.path_off[m], c.path_off[m + 1], P, sigma, t.edge_prob, rm + static_cast<size_t>(m) * (P + 1));
  for (int l = t.D - 1; l >= 0; --l) {
    for (int h = t.level_off[l] + tid; h < t.level_off[l + 1]; h += nt) qv_values_of(t, c, h, sigma, value);
    __syncthreads();
  }
  if (tid < P) c.root[tid] = value[tid];
  if (tid == 0) c.root[P] = c.brv;
  for (int i = tid; i < t.I; i += nt)
    qv_infostate(i, t.info_player[i], t.nact[i], t.A, P, t.mem_off[i], t.mem_off[i + 1], t.mem, t.first_child, rm, value, c.out);
}

size_t qv_small_lds_bytes(const osg_cfr* s) {
  return sizeof(double) * (static_cast<size_t>(s->I) * s->A + s->mem.size() * (s->P + 1) + static_cast<size_t>(s->H) * s->P);
}

// The results of a call, on the device: root [P] | best-response value | reach, cf_reach, chance_reach, player_reach [I]
// | q, cf_q [I, A] | weighted [I, A, P]; best_index [I].  Allocated at the solver's first call.
size_t qv_out_doubles(const osg_cfr* s) {
  const size_t I = s->I, IA = I * s->A;
  return s->P + 1 + 4 * I + 2 * IA + IA * s->P;
}

}  // namespace

extern "C" {

int osg_cfr_action_values(osg_cfr* s, int which_policy, const double* policy, int responder, int on_host,
                          const osg_action_values_out* out) {
  if (!s || !out) return set_error(OSG_ERR_INVALID, "osg_cfr_action_values: null argument");
  if (which_policy < 0 || which_policy > 2) return set_error(OSG_ERR_INVALID, "osg_cfr_action_values: which_policy must be 0, 1 or 2");
  if (which_policy == 2 && !policy) return set_error(OSG_ERR_INVALID, "osg_cfr_action_values: which_policy == 2 needs policy");
  if (responder < -1 || responder >= s->P)
    return set_error(OSG_ERR_INVALID, "osg_cfr_action_values: responder must be -1 or a player (" + std::to_string(responder) + " of " +
                                          std::to_string(s->P) + " players)");
  if (responder >= 0 && s->P != 2)
    return set_error(OSG_ERR_UNSUPPORTED, "osg_cfr_action_values: a best responder needs a 2-player game (" + std::to_string(s->P) + " players)");
  if (!s->eval_ok) return set_error(OSG_ERR_UNSUPPORTED, "osg_cfr_action_values: an information state spans several tree levels");
  if (which_policy != 2)
    if (int rc = cfr_sub_error(s)) return rc;
  hipStream_t st = s->ctx->stream;
  const int P = s->P;
  const size_t I = s->I, IA = I * s->A, M = s->mem.size();
  if (!s->d_qv_out) OSG_HIP(s->d_qv_out.alloc(qv_out_doubles(s)));
  if (!s->d_qv_best) OSG_HIP(s->d_qv_best.alloc(I));
  double* d_pol = eval_policy_slot(s);
  double brv = 0.0;
  if (responder >= 0) {
    // the existing best-response evaluation first: it leaves the argmax of every infostate in d_best
    std::vector<double> h_pol, br(P, 0.0);
    const double* eval_policy = policy;
    if (which_policy == 2 && !on_host) {   // (the evaluation takes its table from the host)
      h_pol.resize(IA);
      OSG_HIP(hipMemcpyAsync(h_pol.data(), policy, sizeof(double) * IA, hipMemcpyDeviceToHost, st));
      OSG_HIP(hipStreamSynchronize(st));
      eval_policy = h_pol.data();
    }
    if (int rc = osg_cfr_evaluate_policy(s, which_policy, eval_policy, nullptr, br.data(), nullptr, nullptr)) return rc;
    brv = br[responder];
  }
  QvCall c;
  c.mode = which_policy == 0 ? 0 : 1;
  c.src = which_policy == 0 ? s->cum() : which_policy == 1 ? s->cur() : policy;
  if (which_policy == 2 && on_host) {
    OSG_HIP(hipMemcpyAsync(d_pol, policy, sizeof(double) * IA, hipMemcpyHostToDevice, st));
    c.src = d_pol;   // (sigma is formed in place)
  }
  c.responder = responder;
  c.brv = brv;
  c.best = s->eval.best;
  c.path_off = s->d_path_off; c.path = s->d_path; c.M = static_cast<int>(M);
  c.sigma = d_pol;
  c.rm = member_reach_in_reach(s);
  c.value = s->eval.scratch;
  double* o = s->d_qv_out;
  c.root = o;
  c.best_out = s->d_qv_best;
  c.out.reach = o + P + 1; c.out.cf_reach = c.out.reach + I; c.out.chance_reach = c.out.cf_reach + I;
  c.out.player_reach = c.out.chance_reach + I; c.out.q = c.out.player_reach + I; c.out.cf_q = c.out.q + IA;
  c.out.weighted = c.out.cf_q + IA;
  const Tree t = s->tree();
  auto blocks = [](size_t n) { return dim3(static_cast<unsigned>(std::max<size_t>((n + kQvThreads - 1) / kQvThreads, 1))); };
  if (action_values_take_the_grid(s)) {
    k_qv_sigma<<<blocks(I), dim3(kQvThreads), 0, st>>>(t, c);
    k_qv_reach<<<blocks(M), dim3(kQvThreads), 0, st>>>(t, c);
    for (int l = s->D - 1; l >= 0; --l)
      k_qv_values<<<blocks(static_cast<size_t>(s->level_off[l + 1] - s->level_off[l])), dim3(kQvThreads), 0, st>>>(t, c, l);
    k_qv_infostates<<<blocks(I * 64), dim3(kQvThreads), 0, st>>>(t, c);
    s->last_eval_kernel = "k_qvalues";
  } else {
    size_t lds = qv_small_lds_bytes(s);
    if (lds > kQvLdsLimit || raise_lds_cap(reinterpret_cast<const void*>(&k_qvalues_small), static_cast<int>(lds)) != hipSuccess) {
      (void)hipGetLastError();
      lds = 0;
    }
    k_qvalues_small<<<dim3(1), dim3(level_threads(s)), lds, st>>>(t, c, lds > 0 ? 1 : 0);
    s->last_eval_kernel = "k_qvalues_small";
  }
  OSG_HIP(hipGetLastError());
  const hipMemcpyKind kind = on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  auto give = [&](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, kind, st) : hipSuccess;
  };
  OSG_HIP(give(out->root_values, c.root, sizeof(double) * P));
  OSG_HIP(give(out->action_values, c.out.q, sizeof(double) * IA));
  OSG_HIP(give(out->cf_reach, c.out.cf_reach, sizeof(double) * I));
  OSG_HIP(give(out->player_reach, c.out.player_reach, sizeof(double) * I));
  OSG_HIP(give(out->reach, c.out.reach, sizeof(double) * I));
  OSG_HIP(give(out->chance_reach, c.out.chance_reach, sizeof(double) * I));
  OSG_HIP(give(out->cf_reach_by_value, c.out.cf_q, sizeof(double) * IA));
  OSG_HIP(give(out->weighted_values, c.out.weighted, sizeof(double) * IA * P));
  if (responder >= 0) {
    OSG_HIP(give(out->best_response_value, c.root + P, sizeof(double)));
    OSG_HIP(give(out->best_index, c.best_out, sizeof(int32_t) * I));
  }
  if (on_host) {
    OSG_HIP(hipStreamSynchronize(st));
    if (which_policy != 2)   // the tables are only as good as the launches that wrote them
      if (int rc = cfr_sub_error(s)) return rc;
  }
  return OSG_OK;
}

}  // extern "C"
