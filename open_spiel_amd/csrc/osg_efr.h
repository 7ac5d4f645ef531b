// Extensive-form regret minimization (Morrill et al. 2021, arXiv 2102.06973; EFRSolver of
// open_spiel/python/algorithms/efr.py): the arithmetic of ONE history, ONE member, ONE (infostate, deviation) and ONE
// infostate, host + device, and the host-side construction of the deviation tables.  The kernels of osg_cfr_efr.hip run
// exactly these functions, and so does tests/native/efr_host_test.cpp on the CPU against the runs the reference's own
// file left in tests/golden/efr_vectors.npz.
//
// A deviation of infostate I is a swap of I's actions (external: every action -> target; internal: source -> target),
// a 0/1 weight per earlier own decision on the way to I ("remembered"), and one remembered action per such decision.
// memreach(d, sigma) is the product, over the remembered decisions root to leaf, of sigma's probability of the
// remembered action at that earlier infostate (1 with nothing remembered).  One iteration, all players at once:
//   regret pass, policy sigma_t:  for every member history h of I in depth-first order, unless every player's reach of h
//     is 0:  cum(I, a) += sigma(a) reach_own(h);  R(I, d) += memreach(d) ((cf(h) (T_d sigma_I) . u(h, .)) - cf(h) v(h))
//   policy pass, top-down:  at every member h of I in depth-first order  y(key d) += max(0, R(I, d)) memreach(d), the
//     row is regret-matched from y and written; the last member's row stands.  Deviations of I with the same swap share
//     one y.  y starts at 0 if the regret pass reached a member of I, else at what the previous iteration left (the
//     reference resets it where the regret pass visits).  memreach here reads, for every earlier own decision, the row
//     as it stood when THAT ancestor history was visited: the policy pass keeps a row per member history (mpol).
//   regret matching:  z = sum y; z <= 0: uniform.  External sets only: sigma(a) = sum of y / z over the keys with
//     target a.  Otherwise the minimum-norm least-squares solution of [sum (y / z) T - Id; 1 ... 1] x = e_last (one-sided
//     Jacobi SVD, singular values <= eps sigma_max dropped as LAPACK's gelsd does), clipped to [0, 1] and divided by
//     its sum.
// Where the reference looks up a remembered action it pairs the i-th LEGAL action of the earlier infostate with the
// probability of ACTION ID i (efr.py:620-629): with legal actions {1, 2} the remembered action 1 reads the probability
// of action 0, which is 0, and 2 reads that of 1.  The tables here hold what it reads (a column, or kEfrZeroCol).
// Every sum has one order (stated at each function); nothing here may be contracted into a fused multiply-add: the
// library and the host test are compiled with -ffp-contract=off.  No floating-point atomics.
#ifndef OSG_EFR_H_
#define OSG_EFR_H_

#include <math.h>
#include <stdint.h>

#include "osg_common.h"

namespace osg {

constexpr int kEfrMaxA = 4;                      // widest policy row (kuhn 2, leduc 3)
constexpr int kEfrMaxKeys = kEfrMaxA * kEfrMaxA;   // distinct swaps of a row: A external + A (A - 1) internal
constexpr int kEfrMaxMemory = 8;                 // earlier own decisions on a path (kuhn 1, leduc 3)
constexpr int kEfrMaxPlayers = 10;
constexpr unsigned kEfrZeroCol = 0xF;            // "reads a probability that is always 0"
constexpr int64_t kEfrMaxDeviations = int64_t{1} << 26;

enum EfrType {
  kEfrBlindAction = 0, kEfrInformedAction, kEfrBlindCf, kEfrInformedCf, kEfrBps, kEfrCfps, kEfrCsps, kEfrTips, kEfrBhv, kEfrTypes
};
OSG_HD bool efr_external_only(int type) { return type == kEfrBlindAction || type == kEfrBlindCf || type == kEfrBps; }

// What an iteration reads, built once per solver (device pointers in the kernels, host ones in the test).  Histories are
// numbered level by level with a parent's children contiguous (first_child + action index).
struct EfrTree {
  int H, I, A, P, D, M, L, ND, external_only;
  int64_t Dtot;
  const int32_t* level_off;    // [D + 1]
  const int32_t* first_child;  // [H]
  const uint8_t* kind;         // [H] 0 chance, 1 decision, 2 terminal
  const uint8_t* nchild;       // [H]
  const int8_t* actor;         // [H]
  const int32_t* info;         // [H]
  const double* edge_prob;     // [H] chance probability of the incoming edge
  const double* term_ret;      // [H, P]
  const int32_t* mem_off;      // [I + 1] member histories of every infostate, depth-first order
  const int32_t* mem;          // [M]
  const int32_t* nact;         // [I]
  const int8_t* info_player;   // [I]
  const int32_t* path_off;     // [M + 1] root path of member m: slot << 24 | is_chance << 23 | index (policy cell / history)
  const int32_t* path;
  const int32_t* dev_off;      // [I + 1] the deviations of an infostate, the reference's order
  const int32_t* dev_info;     // [Dtot]
  const int32_t* dev_desc;     // [Dtot] target | (source + 1) << 4 (0: external) | y slot << 8 | remembered mask << 16
  const uint32_t* dev_cols;    // [Dtot] 4 bits per earlier own decision: the column read there, or kEfrZeroCol
  const int32_t* nkeys;        // [I]
  const int8_t* key_desc;      // [I, kEfrMaxKeys] target | (source + 1) << 4
  const int32_t* own_len;      // [I] earlier own decisions
  const int32_t* own_info;     // [I, L] their infostates, root to leaf
  const int32_t* mown;         // [M, L] the member indices of the ancestor histories where they were taken
  const int32_t* depth_off;    // [ND + 1] the infostates of own-decision depth k: depth_info[depth_off[k] ...)
  const int32_t* depth_info;   // [I]
};

struct EfrState {
  double* pol;       // [I, A] current policy
  double* cum;       // [I, A] cumulative policy
  double* R;         // [Dtot] cumulative regret | y [I, kEfrMaxKeys] behind it (one allocation: the checkpoint)
  double* y;
  double* value;     // [H, P]
  double* mcf;       // [M] counterfactual reach of the member
  double* mown;      // [M] its own-player reach
  double* mpol;      // [M, A] the row written at the member's visit in the policy pass
  int32_t* live;     // [M] 0: every player's reach is 0, the reference's walk does not enter
  int32_t* visited;  // [I] some member is live
};

// ---- evaluation ------------------------------------------------------------------------------------------------
// Returns of every player at h under pol, from the children's (efr.py:311-328, 341-375): 0 + p_0 v_0 + p_1 v_1 + ...
OSG_HD void efr_value_item(const EfrTree& t, const EfrState& s, int h) {
  const int P = t.P, k = t.kind[h];
  if (k == 2) {
    for (int p = 0; p < P; ++p) s.value[static_cast<size_t>(h) * P + p] = t.term_ret[static_cast<size_t>(h) * P + p];
    return;
  }
  const int fc = t.first_child[h], nc = t.nchild[h];
  const int row = k == 1 ? t.info[h] * t.A : 0;
  for (int p = 0; p < P; ++p) {
    double v = 0.0;
    for (int a = 0; a < nc; ++a) {
      const double pr = k == 0 ? t.edge_prob[fc + a] : s.pol[row + a];
      v = v + pr * s.value[static_cast<size_t>(fc + a) * P + p];
    }
    s.value[static_cast<size_t>(h) * P + p] = v;
  }
}

// Reaches of member m (efr.py:319-320, 364-366: each a product from 1 in path order), whether the walk enters it
// (:338), its counterfactual reach prod(reach[:player]) * prod(reach[player + 1:]) (:377-379, chance last).
OSG_HD void efr_reach_item(const EfrTree& t, const EfrState& s, int m) {
  double reach[kEfrMaxPlayers + 1];
  for (int p = 0; p <= t.P; ++p) reach[p] = 1.0;
  for (int e = t.path_off[m]; e < t.path_off[m + 1]; ++e) {
    const int code = t.path[e];
    const int slot = (code >> 24) & 0xF, idx = code & 0x7FFFFF;
    reach[slot] = reach[slot] * (((code >> 23) & 1) ? t.edge_prob[idx] : s.pol[idx]);
  }
  const int me = t.actor[t.mem[m]];
  bool live = false;
  for (int p = 0; p < t.P; ++p) live = live || reach[p] != 0.0;
  double before = 1.0, after = 1.0;
  for (int p = 0; p < me; ++p) before = before * reach[p];
  for (int p = me + 1; p <= t.P; ++p) after = after * reach[p];
  s.mcf[m] = before * after;
  s.mown[m] = reach[me];
  s.live[m] = live ? 1 : 0;
}

// cum(I, a) += sigma(a) reach_own(h) over the live members in order (efr.py:357-362).
OSG_HD void efr_cumulate_item(const EfrTree& t, const EfrState& s, int i) {
  int any = 0;
  for (int m = t.mem_off[i]; m < t.mem_off[i + 1]; ++m) {
    if (!s.live[m]) continue;
    any = 1;
    for (int a = 0; a < t.nact[i]; ++a) s.cum[i * t.A + a] = s.cum[i * t.A + a] + s.pol[i * t.A + a] * s.mown[m];
  }
  s.visited[i] = any;
}

// The product over the remembered decisions, root to leaf, from 1 (efr.py:1100-1120).  rows[j]: the row (infostate, or
// member history) of earlier own decision j in the table `pol`.
OSG_HD double efr_memreach(int desc, uint32_t cols, const int32_t* rows, int A, const double* pol) {
  const int mask = (desc >> 16) & 0xFF;
  double r = 1.0;
  for (int j = 0; j < kEfrMaxMemory; ++j) {
    if (!((mask >> j) & 1)) continue;
    const unsigned c = (cols >> (4 * j)) & 0xF;
    r = r * (c == kEfrZeroCol ? 0.0 : pol[static_cast<size_t>(rows[j]) * A + c]);
  }
  return r;
}

// T_d sigma (efr.py:1310-1317, 1352): row r = sum over the columns c with T[r][c] = 1 of sigma(c), ascending from 0.
OSG_HD void efr_deviate(int target, int source, int n, const double* sigma, double* out) {
  for (int r = 0; r < n; ++r) {
    double v = 0.0;
    for (int c = 0; c < n; ++c) {
      const bool one = source < 0 ? r == target : ((r == c && c != source) || (r == target && c == source));
      if (one) v = v + sigma[c];
    }
    out[r] = v;
  }
}

// R(I, d) += memreach ((dev_value cf) - (cf v)) at every live member in order (efr.py:377-408).  k: deviation index.
OSG_HD void efr_regret_item(const EfrTree& t, const EfrState& s, int64_t k) {
  const int i = t.dev_info[k], n = t.nact[i], P = t.P, pl = t.info_player[i];
  const int desc = t.dev_desc[k];
  const int target = desc & 0xF, source = ((desc >> 4) & 0xF) - 1;
  const double mr = efr_memreach(desc, t.dev_cols[k], t.own_info + static_cast<size_t>(i) * t.L, t.A, s.pol);
  double dev[kEfrMaxA];
  efr_deviate(target, source, n, s.pol + static_cast<size_t>(i) * t.A, dev);
  double r = s.R[k];
  for (int m = t.mem_off[i]; m < t.mem_off[i + 1]; ++m) {
    if (!s.live[m]) continue;
    const int h = t.mem[m], fc = t.first_child[h];
    double dv = 0.0;
    for (int a = 0; a < n; ++a) dv = dv + dev[a] * s.value[static_cast<size_t>(fc + a) * P + pl];
    const double cf = s.mcf[m];
    r = r + mr * ((dv * cf) - (cf * s.value[static_cast<size_t>(h) * P + pl]));
  }
  s.R[k] = r;
}

// ---- regret matching -------------------------------------------------------------------------------------------
// Minimum-norm least-squares solution of G x = e_last for the (n + 1) x n matrix G (column-major g[c][r]) by a
// one-sided Jacobi SVD: columns are rotated in the fixed cyclic order (0,1), (0,2), ..., (n-2,n-1) until a whole sweep
// rotates none; then x = sum over the columns j with |g_j| > eps max|g| of v_j g_j[last] / |g_j|^2.  Returns the rank.
OSG_HD int efr_min_norm_solve(double g[kEfrMaxA][kEfrMaxA + 1], int n, double* x) {
  const double eps = 2.220446049250313e-16;
  double v[kEfrMaxA][kEfrMaxA];
  for (int c = 0; c < n; ++c)
    for (int r = 0; r < n; ++r) v[c][r] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int r = 0; r <= n; ++r) {
          alpha = alpha + g[p][r] * g[p][r];
          beta = beta + g[q][r] * g[q][r];
          gamma = gamma + g[p][r] * g[q][r];
        }
        if (gamma == 0.0 || fabs(gamma) <= eps * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
        for (int r = 0; r <= n; ++r) {
          const double a = g[p][r], b = g[q][r];
          g[p][r] = cs * a - sn * b;
          g[q][r] = sn * a + cs * b;
        }
        for (int r = 0; r < n; ++r) {
          const double a = v[p][r], b = v[q][r];
          v[p][r] = cs * a - sn * b;
          v[q][r] = sn * a + cs * b;
        }
      }
    if (!rotated) break;
  }
  double norm2[kEfrMaxA], largest = 0.0;
  for (int c = 0; c < n; ++c) {
    double sq = 0.0;
    for (int r = 0; r <= n; ++r) sq = sq + g[c][r] * g[c][r];
    norm2[c] = sq;
    largest = sq > largest ? sq : largest;
  }
  for (int r = 0; r < n; ++r) x[r] = 0.0;
  int rank = 0;
  const double cut = eps * sqrt(largest);
  for (int c = 0; c < n; ++c) {
    if (!(sqrt(norm2[c]) > cut)) continue;
    ++rank;
    const double w = g[c][n] / norm2[c];
    for (int r = 0; r < n; ++r) x[r] = x[r] + v[c][r] * w;
  }
  return rank;
}

// EFRSolver._regret_matching (efr.py:498-561) from the y of the row's keys, in key order.  keys: target | (source + 1) << 4.
// rank (may be null): the solve's rank, -1 where none was made.
OSG_HD void efr_regret_match(int n, int nkeys, const int8_t* keys, const double* y, bool external_only, double* out, int* rank) {
  if (rank) *rank = -1;
  double z = 0.0;
  for (int k = 0; k < nkeys; ++k) z = z + y[k];
  if (!(z > 0.0)) {
    for (int a = 0; a < n; ++a) out[a] = 1.0 / n;
    return;
  }
  if (external_only) {   // column 0 of sum (y / z) T
    for (int a = 0; a < n; ++a) out[a] = 0.0;
    for (int k = 0; k < nkeys; ++k) {
      const int target = keys[k] & 0xF;
      out[target] = out[target] + y[k] / z;
    }
    return;
  }
  double g[kEfrMaxA][kEfrMaxA + 1];
  for (int c = 0; c < n; ++c) {
    for (int r = 0; r < n; ++r) g[c][r] = r == c ? -1.0 : 0.0;
    g[c][n] = 1.0;
  }
  for (int k = 0; k < nkeys; ++k) {
    const double w = y[k] / z;
    const int target = keys[k] & 0xF, source = ((keys[k] >> 4) & 0xF) - 1;
    if (source < 0) {
      for (int c = 0; c < n; ++c) g[c][target] = g[c][target] + w;
    } else {
      for (int c = 0; c < n; ++c)
        if (c != source) g[c][c] = g[c][c] + w;
      g[source][target] = g[source][target] + w;
    }
  }
  double x[kEfrMaxA];
  const int rk = efr_min_norm_solve(g, n, x);
  if (rank) *rank = rk;
  double sum = 0.0;
  for (int a = 0; a < n; ++a) {
    x[a] = x[a] < 0.0 ? 0.0 : (x[a] > 1.0 ? 1.0 : x[a]);
    sum = sum + x[a];
  }
  for (int a = 0; a < n; ++a) out[a] = x[a] / sum;
}

// The policy pass at infostate i (efr.py:236-286): every member in order adds max(0, R) memreach of every deviation to
// its key's y, the row is regret-matched and kept as the member's; the last one becomes the infostate's.
OSG_HD void efr_policy_item(const EfrTree& t, const EfrState& s, int i) {
  const int n = t.nact[i], nk = t.nkeys[i];
  double y[kEfrMaxKeys], row[kEfrMaxA];
  for (int k = 0; k < nk; ++k) y[k] = s.visited[i] ? 0.0 : s.y[static_cast<size_t>(i) * kEfrMaxKeys + k];
  for (int a = 0; a < n; ++a) row[a] = s.pol[i * t.A + a];
  for (int m = t.mem_off[i]; m < t.mem_off[i + 1]; ++m) {
    for (int64_t k = t.dev_off[i]; k < t.dev_off[i + 1]; ++k) {
      const int desc = t.dev_desc[k];
      const double r = s.R[k] > 0.0 ? s.R[k] : 0.0;
      const double mr = efr_memreach(desc, t.dev_cols[k], t.mown + static_cast<size_t>(m) * t.L, t.A, s.mpol);
      const int slot = (desc >> 8) & 0xFF;
      y[slot] = y[slot] + r * mr;
    }
    efr_regret_match(n, nk, t.key_desc + static_cast<size_t>(i) * kEfrMaxKeys, y, t.external_only != 0, row, nullptr);
    for (int a = 0; a < n; ++a) s.mpol[static_cast<size_t>(m) * t.A + a] = row[a];
  }
  for (int k = 0; k < nk; ++k) s.y[static_cast<size_t>(i) * kEfrMaxKeys + k] = y[k];
  for (int a = 0; a < n; ++a) s.pol[i * t.A + a] = row[a];
}

}  // namespace osg

// ---- the deviation tables (host) -----------------------------------------------------------------------------------
#include <algorithm>
#include <string>
#include <vector>

namespace osg {

struct EfrHostTree {   // what the tables are built from: the solver's flattened tree
  int H = 0, I = 0, A = 0;
  const int32_t* parent = nullptr;   // [H]
  const uint8_t* kind = nullptr;     // [H]
  const int8_t* actor = nullptr;     // [H]
  const int32_t* info = nullptr;     // [H]
  const uint8_t* aidx = nullptr;     // [H] index of the incoming edge among the parent's children
  const int32_t* mem_off = nullptr;  // [I + 1]
  const int32_t* mem = nullptr;      // [M]
  const int32_t* mem_index = nullptr;  // [H] member position of a decision history
  const int32_t* nact = nullptr;     // [I]
  const int32_t* legal = nullptr;    // [I, A] action ids, ascending
  const int8_t* info_player = nullptr;  // [I]
};

struct EfrTables {
  int type = -1, L = 1, ND = 0, max_per_info = 0;
  std::vector<int32_t> dev_off, dev_info, dev_desc, nkeys, own_len, own_info, mown, depth_off, depth_info;
  std::vector<uint32_t> dev_cols;
  std::vector<int8_t> key_desc;
  // as the reference states them, for comparison: per deviation the source (-1 external), whether the weights are its
  // `None`, and per earlier decision the weight and the remembered ACTION ID (-1 padding)
  std::vector<int8_t> dev_none, dev_weight, dev_memory;
};

inline int efr_type_of(const std::string& name) {
  static const char* const names[][4] = {
      {"blind action", nullptr}, {"informed action", nullptr}, {"blind cf", "blind counterfactual", nullptr},
      {"informed cf", "informed counterfactual", nullptr}, {"bps", "blind partial sequence", nullptr},
      {"cfps", "cf partial sequence", "counterfactual partial sequence", nullptr}, {"csps", "casual partial sequence", nullptr},
      {"tips", "twice informed partial sequence", nullptr}, {"bhv", "single target behavioural", "behavioural", nullptr}};
  for (int t = 0; t < kEfrTypes; ++t)
    for (int k = 0; k < 4 && names[t][k]; ++k)
      if (name == names[t][k]) return t;
  return -1;
}

// Returns an empty string, or why the tables cannot be built.
inline std::string efr_build_tables(const EfrHostTree& tr, int type, EfrTables* out) {
  EfrTables& T = *out;
  T = EfrTables();
  T.type = type;
  const int I = tr.I, A = tr.A, M = tr.mem_off[I];
  if (A > kEfrMaxA) return "a policy row wider than " + std::to_string(kEfrMaxA) + " actions";
  // the earlier own decisions of every member, root to leaf
  std::vector<std::vector<int32_t>> chain_member(M);
  std::vector<std::vector<int32_t>> own_info(I), own_aidx(I);
  int L = 1;
  for (int i = 0; i < I; ++i)
    for (int m = tr.mem_off[i]; m < tr.mem_off[i + 1]; ++m) {
      std::vector<int32_t> infos, aidxs, members;
      for (int32_t v = tr.mem[m]; tr.parent[v] >= 0; v = tr.parent[v]) {
        const int32_t par = tr.parent[v];
        if (tr.kind[par] != 1 || tr.actor[par] != tr.info_player[i]) continue;
        infos.insert(infos.begin(), tr.info[par]);
        aidxs.insert(aidxs.begin(), tr.aidx[v]);
        members.insert(members.begin(), tr.mem_index[par]);
      }
      if (m == tr.mem_off[i]) {
        own_info[i] = infos;
        own_aidx[i] = aidxs;
      } else if (infos != own_info[i] || aidxs != own_aidx[i]) {
        return "imperfect recall: two histories of an information state differ in the player's own earlier decisions";
      }
      chain_member[m] = members;
      L = std::max<int>(L, static_cast<int>(infos.size()));
    }
  if (L > kEfrMaxMemory) return "more than " + std::to_string(kEfrMaxMemory) + " earlier own decisions on a path";
  T.L = L;
  T.own_len.resize(I);
  T.own_info.assign(static_cast<size_t>(I) * L, 0);
  T.mown.assign(static_cast<size_t>(M) * L, 0);
  for (int i = 0; i < I; ++i) {
    T.own_len[i] = static_cast<int32_t>(own_info[i].size());
    T.ND = std::max(T.ND, T.own_len[i] + 1);
    for (size_t j = 0; j < own_info[i].size(); ++j) T.own_info[static_cast<size_t>(i) * L + j] = own_info[i][j];
    for (int m = tr.mem_off[i]; m < tr.mem_off[i + 1]; ++m)
      for (size_t j = 0; j < chain_member[m].size(); ++j) T.mown[static_cast<size_t>(m) * L + j] = chain_member[m][j];
  }
  T.depth_off.assign(T.ND + 1, 0);
  for (int k = 0; k < T.ND; ++k) {
    for (int i = 0; i < I; ++i)
      if (T.own_len[i] == k) T.depth_info.push_back(i);
    T.depth_off[k + 1] = static_cast<int32_t>(T.depth_info.size());
  }

  struct Dev { int target, source; bool none; std::vector<int> weight, memory; };
  T.dev_off.assign(1, 0);
  T.nkeys.assign(I, 0);
  T.key_desc.assign(static_cast<size_t>(I) * kEfrMaxKeys, 0);
  std::vector<Dev> devs;
  for (int i = 0; i < I; ++i) {
    const int n = tr.nact[i], len = T.own_len[i];
    std::vector<int> history(len);
    std::vector<std::vector<int>> prior(len);
    for (int j = 0; j < len; ++j) {
      const int e = own_info[i][j];
      for (int a = 0; a < tr.nact[e]; ++a) prior[j].push_back(tr.legal[e * A + a]);
      history[j] = prior[j][own_aidx[i][j]];
    }
    devs.clear();
    const std::vector<int> ones(len, 1), zeros(len, 0);
    auto prefix = [&](int k) {
      std::vector<int> w(len, 0);
      for (int j = 0; j < k; ++j) w[j] = 1;
      return w;
    };
    auto external = [&](bool none, const std::vector<int>& w, const std::vector<int>& mem) {
      for (int t = 0; t < n; ++t) devs.push_back(Dev{t, -1, none, w, mem});
    };
    auto internal = [&](bool none, const std::vector<int>& w, const std::vector<int>& mem) {
      for (int t = 0; t < n; ++t)
        for (int s = 0; s < n; ++s)
          if (s != t) devs.push_back(Dev{t, s, none, w, mem});
    };
    // weight vectors of the partial-sequence sets: none, everything (if there is a history), every proper prefix
    auto sequences = [&](auto&& add) {
      add(true, zeros, history);
      if (len > 0) add(false, ones, history);
      for (int k = 0; k < len; ++k) add(false, prefix(k), history);
    };
    // a prefix remembered, the first forgotten decision replaced by each of its legal actions in turn
    auto modified = [&](auto&& add) {
      for (int k = 0; k < len; ++k)
        for (int alt : prior[k]) {
          std::vector<int> mem = history;
          mem[k] = alt;
          add(false, prefix(k), mem);
        }
    };
    switch (type) {
      case kEfrBlindAction: external(false, ones, history); break;
      case kEfrInformedAction: internal(false, ones, history); break;
      case kEfrBlindCf: external(true, zeros, zeros); break;
      case kEfrInformedCf: internal(true, zeros, zeros); break;
      case kEfrBps: sequences(external); break;
      case kEfrCfps: sequences(internal); break;
      case kEfrCsps:
        modified(external);
        external(false, ones, history);
        internal(true, zeros, zeros);
        external(true, zeros, zeros);
        break;
      case kEfrTips:
        modified(internal);
        internal(true, zeros, zeros);
        break;
      case kEfrBhv:
        if (len == 0) {
          internal(true, zeros, history);
        } else {
          for (int k = 0; k < len; ++k) {   // decisions 0 .. k - 1 remembered as ANY legal sequence, 0 .. k enumerated
            std::vector<int> pick(k + 1, 0);
            while (true) {
              std::vector<int> mem(len, 0);
              for (int j = 0; j <= k; ++j) mem[j] = prior[j][pick[j]];
              internal(false, prefix(k), mem);
              int j = k;
              while (j >= 0 && ++pick[j] == static_cast<int>(prior[j].size())) pick[j--] = 0;
              if (j < 0) break;
            }
          }
        }
        break;
      default: return "no such deviation set";
    }
    if (static_cast<int64_t>(T.dev_info.size() + devs.size()) > kEfrMaxDeviations)
      return "more than " + std::to_string(kEfrMaxDeviations) + " deviations";
    T.max_per_info = std::max<int>(T.max_per_info, static_cast<int>(devs.size()));
    int8_t* keys = T.key_desc.data() + static_cast<size_t>(i) * kEfrMaxKeys;
    for (const Dev& d : devs) {
      const int8_t key = static_cast<int8_t>(d.target | ((d.source + 1) << 4));
      int slot = 0;
      while (slot < T.nkeys[i] && keys[slot] != key) ++slot;
      if (slot == T.nkeys[i]) keys[T.nkeys[i]++] = key;
      int mask = 0;
      uint32_t cols = 0;
      for (int j = 0; j < len; ++j) {
        T.dev_weight.push_back(d.none ? -1 : static_cast<int8_t>(d.weight[j]));
        T.dev_memory.push_back(static_cast<int8_t>(d.memory[j]));
        if (d.none || !d.weight[j]) continue;
        // the remembered action's POSITION among the legal actions there is read as an ACTION ID (see the top)
        int pos = 0;
        while (prior[j][pos] != d.memory[j]) ++pos;
        unsigned col = kEfrZeroCol;
        for (size_t c = 0; c < prior[j].size(); ++c)
          if (prior[j][c] == pos) col = static_cast<unsigned>(c);
        mask |= 1 << j;
        cols |= col << (4 * j);
      }
      for (int j = len; j < L; ++j) {
        T.dev_weight.push_back(-1);
        T.dev_memory.push_back(-1);
      }
      T.dev_none.push_back(d.none ? 1 : 0);
      T.dev_info.push_back(i);
      T.dev_desc.push_back(key | (slot << 8) | (mask << 16));
      T.dev_cols.push_back(cols);
    }
    T.dev_off.push_back(static_cast<int32_t>(T.dev_info.size()));
  }
  return std::string();
}

}  // namespace osg

#endif  // OSG_EFR_H_
