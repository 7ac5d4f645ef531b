// The tabular solvers' launch plans, worked out on the host tree: plain C++, no device call, no environment switch.
//
//   deal_cut           the first level with a node that is not a chance node, and the subtree of every history below it
//   plan_split         k_cfr_split: one workgroup per deal subtree                         (build_split, osg_cfr_split.hip)
//   plan_sub           k_cfr_sub: bins, forest pieces, member records; plan_sub_fold: the fold's shares once the grid
//                      is known                                                           (build_sub, osg_cfr_sub.hip)
//   plan_eval_jobs     k_eval_jobs: one expected-returns job per subtree, one best-response job per component
//                                                                                         (build_eval_jobs, osg_cfr_eval.hip)
//   plan_resident      the packed records of the LDS-resident MCCFR kernels               (build_resident_tree, osg_cfr_mccfr.hip)
//   mccfr_launch_plan  which MCCFR kernel a mini-batch takes, and its geometry            (mccfr_sample_impl, osg_cfr_mccfr.hip)
//
// Each planner is a pure function of a HostTree (a view of the vectors struct osg_cfr holds) and a few numbers the
// caller read from the device or the environment; its result says `ok`, or `why` not: which gate refused.  The builders
// named on the right add what needs the device: LDS caps, occupancy, uploads.  tests/native/cfr_plan_host_test.cpp
// includes this header alone and decodes every plan back to the tree.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

namespace osg_cfr_impl {

constexpr int kMaxA = 4;        // widest decision node the MCCFR frame holds (kuhn 2, leduc 3)
constexpr int kMaxFrames = 24;  // traverser decision nodes on one path

enum NodeKind : uint8_t { kChanceNode = 0, kDecisionNode = 1, kTerminalNode = 2 };

constexpr int kSplitMaxA = 4;       // widest policy row the split kernel folds
constexpr int kSplitOwnerPath = 10;  // decision entries of a root path kept in registers

// The member records of k_cfr_sub (round 5): 64 bytes per member — regret terms [4], average-policy terms [4] — written
// by the member's thread as whole 16-byte pieces and fetched by the fold the same way (7 eight-byte stores and loads per
// member before).  A record that carries no terms says so in its first word: a quiet NaN whose low word is 1 (the member
// was pruned) or 2 + u (upper member u of the forest form: written once by the host, its terms are formed in the fold).
constexpr unsigned int kSubFlagHi = 0x7FF80000u;
constexpr int kSubRecDoubles = 8;
constexpr int kSubBarWords = 16 + 16 * 64;   // grid barrier words: a cooperative grid of up to 1 024 workgroups

constexpr int kSubThreads = 1024;
constexpr int kSubKD = 4;            // decision histories per thread: ND <= 4096
constexpr int kSubFoldInfos = 64;    // infostates a workgroup folds per round (one wavefront adds them up)
constexpr int kSubFoldX = 2;         // member records a thread fetches per round: <= 2048 per round
constexpr int kSubCodeChunks = 8;    // int4 chunks of path codes a member record holds at most (requested together)

// Where OSG_MCCFR_TREE is unset, the flat kernel's tree goes to global memory when that helps (round 6: 3.04e9 -> 4.23e9 trajectories/s at 16 x 2^20,
// profiles/r06c_mccfr_tree_in_l2_ab.txt).
constexpr bool kMccfrTreeGlobalDefault = true;

// The flattened tree on the host (build_tree, osg_cfr.hip): histories level by level, a parent's children contiguous.
struct HostTree {
  int H = 0, I = 0, A = 0, P = 0, D = 0, M = 0;
  const int32_t* level_off = nullptr;    // [D+1]
  const int32_t* parent = nullptr;       // [H]
  const int32_t* first_child = nullptr;  // [H]
  const uint8_t* kind = nullptr;         // [H]
  const uint8_t* nchild = nullptr;       // [H]
  const uint8_t* aidx = nullptr;         // [H] index of the incoming edge among the parent's children
  const int8_t* actor = nullptr;         // [H] acting player, -1 at chance / terminal nodes
  const int32_t* info = nullptr;         // [H] infostate id of a decision node, else -1
  const int32_t* mem_off = nullptr;      // [I+1]
  const int32_t* mem = nullptr;          // [M] member histories of every infostate, DFS order
  const int32_t* nact = nullptr;         // [I]
  const int8_t* info_player = nullptr;   // [I]
  const double* edge_prob = nullptr;     // [H] chance probability of the incoming edge (parent is chance)
  const double* term_ret = nullptr;      // [H, P] Returns() of terminal nodes
  const int32_t* path_off = nullptr;     // [M+1] root path of every member
  const int32_t* path = nullptr;         // entries: slot << 24 | is_chance << 23 | index
  const int32_t* info_level = nullptr;   // [I] tree level of the infostate's member histories
};

inline bool path_entry_is_chance(int32_t code) { return ((code >> 23) & 1) != 0; }
// The product of the chance probabilities on member m's root path, multiplied in path order.
inline double path_chance_product(const HostTree& t, int m) {
  double chance = 1.0;
  for (int e = t.path_off[m]; e < t.path_off[m + 1]; ++e)
    if (path_entry_is_chance(t.path[e])) chance *= t.edge_prob[t.path[e] & 0x7FFFFF];
  return chance;
}
inline void push_double_bits(std::vector<int32_t>* out, double v) {   // low word, high word
  int64_t bits;
  std::memcpy(&bits, &v, sizeof bits);
  out->push_back(static_cast<int32_t>(bits & 0xFFFFFFFF));
  out->push_back(static_cast<int32_t>(bits >> 32));
}

// ---------------------------------------------------------------------------
// The deal cut: the tree below its leading chance levels falls into one subtree per history of level L.
// ---------------------------------------------------------------------------
struct DealCut {
  int L = -1;                    // -1: no cut, `why`
  int G = 0;                     // histories on level L
  const char* why = nullptr;
  std::vector<int32_t> level_of; // [H]
  std::vector<int32_t> sub_of;   // [H] the subtree of a history at or below level L, -1 above
};

inline DealCut deal_cut(const HostTree& t) {
  DealCut c;
  int L = 0;
  for (; L < t.D; ++L) {
    bool all_chance = true;
    for (int h = t.level_off[L]; h < t.level_off[L + 1]; ++h) all_chance &= t.kind[h] == kChanceNode;
    if (!all_chance) break;
  }
  if (L < 1 || L >= t.D - 1) { c.why = "no deal cut: the tree has no leading chance level, or nothing below the cut"; return c; }
  c.L = L;
  c.G = t.level_off[L + 1] - t.level_off[L];
  c.level_of.assign(t.H, 0);
  c.sub_of.assign(t.H, -1);
  for (int l = 0; l < t.D; ++l)
    for (int h = t.level_off[l]; h < t.level_off[l + 1]; ++h) c.level_of[h] = l;
  for (int h = t.level_off[L]; h < t.H; ++h)
    c.sub_of[h] = h < t.level_off[L + 1] ? h - t.level_off[L] : c.sub_of[t.parent[h]];
  return c;
}

// The histories of every label (a subtree, a bin) in ascending order, which is level order, and each one's position in
// its list: the descendants of a history are a contiguous range on every level.
inline void histories_by_label(const std::vector<int32_t>& label, int first, int H, std::vector<std::vector<int32_t>>* hist,
                               std::vector<int32_t>* loc_of) {
  loc_of->assign(H, -1);
  for (int h = first; h < H; ++h) {
    std::vector<int32_t>& list = (*hist)[label[h]];
    (*loc_of)[h] = static_cast<int32_t>(list.size());
    list.push_back(h);
  }
}
// kind | nchild << 2 | level << 10 | (actor + 1) << 16
inline int32_t history_desc(const HostTree& t, int h, int level) {
  return t.kind[h] | (t.nchild[h] << 2) | (level << 10) | ((t.actor[h] + 1) << 16);
}

// ---------------------------------------------------------------------------
// k_cfr_split: one workgroup per deal subtree, at most one per CU, every subtree small enough for one thread per history.
// ---------------------------------------------------------------------------
struct SplitLimits { int cus = 0; };
struct SplitHostPlan {
  bool ok = false;
  const char* why = nullptr;
  int G = 0, L = 0, NL = 0, NM = 0, NI = 0, threads = 0;
  size_t lds_bytes = 0, br_lds_bytes = 0;   // br: the CFR-BR pass set keeps one more [I, A] array (the effective policy)
  std::vector<int32_t> nloc, desc, fc, row, glob, mem_m, mem_hloc, info_list;   // SplitTree's arrays
};

inline SplitHostPlan plan_split(const HostTree& t, SplitLimits lim) {
  SplitHostPlan p;
  const auto refuse = [&p](const char* why) { p.why = why; return p; };
  if (t.H < 2000 || t.D >= 64) return refuse("fewer than 2000 histories, or 64 levels and more");
  const DealCut cut = deal_cut(t);
  if (cut.L < 0) return refuse(cut.why);
  const int G = cut.G, L = cut.L;
  if (G < 8 || G > lim.cus) return refuse("fewer than 8 deal subtrees, or more than compute units");
  const std::vector<int32_t>& sub_of = cut.sub_of;
  std::vector<std::vector<int32_t>> hist(G);
  std::vector<int32_t> loc_of;
  histories_by_label(sub_of, t.level_off[L], t.H, &hist, &loc_of);
  int NL = 0;
  for (int g = 0; g < G; ++g) NL = std::max<int>(NL, static_cast<int>(hist[g].size()));
  if (NL > 1024) return refuse("a deal subtree of more than 1024 histories");
  const int threads = std::max(64, (NL + 63) / 64 * 64);
  std::vector<std::vector<int32_t>> mem_m(G), infos(G);
  std::vector<int32_t> seen(t.I, -1);
  for (int i = 0; i < t.I; ++i)
    for (int m = t.mem_off[i]; m < t.mem_off[i + 1]; ++m) {
      const int h = t.mem[m];
      if (sub_of[h] < 0) return refuse("a decision node above the cut");
      int decisions = 0;
      for (int e = t.path_off[m]; e < t.path_off[m + 1]; ++e) decisions += path_entry_is_chance(t.path[e]) ? 0 : 1;
      if (decisions > kSplitOwnerPath) return refuse("more decisions on a root path than the owner keeps in registers");
      mem_m[sub_of[h]].push_back(m);
      if (seen[i] != sub_of[h]) {  // members of one infostate inside one subtree are adjacent in DFS order or not: check all
        bool have = false;
        for (int32_t x : infos[sub_of[h]]) have |= x == i;
        if (!have) infos[sub_of[h]].push_back(i);
        seen[i] = sub_of[h];
      }
    }
  int NM = 1, NI = 1;
  for (int g = 0; g < G; ++g) {
    NM = std::max<int>(NM, static_cast<int>(mem_m[g].size()));
    NI = std::max<int>(NI, static_cast<int>(infos[g].size()));
  }
  if (NM > threads || NI > threads) return refuse("more members or infostates in a subtree than threads");
  const size_t IA = static_cast<size_t>(t.I) * t.A;
  const size_t lds = sizeof(double) * (static_cast<size_t>(NL) * t.P + NL + 3 * IA) + 16;
  if (lds > 150 * 1024) return refuse("values and tables beyond 150 KB of LDS");
  const size_t GL = static_cast<size_t>(G) * NL;
  p.nloc.resize(G);
  p.desc.assign(GL, kTerminalNode); p.fc.assign(GL, 0); p.row.assign(GL, 0); p.glob.assign(GL, 0);
  p.mem_m.assign(static_cast<size_t>(G) * NM, -1); p.mem_hloc.assign(static_cast<size_t>(G) * NM, 0);
  p.info_list.assign(static_cast<size_t>(G) * NI, -1);
  for (int g = 0; g < G; ++g) {
    p.nloc[g] = static_cast<int32_t>(hist[g].size());
    for (size_t j = 0; j < hist[g].size(); ++j) {
      const int h = hist[g][j];
      const size_t at = static_cast<size_t>(g) * NL + j;
      p.desc[at] = history_desc(t, h, cut.level_of[h]);
      p.fc[at] = t.kind[h] == kTerminalNode ? 0 : loc_of[t.first_child[h]];
      p.row[at] = t.kind[h] == kDecisionNode ? t.info[h] * t.A : 0;
      p.glob[at] = h;
    }
    for (size_t k = 0; k < mem_m[g].size(); ++k) {
      p.mem_m[static_cast<size_t>(g) * NM + k] = mem_m[g][k];
      p.mem_hloc[static_cast<size_t>(g) * NM + k] = loc_of[t.mem[mem_m[g][k]]];
    }
    for (size_t k = 0; k < infos[g].size(); ++k) p.info_list[static_cast<size_t>(g) * NI + k] = infos[g][k];
  }
  p.G = G; p.L = L; p.NL = NL; p.NM = NM; p.NI = NI; p.threads = threads;
  p.lds_bytes = lds;
  p.br_lds_bytes = lds + sizeof(double) * IA;
  p.ok = true;
  return p;
}

// ---------------------------------------------------------------------------
// k_cfr_sub: the same cut, any number of subtrees (a workgroup takes several in turn when the cooperative grid is
// smaller), up to 8 x 1024 histories each.  Round 5, forest form: with more subtrees than compute units the bins of the
// workgroups are packed — whole subtrees if they fit, else the pieces one level below the cut (SubTree's comment) — so
// that every workgroup sweeps one bin per pass.  pack = false keeps a subtree per bin.
// ---------------------------------------------------------------------------
struct SubLimits {
  int cus = 0;
  bool pack = true;                                      // OSG_CFR_SUB_PACK is not 0
  int max_histories_per_bin = 8 * kSubThreads;           // of a packed bin
  int max_decisions_per_bin = kSubKD * kSubThreads;      // rows of a packed bin, its pieces' upper parents included
  size_t lds_budget_bytes = 150 * 1024;                  // of a packed bin's values and policy rows
};
struct SubHostPlan {
  bool ok = false;
  const char* why = nullptr;
  bool forest = false;          // the bins hold pieces of level L + 1; the histories of level L belong to no bin
  bool packed = false;          // the bins hold several whole subtrees (never with forest)
  int G0 = 0, G = 0, L = 0, NL = 0, K = 0, ND = 0, PL = 0, NCP = 0, NR = 0;
  int piece_roots = 0;          // forest: histories on the pieces' level (root_value's length)
  size_t lds_bytes = 0;
  int fold_cap = 0;             // member records the fold stages per round
  std::vector<int32_t> nloc, desc, fc, aux, dec_row, dec_off, ndec, mem_off, sub_rec, info_off, info_list;   // SubTree's arrays
  std::vector<double> chance_prob, term_val, recbuf;
  std::vector<int32_t> nroot, root_loc, root_idx, upper_rec;
  std::vector<int32_t> bin_histories;   // [G]
  std::vector<int32_t> bin_members;     // [G, P]
};

inline SubHostPlan plan_sub(const HostTree& t, const SubLimits& lim) {
  SubHostPlan p;
  const auto refuse = [&p](const char* why) { p.ok = false; p.why = why; return p; };
  const int P = t.P, A = t.A;
  if (t.H < 4096 || t.D >= 63 || t.H >= (1 << 23)) return refuse("fewer than 4096 histories, 63 levels and more, or 2^23 histories and more");
  const DealCut cut = deal_cut(t);
  if (cut.L < 0) return refuse(cut.why);
  const int L = cut.L, G0 = cut.G;
  if (G0 < 8) return refuse("fewer than 8 deal subtrees");
  const std::vector<int32_t>& level_of = cut.level_of;
  // ---- the bins: which histories a workgroup sweeps together ----
  // sizes of every history's subtree (children have larger indices than their parent)
  std::vector<int32_t> sz(t.H, 1), szd(t.H, 0);
  for (int h = t.H - 1; h >= 1; --h) {
    szd[h] += t.kind[h] == kDecisionNode ? 1 : 0;
    sz[t.parent[h]] += sz[h];
    szd[t.parent[h]] += szd[h];
  }
  const int cus = std::max(1, lim.cus);
  // longest-processing-time packing of the histories of level `lp` into at most `cus` bins, balanced by subtree size
  auto pack = [&](int lp, std::vector<int32_t>* bin_of, int* bins) -> bool {
    const int n = t.level_off[lp + 1] - t.level_off[lp], base = t.level_off[lp];
    const int nb = std::min(n, cus);
    std::vector<int32_t> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sz[base + a] > sz[base + b]; });
    std::vector<int64_t> load(nb, 0), loadd(nb, 0), cnt(nb, 0);
    bin_of->assign(n, 0);
    for (int i : order) {
      int best = 0;
      for (int b = 1; b < nb; ++b)
        if (load[b] < load[best]) best = b;
      (*bin_of)[i] = best;
      load[best] += sz[base + i]; loadd[best] += szd[base + i]; ++cnt[best];
    }
    for (int b = 0; b < nb; ++b) {
      const int64_t nl = load[b], nd = loadd[b] + cnt[b];   // (+ the rows of the pieces' upper parents)
      if (nl > lim.max_histories_per_bin || nd > lim.max_decisions_per_bin || sizeof(double) * (nl + nd * A) > lim.lds_budget_bytes) return false;
    }
    *bins = nb;
    return true;
  };
  int G = G0, piece_level = L;
  bool upper = false;          // the histories of level L belong to no bin
  std::vector<int32_t> bin_of;
  if (G0 > cus && lim.pack) {
    int nb = 0;
    if (pack(L, &bin_of, &nb)) {
      G = nb; p.packed = true;
    } else if (L + 1 < t.D - 1 && pack(L + 1, &bin_of, &nb)) {
      G = nb; piece_level = L + 1; upper = true;
    } else {
      bin_of.clear();
    }
  }
  if (bin_of.empty()) {
    bin_of.resize(G0);
    for (int g = 0; g < G0; ++g) bin_of[g] = g;
  }
  std::vector<int32_t> sub_of(t.H, -1), loc_of;   // (here: the BIN of a history at or below the pieces' level)
  for (int h = t.level_off[piece_level]; h < t.H; ++h)
    sub_of[h] = h < t.level_off[piece_level + 1] ? bin_of[h - t.level_off[piece_level]] : sub_of[t.parent[h]];
  std::vector<std::vector<int32_t>> hist(G);
  histories_by_label(sub_of, t.level_off[piece_level], t.H, &hist, &loc_of);
  int NL = 0;
  for (int g = 0; g < G; ++g) NL = std::max<int>(NL, static_cast<int>(hist[g].size()));
  const int K = NL <= 2 * kSubThreads ? 2 : (NL <= 4 * kSubThreads ? 4 : 8);
  if (NL > 8 * kSubThreads) return refuse("a bin of more than 8 x 1024 histories");
  const size_t M = static_cast<size_t>(t.M);
  std::vector<std::vector<int32_t>> members(static_cast<size_t>(G) * P);
  std::vector<int32_t> upper_members;            // forest form: the members of level L, in member order
  std::vector<int32_t> upper_of(std::max<size_t>(M, 1), -1);
  for (size_t m = 0; m < M; ++m) {
    const int h = t.mem[m];
    if (sub_of[h] < 0) {
      if (!upper || level_of[h] != L) return refuse("a decision node above the cut");
      upper_of[m] = static_cast<int32_t>(upper_members.size());
      upper_members.push_back(static_cast<int32_t>(m));
      continue;
    }
    members[static_cast<size_t>(sub_of[h]) * P + t.actor[h]].push_back(static_cast<int32_t>(m));
  }
  p.bin_histories.resize(G);
  p.bin_members.resize(static_cast<size_t>(G) * P);
  for (int g = 0; g < G; ++g) {
    p.bin_histories[g] = static_cast<int32_t>(hist[g].size());
    for (int q = 0; q < P; ++q) p.bin_members[static_cast<size_t>(g) * P + q] = static_cast<int32_t>(members[static_cast<size_t>(g) * P + q].size());
  }
  const size_t GL = static_cast<size_t>(G) * NL;
  p.nloc.resize(G);
  p.desc.assign(GL, kTerminalNode | (63 << 10)); p.fc.assign(GL, 0); p.aux.assign(GL, 0);
  p.mem_off.assign(static_cast<size_t>(G) * P + 1, 0);
  p.info_off.assign(P + 1, 0);
  std::vector<int32_t>& desc = p.desc; std::vector<int32_t>& fc = p.fc; std::vector<int32_t>& aux = p.aux; std::vector<int32_t>& sub_rec = p.sub_rec;
  // the decisions of one player on a root path: the codes of a member record are P groups of `per_player` int4 chunks
  int most = 0;
  {
    std::vector<int> cnt(P);
    for (size_t m = 0; m < M; ++m) {
      std::fill(cnt.begin(), cnt.end(), 0);
      for (int e = t.path_off[m]; e < t.path_off[m + 1]; ++e)
        if (!path_entry_is_chance(t.path[e])) most = std::max(most, ++cnt[(t.path[e] >> 24) & 0xF]);
    }
  }
  const int per_player = std::max(1, (most + 3) / 4);
  if (per_player * P > kSubCodeChunks) return refuse("more decisions on a path than the packed member record keeps");
  const int PL = 4 * per_player * P;
  std::vector<std::vector<int32_t>> dec_rows(G);
  std::vector<std::map<int32_t, int32_t>> extra_row(G);
  std::vector<int32_t> anc, filled(P);
  int32_t n_members = 0;
  p.dec_off.assign(static_cast<size_t>(G) * (P + 2), 0);
  std::vector<std::vector<double>> chance_probs(G);
  for (int g = 0; g < G; ++g) {
    p.nloc[g] = static_cast<int32_t>(hist[g].size());
    // the bin's decision rows ordered by acting player (a pass re-fetches one player's rows only: SubTree's comment)
    std::vector<int32_t> next(P + 1, 0);
    for (int h : hist[g])
      if (t.kind[h] == kDecisionNode) ++next[t.actor[h] + 1];
    for (int q = 0; q < P; ++q) next[q + 1] += next[q];
    for (int q = 0; q <= P; ++q) p.dec_off[static_cast<size_t>(g) * (P + 2) + q] = next[q];
    dec_rows[g].assign(next[P], 0);
    for (size_t j = 0; j < hist[g].size(); ++j) {
      const int h = hist[g][j];
      const size_t at = static_cast<size_t>(g) * NL + j;
      desc[at] = history_desc(t, h, level_of[h]);
      fc[at] = t.kind[h] == kTerminalNode ? 0 : loc_of[t.first_child[h]];
      aux[at] = h;
      if (t.kind[h] == kDecisionNode) {
        aux[at] = next[t.actor[h]]++;
        dec_rows[g][aux[at]] = t.info[h] * A;
      } else if (t.kind[h] == kChanceNode) {
        aux[at] = static_cast<int32_t>(chance_probs[g].size());   // its outcome probabilities, staged in LDS
        for (int c = 0; c < t.nchild[h]; ++c) chance_probs[g].push_back(t.edge_prob[t.first_child[h] + c]);
      }
    }
    for (int q = 0; q < P; ++q) {
      for (int32_t m : members[static_cast<size_t>(g) * P + q]) {
        const int h = t.mem[m];
        const size_t at = static_cast<size_t>(g) * NL + loc_of[h];
        sub_rec.push_back(m);
        sub_rec.push_back(loc_of[h]);
        sub_rec.push_back(aux[at] | (static_cast<int32_t>(t.nact[t.info[h]]) << 24));
        sub_rec.push_back(fc[at]);
        // the root path, leaf to root: entry e of SmallTree::path is the edge out of the ancestor at depth e
        const int len = t.path_off[m + 1] - t.path_off[m];
        anc.resize(len);
        for (int e = len - 1, x = t.parent[h]; e >= 0; --e, x = t.parent[x]) anc[e] = x;
        std::vector<int32_t> codes(PL, -1);
        std::fill(filled.begin(), filled.end(), 0);
        for (int e = 0; e < len; ++e) {
          const int code = t.path[t.path_off[m] + e];
          if (path_entry_is_chance(code)) continue;
          const int pl = (code >> 24) & 0xF, a_idx = (code & 0x7FFFFF) - t.info[anc[e]] * A;
          if (a_idx < 0 || a_idx >= A) return refuse("a path entry outside its infostate's row (cannot happen)");
          int d_anc;
          if (sub_of[anc[e]] == g) {
            d_anc = aux[static_cast<size_t>(g) * NL + loc_of[anc[e]]];
          } else if (upper && sub_of[anc[e]] < 0 && level_of[anc[e]] == L) {
            // a deal root above the forest: its policy row rides behind the forest's own rows
            auto it = extra_row[g].find(anc[e]);
            if (it == extra_row[g].end()) {
              it = extra_row[g].emplace(anc[e], static_cast<int32_t>(dec_rows[g].size())).first;
              dec_rows[g].push_back(t.info[anc[e]] * A);
            }
            d_anc = it->second;
          } else {
            return refuse("a decision above the cut on a root path (cannot happen)");
          }
          codes[static_cast<size_t>(pl) * 4 * per_player + filled[pl]++] = d_anc * A + a_idx;
        }
        push_double_bits(&sub_rec, path_chance_product(t, m));
        sub_rec.push_back(0);
        sub_rec.push_back(0);
        // the codes as 16-bit halves (a code indexes the bin's ND * A <= 16 384 staged policy entries; 0xFFFF pads), the
        // record padded to whole 16-byte pieces
        for (int c = 0; c < PL; c += 2)
          sub_rec.push_back(static_cast<int32_t>((static_cast<uint32_t>(codes[c]) & 0xFFFFu) |
                                                 ((static_cast<uint32_t>(codes[c + 1]) & 0xFFFFu) << 16)));
        for (int c = PL / 2; c % 4 != 0; ++c) sub_rec.push_back(-1);
        ++n_members;
      }
      p.mem_off[static_cast<size_t>(g) * P + q + 1] = n_members;
    }
  }
  for (int q = 0; q < P; ++q) {
    for (int i = 0; i < t.I; ++i)
      if (t.info_player[i] == q) p.info_list.push_back(i);
    p.info_off[q + 1] = static_cast<int32_t>(p.info_list.size());
  }
  int ND = 2, NCP = 2;
  for (int g = 0; g < G; ++g) {
    ND = std::max<int>(ND, static_cast<int>(dec_rows[g].size()));
    NCP = std::max<int>(NCP, static_cast<int>(chance_probs[g].size()));
  }
  ND += ND & 1; NCP += NCP & 1;   // (even: the values and the fold's stage behind them stay 16-byte aligned)
  p.ndec.resize(G);
  p.dec_row.assign(static_cast<size_t>(G) * ND, 0);
  p.chance_prob.assign(static_cast<size_t>(G) * NCP, 0.0);
  for (int g = 0; g < G; ++g) {
    p.ndec[g] = static_cast<int32_t>(dec_rows[g].size());
    p.dec_off[static_cast<size_t>(g) * (P + 2) + P + 1] = p.ndec[g];   // (the upper parents' rows sit behind the players')
    std::copy(dec_rows[g].begin(), dec_rows[g].end(), p.dec_row.begin() + static_cast<size_t>(g) * ND);
    std::copy(chance_probs[g].begin(), chance_probs[g].end(), p.chance_prob.begin() + static_cast<size_t>(g) * NCP);
  }
  // dynamic LDS: [policy rows ND * A | chance probabilities NCP | values NL | spare]; the fold stages 64-byte member
  // records from the values on (one bin per workgroup: the rows stay) — the spare takes it to 2 048 records where there is room
  const size_t base_doubles = static_cast<size_t>(ND) * A + NCP + NL;
  if (sizeof(double) * base_doubles > 150 * 1024 || ND > kSubKD * kSubThreads) return refuse("a bin's rows, chance probabilities and values beyond 150 KB of LDS, or more than 4096 rows");
  const size_t lds_doubles = std::min<size_t>(static_cast<size_t>(ND) * A + NCP + static_cast<size_t>(kSubFoldX) * kSubThreads * kSubRecDoubles,
                                              (158 * 1024) / sizeof(double));
  const size_t lds = sizeof(double) * std::max(base_doubles, lds_doubles);
  const int fold_cap = static_cast<int>(std::min<size_t>((lds / sizeof(double) - static_cast<size_t>(ND) * A - NCP) / kSubRecDoubles,
                                                         static_cast<size_t>(kSubFoldX) * kSubThreads));
  // forest form: the pieces' roots (their values leave through root_value) and the upper members' records
  int NR = 0;
  const int root_base = t.level_off[piece_level];
  if (upper) {
    std::vector<std::vector<int32_t>> roots(G);
    for (int h = root_base; h < t.level_off[piece_level + 1]; ++h) roots[sub_of[h]].push_back(h);
    for (int g = 0; g < G; ++g) NR = std::max<int>(NR, static_cast<int>(roots[g].size()));
    p.nroot.resize(G);
    p.root_loc.assign(static_cast<size_t>(G) * NR, 0);
    p.root_idx.assign(static_cast<size_t>(G) * NR, 0);
    for (int g = 0; g < G; ++g) {
      p.nroot[g] = static_cast<int32_t>(roots[g].size());
      for (size_t r = 0; r < roots[g].size(); ++r) {
        p.root_loc[static_cast<size_t>(g) * NR + r] = loc_of[roots[g][r]];
        p.root_idx[static_cast<size_t>(g) * NR + r] = roots[g][r] - root_base;
      }
    }
    for (int32_t m : upper_members) {
      const int h = t.mem[m];
      // the root path of a deal root holds chance edges only, multiplied in path order
      for (int e = t.path_off[m]; e < t.path_off[m + 1]; ++e)
        if (!path_entry_is_chance(t.path[e])) return refuse("a decision above a deal root (cannot happen: every level above the cut is a chance level)");
      p.upper_rec.push_back(t.first_child[h] - root_base);
      p.upper_rec.push_back(t.info[h] * A);
      p.upper_rec.push_back(t.nact[t.info[h]]);
      p.upper_rec.push_back(0);
      push_double_bits(&p.upper_rec, path_chance_product(t, m));
      p.upper_rec.push_back(0);
      p.upper_rec.push_back(0);
    }
    p.piece_roots = t.level_off[piece_level + 1] - root_base;
  }
  if (static_cast<unsigned long long>(M) * kSubRecDoubles * 8 >= (1ull << 31)) return refuse("member records beyond 32-bit byte offsets");
  int widest = 0;   // the fold stages an infostate's member records in LDS: all of one infostate must fit a round
  for (int i = 0; i < t.I; ++i) widest = std::max(widest, t.mem_off[i + 1] - t.mem_off[i]);
  if (widest > fold_cap) return refuse("an infostate with more members than the fold stages in a round");
  {
    // the terminal returns of every bin by player, in the bin's local order: a pass starts with one coalesced copy into LDS
    const size_t n = static_cast<size_t>(G) * P * NL;
    if (n * sizeof(double) > (size_t{1} << 31)) return refuse("terminal values beyond 2 GB");
    p.term_val.assign(n, 0.0);
    for (int g = 0; g < G; ++g)
      for (size_t j = 0; j < hist[g].size(); ++j) {
        const int h = hist[g][j];
        if (t.kind[h] != kTerminalNode) continue;
        for (int q = 0; q < P; ++q)
          p.term_val[(static_cast<size_t>(g) * P + q) * NL + j] = t.term_ret[static_cast<size_t>(h) * P + q];
      }
  }
  // the members' 64-byte records: zero, but an upper member's says which one it is (kSubFlagHi | 2 + u)
  p.recbuf.assign(std::max<size_t>(M, 1) * kSubRecDoubles, 0.0);
  for (size_t m = 0; m < M; ++m)
    if (upper_of[m] >= 0) {
      const int64_t bits = (static_cast<int64_t>(kSubFlagHi) << 32) | static_cast<int64_t>(2 + upper_of[m]);
      std::memcpy(&p.recbuf[m * kSubRecDoubles], &bits, sizeof bits);
    }
  p.forest = upper;
  p.G0 = G0; p.G = G; p.L = L; p.NL = NL; p.K = K; p.ND = ND; p.PL = PL; p.NCP = NCP; p.NR = NR;
  p.lds_bytes = lds;
  p.fold_cap = fold_cap;
  p.ok = true;
  return p;
}

// The fold's shares on a cooperative grid of `grid` workgroups: a workgroup's run of the updating player's infostates
// (info_list order), balanced by members.  keep_rows: one bin per workgroup, the policy rows stay in LDS between passes.
struct SubFoldPlan {
  std::vector<int32_t> fold_info;   // [infostates in info_list order, 4] infostate, actions, first member, members
  std::vector<int32_t> fold_off;    // [P, grid + 1]
  bool keep_rows = false;
};

inline SubFoldPlan plan_sub_fold(const HostTree& t, const SubHostPlan& plan, int grid) {
  SubFoldPlan f;
  const std::vector<int32_t>& info_list = plan.info_list;
  const std::vector<int32_t>& info_off = plan.info_off;
  f.fold_info.resize(info_list.size() * 4);
  f.fold_off.assign(static_cast<size_t>(t.P) * (grid + 1), 0);
  for (size_t e = 0; e < info_list.size(); ++e) {
    const int i = info_list[e];
    f.fold_info[4 * e] = i; f.fold_info[4 * e + 1] = t.nact[i]; f.fold_info[4 * e + 2] = t.mem_off[i];
    f.fold_info[4 * e + 3] = t.mem_off[i + 1] - t.mem_off[i];
  }
  for (int q = 0; q < t.P; ++q) {
    int32_t* off = &f.fold_off[static_cast<size_t>(q) * (grid + 1)];
    int64_t total = 0;
    for (int e = info_off[q]; e < info_off[q + 1]; ++e) total += f.fold_info[4 * static_cast<size_t>(e) + 3] + 8;   // (+ the row's own cost)
    int64_t run = 0;
    int e = info_off[q];
    for (int w = 0; w < grid; ++w) {
      off[w] = e;
      const int64_t upto = total * (w + 1) / grid;
      while (e < info_off[q + 1] && run + (f.fold_info[4 * static_cast<size_t>(e) + 3] + 8) / 2 < upto) {
        run += f.fold_info[4 * static_cast<size_t>(e) + 3] + 8;
        ++e;
      }
    }
    off[grid] = info_off[q + 1];
    for (int w = grid - 1; w >= 0; --w)   // (everything is handed out: the last share takes what rounding left)
      if (off[w] > off[w + 1]) off[w] = off[w + 1];
  }
  f.keep_rows = grid >= plan.G;
  return f;
}

// ---------------------------------------------------------------------------
// k_eval_jobs: the deal cut; one expected-returns job per subtree; for every responder r the subtrees grouped into the
// connected components of "holds a member history of the same infostate of r", one best-response job per component.
// Trees of another shape, or with a component that does not fit a workgroup's LDS, keep the one-workgroup kernel.
// ---------------------------------------------------------------------------
struct JobsHostPlan {
  bool ok = false;
  const char* why = nullptr;
  int J = 0, L = 0, G = 0, NT = 0, threads = 0;
  size_t lds_bytes = 0;
  std::vector<int32_t> job, level_off, node_desc, node_fc, node_row, node_glob, info_ent, mem_ent;   // EvalJobs' arrays
};

inline JobsHostPlan plan_eval_jobs(const HostTree& t) {
  JobsHostPlan p;
  const auto refuse = [&p](const char* why) { p.why = why; return p; };
  if (t.H < 2000 || t.D >= 64 || t.P > 15) return refuse("fewer than 2000 histories, 64 levels and more, or more than 15 players");
  const int P = t.P, A = t.A, D = t.D;
  const DealCut cut = deal_cut(t);
  if (cut.L < 0) return refuse(cut.why);
  const int L = cut.L, G = cut.G, NT = t.level_off[L + 1];
  if (G < 4 || G > 65536) return refuse("fewer than 4 deal subtrees, or more than 65536");
  const std::vector<int32_t>& sub_of = cut.sub_of;
  const std::vector<int32_t>& level_of = cut.level_of;
  std::vector<std::vector<int32_t>> hist(G);
  for (int h = t.level_off[L]; h < t.H; ++h) hist[sub_of[h]].push_back(h);  // ascending h = level-major
  const int M = t.M;
  for (int m = 0; m < M; ++m)
    if (sub_of[t.mem[m]] < 0) return refuse("a decision node above the cut");
  // the groups of subtrees, kind by kind
  std::vector<std::vector<int32_t>> groups;  // subtree lists
  std::vector<int32_t> group_kind;
  for (int g = 0; g < G; ++g) { groups.push_back({g}); group_kind.push_back(0); }
  for (int r = 0; r < P; ++r) {
    std::vector<int32_t> uf(G);
    for (int g = 0; g < G; ++g) uf[g] = g;
    auto find = [&](int x) { while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; } return x; };
    for (int i = 0; i < t.I; ++i) {
      if (t.info_player[i] != r) continue;
      for (int m = t.mem_off[i] + 1; m < t.mem_off[i + 1]; ++m) {
        const int a = find(sub_of[t.mem[t.mem_off[i]]]), b = find(sub_of[t.mem[m]]);
        if (a != b) uf[std::max(a, b)] = std::min(a, b);
      }
    }
    std::vector<int32_t> slot(G, -1);
    for (int g = 0; g < G; ++g) {
      const int root = find(g);
      if (slot[root] < 0) { slot[root] = static_cast<int32_t>(groups.size()); groups.push_back({}); group_kind.push_back(1 + r); }
      groups[slot[root]].push_back(g);
    }
  }
  const int J = static_cast<int>(groups.size());
  p.job.assign(static_cast<size_t>(J) * 8, 0);
  p.level_off.assign(static_cast<size_t>(J) * (D + 1), 0);
  std::vector<int32_t> loc(t.H, -1), job_of_sub(G, -1);
  size_t lds = sizeof(double) * 2 * P * NT;
  int max_nodes = 0;
  const size_t IA = static_cast<size_t>(t.I) * A;
  for (int j = 0; j < J; ++j) {
    const int kind = group_kind[j], r = kind - 1;
    std::vector<int32_t> nodes;
    for (int g : groups[j]) nodes.insert(nodes.end(), hist[g].begin(), hist[g].end());
    std::sort(nodes.begin(), nodes.end());
    const int nn = static_cast<int>(nodes.size());
    for (int x = 0; x < nn; ++x) loc[nodes[x]] = x;
    const int n0 = static_cast<int>(p.node_desc.size());
    int at = 0;
    for (int l = 0; l <= D; ++l) {
      while (l < D && at < nn && level_of[nodes[at]] < l) ++at;
      p.level_off[static_cast<size_t>(j) * (D + 1) + l] = l == D ? nn : at;
    }
    for (int x = 0; x < nn; ++x) {
      const int h = nodes[x];
      p.node_desc.push_back(t.kind[h] | (t.nchild[h] << 2) | ((t.actor[h] + 1) << 10));
      p.node_fc.push_back(t.kind[h] == kTerminalNode ? 0 : loc[t.first_child[h]]);
      p.node_row.push_back(t.kind[h] == kDecisionNode ? t.info[h] * A : 0);
      p.node_glob.push_back(h);
    }
    const int i0 = static_cast<int>(p.info_ent.size() / 4), m0 = static_cast<int>(p.mem_ent.size() / 2);
    int ni = 0, nm = 0;
    if (kind != 0) {
      for (int g : groups[j]) job_of_sub[g] = j;
      for (int i = 0; i < t.I; ++i) {
        if (t.info_player[i] != r || t.mem_off[i + 1] == t.mem_off[i]) continue;
        if (job_of_sub[sub_of[t.mem[t.mem_off[i]]]] != j) continue;
        p.info_ent.insert(p.info_ent.end(), {i, t.info_level[i], nm, t.mem_off[i + 1] - t.mem_off[i]});
        ++ni;
        for (int m = t.mem_off[i]; m < t.mem_off[i + 1]; ++m) {
          p.mem_ent.insert(p.mem_ent.end(), {m, loc[t.mem[m]]});
          ++nm;
        }
      }
      for (int g : groups[j]) job_of_sub[g] = -1;
    }
    int32_t* jd = &p.job[static_cast<size_t>(j) * 8];
    jd[0] = kind; jd[1] = n0; jd[2] = nn; jd[3] = i0; jd[4] = ni; jd[5] = m0; jd[6] = nm;
    const size_t bytes = sizeof(double) * (IA + static_cast<size_t>(nn) * (kind == 0 ? P : 1) + nn + nm) +
                         sizeof(int32_t) * (3 * static_cast<size_t>(nn) + nm + t.I);
    lds = std::max(lds, bytes);
    max_nodes = std::max(max_nodes, nn);
  }
  if (lds > 150 * 1024) return refuse("a job beyond 150 KB of LDS");
  p.J = J; p.L = L; p.G = G; p.NT = NT; p.lds_bytes = lds;
  p.threads = std::max(64, std::min(1024, (max_nodes + 63) / 64 * 64));
  p.ok = true;
  return p;
}

// ---------------------------------------------------------------------------
// The LDS-resident MCCFR kernels' tree: 8 bytes per history + the distinct return vectors and chance probabilities.
//   low word:  kind | nchild << 2 | (actor + 1) << 8 | (infostate, or at a chance node whose outcomes all have the same
//              probability that probability's id + 1) << 12
//   high word: first child, or the terminal's return-vector id; | the incoming chance probability's id << 24
// Whether it fits one workgroup's LDS next to three [I, A] tables is the caller's question (lds_bytes).
// ---------------------------------------------------------------------------
struct ResidentHostPlan {
  bool ok = false;
  const char* why = nullptr;
  std::vector<uint64_t> rec;     // [H]
  std::vector<double> uret;      // [n_uret, P]
  std::vector<double> uprob;     // [n_uprob]
  int n_uret = 0, n_uprob = 0;
  size_t lds_bytes = 0;
};

inline ResidentHostPlan plan_resident(const HostTree& t, int solver) {
  ResidentHostPlan p;
  const auto refuse = [&p](const char* why) { p.why = why; return p; };
  if ((solver != 1 && solver != 2) || t.A < 1 || t.A > kMaxA) return refuse("not an MCCFR solver, or rows wider than the frame");
  if (t.H >= (1 << 24) || t.I >= (1 << 20)) return refuse("2^24 histories and more, or 2^20 infostates and more");
  p.rec.resize(t.H);
  std::unordered_map<std::string, uint32_t> ret_id;
  std::unordered_map<uint64_t, uint32_t> prob_id;
  const int P = t.P;
  // traverser frames one path can hold: decision nodes of one player from the root down
  std::vector<uint8_t> own(static_cast<size_t>(t.H) * P, 0);
  int max_frames = 0;
  for (int h = 0; h < t.H; ++h) {
    uint32_t x = t.kind[h] | (static_cast<uint32_t>(t.nchild[h]) << 2) |
                 (static_cast<uint32_t>(t.actor[h] + 1) << 8);
    uint32_t y = 0;
    if (t.nchild[h] > 63 || t.actor[h] + 1 > 15) return refuse("a node with more than 63 children, or more than 14 players");
    if (t.kind[h] == kDecisionNode) x |= static_cast<uint32_t>(t.info[h]) << 12;
    if (t.kind[h] == kTerminalNode) {
      std::string key(reinterpret_cast<const char*>(&t.term_ret[static_cast<size_t>(h) * P]), sizeof(double) * P);
      auto it = ret_id.find(key);
      if (it == ret_id.end()) {
        it = ret_id.emplace(key, static_cast<uint32_t>(ret_id.size())).first;
        for (int q = 0; q < P; ++q) p.uret.push_back(t.term_ret[static_cast<size_t>(h) * P + q]);
      }
      y = it->second;
    } else {
      y = static_cast<uint32_t>(t.first_child[h]);
    }
    if (h > 0 && t.kind[t.parent[h]] == kChanceNode) {
      uint64_t bits;
      std::memcpy(&bits, &t.edge_prob[h], sizeof bits);
      auto it = prob_id.find(bits);
      if (it == prob_id.end()) {
        if (prob_id.size() >= 256) return refuse("more than 256 distinct chance probabilities");
        it = prob_id.emplace(bits, static_cast<uint32_t>(prob_id.size())).first;
        p.uprob.push_back(t.edge_prob[h]);
      }
      y |= it->second << 24;
    }
    p.rec[h] = static_cast<uint64_t>(x) | (static_cast<uint64_t>(y) << 32);
    if (h > 0) {
      const int par = t.parent[h];
      for (int q = 0; q < P; ++q) {
        int d = own[static_cast<size_t>(par) * P + q] + (t.kind[par] == kDecisionNode && t.actor[par] == q ? 1 : 0);
        if (d > 255) return refuse("more than 255 decisions of one player on a path");
        own[static_cast<size_t>(h) * P + q] = static_cast<uint8_t>(d);
        max_frames = std::max(max_frames, d);
      }
    }
  }
  if (max_frames > kMaxFrames) return refuse("more traverser decisions on a path than frames");
  // Chance nodes whose outcomes all have the same probability (every chance node of kuhn and leduc: 1 / cards left)
  // say so in the field decision nodes use for their infostate id: index of that probability + 1, else 0.  The
  // traversal then samples without reading the children's records.
  for (int h = 0; h < t.H; ++h) {
    if (t.kind[h] != kChanceNode || t.nchild[h] == 0) continue;
    const uint32_t id0 = static_cast<uint32_t>(p.rec[t.first_child[h]] >> 56);
    bool same = true;
    for (int c = 1; c < t.nchild[h]; ++c) same &= static_cast<uint32_t>(p.rec[t.first_child[h] + c] >> 56) == id0;
    if (same) p.rec[h] |= static_cast<uint64_t>(id0 + 1) << 12;
  }
  if (p.uprob.empty()) p.uprob.push_back(1.0);
  p.n_uret = static_cast<int>(p.uret.size() / std::max(P, 1));
  p.n_uprob = static_cast<int>(p.uprob.size());
  const size_t IA = static_cast<size_t>(t.I) * t.A;
  p.lds_bytes = sizeof(double) * (3 * IA + p.uret.size() + p.uprob.size()) + sizeof(uint64_t) * t.H;
  p.ok = true;
  return p;
}

// ---------------------------------------------------------------------------
// Which MCCFR kernel a mini-batch of `trajectories` takes, and its launch geometry.
// ---------------------------------------------------------------------------
enum class MccfrForm { kGeneralEs, kGeneralOs, kResidentFlat, kResidentFlatTreeInL2, kResidentSplit1, kResidentSplit2, kResidentOs };
enum class MccfrTreeWhere { kUnset, kGlobal, kLds };   // OSG_MCCFR_TREE

struct MccfrLaunchInput {
  int solver = 1;                 // 1 external sampling, 2 outcome sampling
  int A = 0, P = 0, H = 0;
  size_t IA = 0;                  // I * A: the general kernels' delta tables go to LDS while 16 IA <= 64 KB
  bool resident_ok = false;       // ResidentPlan::ok
  size_t resident_lds_bytes = 0;
  bool general_kernel = false;    // osg_cfr_cfg.kernel == OSG_CFR_KERNEL_GENERAL
  int cus = 0;
  size_t lds_per_cu = 160 * 1024;
  int64_t trajectories = 0;       // > 0
  int split_max = 2;              // OSG_MCCFR_SPLIT: at most that many traverser levels are spread over lanes
  MccfrTreeWhere tree_where = MccfrTreeWhere::kUnset;
};
struct MccfrLaunchPlan {
  MccfrForm form = MccfrForm::kGeneralEs;
  int split = 0;
  bool tree_global = false;
  int threads = 256;
  int64_t groups = 0;
  size_t shmem_bytes = 0;
  int64_t lanes = 0;              // trajectories x the lanes each is spread over
  const char* last_kernel = nullptr;   // null: the general forms leave osg_cfr::last_kernel alone
};

inline MccfrLaunchPlan mccfr_launch_plan(const MccfrLaunchInput& in) {
  MccfrLaunchPlan p;
  p.lanes = in.trajectories;
  if (!(in.resident_ok && !in.general_kernel)) {
    // Persistent workgroups: each flushes its LDS delta tables once, so fewer, longer-lived
    // groups mean fewer global atomics (256 CUs x 4 groups).
    const size_t lds = sizeof(double) * 2 * in.IA;
    p.form = in.solver == 2 ? MccfrForm::kGeneralOs : MccfrForm::kGeneralEs;
    p.threads = 256;
    p.groups = std::min<int64_t>((in.trajectories + 255) / 256, 1024);
    p.shmem_bytes = lds <= 64 * 1024 ? lds : 0;
    return p;
  }
  // As many workgroups per CU as the LDS footprint allows.  A footprint that only fits once (leduc:
  // 143 KB) gets one group per CU, sized to the batch — every CU busy, up to 1024 lanes each; small
  // footprints (kuhn) get several 256- or 1024-lane groups per CU.
  int fit = static_cast<int>(in.lds_per_cu / std::max<size_t>(in.resident_lds_bytes, 1));
  // Mini-batches that leave lanes idle (fewer lanes than one round of the chip even with the split) run the
  // split form of the external-sampling kernel: 2 or 4 lanes per trajectory (split_max 0: never).
  const int q = in.A <= 2 ? 2 : 4;
  int split = 0;   // two levels while the lanes fit one round of the chip (2^14 trajectories: 31.4 us per step against 38.7
                   // with one level; 2^13: 26.7 against 37.2), else one level under the same condition, else the flat kernel
  if (in.solver != 2 && in.A >= 2) {
    const int64_t round = static_cast<int64_t>(in.cus) * 1024;
    if (in.split_max >= 2 && in.trajectories * q * q <= round) split = 2;
    else if (in.split_max >= 1 && in.trajectories * q <= round) split = 1;
  }
  int64_t lanes = in.trajectories;
  if (split) lanes *= split == 2 ? q * q : q;   // (the geometry below counts lanes)
  // Where the flat kernel reads the tree from: when the staged problem allows one workgroup per CU only (leduc: 143 KB,
  // 4 wavefronts per SIMD) but the tables alone would allow two (67 KB), the records can stay in global memory
  // (9 457 x 8 B, read-only: L2-resident) and two 1024-lane workgroups share a CU.
  size_t shmem_bytes = in.resident_lds_bytes;
  bool tree_global = false;
  {
    const size_t tables_only = in.resident_lds_bytes - sizeof(uint64_t) * in.H;
    const bool helps = fit <= 1 && in.lds_per_cu / std::max<size_t>(tables_only, 1) >= 2 &&
                       lanes >= static_cast<int64_t>(in.cus) * 2048;
    const bool want = in.tree_where == MccfrTreeWhere::kUnset ? kMccfrTreeGlobalDefault : in.tree_where == MccfrTreeWhere::kGlobal;
    if (want && helps && split == 0 && in.solver != 2) {
      tree_global = true;
      shmem_bytes = tables_only;
      fit = static_cast<int>(in.lds_per_cu / std::max<size_t>(tables_only, 1));
    }
  }
  int threads, per_cu;
  if (fit <= 1) {
    const int64_t share = (lanes + in.cus - 1) / std::max(in.cus, 1);
    threads = static_cast<int>(std::min<int64_t>(1024, std::max<int64_t>(256, (share + 63) / 64 * 64)));
    per_cu = 1;
  } else {
    threads = lanes >= static_cast<int64_t>(in.cus) * 1024 ? 1024 : 256;
    per_cu = std::max(1, std::min(fit, 2048 / threads));
  }
  p.split = split; p.tree_global = tree_global; p.threads = threads; p.shmem_bytes = shmem_bytes; p.lanes = lanes;
  p.groups = std::min<int64_t>((lanes + threads - 1) / threads, static_cast<int64_t>(in.cus) * per_cu);
  if (in.solver == 2) { p.form = MccfrForm::kResidentOs; p.last_kernel = "k_os_mccfr_resident"; }
  else if (split == 2) { p.form = MccfrForm::kResidentSplit2; p.last_kernel = "k_mccfr_resident<split 2>"; }
  else if (split == 1) { p.form = MccfrForm::kResidentSplit1; p.last_kernel = "k_mccfr_resident<split 1>"; }
  else if (tree_global) { p.form = MccfrForm::kResidentFlatTreeInL2; p.last_kernel = "k_mccfr_resident_flat<tree in L2>"; }
  else { p.form = MccfrForm::kResidentFlat; p.last_kernel = "k_mccfr_resident_flat"; }
  return p;
}

}  // namespace osg_cfr_impl
