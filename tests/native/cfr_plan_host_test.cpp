// The tabular solvers' host planners (open_spiel_amd/csrc/osg_cfr_plan.h) on a recorded tree: every plan is decoded back
// to the tree it was made from.  Stand-alone: includes that header alone, no HIP.
//
//   cfr_plan_host_test <layout file written by efr_cases.write_layout> <kuhn | leduc | leduc_small>
//
// kuhn: kuhn_poker with 2, 3 or 4 players; leduc: a 9 457-history leduc_poker tree; leduc_small: the 1 939-history tree
// of leduc_poker(suit_isomorphism=True).  Prints one line per check; exits non-zero at the first failure.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "osg_cfr_plan.h"

using namespace osg_cfr_impl;

#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);   \
      std::printf(__VA_ARGS__);                                       \
      std::printf("\n");                                              \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

static void ok(const std::string& what) { std::printf("ok  %s\n", what.c_str()); }
static bool has(const char* why, const char* part) { return why && std::strstr(why, part); }
static uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, sizeof b); return b; }
static uint64_t bits_of(int32_t lo, int32_t hi) { return static_cast<uint32_t>(lo) | (static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32); }

struct Loaded {
  std::vector<int32_t> level_off, parent, first_child, info, mem_off, mem, nact, path_off, path, info_level, level_of;
  std::vector<uint8_t> kind, nchild, aidx;
  std::vector<int8_t> actor, info_player;
  std::vector<double> edge_prob, term_ret;
  HostTree t;
};

static Loaded load(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  CHECK(f, "cannot open %s", path);
  const auto ints = [&](size_t n) { std::vector<int32_t> v(n); CHECK(std::fread(v.data(), 4, n, f) == n, "short file"); return v; };
  const auto doubles = [&](size_t n) { std::vector<double> v(n); CHECK(std::fread(v.data(), 8, n, f) == n, "short file"); return v; };
  const std::vector<int32_t> sz = ints(7);
  const int H = sz[0], I = sz[1], A = sz[2], P = sz[3], D = sz[4], M = sz[5], NP = sz[6];
  Loaded x;
  x.level_off = ints(D + 1); x.parent = ints(H); x.first_child = ints(H);
  const std::vector<int32_t> kind = ints(H), nchild = ints(H), aidx = ints(H), actor = ints(H);
  x.info = ints(H); x.mem_off = ints(I + 1); x.mem = ints(M);
  (void)ints(H);   // mem_index
  x.nact = ints(I);
  (void)ints(static_cast<size_t>(I) * A);   // legal
  const std::vector<int32_t> info_player = ints(I);
  x.path_off = ints(M + 1); x.path = ints(NP);
  x.edge_prob = doubles(H); x.term_ret = doubles(static_cast<size_t>(H) * P);
  std::fclose(f);
  x.kind.assign(kind.begin(), kind.end()); x.nchild.assign(nchild.begin(), nchild.end()); x.aidx.assign(aidx.begin(), aidx.end());
  x.actor.assign(actor.begin(), actor.end()); x.info_player.assign(info_player.begin(), info_player.end());
  x.level_of.assign(H, 0);
  for (int l = 0; l < D; ++l)
    for (int h = x.level_off[l]; h < x.level_off[l + 1]; ++h) x.level_of[h] = l;
  x.info_level.assign(I, 0);
  for (int i = 0; i < I; ++i)
    if (x.mem_off[i + 1] > x.mem_off[i]) x.info_level[i] = x.level_of[x.mem[x.mem_off[i]]];
  HostTree& t = x.t;
  t.H = H; t.I = I; t.A = A; t.P = P; t.D = D; t.M = M;
  t.level_off = x.level_off.data(); t.parent = x.parent.data(); t.first_child = x.first_child.data(); t.kind = x.kind.data();
  t.nchild = x.nchild.data(); t.aidx = x.aidx.data(); t.actor = x.actor.data(); t.info = x.info.data();
  t.mem_off = x.mem_off.data(); t.mem = x.mem.data(); t.nact = x.nact.data(); t.info_player = x.info_player.data();
  t.edge_prob = x.edge_prob.data(); t.term_ret = x.term_ret.data(); t.path_off = x.path_off.data(); t.path = x.path.data();
  t.info_level = x.info_level.data();
  return x;
}

// The chance product of member m's root path, in path order (the planners' own helper is not used here).
static double chance_in_path_order(const HostTree& t, int m) {
  double c = 1.0;
  for (int e = t.path_off[m]; e < t.path_off[m + 1]; ++e)
    if ((t.path[e] >> 23) & 1) c = c * t.edge_prob[t.path[e] & 0x7FFFFF];
  return c;
}

// ---- deal_cut ----------------------------------------------------------------------------------------------------------
static DealCut check_deal_cut(const Loaded& x, int want_L, int want_G) {
  const HostTree& t = x.t;
  const DealCut c = deal_cut(t);
  CHECK(c.L == want_L, "L = %d, expected %d (%s)", c.L, want_L, c.why ? c.why : "");
  if (want_G >= 0) CHECK(c.G == want_G, "G = %d, expected %d", c.G, want_G);
  CHECK(c.G == t.level_off[c.L + 1] - t.level_off[c.L], "G");
  CHECK(static_cast<int>(c.sub_of.size()) == t.H && static_cast<int>(c.level_of.size()) == t.H, "sizes");
  for (int l = 0; l < c.L; ++l)
    for (int h = t.level_off[l]; h < t.level_off[l + 1]; ++h) CHECK(t.kind[h] == kChanceNode, "level %d above the cut holds a non-chance node", l);
  bool any = false;
  for (int h = t.level_off[c.L]; h < t.level_off[c.L + 1]; ++h) any |= t.kind[h] != kChanceNode;
  CHECK(any, "level L is all chance");
  for (int h = 0; h < t.H; ++h) {
    CHECK(c.level_of[h] == x.level_of[h], "level_of[%d]", h);
    if (h < t.level_off[c.L]) CHECK(c.sub_of[h] == -1, "sub_of[%d] = %d above the cut", h, c.sub_of[h]);
    else if (h < t.level_off[c.L + 1]) CHECK(c.sub_of[h] == h - t.level_off[c.L], "sub_of[%d] on the cut", h);
    else CHECK(c.sub_of[h] >= 0 && c.sub_of[h] == c.sub_of[t.parent[h]], "sub_of[%d] differs from its parent's", h);
  }
  ok("deal_cut: L = " + std::to_string(c.L) + ", " + std::to_string(c.G) + " subtrees, sub_of constant along parent chains");
  return c;
}

// ---- plan_sub ------------------------------------------------------------------------------------------------------------
enum SubForm { kPerSubtree, kPacked, kForest };

static void check_sub(const Loaded& x, const SubLimits& lim, SubForm want, int want_G, int max_bin, int exact_bin, const std::string& tag) {
  const HostTree& t = x.t;
  const int P = t.P, A = t.A;
  const SubHostPlan p = plan_sub(t, lim);
  CHECK(p.ok, "%s: refused: %s", tag.c_str(), p.why ? p.why : "");
  const SubForm got = p.forest ? kForest : (p.packed ? kPacked : kPerSubtree);
  CHECK(got == want, "%s: form %d, expected %d", tag.c_str(), got, want);
  CHECK(!(p.forest && p.packed), "both forms");
  CHECK(p.G == want_G, "%s: G = %d, expected %d", tag.c_str(), p.G, want_G);
  const DealCut cut = deal_cut(t);
  CHECK(p.L == cut.L && p.G0 == cut.G, "L, G0");
  const int G = p.G, NL = p.NL, ND = p.ND, NCP = p.NCP, L = p.L;
  const int piece_level = p.forest ? L + 1 : L, root_base = t.level_off[piece_level];
  // (e) the limits
  CHECK((p.K == 2 || p.K == 4 || p.K == 8) && NL <= p.K * kSubThreads, "K = %d, NL = %d", p.K, NL);
  CHECK(ND % 2 == 0 && NCP % 2 == 0 && ND <= kSubKD * kSubThreads, "ND = %d, NCP = %d", ND, NCP);
  CHECK(p.lds_bytes <= 158 * 1024 && p.lds_bytes >= sizeof(double) * (static_cast<size_t>(ND) * A + NCP + NL), "lds_bytes = %zu", p.lds_bytes);
  int widest = 0;
  for (int i = 0; i < t.I; ++i) widest = std::max(widest, t.mem_off[i + 1] - t.mem_off[i]);
  CHECK(p.fold_cap >= widest, "fold_cap = %d below the widest infostate %d", p.fold_cap, widest);
  CHECK(sizeof(double) * (static_cast<size_t>(ND) * A + NCP + static_cast<size_t>(p.fold_cap) * kSubRecDoubles) <= p.lds_bytes, "fold stage beyond the LDS");
  CHECK(static_cast<int>(p.nloc.size()) == G && p.desc.size() == static_cast<size_t>(G) * NL && p.fc.size() == p.desc.size() &&
        p.aux.size() == p.desc.size() && p.dec_row.size() == static_cast<size_t>(G) * ND && p.ndec.size() == static_cast<size_t>(G) &&
        p.dec_off.size() == static_cast<size_t>(G) * (P + 2) && p.chance_prob.size() == static_cast<size_t>(G) * NCP &&
        p.term_val.size() == static_cast<size_t>(G) * P * NL && p.mem_off.size() == static_cast<size_t>(G) * P + 1 &&
        p.recbuf.size() == static_cast<size_t>(std::max(t.M, 1)) * kSubRecDoubles, "array sizes");
  const int stride = 8 + (p.PL / 2 + 3) / 4 * 4;
  CHECK(p.PL % (4 * P) == 0 && p.PL / 4 <= kSubCodeChunks, "PL = %d", p.PL);
  CHECK(p.sub_rec.size() == static_cast<size_t>(p.mem_off.back()) * stride, "sub_rec holds %zu words for %d members", p.sub_rec.size(), p.mem_off.back());
  // (a) the histories of every bin: anchored at the members (decision histories) and the terminals (aux), the rest by
  // following fc from a parent
  std::vector<std::vector<int32_t>> glob(G);
  std::vector<int32_t> bin_of(t.H, -1), loc_of(t.H, -1);
  int biggest = 0, total = 0;
  for (int g = 0; g < G; ++g) {
    CHECK(p.nloc[g] >= 1 && p.nloc[g] <= NL && p.nloc[g] == p.bin_histories[g], "nloc[%d]", g);
    glob[g].assign(p.nloc[g], -1);
    biggest = std::max(biggest, p.nloc[g]); total += p.nloc[g];
  }
  CHECK(total == t.H - root_base, "%s: nloc sums to %d, %d histories at or below the pieces' level", tag.c_str(), total, t.H - root_base);
  CHECK(biggest == NL, "NL");
  if (max_bin > 0) CHECK(biggest <= max_bin, "%s: a bin of %d histories, expected at most %d", tag.c_str(), biggest, max_bin);
  if (exact_bin > 0) CHECK(biggest == exact_bin, "%s: the largest bin holds %d histories, expected %d", tag.c_str(), biggest, exact_bin);
  const auto anchor = [&](int g, int j, int h) {
    CHECK(j >= 0 && j < p.nloc[g], "local index %d outside bin %d", j, g);
    CHECK(glob[g][j] == -1 || glob[g][j] == h, "bin %d local %d is both %d and %d", g, j, glob[g][j], h);
    glob[g][j] = h;
  };
  for (int g = 0; g < G; ++g) {
    for (int q = 0; q < P; ++q) {
      CHECK(p.mem_off[g * P + q + 1] - p.mem_off[g * P + q] == p.bin_members[static_cast<size_t>(g) * P + q], "bin_members");
      for (int k = p.mem_off[g * P + q]; k < p.mem_off[g * P + q + 1]; ++k) {
        const int32_t* rec = &p.sub_rec[static_cast<size_t>(k) * stride];
        CHECK(rec[0] >= 0 && rec[0] < t.M, "member index");
        anchor(g, rec[1], t.mem[rec[0]]);
      }
    }
    for (int j = 0; j < p.nloc[g]; ++j)
      if ((p.desc[static_cast<size_t>(g) * NL + j] & 3) == kTerminalNode) {
        const int h = p.aux[static_cast<size_t>(g) * NL + j];
        CHECK(h >= 0 && h < t.H, "terminal aux");
        anchor(g, j, h);
      }
    for (int j = 0; j < p.nloc[g]; ++j) {
      const int h = glob[g][j];
      CHECK(h >= root_base, "%s: bin %d local %d cannot be placed in the tree", tag.c_str(), g, j);
      if (t.kind[h] == kTerminalNode) continue;
      for (int c = 0; c < t.nchild[h]; ++c) anchor(g, p.fc[static_cast<size_t>(g) * NL + j] + c, t.first_child[h] + c);
    }
    for (int j = 0; j < p.nloc[g]; ++j) {
      const int h = glob[g][j];
      CHECK(bin_of[h] == -1, "history %d is in bins %d and %d", h, bin_of[h], g);
      bin_of[h] = g; loc_of[h] = j;
      if (j) CHECK(glob[g][j - 1] < h, "bin %d is not in level order at %d", g, j);
    }
  }
  for (int h = root_base; h < t.H; ++h) CHECK(bin_of[h] >= 0, "history %d is in no bin", h);
  ok(tag + ": (a) every history at or below level " + std::to_string(piece_level) + " is in exactly one of " + std::to_string(G) + " bins, level order, largest " + std::to_string(biggest));
  // (b) desc, fc, aux
  for (int g = 0; g < G; ++g) {
    const int32_t* off = &p.dec_off[static_cast<size_t>(g) * (P + 2)];
    std::vector<int> used(ND, 0);
    int decisions = 0, chance_at = 0;
    CHECK(off[0] == 0, "dec_off[0]");
    for (int q = 0; q <= P; ++q) CHECK(off[q] <= off[q + 1], "dec_off not ascending");
    CHECK(off[P + 1] == p.ndec[g] && p.ndec[g] <= ND, "ndec[%d]", g);
    if (!p.forest) CHECK(off[P] == off[P + 1], "upper rows without a forest");
    for (int j = 0; j < NL; ++j) {
      const size_t at = static_cast<size_t>(g) * NL + j;
      if (j >= p.nloc[g]) {
        CHECK(p.desc[at] == (kTerminalNode | (63 << 10)) && p.fc[at] == 0 && p.aux[at] == 0, "padding of bin %d at %d", g, j);
        for (int q = 0; q < P; ++q) CHECK(p.term_val[(static_cast<size_t>(g) * P + q) * NL + j] == 0.0, "term_val padding");
        continue;
      }
      const int h = glob[g][j];
      CHECK(p.desc[at] == (t.kind[h] | (t.nchild[h] << 2) | (x.level_of[h] << 10) | ((t.actor[h] + 1) << 16)), "desc of history %d", h);
      if (t.kind[h] != kTerminalNode) CHECK(p.fc[at] == loc_of[t.first_child[h]], "fc of history %d", h);
      else CHECK(p.fc[at] == 0, "fc of terminal %d", h);
      for (int q = 0; q < P; ++q) {
        const double want_v = t.kind[h] == kTerminalNode ? t.term_ret[static_cast<size_t>(h) * P + q] : 0.0;
        CHECK(bits_of(p.term_val[(static_cast<size_t>(g) * P + q) * NL + j]) == bits_of(want_v), "term_val of history %d player %d", h, q);
      }
      if (t.kind[h] == kDecisionNode) {
        const int d = p.aux[at], q = t.actor[h];
        CHECK(d >= off[q] && d < off[q + 1], "decision %d of history %d outside player %d's rows", d, h, q);
        CHECK(p.dec_row[static_cast<size_t>(g) * ND + d] == t.info[h] * A, "dec_row of history %d", h);
        CHECK(!used[d]++, "decision index %d twice in bin %d", d, g);
        ++decisions;
      } else if (t.kind[h] == kChanceNode) {
        CHECK(p.aux[at] == chance_at && chance_at + t.nchild[h] <= NCP, "chance offset of history %d", h);
        for (int c = 0; c < t.nchild[h]; ++c)
          CHECK(bits_of(p.chance_prob[static_cast<size_t>(g) * NCP + chance_at + c]) == bits_of(t.edge_prob[t.first_child[h] + c]), "chance_prob of history %d", h);
        chance_at += t.nchild[h];
      } else {
        CHECK(p.aux[at] == h, "aux of terminal %d", h);
      }
    }
    CHECK(decisions == off[P], "bin %d: %d decisions, dec_off says %d", g, decisions, off[P]);
  }
  ok(tag + ": (b) desc, fc, aux, dec_row, dec_off, chance_prob and term_val decode to the tree");
  // (c) the members
  std::vector<int> seen(std::max(t.M, 1), 0);
  std::vector<std::set<int32_t>> upper_rows(G);
  for (int g = 0; g < G; ++g) {
    const int32_t* off = &p.dec_off[static_cast<size_t>(g) * (P + 2)];
    for (int q = 0; q < P; ++q)
      for (int k = p.mem_off[g * P + q]; k < p.mem_off[g * P + q + 1]; ++k) {
        const int32_t* rec = &p.sub_rec[static_cast<size_t>(k) * stride];
        const int m = rec[0], h = t.mem[m];
        const size_t at = static_cast<size_t>(g) * NL + loc_of[h];
        ++seen[m];
        CHECK(bin_of[h] == g && t.actor[h] == q, "member %d listed under bin %d player %d", m, g, q);
        CHECK(rec[1] == loc_of[h] && rec[2] == (p.aux[at] | (t.nact[t.info[h]] << 24)) && rec[3] == p.fc[at], "member %d: local index, decision | actions, first child", m);
        CHECK(t.nact[t.info[h]] == t.nchild[h], "nact");
        CHECK(bits_of(rec[4], rec[5]) == bits_of(chance_in_path_order(t, m)), "member %d: chance product", m);
        CHECK(rec[6] == 0 && rec[7] == 0, "member %d: unused words", m);
        const int per = p.PL / P;
        std::vector<int> filled(P, 0);
        int x_anc = 0;   // walks the ancestors root to leaf beside the path
        std::vector<int32_t> anc(t.path_off[m + 1] - t.path_off[m]);
        x_anc = t.parent[h];
        for (int e = static_cast<int>(anc.size()) - 1; e >= 0; --e, x_anc = t.parent[x_anc]) anc[e] = x_anc;
        const auto code_at = [&](int c) { return (static_cast<uint32_t>(rec[8 + c / 2]) >> (16 * (c % 2))) & 0xFFFFu; };
        for (size_t e = 0; e < anc.size(); ++e) {
          const int code = t.path[t.path_off[m] + e];
          if ((code >> 23) & 1) continue;
          const int pl = (code >> 24) & 0xF;
          CHECK(pl < P && filled[pl] < per, "member %d: more decisions of player %d than codes", m, pl);
          const uint32_t got_code = code_at(pl * per + filled[pl]++);
          CHECK(got_code != 0xFFFFu, "member %d: a decision of player %d is missing", m, pl);
          const int d = static_cast<int>(got_code) / A, a = static_cast<int>(got_code) % A;
          CHECK(d < p.ndec[g] && p.dec_row[static_cast<size_t>(g) * ND + d] + a == (code & 0x7FFFFF), "member %d: code %u does not resolve to entry %d", m, got_code, code & 0x7FFFFF);
          if (x.level_of[anc[e]] < piece_level) {   // an upper parent's row
            CHECK(p.forest && d >= off[P] && d < off[P + 1], "member %d: the row of upper parent %d outside [dec_off[P], dec_off[P + 1])", m, anc[e]);
            upper_rows[g].insert(d);
          } else {
            CHECK(d >= off[pl] && d < off[pl + 1] && d == p.aux[static_cast<size_t>(g) * NL + loc_of[anc[e]]], "member %d: ancestor %d's decision index", m, anc[e]);
          }
        }
        for (int pl = 0; pl < P; ++pl)
          for (int c = filled[pl]; c < per; ++c) CHECK(code_at(pl * per + c) == 0xFFFFu, "member %d: padding of player %d's codes", m, pl);
        for (int w = 8 + p.PL / 2; w < stride; ++w) CHECK(rec[w] == -1, "member %d: padding words", m);
      }
    if (p.forest) CHECK(static_cast<int>(upper_rows[g].size()) == off[P + 1] - off[P], "bin %d: %d upper rows, %zu referred to", g, off[P + 1] - off[P], upper_rows[g].size());
  }
  int uppers = 0;
  for (int m = 0; m < t.M; ++m) {
    const int h = t.mem[m];
    const bool upper = x.level_of[h] < piece_level;
    uint64_t first;
    std::memcpy(&first, &p.recbuf[static_cast<size_t>(m) * kSubRecDoubles], 8);
    if (upper) {
      CHECK(p.forest && x.level_of[h] == L && seen[m] == 0, "member %d above the pieces is also in a bin", m);
      CHECK(first == ((static_cast<uint64_t>(kSubFlagHi) << 32) | static_cast<uint64_t>(2 + uppers)), "recbuf of upper member %d", m);
      const int32_t* u = &p.upper_rec[static_cast<size_t>(uppers) * 8];
      CHECK(static_cast<size_t>(uppers + 1) * 8 <= p.upper_rec.size(), "upper_rec too short");
      CHECK(u[0] == t.first_child[h] - root_base && u[1] == t.info[h] * A && u[2] == t.nact[t.info[h]] && u[3] == 0 && u[6] == 0 && u[7] == 0, "upper_rec of member %d", m);
      CHECK(bits_of(u[4], u[5]) == bits_of(chance_in_path_order(t, m)), "upper_rec of member %d: chance product", m);
      ++uppers;
    } else {
      CHECK(seen[m] == 1, "member %d is listed %d times", m, seen[m]);
      CHECK(first == 0, "recbuf of member %d", m);
    }
    for (int k = 1; k < kSubRecDoubles; ++k) CHECK(bits_of(p.recbuf[static_cast<size_t>(m) * kSubRecDoubles + k]) == 0, "recbuf of member %d", m);
  }
  CHECK(p.upper_rec.size() == static_cast<size_t>(uppers) * 8, "upper_rec length");
  ok(tag + ": (c) every member once; local index, decision, codes and chance product are the tree's (" + std::to_string(uppers) + " upper members)");
  // (d) the forest's roots
  if (p.forest) {
    CHECK(uppers > 0, "a forest without upper members");
    CHECK(p.piece_roots == t.level_off[piece_level + 1] - root_base, "piece_roots");
    std::vector<int> covered(p.piece_roots, 0);
    int most = 0;
    for (int g = 0; g < G; ++g) {
      most = std::max(most, p.nroot[g]);
      CHECK(p.nroot[g] <= p.NR, "nroot");
      for (int r = 0; r < p.nroot[g]; ++r) {
        const int idx = p.root_idx[static_cast<size_t>(g) * p.NR + r];
        CHECK(idx >= 0 && idx < p.piece_roots, "root_idx");
        ++covered[idx];
        CHECK(bin_of[root_base + idx] == g && p.root_loc[static_cast<size_t>(g) * p.NR + r] == loc_of[root_base + idx], "root %d of bin %d", r, g);
      }
    }
    CHECK(most == p.NR, "NR");
    for (int c : covered) CHECK(c == 1, "a piece root is covered %d times", c);
    ok(tag + ": (d) the pieces' roots cover level " + std::to_string(piece_level) + " once; upper records and rows in place");
  } else {
    CHECK(p.nroot.empty() && p.upper_rec.empty() && p.NR == 0 && p.piece_roots == 0, "forest arrays without a forest");
  }
  // info_off / info_list: the infostates by player
  for (int q = 0; q < P; ++q)
    for (int e = p.info_off[q]; e < p.info_off[q + 1]; ++e) CHECK(t.info_player[p.info_list[e]] == q, "info_list");
  CHECK(p.info_off[0] == 0 && p.info_off[P] == t.I && static_cast<int>(p.info_list.size()) == t.I, "info_off");
  // (f) the fold's shares
  for (int grid : {1, G / 2, G}) {
    const SubFoldPlan f = plan_sub_fold(t, p, grid);
    CHECK(f.keep_rows == (grid >= G), "keep_rows at grid %d", grid);
    CHECK(f.fold_off.size() == static_cast<size_t>(P) * (grid + 1) && f.fold_info.size() == static_cast<size_t>(t.I) * 4, "fold sizes");
    std::vector<int> shares(t.I, 0);
    for (int q = 0; q < P; ++q) {
      const int32_t* off = &f.fold_off[static_cast<size_t>(q) * (grid + 1)];
      CHECK(off[0] == p.info_off[q] && off[grid] == p.info_off[q + 1], "player %d's shares do not span its infostates", q);
      for (int w = 0; w < grid; ++w) {
        CHECK(off[w] <= off[w + 1], "fold_off decreases");
        for (int e = off[w]; e < off[w + 1]; ++e) ++shares[p.info_list[e]];
      }
    }
    for (int i = 0; i < t.I; ++i) CHECK(shares[i] == 1, "infostate %d is in %d shares", i, shares[i]);
    for (int e = 0; e < t.I; ++e) {
      const int i = p.info_list[e];
      CHECK(f.fold_info[4 * e] == i && f.fold_info[4 * e + 1] == t.nact[i] && f.fold_info[4 * e + 2] == t.mem_off[i] &&
            f.fold_info[4 * e + 3] == t.mem_off[i + 1] - t.mem_off[i], "fold_info");
    }
  }
  ok(tag + ": (e) limits hold, (f) fold shares at grid 1, G / 2, G partition every player's infostates");
}

// ---- plan_split --------------------------------------------------------------------------------------------------------
static void check_split(const Loaded& x, int cus, const std::string& tag) {
  const HostTree& t = x.t;
  const SplitHostPlan p = plan_split(t, SplitLimits{cus});
  CHECK(p.ok, "%s: refused: %s", tag.c_str(), p.why ? p.why : "");
  const DealCut cut = deal_cut(t);
  const int G = p.G, NL = p.NL;
  CHECK(G == cut.G && p.L == cut.L && G <= cus && G >= 8, "G, L");
  CHECK(NL <= 1024 && p.threads % 64 == 0 && p.threads >= NL && p.threads >= p.NM && p.threads >= p.NI && p.threads <= 1024, "threads");
  const size_t IA = static_cast<size_t>(t.I) * t.A;
  CHECK(p.lds_bytes == 8 * (static_cast<size_t>(NL) * t.P + NL + 3 * IA) + 16 && p.br_lds_bytes == p.lds_bytes + 8 * IA, "lds_bytes");
  std::vector<int32_t> loc_of(t.H, -1);
  int total = 0, biggest = 0;
  for (int g = 0; g < G; ++g) {
    total += p.nloc[g]; biggest = std::max(biggest, p.nloc[g]);
    for (int j = 0; j < NL; ++j) {
      const size_t at = static_cast<size_t>(g) * NL + j;
      if (j >= p.nloc[g]) { CHECK(p.desc[at] == kTerminalNode && p.fc[at] == 0 && p.row[at] == 0 && p.glob[at] == 0, "padding"); continue; }
      const int h = p.glob[at];
      CHECK(h >= t.level_off[p.L] && h < t.H && cut.sub_of[h] == g && loc_of[h] == -1, "history %d in subtree %d", h, g);
      loc_of[h] = j;
      if (j) CHECK(p.glob[at - 1] < h, "level order");
    }
  }
  CHECK(total == t.H - t.level_off[p.L] && biggest == NL, "nloc");
  for (int g = 0; g < G; ++g)
    for (int j = 0; j < p.nloc[g]; ++j) {
      const size_t at = static_cast<size_t>(g) * NL + j;
      const int h = p.glob[at];
      CHECK(p.desc[at] == (t.kind[h] | (t.nchild[h] << 2) | (x.level_of[h] << 10) | ((t.actor[h] + 1) << 16)), "desc");
      CHECK(p.fc[at] == (t.kind[h] == kTerminalNode ? 0 : loc_of[t.first_child[h]]), "fc");
      CHECK(p.row[at] == (t.kind[h] == kDecisionNode ? t.info[h] * t.A : 0), "row");
    }
  std::vector<int> seen(std::max(t.M, 1), 0);
  for (int g = 0; g < G; ++g) {
    std::set<int32_t> infos, listed;
    bool padding = false;
    for (int k = 0; k < p.NM; ++k) {
      const int m = p.mem_m[static_cast<size_t>(g) * p.NM + k];
      if (m < 0) { padding = true; continue; }
      CHECK(!padding && m < t.M && cut.sub_of[t.mem[m]] == g && p.mem_hloc[static_cast<size_t>(g) * p.NM + k] == loc_of[t.mem[m]], "member %d of subtree %d", m, g);
      ++seen[m];
      infos.insert(t.info[t.mem[m]]);
    }
    for (int k = 0; k < p.NI; ++k)
      if (p.info_list[static_cast<size_t>(g) * p.NI + k] >= 0) CHECK(listed.insert(p.info_list[static_cast<size_t>(g) * p.NI + k]).second, "infostate twice");
    CHECK(infos == listed, "info_list of subtree %d", g);
  }
  for (int m = 0; m < t.M; ++m) CHECK(seen[m] == 1, "member %d listed %d times", m, seen[m]);
  ok(tag + ": accepted, " + std::to_string(G) + " subtrees of at most " + std::to_string(NL) + " histories decode to the tree; members and infostates listed once");
}

// ---- plan_eval_jobs --------------------------------------------------------------------------------------------------
static void check_jobs(const Loaded& x, const std::string& tag) {
  const HostTree& t = x.t;
  const int P = t.P, A = t.A, D = t.D;
  const JobsHostPlan p = plan_eval_jobs(t);
  CHECK(p.ok, "%s: refused: %s", tag.c_str(), p.why ? p.why : "");
  const DealCut cut = deal_cut(t);
  const int G = cut.G;
  CHECK(p.G == G && p.L == cut.L && p.NT == t.level_off[cut.L + 1], "G, L, NT");
  // the components per responder: subtrees joined by an infostate of r with members in both
  int components = 0;
  for (int r = 0; r < P; ++r) {
    std::vector<int> label(G);
    for (int g = 0; g < G; ++g) label[g] = g;
    for (bool changed = true; changed;) {
      changed = false;
      for (int i = 0; i < t.I; ++i) {
        if (t.info_player[i] != r) continue;
        int lo = G;
        for (int m = t.mem_off[i]; m < t.mem_off[i + 1]; ++m) lo = std::min(lo, label[cut.sub_of[t.mem[m]]]);
        for (int m = t.mem_off[i]; m < t.mem_off[i + 1]; ++m)
          if (label[cut.sub_of[t.mem[m]]] != lo) { label[cut.sub_of[t.mem[m]]] = lo; changed = true; }
      }
    }
    components += static_cast<int>(std::set<int>(label.begin(), label.end()).size());
  }
  CHECK(p.J == G + components, "%s: J = %d, expected %d + %d", tag.c_str(), p.J, G, components);
  std::vector<std::vector<int>> in_kind(P + 1, std::vector<int>(t.H, 0));
  std::vector<int> info_seen(t.I, 0);
  size_t lds = sizeof(double) * 2 * P * p.NT;
  int max_nodes = 0, nodes_total = 0, infos_total = 0, mems_total = 0;
  const size_t IA = static_cast<size_t>(t.I) * A;
  for (int j = 0; j < p.J; ++j) {
    const int32_t* jd = &p.job[static_cast<size_t>(j) * 8];
    const int kind = jd[0], n0 = jd[1], nn = jd[2], i0 = jd[3], ni = jd[4], m0 = jd[5], nm = jd[6];
    CHECK(kind >= 0 && kind <= P && n0 == nodes_total && i0 == infos_total && m0 == mems_total, "job %d header", j);
    if (j < G) CHECK(kind == 0, "the first G jobs are the expected-returns jobs");
    nodes_total += nn; infos_total += ni; mems_total += nm;
    std::vector<int32_t> loc(t.H, -1);
    for (int k = 0; k < nn; ++k) {
      const int h = p.node_glob[n0 + k];
      CHECK(h >= t.level_off[cut.L] && h < t.H && loc[h] == -1, "job %d node %d", j, k);
      loc[h] = k;
      ++in_kind[kind][h];
      if (k) CHECK(p.node_glob[n0 + k - 1] < h, "job %d is not in level order", j);
    }
    const int32_t* lo = &p.level_off[static_cast<size_t>(j) * (D + 1)];
    CHECK(lo[0] == 0 && lo[D] == nn, "job %d level_off ends", j);
    for (int l = 0; l < D; ++l) {
      CHECK(lo[l] <= lo[l + 1], "level_off");
      for (int k = lo[l]; k < lo[l + 1]; ++k) CHECK(x.level_of[p.node_glob[n0 + k]] == l, "job %d: node %d is not on level %d", j, k, l);
    }
    for (int k = 0; k < nn; ++k) {
      const int h = p.node_glob[n0 + k];
      CHECK(p.node_desc[n0 + k] == (t.kind[h] | (t.nchild[h] << 2) | ((t.actor[h] + 1) << 10)), "node_desc");
      CHECK(p.node_row[n0 + k] == (t.kind[h] == kDecisionNode ? t.info[h] * A : 0), "node_row");
      if (t.kind[h] == kTerminalNode) { CHECK(p.node_fc[n0 + k] == 0, "node_fc of a terminal"); continue; }
      CHECK(p.node_fc[n0 + k] == loc[t.first_child[h]] && loc[t.first_child[h]] >= 0, "node_fc");
      for (int c = 0; c < t.nchild[h]; ++c) CHECK(loc[t.first_child[h] + c] == p.node_fc[n0 + k] + c, "a child outside its parent's job");
    }
    if (kind == 0) CHECK(ni == 0 && nm == 0, "an expected-returns job with infostates");
    int members = 0;
    for (int e = 0; e < ni; ++e) {
      const int32_t* ie = &p.info_ent[static_cast<size_t>(i0 + e) * 4];
      const int i = ie[0];
      CHECK(i >= 0 && i < t.I && t.info_player[i] == kind - 1 && ie[1] == t.info_level[i] && ie[2] == members && ie[3] == t.mem_off[i + 1] - t.mem_off[i], "job %d infostate %d", j, i);
      ++info_seen[i];
      for (int k = 0; k < ie[3]; ++k) {
        const int32_t* me = &p.mem_ent[static_cast<size_t>(m0 + members + k) * 2];
        CHECK(me[0] == t.mem_off[i] + k && me[1] == loc[t.mem[me[0]]] && me[1] >= 0, "job %d: member %d of infostate %d", j, k, i);
      }
      members += ie[3];
    }
    CHECK(members == nm, "job %d members", j);
    lds = std::max(lds, sizeof(double) * (IA + static_cast<size_t>(nn) * (kind == 0 ? P : 1) + nn + nm) + sizeof(int32_t) * (3 * static_cast<size_t>(nn) + nm + t.I));
    max_nodes = std::max(max_nodes, nn);
  }
  CHECK(static_cast<size_t>(nodes_total) == p.node_glob.size() && static_cast<size_t>(infos_total) * 4 == p.info_ent.size() && static_cast<size_t>(mems_total) * 2 == p.mem_ent.size(), "totals");
  for (int kind = 0; kind <= P; ++kind)
    for (int h = 0; h < t.H; ++h) CHECK(in_kind[kind][h] == (h >= t.level_off[cut.L] ? 1 : 0), "history %d is in %d jobs of kind %d", h, in_kind[kind][h], kind);
  for (int i = 0; i < t.I; ++i) CHECK(info_seen[i] == (t.mem_off[i + 1] > t.mem_off[i] ? 1 : 0), "infostate %d is in %d jobs", i, info_seen[i]);
  CHECK(p.lds_bytes == lds && lds <= 150 * 1024, "lds_bytes = %zu, the largest job needs %zu", p.lds_bytes, lds);
  CHECK(p.threads == std::max(64, std::min(1024, (max_nodes + 63) / 64 * 64)), "threads");
  ok(tag + ": " + std::to_string(p.J) + " jobs = " + std::to_string(G) + " subtrees + " + std::to_string(components) + " components; histories, infostates, levels and LDS check");
}

// ---- plan_resident -----------------------------------------------------------------------------------------------------
static ResidentHostPlan check_resident(const Loaded& x, const std::string& tag) {
  const HostTree& t = x.t;
  const int P = t.P;
  const ResidentHostPlan p = plan_resident(t, 1);
  CHECK(p.ok, "%s: refused: %s", tag.c_str(), p.why ? p.why : "");
  CHECK(static_cast<int>(p.rec.size()) == t.H && p.n_uret * P == static_cast<int>(p.uret.size()) && p.n_uprob == static_cast<int>(p.uprob.size()), "sizes");
  for (int h = 0; h < t.H; ++h) {
    const uint32_t lo = static_cast<uint32_t>(p.rec[h]), hi = static_cast<uint32_t>(p.rec[h] >> 32);
    CHECK((lo & 3) == t.kind[h] && ((lo >> 2) & 63) == t.nchild[h] && static_cast<int>((lo >> 8) & 15) == t.actor[h] + 1, "record %d: kind, children, actor", h);
    const uint32_t field = lo >> 12;
    if (t.kind[h] == kDecisionNode) CHECK(static_cast<int>(field) == t.info[h], "record %d: infostate", h);
    if (t.kind[h] == kTerminalNode) {
      CHECK(field == 0 && static_cast<int>(hi & 0xFFFFFF) < p.n_uret, "record %d", h);
      for (int q = 0; q < P; ++q) CHECK(bits_of(p.uret[static_cast<size_t>(hi & 0xFFFFFF) * P + q]) == bits_of(t.term_ret[static_cast<size_t>(h) * P + q]), "record %d: returns", h);
    } else {
      CHECK(static_cast<int>(hi & 0xFFFFFF) == t.first_child[h], "record %d: first child", h);
    }
    if (h > 0 && t.kind[t.parent[h]] == kChanceNode) CHECK(static_cast<int>(hi >> 24) < p.n_uprob && bits_of(p.uprob[hi >> 24]) == bits_of(t.edge_prob[h]), "record %d: incoming probability", h);
    else CHECK((hi >> 24) == 0, "record %d: a probability id without a chance parent", h);
    if (t.kind[h] == kChanceNode) {
      bool same = t.nchild[h] > 0;
      for (int c = 1; c < t.nchild[h]; ++c) same &= bits_of(t.edge_prob[t.first_child[h] + c]) == bits_of(t.edge_prob[t.first_child[h]]);
      if (same) CHECK(field >= 1 && bits_of(p.uprob[field - 1]) == bits_of(t.edge_prob[t.first_child[h]]), "record %d: equal-probability flag", h);
      else CHECK(field == 0, "record %d: equal-probability flag set", h);
    }
  }
  std::set<uint64_t> probs;
  for (double v : p.uprob) CHECK(probs.insert(bits_of(v)).second, "uprob repeats a value");
  std::set<std::vector<uint64_t>> rets;
  for (int k = 0; k < p.n_uret; ++k) {
    std::vector<uint64_t> key;
    for (int q = 0; q < P; ++q) key.push_back(bits_of(p.uret[static_cast<size_t>(k) * P + q]));
    CHECK(rets.insert(key).second, "uret repeats a vector");
  }
  CHECK(p.lds_bytes == 8 * (3 * static_cast<size_t>(t.I) * t.A + p.uret.size() + p.uprob.size()) + 8 * static_cast<size_t>(t.H), "lds_bytes");
  ok(tag + ": " + std::to_string(t.H) + " records decode; " + std::to_string(p.n_uret) + " return vectors, " + std::to_string(p.n_uprob) + " probabilities, " + std::to_string(p.lds_bytes) + " bytes");
  return p;
}

// ---- mccfr_launch_plan -----------------------------------------------------------------------------------------------
static MccfrLaunchInput launch_input(const HostTree& t, const ResidentHostPlan& r, int solver, int64_t trajectories) {
  MccfrLaunchInput in;
  in.solver = solver; in.A = t.A; in.P = t.P; in.H = t.H; in.IA = static_cast<size_t>(t.I) * t.A;
  in.resident_ok = true; in.resident_lds_bytes = r.lds_bytes; in.cus = 256; in.lds_per_cu = 160 * 1024; in.trajectories = trajectories;
  return in;
}
static void check_geometry(const MccfrLaunchInput& in, const MccfrLaunchPlan& p, const char* what) {
  const size_t full = in.resident_lds_bytes, tables = full - 8 * static_cast<size_t>(in.H);
  const bool general = p.form == MccfrForm::kGeneralEs || p.form == MccfrForm::kGeneralOs;
  if (general) {
    CHECK(p.threads == 256 && p.groups >= 1 && p.groups <= 1024 && p.groups * 256 < in.trajectories + 256 && p.last_kernel == nullptr, "%s: general geometry", what);
    CHECK(p.shmem_bytes == (16 * in.IA <= 64 * 1024 ? 16 * in.IA : 0), "%s: LDS deltas", what);
    return;
  }
  const bool l2 = p.form == MccfrForm::kResidentFlatTreeInL2;
  CHECK(p.tree_global == l2 && p.shmem_bytes == (l2 ? tables : full), "%s: shmem_bytes = %zu", what, p.shmem_bytes);
  const int q = in.A <= 2 ? 2 : 4;
  CHECK(p.lanes == in.trajectories * (p.split == 2 ? q * q : (p.split == 1 ? q : 1)), "%s: lanes", what);
  CHECK(p.threads >= 256 && p.threads <= 1024 && p.threads % 64 == 0, "%s: threads = %d", what, p.threads);
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(static_cast<int64_t>(in.lds_per_cu / p.shmem_bytes), 2048 / p.threads));
  CHECK(p.groups >= 1 && p.groups <= in.cus * per_cu && (p.groups - 1) * p.threads < p.lanes, "%s: %lld groups of %d lanes, %lld per CU allowed", what, static_cast<long long>(p.groups), p.threads, static_cast<long long>(per_cu));
  CHECK(p.groups * p.shmem_bytes <= static_cast<size_t>(in.cus) * in.lds_per_cu, "%s: LDS", what);
  CHECK(p.last_kernel != nullptr, "%s: no last_kernel", what);
}
static MccfrLaunchPlan launch(const MccfrLaunchInput& in, MccfrForm want, const char* want_name, const char* what) {
  const MccfrLaunchPlan p = mccfr_launch_plan(in);
  CHECK(p.form == want, "%s: form %d, expected %d", what, static_cast<int>(p.form), static_cast<int>(want));
  CHECK((want_name == nullptr) == (p.last_kernel == nullptr) && (!want_name || std::strcmp(want_name, p.last_kernel) == 0), "%s: last_kernel %s", what, p.last_kernel ? p.last_kernel : "(none)");
  check_geometry(in, p, what);
  return p;
}

static void check_launch_plans(const Loaded& x, const ResidentHostPlan& r, bool leduc) {
  const HostTree& t = x.t;
  const int P = t.P, q = t.A <= 2 ? 2 : 4;
  if (leduc) {
    for (int64_t n : {int64_t{2} << 27, int64_t{16} << 20}) {
      const MccfrLaunchPlan p = launch(launch_input(t, r, 1, n), MccfrForm::kResidentFlatTreeInL2, "k_mccfr_resident_flat<tree in L2>", "leduc flat");
      CHECK(p.threads == 1024 && p.groups == 2 * 256, "leduc flat: %lld groups of %d", static_cast<long long>(p.groups), p.threads);
    }
    MccfrLaunchInput in = launch_input(t, r, 1, int64_t{16} << 20);
    in.tree_where = MccfrTreeWhere::kLds;
    const MccfrLaunchPlan p = launch(in, MccfrForm::kResidentFlat, "k_mccfr_resident_flat", "leduc, tree in LDS");
    CHECK(p.groups == 256 && p.threads == 1024, "leduc, tree in LDS: one group per CU");
    in.tree_where = MccfrTreeWhere::kGlobal;
    launch(in, MccfrForm::kResidentFlatTreeInL2, "k_mccfr_resident_flat<tree in L2>", "leduc, tree global");
  } else {
    const int64_t n = P == 2 ? int64_t{2} << 23 : (P == 3 ? int64_t{3} << 25 : int64_t{4} << 22);
    MccfrLaunchInput in = launch_input(t, r, 1, n);
    launch(in, MccfrForm::kResidentFlat, "k_mccfr_resident_flat", "kuhn flat");
    in.tree_where = MccfrTreeWhere::kLds;
    launch(in, MccfrForm::kResidentFlat, "k_mccfr_resident_flat", "kuhn flat, tree in LDS");
    in.tree_where = MccfrTreeWhere::kGlobal;   // (helps only where the staged tree allows one workgroup per CU)
    launch(in, MccfrForm::kResidentFlat, "k_mccfr_resident_flat", "kuhn flat, tree global");
    launch(launch_input(t, r, 2, int64_t{P} << 26), MccfrForm::kResidentOs, "k_os_mccfr_resident", "outcome sampling");
    launch(launch_input(t, r, 2, 64), MccfrForm::kResidentOs, "k_os_mccfr_resident", "outcome sampling, small batch");
  }
  int64_t b2 = (1 << 18) / (q * q), b1 = (1 << 18) / q;
  b2 -= b2 % P; b1 -= b1 % P;
  launch(launch_input(t, r, 1, b2), MccfrForm::kResidentSplit2, "k_mccfr_resident<split 2>", "split 2 batch");
  launch(launch_input(t, r, 1, b1), MccfrForm::kResidentSplit1, "k_mccfr_resident<split 1>", "split 1 batch");
  // the thresholds: trajectories q q against cus 1024, then trajectories q
  const int64_t at2 = 256 * 1024 / (q * q), at1 = 256 * 1024 / q;
  launch(launch_input(t, r, 1, at2), MccfrForm::kResidentSplit2, "k_mccfr_resident<split 2>", "split 2 at equality");
  launch(launch_input(t, r, 1, at2 + 1), MccfrForm::kResidentSplit1, "k_mccfr_resident<split 1>", "one above split 2");
  launch(launch_input(t, r, 1, at1), MccfrForm::kResidentSplit1, "k_mccfr_resident<split 1>", "split 1 at equality");
  launch(launch_input(t, r, 1, at1 + 1), MccfrForm::kResidentFlat, "k_mccfr_resident_flat", "one above split 1");
  MccfrLaunchInput in = launch_input(t, r, 1, at2);
  in.split_max = 1;
  launch(in, MccfrForm::kResidentSplit1, "k_mccfr_resident<split 1>", "split_max 1");
  in.split_max = 0;
  launch(in, MccfrForm::kResidentFlat, "k_mccfr_resident_flat", "split_max 0");
  // the general kernels: asked for, or the resident form refused
  for (int solver : {1, 2}) {
    in = launch_input(t, r, solver, int64_t{P} << 22);
    in.general_kernel = true;
    MccfrLaunchPlan p = launch(in, solver == 2 ? MccfrForm::kGeneralOs : MccfrForm::kGeneralEs, nullptr, "general kernel");
    CHECK((p.shmem_bytes != 0) == (16 * in.IA <= 64 * 1024) && p.groups == 1024, "general kernel: LDS deltas, 1024 groups");
    in.general_kernel = false; in.resident_ok = false; in.trajectories = 1000;
    p = launch(in, solver == 2 ? MccfrForm::kGeneralOs : MccfrForm::kGeneralEs, nullptr, "resident refused");
    CHECK(p.groups == 4, "resident refused: 1000 trajectories take 4 groups");
    in.IA = 64 * 1024 / 16;   // 16 IA = 64 KB: the last size whose deltas go to LDS
    CHECK(launch(in, p.form, nullptr, "deltas at 64 KB").shmem_bytes == 64 * 1024, "deltas at 64 KB");
    in.IA += 1;
    CHECK(launch(in, p.form, nullptr, "deltas above 64 KB").shmem_bytes == 0, "deltas above 64 KB");
  }
  ok("mccfr_launch_plan: flat, split 1 / 2 and their thresholds, split_max, tree_where, outcome sampling, general forms; geometry within the device");
}

int main(int argc, char** argv) {
  CHECK(argc == 3, "usage: cfr_plan_host_test <layout file> <kuhn | leduc | leduc_small>");
  const Loaded x = load(argv[1]);
  const HostTree& t = x.t;
  const std::string kind = argv[2];
  const bool leduc = kind == "leduc", kuhn = kind == "kuhn";
  CHECK(leduc || kuhn || kind == "leduc_small", "unknown tree kind %s", kind.c_str());
  std::printf("tree: %d histories, %d infostates, %d players, %d levels\n", t.H, t.I, t.P, t.D);
  if (leduc) CHECK(t.H == 9457 && t.P == 2, "not the 9 457-history leduc tree");
  check_deal_cut(x, kuhn ? t.P : 2, leduc ? 30 : -1);

  if (leduc) {
    SubLimits lim;
    lim.cus = 32;
    check_sub(x, lim, kPerSubtree, 30, 0, 0, "plan_sub cus 32");
    lim.cus = 8;
    check_sub(x, lim, kPacked, 8, 0, 1260, "plan_sub cus 8");
    lim.cus = 24; lim.max_histories_per_bin = 512;
    check_sub(x, lim, kForest, 24, 440, 0, "plan_sub cus 24, 512 histories per bin");
    // no packing fits one bin (9 455 histories against 8 192, and the pieces no better): a subtree per bin, 30 bins
    lim = SubLimits{};
    lim.cus = 1;
    check_sub(x, lim, kPerSubtree, 30, 0, 0, "plan_sub cus 1");
    lim.cus = 8; lim.pack = false;
    check_sub(x, lim, kPerSubtree, 30, 0, 0, "plan_sub cus 8, pack off");
  } else if (kuhn && t.P == 4) {
    // 7 886 histories are past the 4 096 the form asks for: 120 deal subtrees, one per bin on 256 compute units, and
    // packed (120 / 16 subtrees of at most 66 histories each, far inside every limit) on 16
    SubLimits lim;
    lim.cus = 256;
    check_sub(x, lim, kPerSubtree, 120, 0, 0, "plan_sub cus 256");
    lim.cus = 16;
    check_sub(x, lim, kPacked, 16, 0, 0, "plan_sub cus 16");
  } else {
    SubLimits lim;
    lim.cus = 256;
    const SubHostPlan p = plan_sub(t, lim);
    CHECK(!p.ok && has(p.why, "4096 histories"), "plan_sub accepted %d histories, or refused for another reason: %s", t.H, p.why ? p.why : "");
    ok(std::string("plan_sub refused: ") + p.why);
  }

  if (leduc) {
    check_split(x, 32, "plan_split cus 32");
    check_split(x, 30, "plan_split cus 30");
    const SplitHostPlan p = plan_split(t, SplitLimits{8});
    CHECK(!p.ok && has(p.why, "more than compute units"), "plan_split cus 8: %s", p.why ? p.why : "accepted");
    ok(std::string("plan_split cus 8 refused: ") + p.why);
  } else if (kuhn && t.P == 4) {
    // 7 886 histories under 120 deals of 4 cards out of 5: each subtree has at most 1 024 histories, few members and
    // paths of at most 7 decisions, and 8 (NL (P + 1) + 3 I A) + 16 bytes stay far below 150 KB: accepted
    check_split(x, 256, "plan_split kuhn_poker(players=4) cus 256");
    const SplitHostPlan p = plan_split(t, SplitLimits{64});
    CHECK(!p.ok && has(p.why, "more than compute units"), "plan_split cus 64: %s", p.why ? p.why : "accepted");
    ok(std::string("plan_split cus 64 refused: ") + p.why);
  } else {
    const SplitHostPlan p = plan_split(t, SplitLimits{256});
    CHECK(!p.ok && has(p.why, "2000 histories"), "plan_split: %s", p.why ? p.why : "accepted");
    ok(std::string("plan_split refused: ") + p.why);
  }

  if (leduc || (kuhn && t.P == 4)) {
    check_jobs(x, "plan_eval_jobs");
  } else {
    const JobsHostPlan p = plan_eval_jobs(t);
    CHECK(!p.ok && has(p.why, "2000 histories"), "plan_eval_jobs: %s", p.why ? p.why : "accepted");
    ok(std::string("plan_eval_jobs refused: ") + p.why);
  }

  const ResidentHostPlan r = check_resident(x, "plan_resident");
  CHECK(!plan_resident(t, 0).ok && has(plan_resident(t, 0).why, "not an MCCFR solver"), "plan_resident accepted solver 0");
  if (leduc || (kuhn && t.P <= 3)) check_launch_plans(x, r, leduc);
  std::printf("all checks passed\n");
  return 0;
}
