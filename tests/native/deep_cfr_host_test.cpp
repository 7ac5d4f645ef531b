// The Deep CFR arithmetic of open_spiel_amd/csrc/osg_deep_cfr.h run on the CPU: one osg_deep_cfr_traverse call over a
// tree handed in depth first, with the reservoir appends of its rows.  Stand-alone (its own main; compiled as host-only
// HIP so that the header's functions are the ones the kernels run); tests/deep_cfr_cases.py writes the input and reads
// the output, tests/test_deep_cfr_host.py holds both against the NumPy restatement.
//
//   deep_cfr_host_test <in> <out>
//
// in:  i32 [8] H, I, A, P, player, iteration, trajectories, buffers (0 or 2: advantage, strategy); u64 [2] seed, first;
//      i32 parent [H], kind [H], actor [H], info [H]; f64 prob [H], returns [H, P]; i32 legal [I, A]; f32 advantages [I, A];
//      per buffer: i64 capacity, add_calls; u64 seed, stream; i32 info [cap], iteration [cap]; f32 values [cap, A]
// out: i64 [2] row bounds; i32 branch [I]; i32 draws [T]; twice (advantage, strategy): i64 offsets [T + 1], i32 info [R],
//      f32 values [R, A]; per buffer: i64 add_calls, i32 info [cap], iteration [cap], f32 values [cap, A]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "osg_deep_cfr.h"

using namespace osg;

namespace {

struct Reader {
  std::vector<unsigned char> buf;
  size_t at = 0;
  template <class T>
  std::vector<T> take(size_t n) {
    if (at + n * sizeof(T) > buf.size()) { fprintf(stderr, "input too short\n"); exit(2); }
    std::vector<T> v(n);
    if (n) memcpy(v.data(), buf.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
  }
};
struct Writer {
  std::vector<unsigned char> buf;
  template <class T>
  void put(const std::vector<T>& v) {
    const size_t at = buf.size();
    buf.resize(at + v.size() * sizeof(T));
    if (!v.empty()) memcpy(buf.data() + at, v.data(), v.size() * sizeof(T));
  }
};

struct Buffer {
  int64_t capacity = 0, add_calls = 0;
  uint64_t seed = 0, stream = 0;
  std::vector<int32_t> info, iteration;
  std::vector<float> values;
  void append(int A, int32_t i, int32_t it, const float* row) {
    const int64_t slot = dcfr_reservoir_slot(seed, stream, add_calls, capacity);
    if (slot >= 0) {
      info[slot] = i;
      iteration[slot] = it;
      for (int a = 0; a < A; ++a) values[slot * A + a] = row[a];
    }
    ++add_calls;
  }
};

struct Walk {
  int A, P, player;
  const std::vector<int32_t>&kind, &actor, &info, &first_child, &nchild, &child, &legal, &nact;
  const std::vector<double>&prob, &returns, &table;
  Rng rng;
  int draws = 0;
  std::vector<int32_t> adv_info, strat_info;
  std::vector<float> adv_vals, strat_vals;

  double walk(int h) {
    if (kind[h] == 2) return returns[static_cast<size_t>(h) * P + player];
    const int fc = first_child[h], nc = nchild[h];
    if (kind[h] == 0) {
      const double u = rng.unit();
      ++draws;
      return walk(child[fc + dcfr_choice(nc, u, [&](int c) { return prob[child[fc + c]]; })]);
    }
    const int i = info[h];
    const double* p = &table[static_cast<size_t>(i) * A];
    const int32_t* ids = &legal[static_cast<size_t>(i) * A];
    if (actor[h] == player) {
      std::vector<double> payoff(nc);
      for (int c = 0; c < nc; ++c) payoff[c] = walk(child[fc + c]);
      std::vector<float> row(A);
      const double cfv = dcfr_advantage_row(p, payoff.data(), ids, nc, A, row.data());
      adv_info.push_back(i);
      adv_vals.insert(adv_vals.end(), row.begin(), row.end());
      return cfv;
    }
    strat_info.push_back(i);
    for (int a = 0; a < A; ++a) strat_vals.push_back(static_cast<float>(p[a]));
    const double u = rng.unit();
    ++draws;
    const int id = dcfr_opponent_draw(p, A, u);
    int pick = 0;
    for (int c = 0; c < nc; ++c)
      if (ids[c] == id) pick = c;
    return walk(child[fc + pick]);
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: deep_cfr_host_test <in> <out>\n"); return 2; }
  Reader in;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    unsigned char chunk[1 << 16];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) in.buf.insert(in.buf.end(), chunk, chunk + n);
    fclose(f);
  }
  const auto head = in.take<int32_t>(8);
  const int H = head[0], I = head[1], A = head[2], P = head[3], player = head[4], iteration = head[5], T = head[6], NB = head[7];
  if (H < 1 || I < 1 || A < 1 || A > kDcfrMaxA || P < 1 || player < 0 || player >= P || T < 0 || (NB != 0 && NB != 2)) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  const auto keys = in.take<uint64_t>(2);
  const auto parent = in.take<int32_t>(H), kind = in.take<int32_t>(H), actor = in.take<int32_t>(H), info = in.take<int32_t>(H);
  const auto prob = in.take<double>(H), returns = in.take<double>(static_cast<size_t>(H) * P);
  const auto legal = in.take<int32_t>(static_cast<size_t>(I) * A);
  const auto adv = in.take<float>(static_cast<size_t>(I) * A);
  std::vector<Buffer> buffers(NB);
  for (Buffer& b : buffers) {
    const auto sz = in.take<int64_t>(2);
    const auto ks = in.take<uint64_t>(2);
    b.capacity = sz[0]; b.add_calls = sz[1]; b.seed = ks[0]; b.stream = ks[1];
    if (b.capacity < 1) { fprintf(stderr, "bad capacity\n"); return 2; }
    b.info = in.take<int32_t>(b.capacity);
    b.iteration = in.take<int32_t>(b.capacity);
    b.values = in.take<float>(static_cast<size_t>(b.capacity) * A);
  }
  // children lists (depth first: a node's children follow it in action order)
  std::vector<int32_t> nchild(H, 0), first_child(H, 0), child, fill(H, 0), nact(I, 0);
  for (int h = 1; h < H; ++h) {
    if (parent[h] < 0 || parent[h] >= h) { fprintf(stderr, "bad tree\n"); return 2; }
    ++nchild[parent[h]];
  }
  for (int h = 0, at = 0; h < H; ++h) { first_child[h] = at; at += nchild[h]; }
  child.resize(H > 1 ? H - 1 : 0);
  for (int h = 1; h < H; ++h) child[first_child[parent[h]] + fill[parent[h]]++] = h;
  for (int i = 0; i < I; ++i)
    for (int a = 0; a < A; ++a) nact[i] += legal[static_cast<size_t>(i) * A + a] >= 0;
  for (int h = 0; h < H; ++h)
    if (kind[h] == 1 && (info[h] < 0 || info[h] >= I || nact[info[h]] != nchild[h])) { fprintf(stderr, "bad infostate\n"); return 2; }

  std::vector<int64_t> work(3 * static_cast<size_t>(H));
  const DcfrBounds bounds = dcfr_row_bounds(H, kind.data(), nchild.data(), actor.data(), player,
                                            [&](int h, int c) { return child[first_child[h] + c]; }, work.data());

  std::vector<double> table(static_cast<size_t>(I) * A);
  std::vector<int32_t> branch(I);
  for (int i = 0; i < I; ++i)
    branch[i] = dcfr_strategy(&adv[static_cast<size_t>(i) * A], &legal[static_cast<size_t>(i) * A], nact[i], A, &table[static_cast<size_t>(i) * A]);

  std::vector<int32_t> draws(T), adv_info, strat_info;
  std::vector<int64_t> adv_off(T + 1, 0), strat_off(T + 1, 0);
  std::vector<float> adv_vals, strat_vals;
  for (int j = 0; j < T; ++j) {
    Walk w{A, P, player, kind, actor, info, first_child, nchild, child, legal, nact, prob, returns, table,
           Rng(keys[0], keys[1] + static_cast<uint64_t>(j), 0)};
    w.walk(0);
    draws[j] = w.draws;
    if (static_cast<int64_t>(w.adv_info.size()) > bounds.adv || static_cast<int64_t>(w.strat_info.size()) > bounds.strat || bounds.frames > 24) {
      fprintf(stderr, "a trajectory passed its row bound\n");
      return 3;
    }
    if (NB == 2) {
      for (size_t r = 0; r < w.adv_info.size(); ++r) buffers[0].append(A, w.adv_info[r], iteration, &w.adv_vals[r * A]);
      for (size_t r = 0; r < w.strat_info.size(); ++r) buffers[1].append(A, w.strat_info[r], iteration, &w.strat_vals[r * A]);
    }
    adv_info.insert(adv_info.end(), w.adv_info.begin(), w.adv_info.end());
    adv_vals.insert(adv_vals.end(), w.adv_vals.begin(), w.adv_vals.end());
    strat_info.insert(strat_info.end(), w.strat_info.begin(), w.strat_info.end());
    strat_vals.insert(strat_vals.end(), w.strat_vals.begin(), w.strat_vals.end());
    adv_off[j + 1] = static_cast<int64_t>(adv_info.size());
    strat_off[j + 1] = static_cast<int64_t>(strat_info.size());
  }

  Writer out;
  out.put(std::vector<int64_t>{bounds.adv, bounds.strat});
  out.put(branch);
  out.put(draws);
  out.put(adv_off); out.put(adv_info); out.put(adv_vals);
  out.put(strat_off); out.put(strat_info); out.put(strat_vals);
  for (const Buffer& b : buffers) {
    out.put(std::vector<int64_t>{b.add_calls});
    out.put(b.info); out.put(b.iteration); out.put(b.values);
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  const bool ok = out.buf.empty() || fwrite(out.buf.data(), 1, out.buf.size(), f) == out.buf.size();
  fclose(f);
  if (!ok) return 2;
  printf("ok: %d trajectories, %zu + %zu rows\n", T, adv_info.size(), strat_info.size());
  return 0;
}
