// The search loop of open_spiel_amd/csrc/osg_alpha_beta.h (the body of k_alpha_beta, host + device) instantiated on the
// host with plain ARRAY models of tic_tac_toe and connect_four written here from the rules as the reference states them
// (tic_tac_toe.cc:109-148,215-227; connect_four.cc:122-209,277-285) — no bitboards, nothing shared with the device rules —
// and a std::vector as the stack.  Cases come from a flat text file the Python test writes from
// tests/golden/minimax_vectors.npz (results of the reference's own minimax.py):
//   set <game> <rows> <cols> <depth_limit> <leaf_mode> <leaf_value> <n>
//   <maximizing_player> <max_nodes> <value bits, hex> <best_action> <nodes> <status> <len> <a0> <a1> ...     (n lines)
// value is compared bit for bit (NaN where the status is not 0), best_action / nodes / status for equality; nodes are
// not compared where the status is not 0 (unspecified).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "osg_alpha_beta.h"

namespace {

struct BitTodo {   // a set of up to 32 actions; the lowest first
  uint32_t bits = 0;
};
struct ModelBase {
  using Todo = BitTodo;
  static bool todo_any(const Todo& t) { return t.bits != 0; }
  static int todo_pop(Todo& t) {
    for (int a = 0; a < 32; ++a)
      if (t.bits & (1u << a)) { t.bits &= ~(1u << a); return a; }
    return -1;
  }
  static void todo_clear(Todo& t) { t.bits = 0; }
};

// tic_tac_toe: cell[a] = 0 empty, 1 x (player 0), 2 o (player 1).
struct TttModel : ModelBase {
  struct State {
    signed char cell[9];
    int stones;
  };
  static State initial() {
    State s;
    std::memset(&s, 0, sizeof(s));
    return s;
  }
  static bool has_line(const State& s, int mark) {   // BoardHasLine, tic_tac_toe.cc:109-120
    const signed char* b = s.cell;
    return (b[0] == mark && b[1] == mark && b[2] == mark) || (b[3] == mark && b[4] == mark && b[5] == mark) ||
           (b[6] == mark && b[7] == mark && b[8] == mark) || (b[0] == mark && b[3] == mark && b[6] == mark) ||
           (b[1] == mark && b[4] == mark && b[7] == mark) || (b[2] == mark && b[5] == mark && b[8] == mark) ||
           (b[0] == mark && b[4] == mark && b[8] == mark) || (b[2] == mark && b[4] == mark && b[6] == mark);
  }
  bool terminal(const State& s) const { return has_line(s, 1) || has_line(s, 2) || s.stones == 9; }
  int mover(const State& s) const { return s.stones & 1; }
  double player_return(const State& s, int player) const {
    const double r0 = has_line(s, 1) ? 1.0 : (has_line(s, 2) ? -1.0 : 0.0);
    return player == 0 ? r0 : -r0 + 0.0;
  }
  Todo legal(const State& s) const {
    Todo t;
    for (int a = 0; a < 9; ++a)
      if (s.cell[a] == 0) t.bits |= 1u << a;
    return t;
  }
  void apply(State& s, int a) const {
    s.cell[a] = static_cast<signed char>(1 + (s.stones & 1));
    ++s.stones;
  }
};

// connect_four: cell[r][c], row 0 the bottom row; outcome kept as the reference keeps outcome_ (connect_four.cc:138-142).
struct C4Model : ModelBase {
  static constexpr int kMax = 10;
  int rows, cols, k;
  struct State {
    signed char cell[kMax][kMax];
    int stones;
    int outcome;   // -1 running, 0 player 0 won, 1 player 1 won, 2 draw
  };
  State initial() const {
    State s;
    std::memset(&s, 0, sizeof(s));
    s.outcome = -1;
    return s;
  }
  int at(const State& s, int r, int c) const { return (r < 0 || r >= rows || c < 0 || c >= cols) ? -1 : s.cell[r][c]; }
  bool has_line(const State& s, int mark) const {   // HasLine / HasLineFrom, connect_four.cc:163-201
    const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c)
        for (int d = 0; d < 4; ++d) {
          int run = 0;
          while (run < k && at(s, r + run * dr[d], c + run * dc[d]) == mark) ++run;
          if (run == k) return true;
        }
    return false;
  }
  bool terminal(const State& s) const { return s.outcome >= 0; }
  int mover(const State& s) const { return s.stones & 1; }
  double player_return(const State& s, int player) const {
    const double r0 = s.outcome == 0 ? 1.0 : (s.outcome == 1 ? -1.0 : 0.0);
    return player == 0 ? r0 : -r0 + 0.0;
  }
  Todo legal(const State& s) const {
    Todo t;
    for (int c = 0; c < cols; ++c)
      if (s.cell[rows - 1][c] == 0) t.bits |= 1u << c;
    return t;
  }
  void apply(State& s, int c) const {
    const int player = s.stones & 1;
    int r = 0;
    while (s.cell[r][c] != 0) ++r;
    s.cell[r][c] = static_cast<signed char>(1 + player);
    ++s.stones;
    if (has_line(s, 1 + player)) s.outcome = player;
    else if (s.stones == rows * cols) s.outcome = 2;
  }
};

template <class R>
struct VectorStack {
  std::vector<osg::AbFrame<R>> frames;
  void store(int ply, const osg::AbFrame<R>& f) {
    if (static_cast<size_t>(ply) >= frames.size()) frames.resize(ply + 1);
    frames[ply] = f;
  }
  void load(int ply, osg::AbFrame<R>& f) { f = frames[ply]; }
};

struct Totals {
  long cases = 0, failures = 0, nodes = 0;
};

template <class R>
void run_set(const R& rules, FILE* in, int n, osg::AbConfig cfg, const char* game, Totals* tot) {
  for (int i = 0; i < n; ++i) {
    int maxp, best, status, len;
    long long max_nodes, nodes;
    unsigned long long bits;
    if (std::fscanf(in, "%d %lld %llx %d %lld %d %d", &maxp, &max_nodes, &bits, &best, &nodes, &status, &len) != 7) {
      std::printf("malformed case %d of %s\n", i, game);
      std::exit(2);
    }
    typename R::State s = rules.initial();
    for (int j = 0; j < len; ++j) {
      int a;
      if (std::fscanf(in, "%d", &a) != 1) std::exit(2);
      rules.apply(s, a);
    }
    cfg.maximizing_player = maxp;
    cfg.max_nodes = max_nodes;
    VectorStack<R> stack;
    double value;
    int got_best, got_status;
    int64_t got_nodes;
    osg::alpha_beta_search(rules, stack, s, cfg, &value, &got_best, &got_nodes, &got_status);
    uint64_t got_bits;
    std::memcpy(&got_bits, &value, 8);
    bool ok = got_status == status && got_best == best;
    if (status == 0) ok = ok && got_bits == bits && got_nodes == nodes;
    else ok = ok && std::isnan(value);
    ++tot->cases;
    tot->nodes += status == 0 ? static_cast<long>(got_nodes) : 0;
    if (!ok) {
      if (++tot->failures <= 20)
        std::printf("MISMATCH %s case %d (depth %d, player %d, budget %lld): value %.17g (want bits %llx) best %d (%d) nodes %lld (%lld) "
                    "status %d (%d)\n", game, i, cfg.depth_limit, maxp, max_nodes, value, bits, got_best, best,
                    static_cast<long long>(got_nodes), nodes, got_status, status);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = std::fopen(argv[1], "r");
  if (!in) return 2;
  Totals tot;
  char word[16], game[64];
  int rows, cols, depth, leaf_mode, n, sets = 0;
  double leaf_value;
  while (std::fscanf(in, "%15s %63s %d %d %d %d %lf %d", word, game, &rows, &cols, &depth, &leaf_mode, &leaf_value, &n) == 8) {
    osg::AbConfig cfg{depth, -1, leaf_mode, leaf_value, 1};
    if (std::strcmp(game, "tic_tac_toe") == 0) run_set(TttModel{}, in, n, cfg, game, &tot);
    else if (std::strcmp(game, "connect_four") == 0) run_set(C4Model{{}, rows, cols, 4}, in, n, cfg, game, &tot);
    else return 2;
    ++sets;
  }
  std::fclose(in);
  if (tot.failures) {
    std::printf("FAILED: %ld of %ld cases\n", tot.failures, tot.cases);
    return 1;
  }
  std::printf("ok: %ld cases in %d sets, %ld nodes\n", tot.cases, sets, tot.nodes);
  return 0;
}
