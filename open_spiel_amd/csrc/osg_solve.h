// Exhaustive enumeration and retrograde solve of the perfect-information board games: the arithmetic of
// algorithms::GetAllStates (open_spiel/algorithms/get_all_states.cc:28-91; python/algorithms/get_all_states.py:27-142)
// and algorithms::ValueIteration (open_spiel/algorithms/value_iteration.cc:36-138; python/algorithms/
// value_iteration.py:73-159) level by level — host + device.  osg_solve.hip maps these functions over a level per
// launch; tests/native/solve_host_test.cpp runs the same functions on the CPU.
//
// Levels.  In tic_tac_toe, connect_four and hex without the swap move a ply adds one stone, so the positions after d
// plies (level d) are exactly those with d stones and no position lies on two levels: the value of a level-d
// position depends on level d + 1 only, and ONE backward sweep gives the fixed point that the reference's repeated
// sweeps converge to (values are the games' exact -1 / 0 / +1, copied and compared, never added).
//
// Canonical key: what the POSITION determines, in at most 128 bits.
//   tic_tac_toe   the record's one word (x stones | o stones << 16).
//   connect_four  per column of rows + 1 bits: 2^height + the x stones of the column, i.e. ((x | o) + bottom) | x —
//                 the bit above the highest stone marks the height, the bits below tell x from o.  (rows + 1) * cols
//                 bits: one word for the 64-bit boards, two for the wide ones.
//   hex           the black plane, then the white plane (32 * NW bits each): boards of up to 64 cells.  The
//                 edge-connection planes follow from the stones where the game goes on, and at the end of the game
//                 differ only in which stone carries the Win label, which the standard string does not show; the
//                 meta word's plies / first-move fields say how the position was reached, not what it is.
// Two positions have the same key iff the reference's ToString() (standard string_rep) prints the same board.
//
// Distance to the end under optimal play (defined here once): 0 at a terminal position; otherwise 1 + the distance of
// the child the mover prefers — among the children whose value equals the position's value, the NEAREST end where
// that value is a win for the mover, the FARTHEST where it is a loss or a draw; ties go to the lowest action.
#ifndef OSG_SOLVE_H_
#define OSG_SOLVE_H_

#include "osg_common.h"
#include "osg_game_boards.h"

namespace osg {

struct SolveKey {
  uint64_t lo, hi;
};
OSG_HD bool solve_key_less(const SolveKey& a, const SolveKey& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
OSG_HD bool solve_key_equal(const SolveKey& a, const SolveKey& b) { return a.hi == b.hi && a.lo == b.lo; }
// The key of a child that the limits drop (beyond depth_limit, or terminal without include_terminals): sorts after
// every position's key and is no position's key (it would be a board with every cell taken by x).
OSG_HD SolveKey solve_key_dropped() { return {~0ull, ~0ull}; }

template <class G> struct SolveTraits;   // kKeyBits (0: no key of at most 128 bits), key(), mover(), plies()

template <>
struct SolveTraits<Ttt> {
  static constexpr int kKeyBits = 25;
  OSG_HD static int key_bits(const Ttt::Params&) { return kKeyBits; }
  OSG_HD static SolveKey key(const Ttt::Params&, const Ttt::State& s) { return {static_cast<uint64_t>(s.x | (s.o << 16)), 0ull}; }
  OSG_HD static int mover(const Ttt::State& s) { return Ttt::plies(s) & 1; }
  OSG_HD static int plies(const Ttt::State& s) { return Ttt::plies(s); }
};

template <int R, int C, int K, class BB>
struct SolveTraits<C4T<R, C, K, BB>> {
  using G = C4T<R, C, K, BB>;
  static constexpr int kKeyBits = 64 * BitboardOps<BB>::kWords;
  OSG_HD static int key_bits(const typename G::Params& p) { return ((R ? R : p.rows) + 1) * (C ? C : p.cols); }
  OSG_HD static SolveKey key(const typename G::Params& p, const typename G::State& s) {
    const BB bottom = G::top(p) >> (G::R(p) - 1);
    const BB k = ((s.x | s.o) + bottom) | s.x;
    if constexpr (BitboardOps<BB>::kWords == 2) return {static_cast<uint64_t>(k), static_cast<uint64_t>(k >> 64)};
    else return {static_cast<uint64_t>(k), 0ull};
  }
  OSG_HD static int mover(const typename G::State& s) { return G::plies(s) & 1; }
  OSG_HD static int plies(const typename G::State& s) { return G::plies(s); }
};

template <int NW>
struct SolveTraits<HexT<NW>> {
  using G = HexT<NW>;
  static constexpr int kKeyBits = NW <= 2 ? 64 * NW : 0;
  OSG_HD static int key_bits(const typename G::Params&) { return kKeyBits; }
  OSG_HD static SolveKey key(const typename G::Params&, const typename G::State& s) {
    if constexpr (NW == 1) return {static_cast<uint64_t>(s.black.w[0]) | (static_cast<uint64_t>(s.white.w[0]) << 32), 0ull};
    else if constexpr (NW == 2)
      return {static_cast<uint64_t>(s.black.w[0]) | (static_cast<uint64_t>(s.black.w[1]) << 32),
              static_cast<uint64_t>(s.white.w[0]) | (static_cast<uint64_t>(s.white.w[1]) << 32)};
    else return {0ull, 0ull};
  }
  OSG_HD static int mover(const typename G::State& s) { return G::to_move(s); }
  // the stones on the board, not the meta word's counter (it saturates, and an uploaded record may carry any)
  OSG_HD static int plies(const typename G::State& s) { return G::popcount(s.black) + G::popcount(s.white); }
};

// LegalActions() of a position that is not terminal, ascending, as a mask of G::kMaskW words.
template <class G>
OSG_HD MaskT<G::kMaskW> solve_legal(const typename G::Params& p, const typename G::State& s) {
  MaskT<G::kMaskW> m;
  const auto l = G::legal(p, s);
#pragma unroll
  for (int k = 0; k < G::kMaskW; ++k) m.w[k] = l.w[k];
  return m;
}

// get_all_states.cc:36-48: a terminal child is listed iff include_terminals, whatever the depth; any other child iff
// its depth does not exceed the limit.
OSG_HD bool solve_child_kept(bool terminal, int child_depth, int depth_limit, bool include_terminals) {
  return terminal ? include_terminals : (depth_limit < 0 || child_depth <= depth_limit);
}

// Child number k (in ascending action order) of a position that is not terminal: the action, the child's record, its
// key (solve_key_dropped() where the limits drop it).
template <class G>
OSG_HD void solve_expand(const typename G::Params& p, const typename G::State& parent, int parent_depth, int k, int depth_limit,
                         bool include_terminals, int* action, typename G::State* child, SolveKey* key) {
  const int a = select_action(solve_legal<G>(p, parent), k);
  typename G::State c = parent;
  G::apply(p, c, a);
  *action = a;
  *child = c;
  *key = solve_child_kept(G::terminal(p, c), parent_depth + 1, depth_limit, include_terminals) ? SolveTraits<G>::key(p, c)
                                                                                             : solve_key_dropped();
}

// The backward pass at one position: fold() once per legal action in ascending order.
struct SolveFold {
  double value;
  int32_t distance;
  int mover;
  bool any;
  OSG_HD void start(int mover_) { value = 0.0; distance = 0; mover = mover_; any = false; }
  // value_iteration.cc:111-125: player 0 takes the max, player 1 the min of the children's values; among equal
  // values the distance rule of the head comment.  A child the limits dropped counts 0 (value_iteration.cc:118: the
  // map's default) at distance 0.
  OSG_HD void fold(double child_value, int32_t child_distance) {
    bool take;
    if (!any) {
      take = true;
    } else if (child_value != value) {
      take = mover == 0 ? child_value > value : child_value < value;
    } else {
      const bool win = mover == 0 ? value > 0.0 : value < 0.0;
      take = win ? child_distance < distance : child_distance > distance;
    }
    if (take) { value = child_value; distance = child_distance; }
    any = true;
  }
  OSG_HD int32_t result_distance() const { return any ? distance + 1 : 0; }
};

// Index of `key` in the ascending keys [first, last) of one level, -1 if absent.
OSG_HD int64_t solve_find(const uint64_t* lo, const uint64_t* hi, int64_t first, int64_t last, const SolveKey& key) {
  int64_t a = first, b = last;
  while (a < b) {
    const int64_t m = a + (b - a) / 2;
    const SolveKey km{lo[m], hi ? hi[m] : 0ull};
    if (solve_key_less(km, key)) a = m + 1; else b = m;
  }
  if (a < last && solve_key_equal(SolveKey{lo[a], hi ? hi[a] : 0ull}, key)) return a;
  return -1;
}

// Largest i in [0, n) with off[i] <= e (off ascending, off[0] = 0 <= e < off[n]): the parent of edge e.
OSG_HD int64_t solve_edge_parent(const int64_t* off, int64_t n, int64_t e) {
  int64_t a = 0, b = n;
  while (b - a > 1) {
    const int64_t m = a + (b - a) / 2;
    if (off[m] <= e) a = m; else b = m;
  }
  return a;
}

}  // namespace osg
#endif  // OSG_SOLVE_H_
