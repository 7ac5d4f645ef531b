// Host-side check of step/osg_c4_step_split.h (c4_place + c4_finish, the body of k_step_c4std2 / k_step_c4std)
// against c4_fused_step (osg_c4_step.h, itself checked against an array model by c4_step_host_test.cpp):
// bit-identical planes, mask and status on every move of 200 000 random games played to the end.  Every position
// met is also fed "no action" (0xFF), an action >= 7 and, where a column is full, a move into it; finished games
// are stepped again.  The program counts what it exercised and fails if a kind never occurred.
//   hipcc --cuda-host-only -x hip -O2 -I open_spiel_amd/csrc tests/native/c4_step_split_host_test.cpp
#include <cstdio>
#include <cstdlib>
#include "step/osg_c4_step_split.h"

namespace {

long g_compared = 0;

// one action on one position through both forms; returns c4_fused_step's result and leaves its successor in x, o
bool both(uint64_t& x, uint64_t& o, uint32_t a, uint32_t* result) {
  uint64_t fx = x, fo = o, sx = x, so = o;
  const uint32_t fr = osg::c4_fused_step(fx, fo, a);
  const uint32_t sr = osg::c4_split_step(sx, so, a);
  // the pieces the kernels store: the o plane from c4_place alone, the rest after c4_finish
  const osg::C4Placed p = osg::c4_place(x, o, a);
  const uint64_t early_o = (static_cast<uint64_t>(p.no_hi) << 32) | p.no_lo;
  ++g_compared;
  if (fx != sx || fo != so || fr != sr || early_o != fo) {
    printf("MISMATCH action %u on %016llx %016llx: fused %016llx %016llx %04x, split %016llx %016llx %04x, o after placement %016llx\n",
           a, (unsigned long long)x, (unsigned long long)o, (unsigned long long)fx, (unsigned long long)fo, fr,
           (unsigned long long)sx, (unsigned long long)so, sr, (unsigned long long)early_o);
    return false;
  }
  x = fx;
  o = fo;
  *result = fr;
  return true;
}

// which of the four directions hold a run of four in plane b (bit = col * 7 + row)
unsigned directions(uint64_t b) {
  const int d[4] = {1, 7, 6, 8};  // vertical, horizontal, falling diagonal, rising diagonal
  unsigned r = 0;
  for (int k = 0; k < 4; ++k) {
    const uint64_t m = b & (b >> d[k]);
    if (m & (m >> (2 * d[k]))) r |= 1u << k;
  }
  return r;
}

}  // namespace

int main() {
  uint64_t z = 0xC4C4;
  long games = 0, wins[4] = {0, 0, 0, 0}, draws = 0, full_column = 0, no_action = 0, out_of_range = 0, after_end = 0;
  for (int game = 0; game < 200000; ++game) {
    uint64_t x = 0, o = 0;
    bool over = false;
    int extra = 0;
    for (int t = 0; t < 200 && extra < 3; ++t) {
      z = osg::mix64(z + 0x9E3779B97F4A7C15ULL);
      uint32_t r;
      // the three probes of this position, each on a copy
      {
        uint64_t cx = x, co = o;
        if (!both(cx, co, 0xFFu, &r)) return 1;
        if (cx != x || co != o || (r >> 8) & 0x40u) { printf("no action changed the state or was refused\n"); return 1; }
        ++no_action;
        cx = x; co = o;
        const uint32_t big = 7u + static_cast<uint32_t>((z >> 8) % 248u);  // 7 .. 254
        if (!both(cx, co, big, &r)) return 1;
        if (cx != x || co != o || !((r >> 8) & 0x40u)) { printf("action %u was not refused\n", big); return 1; }
        ++out_of_range;
        const uint64_t all = (x & ((1ull << 56) - 1ull)) | o;
        for (uint32_t c = 0; c < 7; ++c) {
          if (((all >> (7 * c)) & 0x3Full) != 0x3Full) continue;
          cx = x; co = o;
          if (!both(cx, co, c, &r)) return 1;
          if (cx != x || co != o || !((r >> 8) & 0x40u)) { printf("a move into full column %u was not refused\n", c); return 1; }
          ++full_column;
        }
      }
      // the move of the game: a random column with room (the full ones were fed above); a finished game is stepped
      // three more times
      uint32_t a = static_cast<uint32_t>(z % 7u);
      {
        const uint64_t all = (x & ((1ull << 56) - 1ull)) | o;
        for (int k = 0; k < 7 && !over && ((all >> (7 * a)) & 0x3Full) == 0x3Full; ++k) a = (a + 1u) % 7u;
      }
      const uint64_t px = x, po = o;
      if (!both(x, o, a, &r)) return 1;
      if (over) {
        if (x != px || o != po || !((r >> 8) & 0x40u)) { printf("a finished game moved\n"); return 1; }
        ++after_end;
        ++extra;
        continue;
      }
      if ((r >> 8) & 0x80u) {
        over = true;
        const unsigned outcome = (r >> 8) & 7u;
        if (outcome == 2u) {
          if (__builtin_popcountll((x & ((1ull << 56) - 1ull)) | o) != 42) { printf("a draw short of 42 stones\n"); return 1; }
          ++draws;
        } else {
          const unsigned dirs = directions(outcome == 0u ? (x & ((1ull << 56) - 1ull)) : o);
          if (!dirs) { printf("a win without a line\n"); return 1; }
          for (int k = 0; k < 4; ++k) wins[k] += (dirs >> k) & 1u;
        }
      }
    }
    if (!over) { printf("game %d did not end\n", game); return 1; }
    ++games;
  }
  printf("ok: %ld games, %ld steps compared; wins vertical %ld horizontal %ld falling %ld rising %ld, draws %ld, "
         "full-column refusals %ld, no-action %ld, out-of-range %ld, steps after the end %ld\n",
         games, g_compared, wins[0], wins[1], wins[2], wins[3], draws, full_column, no_action, out_of_range, after_end);
  if (!wins[0] || !wins[1] || !wins[2] || !wins[3] || !draws || !full_column || !no_action || !out_of_range || !after_end) {
    printf("FAIL: a kind of step was never exercised\n");
    return 1;
  }
  return 0;
}
