// The fused connect_four step of osg_c4_step.h (c4_fused_step) cut in two at the point where the o plane is final,
// and written against the 32-bit halves of the planes so that no 64-bit vector instruction is paid where a half is
// known empty.  c4_place: legality, the dropped stone, both successor planes, the stone count.  c4_finish: the mover's
// line test, the result flags, the successor's legal mask and the status byte.  c4_finish(c4_place(x, o, a)) gives
// c4_fused_step's planes, mask and status bit for bit on every state whose planes keep bits 48-55 (x) / 48-63 (o)
// empty, as every state of the engine does (tests/native/c4_step_split_host_test.cpp); the kernels k_step_c4std2 /
// k_step_c4std (osg_step.hip) store the o plane between the two.  Host + device.
//
// Layout as in osg_c4_step.h: bit = col * 7 + row, row 6 of every column an always-empty sentinel, so the high word
// of a plane holds bits 0-15 only (columns 4-6 from row 4 of column 4 on); plane 0's top byte = result flags.
#ifndef OSG_C4_STEP_SPLIT_H_
#define OSG_C4_STEP_SPLIT_H_

#include "../osg_c4_step.h"

namespace osg {

// What c4_place hands to c4_finish.  nx_hi carries no flags yet.
struct C4Placed {
  uint32_t nx_lo, nx_hi, no_lo, no_hi;  // successor planes
  uint32_t b_lo, b_hi;                  // the mover's plane after the move: the only one that can hold a new line
  uint32_t flags;                       // result flags of the source state
  uint32_t mover;                       // 0 x, 1 o
  uint32_t stones_after;
  bool apply;                           // the stone was placed
  bool refused;                         // an action other than 0xFF that was not applied
};

OSG_HD C4Placed c4_place(uint64_t x, uint64_t o, uint32_t a) {
  C4Placed p;
  const uint32_t x_lo = static_cast<uint32_t>(x), x_hi = static_cast<uint32_t>(x >> 32) & 0x00FFFFFFu;
  const uint32_t o_lo = static_cast<uint32_t>(o), o_hi = static_cast<uint32_t>(o >> 32);
  p.flags = static_cast<uint32_t>(x >> 56);
  const uint32_t all_lo = x_lo | o_lo, all_hi = x_hi | o_hi;
  const uint32_t stones = static_cast<uint32_t>(__builtin_popcount(all_lo) + __builtin_popcount(all_hi));
  p.mover = stones & 1u;
  const bool valid = a < 7u;
  const uint32_t sh = valid ? a * 7u : 0u;
  // the column's cells from bit 0 on (one 64-bit shift whose low word alone is used); cells fill from the bottom, so
  // + 1 carries to the lowest empty cell, and to bit 6 (masked off) when all six are taken
  const uint32_t col = static_cast<uint32_t>(((static_cast<uint64_t>(all_hi) << 32) | all_lo) >> sh);
  const uint32_t cell = (col + 1u) & 0x3Fu;
  p.apply = valid & ((p.flags & 1u) == 0u) & (cell != 0u);
  p.refused = (a != 0xFFu) & !p.apply;
  const uint64_t put = static_cast<uint64_t>(p.apply ? cell : 0u) << sh;
  const uint32_t put_lo = static_cast<uint32_t>(put), put_hi = static_cast<uint32_t>(put >> 32);
  p.b_lo = (p.mover ? o_lo : x_lo) | put_lo;
  p.b_hi = (p.mover ? o_hi : x_hi) | put_hi;
  p.nx_lo = p.mover ? x_lo : p.b_lo;
  p.nx_hi = p.mover ? x_hi : p.b_hi;
  p.no_lo = p.mover ? p.b_lo : o_lo;
  p.no_hi = p.mover ? p.b_hi : o_hi;
  p.stones_after = stones + (p.apply ? 1u : 0u);
  return p;
}

// Run-of-four test on the halves of one player's stones (c4_fours != 0).  A line of step d starting in the high word
// would end at bit 32 + 3d or beyond: past the board for the horizontal and both diagonal steps (d = 7, 6, 8: bits
// 53, 50, 56 at the least), so those three have a low-word term only; the vertical step has both.
// Each low-word term is the plane and its three funnel shifts by d, 2d, 3d (<= 24 bits: one v_alignbit_b32 each),
// and-ed: five vector instructions per step with the or into `hit`, where two 64-bit shifts and their ands took ten
// issue slots.
OSG_HD uint32_t c4_window(uint32_t lo, uint32_t hi, uint32_t s) { return (lo >> s) | (hi << (32u - s)); }  // 0 < s < 32
OSG_HD bool c4_has_four(uint32_t lo, uint32_t hi) {
  uint32_t hit = hi & (hi >> 1) & (hi >> 2) & (hi >> 3);
  hit |= lo & c4_window(lo, hi, 1) & c4_window(lo, hi, 2) & c4_window(lo, hi, 3);
  hit |= lo & c4_window(lo, hi, 7) & c4_window(lo, hi, 14) & c4_window(lo, hi, 21);
  hit |= lo & c4_window(lo, hi, 6) & c4_window(lo, hi, 12) & c4_window(lo, hi, 18);
  hit |= lo & c4_window(lo, hi, 8) & c4_window(lo, hi, 16) & c4_window(lo, hi, 24);
  return hit != 0u;
}

// The rest of the step.  Returns mask | status << 8; flags_out = the successor's result flags (plane 0's top byte).
OSG_HD uint32_t c4_finish(const C4Placed& p, uint32_t& flags_out) {
  const bool win = c4_has_four(p.b_lo, p.b_hi);
  const bool done = win | (p.stones_after == 42u);
  const uint32_t fresh = done ? (((win ? p.mover : 2u) << 1) | 1u) : 0u;
  const uint32_t nflags = p.apply ? fresh : p.flags;
  const uint32_t open = c4_open_columns(p.nx_lo | p.no_lo, p.nx_hi | p.no_hi);
  const bool over = (nflags & 1u) != 0u;
  const uint32_t st_run = (p.stones_after & 1u) + 1u;
  const uint32_t st_over = 0x80u | (nflags >> 1);
  const uint32_t st = (over ? st_over : st_run) | (p.refused ? 0x40u : 0u);
  flags_out = nflags;
  return (over ? 0u : open) | (st << 8);
}

// The two halves put together again: c4_fused_step's signature and meaning.
OSG_HD uint32_t c4_split_step(uint64_t& x, uint64_t& o, uint32_t a) {
  const C4Placed p = c4_place(x, o, a);
  uint32_t nflags;
  const uint32_t r = c4_finish(p, nflags);
  x = (static_cast<uint64_t>(p.nx_hi | (nflags << 24)) << 32) | p.nx_lo;
  o = (static_cast<uint64_t>(p.no_hi) << 32) | p.no_lo;
  return r;
}

}  // namespace osg
#endif  // OSG_C4_STEP_SPLIT_H_
