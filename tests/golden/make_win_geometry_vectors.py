#!/usr/bin/env python3
"""Directed histories for the board rules: every connect_four line, draws, wins on the board's last cell, column-wrap
near misses, and hex chains whose flood fill is deeper than 128 steps.  Random playouts (what every other device check
of the board rules replays) decide by chance which win geometries are ever seen; these histories are SEARCHED FOR, by a
small pure-Python rules model written for this file, and every history kept is then replayed on the genuine reference
build (oracle/_ref/libspiel_ref.so through oracle/reference_py.py), whose answers are what is recorded.  Run in the
build container (needs the reference sources):

    python tests/golden/make_win_geometry_vectors.py

Output: tests/golden/win_geometry_vectors.npz (fixed seeds, fixed zip timestamps: byte for byte reproducible) and
tests/golden/win_geometry_edge_vectors.npz (`--edge` writes only this one): the connect_four geometries at the edges of
what the device's bitboards hold (C4_EDGE_SETS), same arrays, searched with their own seeds so that the first file
keeps its bytes.  Per set <set> (SETS below: five connect_four geometries, five hex boards; seven edge geometries):

  <set>/game        the game string (bytes)
  <set>/histories   [n, L] action histories from the initial state, padded with -1 (int8 connect_four, int16 hex)
  <set>/end_ply     [n] int16: the number of plies after which the reference first says IsTerminal(); -1 = it never does
                    (the near misses); the reference says "not terminal" after every shorter prefix
  <set>/returns     [n, 2] int8: the reference's Returns() after the whole history
  <set>/kind        [n] int8: 0 line, 1 draw, 2 win on the board's last cell, 3 column-wrap near miss,
                    4 hex chain, near edge stone first, 5 hex chain, far edge stone first
  <set>/winner      [n] int8: the colour that wins (0 = first player) or, for a near miss, that holds the cells; -1 draw
  connect_four only
  <set>/direction   [n] int8: 0 vertical, 1 horizontal, 2 rising diagonal, 3 falling diagonal; -1 = none (draws, near misses)
  <set>/cells       [n, x_in_row] int16: the line (kinds 0, 2: a line the last move completes; kind 0: the ONLY one) or
                    the near miss's cells, as row * columns + column with row 0 at the bottom; -1 = none
  hex only
  <set>/depth       [n] int16: breadth-first depth of the winner's group from its first edge stone (what a flood that
                    relabels the group has to cover: above 128 on the three large boards, below on the two controls)

connect_four kinds.  0: for every placement of x_in_row cells in each direction and each colour, one history whose last
move completes exactly that placement (no other, so no five in a row either).  1: the board fills without a line.
2: the move into the board's last empty cell makes a line.  3: for adjacent columns c, c + 1 and a split j, one colour
holds the top j cells of column c and the bottom x_in_row - j cells of column c + 1 — consecutive bits of a column-major
bitboard but for the sentinel bit between the columns — and the game is not over.

hex.  White holds rows 0, 2, ... in columns 1 .. C - 2, joined into one serpentine chain by a single cell in each odd
row (alternately at column C - 2 and column 1); black fills other cells and never plays in row 0.  White then plays
(0, 0) and the far end of the chain's last row, in either order: the first of the two relabels the whole chain (a flood
as deep as the chain is long), the second wins.  The transposed construction gives black the chain.  (Where the chain
would hold an even number of rows it would end on the edge it started from: there one more row joins it and the last two
rows are shortened until the other colour has cells enough — chain_layout; black's chain on 17 columns x 19 rows.)

Consumers: tests/test_win_geometry_goldens.py (CPU), tests/test_z15_gpu_win_geometry.py (the HIP engine).
"""
import io
import os
import random
import sys
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "win_geometry_vectors.npz")
OUT_EDGE = os.path.join(ROOT, "tests", "golden", "win_geometry_edge_vectors.npz")

KIND_LINE, KIND_DRAW, KIND_LAST_CELL, KIND_NEAR_MISS, KIND_CHAIN_NEAR_FIRST, KIND_CHAIN_FAR_FIRST = range(6)
DIRS = ((1, 0), (0, 1), (1, 1), (-1, 1))   # (d_row, d_col): vertical, horizontal, rising, falling

# name: game string, rows, columns, x_in_row, attempts per top-row line of the last-cell search (the other bounds are below)
C4_SETS = {
    "c4_6x7": dict(game="connect_four", R=6, C=7, K=4, last_tries=1500),
    "c4_5x6x3": dict(game="connect_four(rows=5,columns=6,x_in_row=3)", R=5, C=6, K=3, last_tries=300),
    "c4_8x8": dict(game="connect_four(rows=8,columns=8)", R=8, C=8, K=4, last_tries=1000),
    "c4_9x10x5": dict(game="connect_four(rows=9,columns=10,x_in_row=5)", R=9, C=10, K=5, last_tries=150),
    "c4_7x15": dict(game="connect_four(rows=7,columns=15)", R=7, C=15, K=4, last_tries=100),
}
# The edges of the accepted geometries (H = rows + 1 bits per column; one 64-bit word per colour up to 64 bits, two up
# to 128): boards so tall that a shift of the line test reaches the word width, boards that fill their words exactly
# with x_in_row = columns (only whole rows are lines) and columns + 1 (no line exists: zero cases of kinds 0 and 2),
# and x_in_row = 1 (the first stone wins: one line case per column, nothing else).  Kinds that cannot exist on a board
# are recorded with zero cases (tests/test_win_geometry_goldens.py asserts which).  `tries` thins the searches: the long
# histories of these boards cost more per attempt; a line or near miss not found within them is left out.
C4_EDGE_SETS = {
    "c4e_31x2": dict(game="connect_four(rows=31,columns=2)", R=31, C=2, K=4, last_tries=300, tries=3000),
    "c4e_63x2": dict(game="connect_four(rows=63,columns=2)", R=63, C=2, K=4, last_tries=300, tries=3000),
    "c4e_7x8x8": dict(game="connect_four(rows=7,columns=8,x_in_row=8)", R=7, C=8, K=8, last_tries=300, tries=3000),
    "c4e_7x8x9": dict(game="connect_four(rows=7,columns=8,x_in_row=9)", R=7, C=8, K=9, last_tries=10, tries=3000),
    "c4e_7x16x16": dict(game="connect_four(rows=7,columns=16,x_in_row=16)", R=7, C=16, K=16, last_tries=300, tries=3000),
    "c4e_7x16x17": dict(game="connect_four(rows=7,columns=16,x_in_row=17)", R=7, C=16, K=17, last_tries=10, tries=3000),
    "c4e_4x5x1": dict(game="connect_four(rows=4,columns=5,x_in_row=1)", R=4, C=5, K=1, last_tries=10, tries=50),
}
HEX_SETS = {
    "hex_19": dict(game="hex(board_size=19)", R=19, C=19, deep=True),
    "hex_18": dict(game="hex(board_size=18)", R=18, C=18, deep=True),
    "hex_17x19": dict(game="hex(num_cols=17,num_rows=19)", R=19, C=17, deep=True),
    "hex_16": dict(game="hex(board_size=16)", R=16, C=16, deep=False),
    "hex_11": dict(game="hex", R=11, C=11, deep=False),
}
FLOOD_CAP = 128   # the depth the hex sets straddle
LINE_TRIES, NEAR_TRIES, DRAW_TRIES, DRAWS_KEPT = 3000, 3000, 60000, 4


# ---------------------------------------------------------------------------------------------------------------------
# connect_four: a rules model for the search (columns of stones; a line = x_in_row equal stones in a row)
# ---------------------------------------------------------------------------------------------------------------------
def all_lines(R, C, K):
    """Every placement of K cells in a row: (direction, ((row, col), ...)) in a fixed order."""
    out = []
    for d, (dr, dc) in enumerate(DIRS[:1] if K == 1 else DIRS):     # (one cell is the same placement in every direction)
        for r in range(R):
            for c in range(C):
                r1, c1 = r + (K - 1) * dr, c + (K - 1) * dc
                if 0 <= r1 < R and 0 <= c1 < C:
                    out.append((d, tuple((r + i * dr, c + i * dc) for i in range(K))))
    return out


class Board:
    def __init__(self, R, C, K):
        self.R, self.C, self.K = R, C, K
        self.height = [0] * C
        self.at = {}          # (row, col) -> colour
        self.history = []

    def runs(self, r, c, colour):
        """Per direction, the length of the run of `colour` through (r, c) if that cell were (or is) `colour`."""
        out = []
        for dr, dc in DIRS:
            n = 1
            for s in (1, -1):
                rr, cc = r + s * dr, c + s * dc
                while self.at.get((rr, cc)) == colour:
                    n += 1
                    rr, cc = rr + s * dr, cc + s * dc
            out.append(n)
        return out

    def play(self, c):
        r = self.height[c]
        self.at[(r, c)] = len(self.history) & 1
        self.height[c] = r + 1
        self.history.append(c)


def pick(rng, weighted):
    total = sum(w for _, w in weighted)
    x = rng.random() * total
    for item, w in weighted:
        x -= w
        if x < 0:
            return item
    return weighted[-1][0]


def guided(geom, rng, mode, targets=(), winner=-1, hold=None):
    """One attempt.  mode "line": `winner` completes exactly `targets` with its last move; "near": `winner` comes to
    hold `targets` and nobody has a line; "draw": the board fills without a line; "last": `winner` completes `targets`
    by playing `hold` into the board's last empty cell.  Nobody completes any other line on the way.  Returns the
    history, or None on a dead end."""
    R, C, K = geom["R"], geom["C"], geom["K"]
    b = Board(R, C, K)
    T = set(targets)
    missing = set(T)
    cells = R * C
    while True:
        mover = len(b.history) & 1
        left = cells - len(b.history)
        if left == 0:
            return b.history if mode == "draw" else None
        options = []
        for c in range(C):
            r = b.height[c]
            if r >= R:
                continue
            cell = (r, c)
            if cell in T and mover != winner:
                continue
            if mode == "last" and cell == hold and left > 1:
                continue
            runs = b.runs(r, c, mover)
            if max(runs) >= K:
                closes = mover == winner and missing == {cell} and (mode == "line" or (mode == "last" and left == 1))
                if not closes:
                    continue
                if mode == "line" and K > 1 and sum(max(0, n - K + 1) for n in runs) != 1:
                    continue          # would complete a second placement as well
                b.play(c)
                return b.history
            if mode == "last" and left == 1:
                continue              # the last cell must win
            if cell in T:
                weight = 10.0
            elif any(tc == c and tr > r and (tr, tc) in missing for tr, tc in T):
                weight = 3.0          # build up towards a target cell
            else:
                weight = 1.0
            options.append((c, weight))
        if not options:
            return None
        c = pick(rng, options)
        missing.discard((b.height[c], c))
        b.play(c)
        if mode == "near" and not missing:
            return b.history if len(b.history) < cells else None


def search(geom, seed, tries, mode, **kw):
    rng = random.Random(seed)
    for t in range(tries):
        if mode == "last" and kw.get("holds"):
            hold = kw["holds"][int(rng.random() * len(kw["holds"]))]
            h = guided(geom, rng, mode, targets=kw["targets"], winner=kw["winner"], hold=hold)
        else:
            h = guided(geom, rng, mode, **{k: v for k, v in kw.items() if k != "holds"})
        if h is not None:
            return h, t + 1
    return None, tries


def c4_cases(name, sets=None, first_base=0):
    """[(kind, history, winner, direction, cells)] of one geometry, in a fixed order.  The edge sets (`tries` given) keep
    what their thinned searches find; the others must find every line and DRAWS_KEPT draws."""
    sets = C4_SETS if sets is None else sets
    geom = sets[name]
    R, C, K = geom["R"], geom["C"], geom["K"]
    edge = "tries" in geom
    base = (first_base + sorted(sets).index(name)) * 1_000_000
    cases, worst = [], 0
    lines = all_lines(R, C, K)
    for li, (d, cells) in enumerate(lines):
        for colour in (0, 1):
            h, t = search(geom, base + 10 * li + colour, geom.get("tries", LINE_TRIES), "line", targets=cells, winner=colour)
            if h is None and edge:
                continue
            assert h is not None, f"{name}: no history for line {cells} colour {colour}"
            worst = max(worst, t)
            cases.append((KIND_LINE, h, colour, d, cells))
    print(f"{name}: {len(cases)} (line, colour) pairs of {len(lines)} lines, at most {worst} tries", flush=True)
    rng_seed, found, tries_used = base + 500_000, 0, 0
    rng = random.Random(rng_seed)
    while found < DRAWS_KEPT:
        tries_used += 1
        if edge and tries_used > geom["tries"]:
            break
        assert tries_used <= DRAW_TRIES, f"{name}: {found} draws in {DRAW_TRIES} tries"
        h = guided(geom, rng, "draw")
        if h is not None:
            cases.append((KIND_DRAW, h, -1, -1, None))
            found += 1
    print(f"{name}: {found} draws in {tries_used} tries", flush=True)
    last_mover = (R * C - 1) & 1
    n_last, top_lines = 0, [(d, cells) for d, cells in lines if any(r == R - 1 for r, _ in cells)]
    for li, (d, cells) in enumerate(top_lines):
        holds = [cell for cell in cells if cell[0] == R - 1]
        h, _ = search(geom, base + 600_000 + li, geom["last_tries"], "last", targets=cells, winner=last_mover, holds=holds)
        if h is not None:
            cases.append((KIND_LAST_CELL, h, last_mover, d, cells))
            n_last += 1
    print(f"{name}: wins on the last cell for {n_last} of {len(top_lines)} top-row lines", flush=True)
    n_near = 0
    for c in range(C - 1):
        for j in range(1, K):
            if j > R or K - j > R:
                continue              # (x_in_row above the rows: the split does not fit the two columns)
            cells = tuple((R - j + i, c) for i in range(j)) + tuple((i, c + 1) for i in range(K - j))
            for colour in (0, 1):
                h, _ = search(geom, base + 700_000 + 100 * c + 10 * j + colour, geom.get("tries", NEAR_TRIES), "near", targets=cells, winner=colour)
                if h is not None:
                    cases.append((KIND_NEAR_MISS, h, colour, -1, cells))
                    n_near += 1
    print(f"{name}: {n_near} of {(C - 1) * (K - 1) * 2} column-wrap near misses", flush=True)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# hex: the serpentine chain
# ---------------------------------------------------------------------------------------------------------------------
def hex_neighbours(r, c, R, C):
    for rr, cc in ((r - 1, c), (r - 1, c + 1), (r, c - 1), (r, c + 1), (r + 1, c - 1), (r + 1, c)):
        if 0 <= rr < R and 0 <= cc < C:
            yield rr, cc


def bfs_depth(stones, start, R, C):
    """The largest breadth-first distance from `start` within `stones` (start itself not among them)."""
    seen, frontier, depth = {start}, [start], 0
    while True:
        grow = []
        for r, c in frontier:
            for n in hex_neighbours(r, c, R, C):
                if n in stones and n not in seen:
                    seen.add(n)
                    grow.append(n)
        if not grow:
            return depth
        depth += 1
        frontier = grow


def chain_layout(R, C, lo):
    """(chain cells in order, the two end stones, the other colour's cells), or None where the other colour is short of
    cells.  The chain holds rows 0, 2, ... up to row R - 2 at most; it leaves row 0 eastwards, so an even number of
    rows would bring it back to the west edge: then, where row R - 1 is even, that row joins the chain and it and the
    row before span columns lo .. C - 2 only (the cells west of them are the other colour's; `lo` = 1 otherwise)."""
    last_row = (R - 2) // 2 * 2
    spans = {r: 1 for r in range(0, last_row + 1, 2)}
    if len(spans) % 2 == 0 and last_row + 2 == R - 1:
        last_row += 2
        spans[last_row - 2] = spans[last_row] = lo
    elif lo > 1:
        return None
    chain = []
    for r in range(0, last_row + 1, 2):
        eastwards = (r // 2) % 2 == 0
        cols = range(spans[r], C - 1)
        chain += [(r, c) for c in (cols if eastwards else reversed(cols))]
        if r < last_row:
            chain.append((r + 1, C - 2 if eastwards else spans[r + 2]))
    ends = [(0, 0), (last_row, C - 1)]     # (the last row reaches column C - 2 whichever way the chain runs through it)
    taken = set(chain) | set(ends)
    filler = [(r, c) for r in range(1, R) for c in range(C)
              if (r % 2 == 1 or r > last_row or (spans[r] > 1 and c < spans[r])) and (r, c) not in taken]
    return (chain, ends, filler) if len(filler) >= len(chain) + 2 else None


def chain_case(R, C, far_first):
    """White's chain on a board of R rows and C columns: (history as (row, col) moves, depth)."""
    for lo in range(1, C - 2):
        moves = chain_layout(R, C, lo)
        if moves is not None:
            chain, ends, filler = moves
            break
    white = chain + (ends[::-1] if far_first else ends)
    moves = []
    for i, w in enumerate(white):          # black (the filler) moves first
        moves += [filler[i], w]
    depth = bfs_depth(set(chain), white[-2], R, C)
    assert bfs_depth(set(chain) | {white[-2]}, white[-1], R, C) > 0
    return moves, depth


def hex_cases(name):
    """[(kind, history, winner, depth)]: white's chain and its transpose for black, both orders of the end stones."""
    spec = HEX_SETS[name]
    R, C = spec["R"], spec["C"]
    cases = []
    for winner in (1, 0):
        for far_first in (False, True):
            if winner == 1:
                moves, depth = chain_case(R, C, far_first)
            else:   # the transpose: black's chain runs down the columns, white is the filler and black moves first
                moves, depth = chain_case(C, R, far_first)
                moves = [(c, r) for r, c in moves][1:]
            assert (depth > FLOOD_CAP) == spec["deep"] and depth != FLOOD_CAP, (name, winner, depth)
            cases.append((KIND_CHAIN_FAR_FIRST if far_first else KIND_CHAIN_NEAR_FIRST, [r * C + c for r, c in moves], winner, depth))
    print(f"{name}: depths {[c[3] for c in cases]}, plies {[len(c[1]) for c in cases]}", flush=True)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# the reference's answers, and the file
# ---------------------------------------------------------------------------------------------------------------------
def reference_results(ref_game, history):
    """(end_ply, returns) as the reference build says: the first prefix length at which IsTerminal() holds (-1: none)."""
    s = ref_game.new_initial_state()
    end = -1
    for t, a in enumerate(history):
        assert not s.is_terminal() and a in s.legal_actions(), (history, t)
        s.apply_action(a)
        if s.is_terminal():
            end = t + 1
            assert end == len(history), "the history goes on after the end"
    return end, [int(x) for x in s.returns()]


def pack(histories, dtype):
    width = max(len(h) for h in histories)
    out = np.full((len(histories), width), -1, dtype)
    for i, h in enumerate(histories):
        out[i, :len(h)] = h
    return out


def build_sets(reference_py, edge=False):
    out = {}
    for name, spec in (C4_EDGE_SETS if edge else C4_SETS).items():
        cases = c4_cases(name, C4_EDGE_SETS, 100) if edge else c4_cases(name)
        game = reference_py.Game(spec["game"])
        res = [reference_results(game, c[1]) for c in cases]
        for (kind, _, winner, _, _), (end, rets) in zip(cases, res):   # the search's claims, checked on the reference
            want = {KIND_LINE: [1, -1] if winner == 0 else [-1, 1], KIND_LAST_CELL: [1, -1] if winner == 0 else [-1, 1],
                    KIND_DRAW: [0, 0], KIND_NEAR_MISS: [0, 0]}[kind]
            assert rets == want and (end == -1) == (kind == KIND_NEAR_MISS), (name, kind, end, rets)
        cells = np.full((len(cases), spec["K"]), -1, np.int16)
        for i, c in enumerate(cases):
            if c[4] is not None:
                cells[i] = [r * spec["C"] + col for r, col in c[4]]
        out[name] = dict(game=np.frombuffer(spec["game"].encode(), np.uint8), histories=pack([c[1] for c in cases], np.int8),
                         end_ply=np.array([r[0] for r in res], np.int16), returns=np.array([r[1] for r in res], np.int8),
                         kind=np.array([c[0] for c in cases], np.int8), winner=np.array([c[2] for c in cases], np.int8),
                         direction=np.array([c[3] for c in cases], np.int8), cells=cells)
    for name, spec in ({} if edge else HEX_SETS).items():
        cases = hex_cases(name)
        game = reference_py.Game(spec["game"])
        res = [reference_results(game, c[1]) for c in cases]
        for (_, h, winner, _), (end, rets) in zip(cases, res):
            assert end == len(h) and rets == ([1, -1] if winner == 0 else [-1, 1]), (name, end, rets)
        out[name] = dict(game=np.frombuffer(spec["game"].encode(), np.uint8), histories=pack([c[1] for c in cases], np.int16),
                         end_ply=np.array([r[0] for r in res], np.int16), returns=np.array([r[1] for r in res], np.int8),
                         kind=np.array([c[0] for c in cases], np.int8), winner=np.array([c[2] for c in cases], np.int8),
                         depth=np.array([c[3] for c in cases], np.int16))
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    for path, edge in ((OUT_EDGE, True),) if "--edge" in sys.argv[1:] else ((OUT, False), (OUT_EDGE, True)):
        t0 = time.time()
        sets = build_sets(reference_py, edge)
        write_npz(path, {f"{name}/{k}": v for name, s in sets.items() for k, v in s.items()})
        n = sum(len(s["kind"]) for s in sets.values())
        print(path, os.path.getsize(path), "bytes,", n, "histories,", f"{time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
