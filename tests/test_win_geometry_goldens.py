"""tests/golden/win_geometry_vectors.npz (tests/golden/make_win_geometry_vectors.py): directed histories for the board
rules — every connect_four line placement for both colours on five geometries, draws, wins on the board's last cell,
column-wrap near misses, and hex chains whose flood fill is deeper than 128 steps.

What the file claims to cover is RECOMPUTED here from the histories alone, by a few lines of plain Python that share
nothing with the generator's search (its rules model is not imported for this); then the oracle, and where it is built
the genuine reference build, replay every history and must give the recorded results at every recorded point.  The
device is held to the same histories by tests/test_z15_gpu_win_geometry.py.

tests/golden/win_geometry_edge_vectors.npz holds the same for seven connect_four geometries at the edges of what the
device's bitboards hold (boards two columns wide and 31 / 63 rows tall, boards of exactly 64 and 128 bits with x_in_row =
columns and columns + 1, and x_in_row = 1).  A kind that cannot exist on a board has zero cases there, and which kinds
those are is worked out here from the geometry, not read from the file."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

C4_GEOMETRY = {   # set: rows, columns, x_in_row, number of line placements (connect_four.cc HasLine's four directions)
    "c4_6x7": (6, 7, 4, 69), "c4_5x6x3": (5, 6, 3, 62), "c4_8x8": (8, 8, 4, 130), "c4_9x10x5": (9, 10, 5, 164),
    "c4_7x15": (7, 15, 4, 240)}
C4_EDGE_GEOMETRY = {   # the second file: 28 / 60 vertical placements per column; whole rows only; none; single cells
    "c4e_31x2": (31, 2, 4, 56), "c4e_63x2": (63, 2, 4, 120), "c4e_7x8x8": (7, 8, 8, 7), "c4e_7x8x9": (7, 8, 9, 0),
    "c4e_7x16x16": (7, 16, 16, 7), "c4e_7x16x17": (7, 16, 17, 0), "c4e_4x5x1": (4, 5, 1, 20)}
C4_ALL = {**C4_GEOMETRY, **C4_EDGE_GEOMETRY}
HEX_BOARD = {     # set: rows, columns, whether the chain is deeper than the 128 flood steps HexT::apply once stopped at
    "hex_19": (19, 19, True), "hex_18": (18, 18, True), "hex_17x19": (19, 17, True), "hex_16": (16, 16, False),
    "hex_11": (11, 11, False)}
LINE, DRAW, LAST_CELL, NEAR_MISS, CHAIN_NEAR_FIRST, CHAIN_FAR_FIRST = range(6)
STEPS = ((1, 0), (0, 1), (1, 1), (-1, 1))   # (d_row, d_col) of direction codes 0 .. 3


@pytest.fixture(scope="module")
def vectors():
    out = {}
    for name in ("win_geometry_vectors.npz", "win_geometry_edge_vectors.npz"):
        path = os.path.join(GOLDEN, name)
        assert os.path.getsize(path) < 100 * 1024
        with np.load(path) as z:
            assert not set(z.files) & set(out)
            out.update({k: z[k] for k in z.files})
    return out


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_win_geometry_vectors", os.path.join(GOLDEN, "make_win_geometry_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_set(vectors, name):
    return {k.split("/", 1)[1]: v for k, v in vectors.items() if k.startswith(name + "/")}


def placements(R, C, K):
    """{frozenset of cells: direction} of every K in a row that fits the board (cell = row * C + column)."""
    out = {}
    for d, (dr, dc) in enumerate(STEPS):
        for r in range(R):
            for c in range(C):
                if 0 <= r + (K - 1) * dr < R and 0 <= c + (K - 1) * dc < C:
                    out.setdefault(frozenset((r + i * dr) * C + c + i * dc for i in range(K)), d)   # (K = 1: one cell, direction 0)
    return out


def drop_stones(history, R, C):
    """({cell: colour}, the cell of the last stone) after dropping the history's stones into their columns."""
    owner, height, cell = {}, [0] * C, -1
    for t, col in enumerate(history):
        assert 0 <= col < C and height[col] < R
        cell = height[col] * C + col
        owner[cell] = t & 1
        height[col] += 1
    return owner, cell


def owned_lines(owner, lines, colour, through=None):
    return {l for l in lines if (through is None or through in l) and all(owner.get(c) == colour for c in l)}


def test_the_sets_are_recorded_with_consistent_shapes(vectors):
    assert {k.split("/")[0] for k in vectors} == set(C4_ALL) | set(HEX_BOARD)
    for name in list(C4_ALL) + list(HEX_BOARD):
        s = case_set(vectors, name)
        is_c4 = name in C4_ALL
        assert set(s) == {"game", "histories", "end_ply", "returns", "kind", "winner"} | ({"direction", "cells"} if is_c4 else {"depth"})
        n = len(s["kind"])
        assert s["histories"].dtype == (np.int8 if is_c4 else np.int16) and s["histories"].shape[0] == n
        plies = (s["histories"] >= 0).sum(axis=1)
        assert ((s["histories"] >= 0) == (np.arange(s["histories"].shape[1])[None, :] < plies[:, None])).all()   # padded at the end
        assert s["end_ply"].shape == (n,) and s["returns"].shape == (n, 2) and s["winner"].shape == (n,)
        ends = s["end_ply"] >= 0
        assert (s["end_ply"][ends] == plies[ends]).all() and (s["end_ply"][~ends] == -1).all()
        assert ((s["kind"] == NEAR_MISS) == ~ends).all()
        won = np.isin(s["kind"], (LINE, LAST_CELL, CHAIN_NEAR_FIRST, CHAIN_FAR_FIRST))
        assert (s["returns"][won, 0] == 1 - 2 * s["winner"][won]).all() and (s["returns"][:, 1] == -s["returns"][:, 0]).all()
        assert (s["returns"][~won] == 0).all()
        if is_c4:
            R, C, K, _ = C4_ALL[name]
            assert s["cells"].shape == (n, K) and s["histories"].shape[1] <= R * C
            assert f"rows={R}" in bytes(s["game"]).decode() or (R, C) == (6, 7)


def reachable_line_cases(R, C, K, lines):
    """The (placement, colour) pairs a game can end on.  x_in_row = 1: the first stone wins, so only the first player
    and only the bottom row.  A whole bottom row (x_in_row = columns) can only be the first player's, whose first stone
    lies in it; a whole top row means a full board, an even number of stones, so the second player made the last move.
    Everything else on these boards is reachable (and found)."""
    if K == 1:
        return {(l, 0) for l in lines if min(l) < C}
    out = {(l, colour) for l in lines for colour in (0, 1)}
    if K == C:
        out -= {(frozenset(range(C)), 1), (frozenset(range((R - 1) * C, R * C)), (R * C) & 1)}
    return out


@pytest.mark.parametrize("name", list(C4_ALL))
def test_connect_four_coverage_recomputed_from_the_histories(vectors, name):
    R, C, K, n_lines = C4_ALL[name]
    s = case_set(vectors, name)
    lines = placements(R, C, K)
    assert len(lines) == n_lines
    covered, draws, last_cell, near = set(), 0, 0, set()
    for i in range(len(s["kind"])):
        h = [int(a) for a in s["histories"][i] if a >= 0]
        kind, winner = int(s["kind"][i]), int(s["winner"][i])
        recorded = frozenset(int(c) for c in s["cells"][i] if c >= 0)
        owner, last = drop_stones(h, R, C)
        mover = (len(h) - 1) & 1
        before = dict(owner)
        del before[last]
        assert not owned_lines(before, lines, 0) and not owned_lines(before, lines, 1), (name, i, "a line before the last move")
        done = owned_lines(owner, lines, mover, through=last)
        assert not owned_lines(owner, lines, 1 - mover)
        if kind == LINE:
            assert done == {recorded} and winner == mover and lines[recorded] == int(s["direction"][i]), (name, i)   # that line and no other
            covered.add((recorded, winner))
        elif kind == DRAW:
            assert not done and len(h) == R * C and winner == -1, (name, i)
            draws += 1
        elif kind == LAST_CELL:
            assert recorded in done and len(h) == R * C and winner == mover and lines[recorded] == int(s["direction"][i]), (name, i)
            assert last // C == R - 1
            last_cell += 1
        else:
            assert kind == NEAR_MISS and not done and len(h) < R * C and not owned_lines(owner, lines, mover), (name, i)
            assert all(owner.get(c) == winner for c in recorded) and len(recorded) == K
            cols = sorted({c % C for c in recorded})
            assert len(cols) == 2 and cols[1] == cols[0] + 1
            upper = sorted(c // C for c in recorded if c % C == cols[0])
            lower = sorted(c // C for c in recorded if c % C == cols[1])
            j = len(upper)
            assert 1 <= j < K and upper == list(range(R - j, R)) and lower == list(range(K - j))   # top j of column c, bottom K - j of c + 1
            near.add((cols[0], j, winner))
    print(f"{name}: {len(covered)} (line, colour) pairs of {2 * n_lines}, {draws} draws, {last_cell} wins on the last cell, "
          f"{len(near)} near misses of {(C - 1) * (K - 1) * 2}")
    assert covered == reachable_line_cases(R, C, K, lines)
    # kinds that cannot exist have zero cases: no draw where the first stone wins; no win on the last cell without a
    # line to complete there (none exists, or the game ended long before); a near miss needs a split of x_in_row that
    # fits two columns (j and x_in_row - j cells, neither above the rows)
    assert draws >= 4 if K > 1 else draws == 0
    if name in ("c4_6x7", "c4_8x8"):
        assert last_cell >= 8
    if name in C4_EDGE_GEOMETRY:
        assert last_cell >= 1 if (lines and K > 1) else last_cell == 0
    splits = [j for j in range(1, K) if j <= R and K - j <= R]
    assert near == {(c, j, colour) for c in range(C - 1) for j in splits for colour in (0, 1)}   # every split
    if name in C4_GEOMETRY:
        assert len(near) == (C - 1) * (K - 1) * 2
    if K > 2 * R or K == 1:
        assert not near                  # (7 x 16 with 16 / 17 in a row: no split fits two columns of 7)


def hex_adjacent(cell, R, C):
    r, c = divmod(cell, C)
    return [rr * C + cc for rr, cc in ((r - 1, c), (r - 1, c + 1), (r, c - 1), (r, c + 1), (r + 1, c - 1), (r + 1, c))
            if 0 <= rr < R and 0 <= cc < C]


def flood_depth(history, R, C):
    """Breadth-first depth of the winner's group from its last stone but one, over its stones placed before (none of which
    may lie on one of its edges: they are all still plain, so the reference's relabelling flood covers exactly them)."""
    winner = (len(history) - 1) & 1
    stones = set(history[winner:-3:2])
    first_edge, second_edge = history[-3], history[-1]
    on_edge = (lambda x: x // C in (0, R - 1)) if winner == 0 else (lambda x: x % C in (0, C - 1))
    assert not any(on_edge(x) for x in stones) and on_edge(first_edge) and on_edge(second_edge)
    seen, frontier, depth = {first_edge}, [first_edge], 0
    while True:
        grow = {n for x in frontier for n in hex_adjacent(x, R, C) if n in stones and n not in seen}
        if not grow:
            break
        seen |= grow
        frontier = list(grow)
        depth += 1
    assert seen == stones | {first_edge} and any(n in seen for n in hex_adjacent(second_edge, R, C))   # one group; the last stone joins it
    return depth


@pytest.mark.parametrize("name", list(HEX_BOARD))
def test_hex_chain_depths_are_on_the_right_side_of_128(vectors, name):
    R, C, deep = HEX_BOARD[name]
    s = case_set(vectors, name)
    seen = set()
    for i in range(len(s["kind"])):
        h = [int(a) for a in s["histories"][i] if a >= 0]
        assert len(set(h)) == len(h) and all(0 <= a < R * C for a in h)
        winner = (len(h) - 1) & 1
        assert winner == int(s["winner"][i])
        depth = flood_depth(h, R, C)
        assert depth == int(s["depth"][i]) and (depth > 128 if deep else depth < 128), (name, i, depth)
        near_edge = (lambda x: x // C == 0) if winner == 0 else (lambda x: x % C == 0)   # black's first row / white's first column
        kind = CHAIN_NEAR_FIRST if near_edge(h[-3]) else CHAIN_FAR_FIRST
        assert kind == int(s["kind"][i]) and near_edge(h[-3]) != near_edge(h[-1])
        seen.add((winner, kind))
    assert seen == {(w, k) for w in (0, 1) for k in (CHAIN_NEAR_FIRST, CHAIN_FAR_FIRST)}


def replay_and_compare(binding, vectors, name):
    s = case_set(vectors, name)
    game = binding.Game(bytes(s["game"]).decode())
    for i in range(len(s["kind"])):
        h = [int(a) for a in s["histories"][i] if a >= 0]
        state = game.new_initial_state()
        for t, a in enumerate(h):
            assert not state.is_terminal() and state.current_player() == (t & 1), (name, i, t)
            assert a in state.legal_actions(), (name, i, t)
            state.apply_action(a)
        end = int(s["end_ply"][i])
        assert state.is_terminal() == (end == len(h)) and (end >= 0) == (state.legal_actions() == []), (name, i)
        assert state.returns() == [float(x) for x in s["returns"][i]], (name, i)


@pytest.mark.parametrize("name", list(C4_ALL) + list(HEX_BOARD))
def test_the_oracle_replays_every_history_to_the_recorded_results(oracle, vectors, name):
    replay_and_compare(oracle, vectors, name)


@pytest.mark.parametrize("name", list(C4_ALL) + list(HEX_BOARD))
def test_the_reference_build_replays_every_history_to_the_recorded_results(reference, vectors, name):
    replay_and_compare(reference, vectors, name)


def test_the_generator_reproduces_a_sample_of_the_file(gen, vectors):
    """Every directed search has a seed of its own, so single cases can be searched for again: a sample of the line
    histories of every geometry and every hex case come out as recorded (the whole file takes two minutes)."""
    assert set(gen.C4_SETS) == set(C4_GEOMETRY) and set(gen.HEX_SETS) == set(HEX_BOARD)
    for name, geom in gen.C4_SETS.items():
        s = case_set(vectors, name)
        assert bytes(s["game"]).decode() == geom["game"]
        base = sorted(gen.C4_SETS).index(name) * 1_000_000
        lines = gen.all_lines(geom["R"], geom["C"], geom["K"])
        for li in range(0, len(lines), 17):
            for colour in (0, 1):
                h, _ = gen.search(geom, base + 10 * li + colour, gen.LINE_TRIES, "line", targets=lines[li][1], winner=colour)
                row = s["histories"][2 * li + colour]
                assert h == [int(a) for a in row if a >= 0], (name, li, colour)
    for name, spec in gen.HEX_SETS.items():
        s = case_set(vectors, name)
        assert bytes(s["game"]).decode() == spec["game"]
        for i, (kind, h, winner, depth) in enumerate(gen.hex_cases(name)):
            assert h == [int(a) for a in s["histories"][i] if a >= 0]
            assert (kind, winner, depth) == (int(s["kind"][i]), int(s["winner"][i]), int(s["depth"][i]))


@pytest.mark.parametrize("name", ["c4e_7x8x8", "c4e_7x8x9", "c4e_4x5x1", "c4e_31x2"])
def test_the_generator_reproduces_edge_sets(gen, vectors, name):
    """Whole edge sets searched for again (their own seeds: the first file's do not move when a set is added here)."""
    assert set(gen.C4_EDGE_SETS) == set(C4_EDGE_GEOMETRY)
    s = case_set(vectors, name)
    geom = gen.C4_EDGE_SETS[name]
    assert bytes(s["game"]).decode() == geom["game"] and (geom["R"], geom["C"], geom["K"]) == C4_EDGE_GEOMETRY[name][:3]
    cases = gen.c4_cases(name, gen.C4_EDGE_SETS, 100)
    assert len(cases) == len(s["kind"])
    for i, (kind, h, winner, direction, _) in enumerate(cases):
        assert h == [int(a) for a in s["histories"][i] if a >= 0], (name, i)
        assert (kind, winner, direction) == (int(s["kind"][i]), int(s["winner"][i]), int(s["direction"][i]))
