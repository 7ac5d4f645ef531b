#!/usr/bin/env python3
"""Golden state sets and game-theoretic values of small board games, produced by RUNNING the reference's own
open_spiel/python/algorithms/value_iteration.py and get_all_states.py, imported unmodified from where they lie, over
the genuine games (oracle/_ref/libspiel_ref.so through oracle/pyspiel_over_capi.py).  Run in the build container
(needs the reference tree):

    python tests/golden/make_solve_vectors.py

value_iteration.py imports open_spiel.python.algorithms.lp_solver, which needs cvxpy (not installed); that module is
only reached at simultaneous nodes, which none of these games has, so an EMPTY stand-in module of that name is put
into sys.modules before the import.  Nothing else is patched.

value_iteration() is called with its own argument cyclic_game=True: it hands it to get_all_states as
stop_if_encountered, so the enumeration stops at a position it has already seen.  With the default (False) the
reference walks the whole game TREE (every move order) to collect the same dict — 5 * 10^5 nodes for tic_tac_toe, more
than 10^9 for hex 3 x 4 — which the Python reference cannot do in ten minutes per case; the set of reachable positions
and the sweeps over it are the same either way (none of these games has a cycle).  No geometry of the issue's list had
to be replaced.

Output: tests/golden/solve_vectors.npz (np.savez_compressed).
  cases                      newline-joined case names; per case C:
  <C>/game                   the game string
  <C>/depth_limit, <C>/include_terminals
  <C>/count                  number of states
  <C>/keys_sha256            SHA-256 of "\x1e".join(sorted(str(state))) — state strings hold newlines, so the separator
                             is the ASCII record separator
  <C>/keys                   the "\x1e"-joined sorted strings themselves, cases of at most KEEP_KEYS states
  <C>/level_counts           states per ply (the ply of a position is its stone count)
  <C>/level_terminals        terminal states per ply
  <C>/level_children         sum of len(legal_actions()) over the non-terminal states of the ply (children before
                             duplicates are merged)
  <C>/values  int8 [count]   value_iteration's value of every state, in sorted-string order (full solves only)
  <C>/root_value             value of str(initial state) (full solves only)
The enumeration-only cases (a depth limit, include_terminals=False: value_iteration.py cannot run there, it looks up
children that the limited dict lacks) come from get_all_states(game, depth_limit, include_terminals, False,
to_string=str).

Consumers: tests/test_solve_goldens.py, tests/test_solve_native.py (CPU), tests/test_z19_gpu_solve.py (the HIP engine).
"""
import hashlib
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "solve_vectors.npz")
KEEP_KEYS = 6000
SEP = "\x1e"

SOLVE_CASES = [
    ("ttt", "tic_tac_toe"),
    ("hex2", "hex(board_size=2)"),
    ("hex3", "hex(board_size=3)"),
    ("hex3x4", "hex(num_rows=3,num_cols=4)"),
    ("c4_4x4", "connect_four(rows=4,columns=4)"),
    ("c4_4x4k3", "connect_four(rows=4,columns=4,x_in_row=3)"),
    ("c4_3x5k3", "connect_four(rows=3,columns=5,x_in_row=3)"),
]
# (name, game, depth_limit, include_terminals): enumeration only
ENUM_CASES = [
    ("ttt_d3", "tic_tac_toe", 3, True),
    ("ttt_noterm", "tic_tac_toe", -1, False),
    ("ttt_d5", "tic_tac_toe", 5, True),          # terminals one ply below the limit are listed, other states there not
    ("c4_8x8_d6", "connect_four(rows=8,columns=8)", 6, True),   # 72 board bits: the two-word bitboard
    ("hex6_d3", "hex(board_size=6)", 3, True),   # 36 cells: two words per plane, the 128-bit key
]


def reference_modules():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference_py)
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    sys.modules.setdefault("open_spiel.python.algorithms.lp_solver",
                           types.ModuleType("open_spiel.python.algorithms.lp_solver"))
    from open_spiel.python.algorithms import get_all_states, value_iteration
    return pyspiel, get_all_states, value_iteration


def stones(s):
    return s.count("x") + s.count("o")


def describe(out, name, game_string, states, depth_limit, include_terminals):
    keys = sorted(states)
    joined = SEP.join(keys)
    out[f"{name}/game"] = np.array(game_string)
    out[f"{name}/depth_limit"] = np.int32(depth_limit)
    out[f"{name}/include_terminals"] = np.int32(include_terminals)
    out[f"{name}/count"] = np.int64(len(keys))
    out[f"{name}/keys_sha256"] = np.array(hashlib.sha256(joined.encode()).hexdigest())
    if len(keys) <= KEEP_KEYS:
        out[f"{name}/keys"] = np.array(joined)
    levels = max(stones(k) for k in keys) + 1
    counts, terms, children = np.zeros(levels, np.int64), np.zeros(levels, np.int64), np.zeros(levels, np.int64)
    for k in keys:
        d, st = stones(k), states[k]
        counts[d] += 1
        if st.is_terminal():
            terms[d] += 1
        else:
            children[d] += len(st.legal_actions())
    out[f"{name}/level_counts"], out[f"{name}/level_terminals"], out[f"{name}/level_children"] = counts, terms, children
    return keys


def main():
    pyspiel, get_all_states, value_iteration = reference_modules()
    out = {"cases": np.array("\n".join(n for n, _ in SOLVE_CASES)),
           "enum_cases": np.array("\n".join(c[0] for c in ENUM_CASES))}
    for name, game_string in SOLVE_CASES:
        t0 = time.time()
        game = pyspiel.load_game(game_string)
        values = value_iteration.value_iteration(game, -1, 0.01, cyclic_game=True)
        states = get_all_states.get_all_states(game, -1, True, False, to_string=str, stop_if_encountered=True)
        assert set(states) == set(values)
        keys = describe(out, name, game_string, states, -1, True)
        vals = np.array([values[k] for k in keys], dtype=np.float64)
        assert np.isin(vals, (-1.0, 0.0, 1.0)).all()
        out[f"{name}/values"] = vals.astype(np.int8)
        out[f"{name}/root_value"] = np.int8(values[str(game.new_initial_state())])
        print(f"{name}: {len(keys)} states, root value {values[str(game.new_initial_state())]}, "
              f"{time.time() - t0:.1f} s", flush=True)
    for name, game_string, depth_limit, include_terminals in ENUM_CASES:
        t0 = time.time()
        game = pyspiel.load_game(game_string)
        states = get_all_states.get_all_states(game, depth_limit, include_terminals, False, to_string=str,
                                               stop_if_encountered=True)
        keys = describe(out, name, game_string, states, depth_limit, include_terminals)
        print(f"{name}: {len(keys)} states, {time.time() - t0:.1f} s", flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
