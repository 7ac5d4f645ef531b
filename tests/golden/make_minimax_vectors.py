#!/usr/bin/env python3
"""Golden results of alpha-beta search, produced by RUNNING the reference's own open_spiel/python/algorithms/minimax.py
(imported unmodified from where it lies) over the genuine games (oracle/_ref/libspiel_ref.so through
oracle/pyspiel_over_capi.py).  Run in the build container (needs the reference sources):

    python tests/golden/make_minimax_vectors.py

Output: tests/golden/minimax_vectors.npz (np.savez_compressed).  Per case set <set>:

  <set>/game               the game string (bytes)
  <set>/histories          [n, L] int16 action histories from the initial state, padded with -1
  <set>/depth_limit        int32; < 0 = unlimited (minimax.py counts `depth` down and never meets 0)
  <set>/leaf_mode          int32: 0 no value function, 1 `value_function=lambda s: leaf_value`
  <set>/leaf_value         float64
  <set>/maximizing_player  [n] int8 as handed to the device: -1 = the player to move at the root (the reference's None)
  <set>/value              [n] float64 (NaN where status != 0)
  <set>/best_action        [n] int32 (-1 for the reference's None)
  <set>/nodes              [n] int64: the number of _alpha_beta invocations, the root's included (0 where status != 0)
  <set>/status             [n] uint8: 0 done, 1 NotImplementedError (the depth limit reached with no value function)

Nodes are counted by rebinding the module attribute minimax._alpha_beta to a counting wrapper: the recursion resolves
the name through the module's globals, so every invocation is counted and the file is not touched.

Positions are numpy-seeded random playouts cut at a random ply, terminal positions included.  A terminal root under
maximizing_player None has no player to name (the reference indexes Returns() with kTerminalPlayer); it is run with the
player who would be to move — the parity of the history, black / x first in all three games — which is what the device
does with -1 there.  The `*_opp` sets repeat the positions of another set with maximizing_player = 1 - mover.

Consumers: tests/test_minimax_goldens.py, tests/test_alpha_beta_host.py (CPU), tests/test_z14_gpu_minimax.py (the HIP engine).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")

TTT_FIXED = [[], [4, 1], [5, 4, 3, 8]]   # minimax_test.cc: values 0, 1, -1
# name: game, positions, seed, depth_limit, leaf constant (None = no value function), minimum plies of a cut,
#       extra fixed histories, `opp` = the set whose positions are repeated with maximizing_player = 1 - mover
SETS = {
    "ttt_full": dict(game="tic_tac_toe", n=2000, seed=1, depth=-1, leaf=None, fixed=TTT_FIXED),
    "ttt_full_opp": dict(game="tic_tac_toe", opp="ttt_full", first=400, depth=-1, leaf=None),
    "ttt_d1_none": dict(game="tic_tac_toe", n=200, seed=2, depth=1, leaf=None, fixed=[[]]),
    "ttt_d2_none": dict(game="tic_tac_toe", n=200, seed=3, depth=2, leaf=None),
    "ttt_d3_none": dict(game="tic_tac_toe", n=200, seed=4, depth=3, leaf=None, fixed=[[]]),
    "ttt_d1_c0": dict(game="tic_tac_toe", n=300, seed=5, depth=1, leaf=0.0, fixed=[[]]),
    "ttt_d4_c025": dict(game="tic_tac_toe", n=300, seed=6, depth=4, leaf=0.25, fixed=[[]]),
    "c4_d6_c0": dict(game="connect_four", n=300, seed=7, depth=6, leaf=0.0, fixed=[[]]),
    "c4_d6_c0_opp": dict(game="connect_four", opp="c4_d6_c0", first=300, depth=6, leaf=0.0),
    "c4_d8_c0": dict(game="connect_four", n=200, seed=8, depth=8, leaf=0.0, fixed=[[], [3, 3, 2, 4, 2, 2, 5, 1]]),
    "c4_5x5_d10_c025": dict(game="connect_four(rows=5,columns=5)", n=100, seed=9, depth=10, leaf=0.25, fixed=[[]]),
    "c4_8x8_d5_c0": dict(game="connect_four(rows=8,columns=8)", n=200, seed=10, depth=5, leaf=0.0, fixed=[[]]),
    "hex3_full": dict(game="hex(board_size=3)", n=300, seed=11, depth=-1, leaf=None, fixed=[[]]),
    "hex3_full_opp": dict(game="hex(board_size=3)", opp="hex3_full", first=150, depth=-1, leaf=None),
    "hex4_d6_c0": dict(game="hex(board_size=4)", n=150, seed=12, depth=6, leaf=0.0, fixed=[[]]),
    "hex4_full_6plus": dict(game="hex(board_size=4)", n=80, seed=13, depth=-1, leaf=None, min_plies=6),
    "hex5_swap_d4_c0": dict(game="hex(board_size=5,swap=True)", n=120, seed=14, depth=4, leaf=0.0, fixed=[[], [7], [7, 25]]),
    "hex9_d3_c0": dict(game="hex(board_size=9)", n=60, seed=15, depth=3, leaf=0.0, fixed=[[]]),
}


def reference_modules():
    """(pyspiel stand-in, minimax) of the reference tree."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference_py)
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from open_spiel.python.algorithms import minimax
    return pyspiel, minimax


def positions(name):
    """The set's action histories (lists of ints) — the fixed ones first, then the seeded random cuts."""
    spec = SETS[name]
    if "opp" in spec:
        return positions(spec["opp"])[:spec["first"]]
    pyspiel, _ = reference_modules()
    game = pyspiel.load_game(spec["game"])
    rng = np.random.RandomState(spec["seed"])
    out = [list(h) for h in spec.get("fixed", [])]
    lo = spec.get("min_plies", 0)
    while len(out) < spec["n"] + len(spec.get("fixed", [])):
        state, history = game.new_initial_state(), []
        while not state.is_terminal():
            legal = state.legal_actions()
            action = int(legal[rng.randint(len(legal))])
            state.apply_action(action)
            history.append(action)
        if len(history) < lo:
            continue
        out.append(history[:rng.randint(lo, len(history) + 1)])
    return out


def reference_case(game, minimax, history, depth, leaf, opposite):
    """One alpha_beta_search of the reference: (maximizing_player for the device, value, best_action, nodes, status)."""
    state = game.new_initial_state()
    for a in history:
        state.apply_action(a)
    mover = len(history) % 2
    assert state.is_terminal() or state.current_player() == mover
    device_player = 1 - mover if opposite else -1
    if opposite:
        ref_player = 1 - mover
    else:
        ref_player = mover if state.is_terminal() else None
    count = [0]
    inner = minimax._alpha_beta
    assert inner.__module__ == minimax.__name__, "minimax._alpha_beta is already wrapped"

    def counting(*args, **kw):
        count[0] += 1
        return inner(*args, **kw)

    minimax._alpha_beta = counting
    try:
        value_function = None if leaf is None else (lambda s: leaf)
        try:
            value, best = minimax.alpha_beta_search(game, state=state, value_function=value_function, maximum_depth=depth,
                                                    maximizing_player_id=ref_player)
        except NotImplementedError:
            return device_player, float("nan"), -1, 0, 1
    finally:
        minimax._alpha_beta = inner
    return device_player, float(value), -1 if best is None else int(best), count[0], 0


def reference_set(name, indices=None):
    """The arrays of one set (all its positions, or those listed)."""
    spec = SETS[name]
    pyspiel, minimax = reference_modules()
    game = pyspiel.load_game(spec["game"])
    hist = positions(name)
    if indices is not None:
        hist = [hist[i] for i in indices]
    rows = [reference_case(game, minimax, h, spec["depth"], spec["leaf"], "opp" in spec) for h in hist]
    width = max(1, max(len(h) for h in hist))
    histories = np.full((len(hist), width), -1, np.int16)
    for i, h in enumerate(hist):
        histories[i, :len(h)] = h
    return {
        "game": np.frombuffer(spec["game"].encode(), np.uint8),
        "histories": histories,
        "depth_limit": np.int32(spec["depth"]),
        "leaf_mode": np.int32(0 if spec["leaf"] is None else 1),
        "leaf_value": np.float64(0.0 if spec["leaf"] is None else spec["leaf"]),
        "maximizing_player": np.array([r[0] for r in rows], np.int8),
        "value": np.array([r[1] for r in rows], np.float64),
        "best_action": np.array([r[2] for r in rows], np.int32),
        "nodes": np.array([r[3] for r in rows], np.int64),
        "status": np.array([r[4] for r in rows], np.uint8),
    }


def main():
    out = {}
    t_all = time.time()
    for name in SETS:
        t0 = time.time()
        arrays = reference_set(name)
        for k, v in arrays.items():
            out[f"{name}/{k}"] = v
        print(f"{name}: {len(arrays['status'])} positions, {int(arrays['nodes'].sum())} nodes (largest {int(arrays['nodes'].max())}), "
              f"{int((arrays['status'] != 0).sum())} with status 1, {time.time() - t0:.1f} s", flush=True)
    path = os.path.join(ROOT, "tests", "golden", "minimax_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays,", f"{time.time() - t_all:.0f} s of reference time")


if __name__ == "__main__":
    main()
