#!/usr/bin/env python3
"""Golden tables of Discounted CFR, produced by RUNNING the reference's own open_spiel/python/algorithms/discounted_cfr.py
(imported unmodified from where it lies) over the genuine games (oracle/_ref/libspiel_ref.so through
oracle/pyspiel_over_capi.py).  Run in the build container (needs /root/reference):

    python tests/golden/make_dcfr_vectors.py

Output: tests/golden/dcfr_vectors.npz (np.savez_compressed, float64):

  <game>/keys, <game>/nact, <game>/legal       infostate strings (sorted, newline-joined bytes), legal actions per row
  <game>/<set>/<T>/regrets, .../cum_policy      [I, Amax] cumulative regrets / cumulative policy after T iterations of
                                                _DCFRSolver(alternating, linear averaging, no RM+, *set), columns = the
                                                row's legal actions in ascending order; the current policy is regret
                                                matching of the regrets and is not stored
  nash_conv/<game>/<T>                          the reference's NashConv of the average policy (set D), for the record

Parameter sets: D = (3/2, 0, 2) (DCFRSolver's defaults), L = (1, 1, 1) (LCFRSolver), X = (1.5, 0.5, 3).
A checkpoint pair (t, t + 1) deep into a run serves the single-step tests: upload the tables of t, run one iteration,
compare with t + 1.  Consumers: tests/test_dcfr_goldens.py (CPU), tests/test_z13_gpu_dcfr.py (the HIP engine).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")

SETS = {"D": (3 / 2, 0, 2), "L": (1, 1, 1), "X": (1.5, 0.5, 3)}
SHORT = [1, 2, 3, 5, 10]
RUNS = [  # game, set, checkpoints of one run from the initial tables
    ("kuhn_poker", "D", SHORT + [100, 101, 1000, 1001]),
    ("kuhn_poker", "L", SHORT),
    ("kuhn_poker", "X", SHORT),
    ("kuhn_poker(players=3)", "D", SHORT + [100, 101]),
    ("kuhn_poker(players=3)", "L", SHORT),
    ("kuhn_poker(players=3)", "X", SHORT),
    ("leduc_poker", "D", SHORT + [50, 51, 100, 101]),
    ("leduc_poker", "L", [1, 5, 10]),
    ("leduc_poker", "X", [1, 5, 10]),
]
STEPS = {"kuhn_poker": [100, 1000], "kuhn_poker(players=3)": [100], "leduc_poker": [50, 100]}   # (t, t + 1) pairs, set D
NASH_CONV = {"kuhn_poker": 300, "leduc_poker": 100}   # set D
INFOSTATES = {"kuhn_poker": 12, "kuhn_poker(players=3)": 48, "leduc_poker": 936}


def reference_modules():
    """(pyspiel stand-in, discounted_cfr, exploitability, expected_game_score) of the reference tree."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference_py)
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from open_spiel.python.algorithms import discounted_cfr, expected_game_score, exploitability
    return pyspiel, discounted_cfr, exploitability, expected_game_score


def layout(solver):
    """Sorted infostate strings and each row's legal actions in ascending order."""
    keys = sorted(solver._info_state_nodes)
    legal = [sorted(solver._info_state_nodes[k].legal_actions) for k in keys]
    return keys, legal


def tables(solver, keys, legal):
    amax = max(len(l) for l in legal)
    reg, cum = np.zeros((len(keys), amax)), np.zeros((len(keys), amax))
    for i, k in enumerate(keys):
        node = solver._info_state_nodes[k]
        for a, action in enumerate(legal[i]):
            reg[i, a] = node.cumulative_regret[action]
            cum[i, a] = node.cumulative_policy[action]
    return reg, cum


def reference_run(game_string, params, checkpoints, nash_conv_at=None):
    """Runs the reference's _DCFRSolver; returns (keys, legal, {T: (regrets, cum_policy)}, NashConv at nash_conv_at or None)."""
    pyspiel, discounted_cfr, exploitability, _ = reference_modules()
    game = pyspiel.load_game(game_string)
    solver = discounted_cfr._DCFRSolver(game, True, True, False, *params)   # what DCFRSolver / LCFRSolver construct
    keys, legal = layout(solver)
    out, nc = {}, None
    for t in range(1, max(list(checkpoints) + [nash_conv_at or 0]) + 1):
        solver.evaluate_and_update_policy()
        if t in checkpoints:
            out[t] = tables(solver, keys, legal)
        if t == nash_conv_at:
            nc = exploitability.nash_conv(game, solver.average_policy(), use_cpp_br=False)
    return keys, legal, out, nc


def main():
    out = {}
    for game, name, checkpoints in RUNS:
        nc_at = NASH_CONV.get(game) if name == "D" else None
        keys, legal, tabs, nc = reference_run(game, SETS[name], checkpoints, nc_at)
        amax = max(len(l) for l in legal)
        out[f"{game}/keys"] = np.frombuffer("\n".join(keys).encode(), np.uint8)
        out[f"{game}/nact"] = np.array([len(l) for l in legal], np.int32)
        out[f"{game}/legal"] = np.array([l + [0] * (amax - len(l)) for l in legal], np.int32)
        for t, (reg, cum) in tabs.items():
            out[f"{game}/{name}/{t}/regrets"] = reg
            out[f"{game}/{name}/{t}/cum_policy"] = cum
        if nc is not None:
            out[f"nash_conv/{game}/{nc_at}"] = np.float64(nc)
        print(game, name, sorted(tabs), "" if nc is None else f"NashConv({nc_at}) = {nc:.6g}", flush=True)
    path = os.path.join(ROOT, "tests", "golden", "dcfr_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
