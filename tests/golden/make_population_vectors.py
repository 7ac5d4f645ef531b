#!/usr/bin/env python3
"""Golden payoff-tensor cells and aggregated policies of a population of policy tables, produced by RUNNING the
reference's own open_spiel/python/algorithms/expected_game_score.py (policy_value) and policy_aggregator.py
(PolicyAggregator) with policy.py (TabularPolicy), imported unmodified from where they lie, over the genuine games
(oracle/_ref/libspiel_ref.so through oracle/pyspiel_over_capi.py).  Run in the build container (needs the reference
tree):

    python tests/golden/make_population_vectors.py [--jobs N]

Output: tests/golden/population_vectors.npz (np.savez_compressed).  Rows of [I, Amax] arrays are the infostate strings
in sorted order, columns the row's legal actions ascending (the legal-index layout of action_value_vectors.npz), padding
cells 0.  The policy tables themselves are not stored: population_cases.table() makes them from the kind and the seed.

  seed                        the RandomState seed of the "random" table: action_value_vectors.npz's own, so that a profile
                              that names one table for every player is that file's root_values
  epsilon                     PolicyAggregator's epsilon (its default, 1e-40)
  <game>/keys_sha256, nact, player, num_players, amax     the layout, as in action_value_vectors.npz
  <game>/tables               newline-joined table kinds, in stack order (population_cases.RECORDED_KINDS)
  <game>/profiles [M, P] int32, <game>/returns [M, P]     policy_value(root, [table profiles[m, q] for player q])
  <game>/weight_kinds         newline-joined names of the recorded weight matrices (population_cases.weight_matrix)
  <game>/weights/<name> [P, K]
  <game>/aggregate/<name> [I, Amax]   PolicyAggregator(game).aggregate(range(P), [the K tables] * P, weights): player p's
                              dictionary at p's rows
  the large game (leduc_poker(players=3)) records, to stay a small file,
  <game>/aggregate/<name>_rows, _colsum   rows 0, 16, 32, ... of the table and the sum over all rows

The work is cut into one reference walk per job (a profile; a player of a weight matrix) and spread over forked worker
processes.  Measured with 7 workers on 8 cores: 102 s of wall time in all.  leduc_poker(players=3): the layout 33 s, a
policy_value walk 30 to 32 s (3 s where the profile holds the table of exact zeros, whose branches the reference skips),
an aggregation walk (one player) 64 to 66 s; every job of the four small games under 2 s.

Consumers: tests/test_population_goldens.py, tests/test_population_native.py (CPU), tests/test_z24_gpu_population.py
(the HIP engine).
"""
import argparse
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import action_value_cases as avc  # noqa: E402
import make_action_value_vectors as mav  # noqa: E402
import population_cases as pc  # noqa: E402

GAMES = {}   # game string -> what the jobs need (made before the workers fork)


def prepare(game_string, seed, av):
    pyspiel, policy = MODULES[0], MODULES[1]
    t0 = time.time()
    game = pyspiel.load_game(game_string)
    P = game.num_players()
    base = policy.TabularPolicy(game)
    keys = sorted(base.state_lookup)
    legal = [[a for a, on in enumerate(base.legal_actions_mask[base.state_lookup[k]]) if on] for k in keys]
    nact = np.array([len(l) for l in legal], np.int32)
    amax = int(nact.max())
    assert np.array_equal(nact, av[f"{game_string}/nact"])
    kinds = pc.RECORDED_KINDS[game_string]
    stack = pc.table_stack(kinds, nact, amax, seed)
    policies = [mav.tabular(policy, game, base, keys, legal, t) for t in stack]
    GAMES[game_string] = dict(game=game, P=P, keys=keys, legal=legal, nact=nact, amax=amax, kinds=kinds, policies=policies,
                              profiles=pc.recorded_profiles(game_string, P),
                              weights={n: pc.weight_matrix(n, P, len(kinds)) for n in pc.RECORDED_WEIGHTS[game_string]})
    print(f"{game_string}: {len(keys)} infostates, {len(kinds)} tables, layout in {time.time() - t0:.1f} s", flush=True)


def run(job):
    expected_game_score, policy_aggregator = MODULES[2], MODULES[3]
    t0 = time.time()
    what, game_string = job[0], job[1]
    g = GAMES[game_string]
    if what == "returns":
        profile = g["profiles"][job[2]]
        res = np.array(expected_game_score.policy_value(g["game"].new_initial_state(), [g["policies"][k] for k in profile]), np.float64)
    else:
        name, pid = job[2], job[3]
        weights = [[float(x) for x in row] for row in g["weights"][name]]
        aggregator = policy_aggregator.PolicyAggregator(g["game"], epsilon=pc.EPSILON)
        rows = aggregator.aggregate([pid], [list(g["policies"]) for _ in range(g["P"])], weights).policy[0]
        res = np.zeros((len(g["keys"]), g["amax"]))
        for i, k in enumerate(g["keys"]):
            if k in rows:
                res[i, :g["nact"][i]] = [rows[k][a] for a in g["legal"][i]]
    print(f"{job}: {time.time() - t0:.1f} s", flush=True)
    return job, res


def reference_modules():
    pyspiel, policy = mav.reference_modules()[:2]
    from open_spiel.python.algorithms import expected_game_score, policy_aggregator
    return pyspiel, policy, expected_game_score, policy_aggregator


MODULES = None


def main(path=None, games=None, jobs=8):
    global MODULES
    MODULES = reference_modules()
    av = avc.load()
    seed = int(av["seed"])
    games = list(games or pc.GAMES)
    t0 = time.time()
    for g in games:
        prepare(g, seed, av)
    work = []
    for g in reversed(games):   # the long walks first
        work += [("aggregate", g, n, p) for n in GAMES[g]["weights"] for p in range(GAMES[g]["P"])]
        work += [("returns", g, m) for m in range(len(GAMES[g]["profiles"]))]
    with multiprocessing.get_context("fork").Pool(jobs) as pool:
        results = dict(pool.imap_unordered(run, work))
    out = {"seed": np.int32(seed), "epsilon": np.float64(pc.EPSILON)}
    for g in games:
        d = GAMES[g]
        for name in ("keys_sha256", "nact", "player", "num_players"):
            out[f"{g}/{name}"] = av[f"{g}/{name}"]
        out[f"{g}/amax"] = np.int32(d["amax"])
        out[f"{g}/tables"] = np.frombuffer("\n".join(d["kinds"]).encode(), np.uint8)
        out[f"{g}/profiles"] = d["profiles"]
        out[f"{g}/returns"] = np.stack([results[("returns", g, m)] for m in range(len(d["profiles"]))])
        out[f"{g}/weight_kinds"] = np.frombuffer("\n".join(d["weights"]).encode(), np.uint8)
        player = av[f"{g}/player"]
        for n, w in d["weights"].items():
            out[f"{g}/weights/{n}"] = w
            table = np.zeros((len(d["keys"]), d["amax"]))
            for p in range(d["P"]):
                table[player == p] = results[("aggregate", g, n, p)][player == p]
            if g == pc.LARGE_GAME:
                out[f"{g}/aggregate/{n}_rows"] = table[::pc.ROW_STRIDE]
                out[f"{g}/aggregate/{n}_colsum"] = table.sum(axis=0)
            else:
                out[f"{g}/aggregate/{n}"] = table
    path = path or os.path.join(ROOT, "tests", "golden", "population_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays,", f"{time.time() - t0:.0f} s", flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--games", nargs="*")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    main(a.out, a.games, a.jobs)
