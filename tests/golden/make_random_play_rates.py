#!/usr/bin/env python3
"""Black's win rate under uniformly random play from the empty board of the hex boards no table can cover, estimated
with the GENUINE reference build's own playouts (oracle/_ref/libspiel_ref.so: RandomRolloutEvaluator on std::mt19937
inside MCTSBot, mcts.cc:43-72).  Run where the reference tree is present:

    python tests/golden/make_random_play_rates.py

One sample = MCTSBot(RandomRolloutEvaluator(n_rollouts=1, seed), max_simulations=2, seed).MCTSearch(empty board): the
first simulation evaluates the root, the second expands it, takes the first child of its std::shuffle'd order and plays
ONE random playout from there — a uniformly random first move followed by random play, i.e. one random playout from
the empty board.  The visited child's total_reward is that playout's return for black (+1 / -1).  Seeds 0 .. N - 1.

Output: tests/golden/random_play_rates.json — recorded results only:
  {"samples": "...", "boards": {<game string>: {"playouts": N, "black_wins": k}}}
Consumer: tests/test_z22_gpu_sampling_statistics.py (two-sample z against the device's wave-per-root search).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

BOARDS = ["hex(board_size=9)", "hex(board_size=13)", "hex(board_size=15)", "hex(board_size=19)"]
PLAYOUTS = 1 << 16


def main():
    import reference_py
    reference_py.build()
    assert reference_py.available(), "needs the genuine reference build"
    boards = {}
    for game in BOARDS:
        root = reference_py.Game(game).new_initial_state()
        wins = 0
        for seed in range(PLAYOUTS):
            children = root.mcts_search(2.0, 2, 1, 1000, False, seed)["children"]
            visited = children[children[:, 1] > 0]
            assert len(visited) == 1 and visited[0, 1] == 1 and visited[0, 2] in (-1.0, 1.0)
            wins += visited[0, 2] > 0
        boards[game] = {"playouts": PLAYOUTS, "black_wins": int(wins)}
        print(game, boards[game], flush=True)
    out = {"samples": "one random playout from the empty board per sample (reference build, std::mt19937, seeds 0 .. playouts - 1)",
           "boards": boards}
    with open(os.path.join(ROOT, "tests", "golden", "random_play_rates.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
