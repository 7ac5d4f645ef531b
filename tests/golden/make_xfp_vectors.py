#!/usr/bin/env python3
"""Golden trajectories of extensive-form fictitious play, produced by RUNNING the reference's own
open_spiel/python/algorithms/fictitious_play.py (XFPSolver, imported unmodified from where it lies) over the genuine
games (oracle/_ref/libspiel_ref.so through oracle/pyspiel_over_capi.py).  Run in the build container (needs the
reference tree):

    python tests/golden/make_xfp_vectors.py

Output: tests/golden/xfp_vectors.npz (np.savez_compressed).  T = the iterations recorded for the game, row t - 1 holds
iteration t; rows of [I] arrays are the infostate strings in sorted order, columns the row's legal actions ascending:

  <game>/keys, <game>/nact, <game>/legal   infostate strings (sorted, newline-joined bytes), legal actions per row
  <game>/player                            [I] the acting player
  <game>/pred_info, <game>/pred_action     [I] the row of the same player's previous infostate on the way from the root
                                           and the index (among that row's legal actions) of the action taken there;
                                           -1 at a player's first infostate
  <game>/br                                [T, I] int32: iteration t's best response, as an index among the legal actions
                                           (exploitability.best_response(...)["best_response_action"])
  <game>/cf_nonzero                        [T, I] bool: the infostate has a history with non-zero counterfactual reach
  <game>/avg_reach, <game>/br_reach        [T, I] the two own-player reach products update_average_policies uses at the
                                           infostate in iteration t (formed here by the reference's statements: a copy
                                           of the vector, `*=` per action, root to leaf, first visit of the infostate)
  <game>/policy                            [T, I, Amax] XFPSolver.average_policy_tables() after iteration t
  <game>/min_gap, <game>/ties              [T] over the infostates with non-zero counterfactual reach: the smallest
                                           POSITIVE difference between the best and the second-best
                                           counterfactual-weighted action value (inf if there is none), and how many
                                           infostates have the two exactly equal
  nash_conv/<game>/<t>                     exploitability.nash_conv of the average policy after t iterations

Consumers: tests/test_xfp_goldens.py, tests/test_xfp_native.py (CPU), tests/test_z14_gpu_xfp.py (the HIP engine).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")

RUNS = [  # game, iterations, NashConv checkpoints
    ("kuhn_poker", 120, [1, 30, 120]),
    ("kuhn_poker(players=3)", 40, [1, 40]),
    ("leduc_poker", 25, [10, 20, 25]),
]


def reference_modules():
    """(pyspiel stand-in, fictitious_play, exploitability, best_response) of the reference tree."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference_py)
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from open_spiel.python.algorithms import best_response, exploitability, fictitious_play
    return pyspiel, fictitious_play, exploitability, best_response


def layout(game):
    """One walk of the game: sorted keys, legal actions, acting player and own-player predecessor of every infostate."""
    info = {}   # key -> (player, legal, predecessor key or None, action taken there)

    def walk(state, last):
        if state.is_terminal():
            return
        if state.is_chance_node():
            for action, _ in state.chance_outcomes():
                walk(state.child(action), last)
            return
        player = state.current_player()
        key = state.information_state_string(player)
        legal = sorted(state.legal_actions())
        if key not in info:
            info[key] = (player, legal, last[player][0], last[player][1])
        for action in legal:
            nxt = list(last)
            nxt[player] = (key, action)
            walk(state.child(action), nxt)

    walk(game.new_initial_state(), [(None, -1)] * game.num_players())
    keys = sorted(info)
    row = {k: i for i, k in enumerate(keys)}
    legal = [info[k][1] for k in keys]
    player = np.array([info[k][0] for k in keys], np.int32)
    pred_info = np.array([-1 if info[k][2] is None else row[info[k][2]] for k in keys], np.int32)
    pred_action = np.array([-1 if info[k][2] is None else info[info[k][2]][1].index(info[k][3]) for k in keys], np.int32)
    return keys, row, legal, player, pred_info, pred_action


def reaches(fictitious_play, solver, game, row):
    """avg_reach / br_reach at the first visit of every infostate, by the statements of
    _recursively_update_average_policies (fictitious_play.py:196-225) on the solver's policies as they are."""
    avg_out, br_out = np.full(len(row), np.nan), np.full(len(row), np.nan)
    seen = set()

    def walk(state, avg_reach_probs, br_reach_probs):
        if state.is_terminal():
            return
        if state.is_chance_node():
            for action, _ in state.chance_outcomes():
                walk(state.child(action), avg_reach_probs, br_reach_probs)
            return
        player = state.current_player()
        avg_policy = fictitious_play._policy_dict_at_state(solver._policies[player], state)
        br_policy = fictitious_play._policy_dict_at_state(solver._best_responses[player], state)
        key = state.information_state_string(player)
        for action in state.legal_actions():
            new_avg_reach = np.copy(avg_reach_probs)
            new_avg_reach[player] *= avg_policy[action]
            new_br_reach = np.copy(br_reach_probs)
            new_br_reach[player] *= br_policy[action]
            walk(state.child(action), new_avg_reach, new_br_reach)
        if key not in seen:
            seen.add(key)
            avg_out[row[key]] = avg_reach_probs[player]
            br_out[row[key]] = br_reach_probs[player]

    walk(game.new_initial_state(), np.ones(game.num_players()), np.ones(game.num_players()))
    assert len(seen) == len(row)
    return avg_out, br_out


def reference_run(game_string, iterations, nash_conv_at, action_values=False):
    """action_values=True adds <game>/q [T, I, Amax]: the counterfactual-weighted action values the best response
    maximised over (NaN at an infostate without counterfactual reach); tests/golden/make_solver_variant_vectors.py."""
    pyspiel, fictitious_play, exploitability, best_response = reference_modules()
    game = pyspiel.load_game(game_string)
    keys, row, legal, player, pred_info, pred_action = layout(game)
    I, amax = len(keys), max(len(l) for l in legal)

    # the best-response objects exploitability.best_response builds inside compute_best_responses: kept, so that their
    # (memoised) action values can be read afterwards
    made = []
    genuine = best_response.BestResponsePolicy

    class Recorded(genuine):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    best_response.BestResponsePolicy = Recorded
    try:
        solver = fictitious_play.XFPSolver(game)
        captured = {}
        update = solver.update_average_policies

        def recording_update():   # between compute_best_responses and the update: the reaches the update will use
            captured["reach"] = reaches(fictitious_play, solver, game, row)
            update()

        solver.update_average_policies = recording_update
        out = dict(br=np.zeros((iterations, I), np.int32), cf_nonzero=np.zeros((iterations, I), bool),
                   avg_reach=np.zeros((iterations, I)), br_reach=np.zeros((iterations, I)),
                   policy=np.zeros((iterations, I, amax)), min_gap=np.full(iterations, np.inf),
                   ties=np.zeros(iterations, np.int32))
        if action_values:
            out["q"] = np.full((iterations, I, amax), np.nan)
        nash = {}
        for t in range(1, iterations + 1):
            del made[:]
            solver.iteration()
            assert len(made) == game.num_players()
            for br in made:
                for key, infoset in br.infosets.items():
                    i = row[key]
                    out["br"][t - 1, i] = legal[i].index(br.best_response_action(key))
                    if not any(cf_p != 0 for _, cf_p in infoset):
                        continue
                    out["cf_nonzero"][t - 1, i] = True
                    values = [sum(cf_p * br.q_value(s, a) for s, cf_p in infoset) for a in legal[i]]
                    if action_values:
                        out["q"][t - 1, i, :len(values)] = values
                    values = sorted(values, reverse=True)
                    if len(values) < 2:
                        continue
                    gap = values[0] - values[1]
                    if gap == 0:
                        out["ties"][t - 1] += 1
                    else:
                        out["min_gap"][t - 1] = min(out["min_gap"][t - 1], gap)
            out["avg_reach"][t - 1], out["br_reach"][t - 1] = captured["reach"]
            tables = solver.average_policy_tables()
            for i, k in enumerate(keys):
                for a, action in enumerate(legal[i]):
                    out["policy"][t - 1, i, a] = tables[player[i]][k][action]
            if t in nash_conv_at:
                nash[t] = exploitability.nash_conv(game, solver.average_policy(), use_cpp_br=False)
            print(f"{game_string} t={t} ties={out['ties'][t - 1]} min_gap={out['min_gap'][t - 1]:.3g}"
                  + (f" NashConv={nash[t]:.6g}" if t in nash else ""), flush=True)
    finally:
        best_response.BestResponsePolicy = genuine
    out.update(keys=np.frombuffer("\n".join(keys).encode(), np.uint8), nact=np.array([len(l) for l in legal], np.int32),
               legal=np.array([l + [0] * (amax - len(l)) for l in legal], np.int32), player=player,
               pred_info=pred_info, pred_action=pred_action)
    return out, nash


def main():
    out = {}
    for game, iterations, nash_conv_at in RUNS:
        arrays, nash = reference_run(game, iterations, nash_conv_at)
        for name, value in arrays.items():
            out[f"{game}/{name}"] = value
        for t, nc in nash.items():
            out[f"nash_conv/{game}/{t}"] = np.float64(nc)
    path = os.path.join(ROOT, "tests", "golden", "xfp_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
