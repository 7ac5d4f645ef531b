#!/usr/bin/env python3
"""Golden trajectories of magnetic mirror descent, produced by RUNNING the reference's own
open_spiel/python/algorithms/mmd_dilated.py (MMDDilatedEnt, imported unmodified from where it lies) over the genuine
games (oracle/_ref/libspiel_ref.so through oracle/pyspiel_over_capi.py).  Run in the build container (needs the
reference tree and scipy):

    python tests/golden/make_mmd_vectors.py

Output: tests/golden/mmd_vectors.npz (np.savez_compressed).  Rows of [I] arrays are the infostate strings in sorted
order, columns the row's legal actions ascending; a sequence (I, a) is the cell I * Amax + a, the empty sequence -1.

  <game>/keys, nact, legal, player, pred_info, pred_action    the layout, as in xfp_vectors.npz
  <game>/term_seq   [Z, 2] int32   every terminal history, level by level and a level by its action sequences
                                   (breadth-first order): the last sequence (cell) of player 0 and of player 1 on the
                                   way to it
  <game>/term_cu    [Z, 2]         chance(z) * u_p(z), formed as sequence_form_utils.py:152 forms it.  Player p's
                                   terminal list is (term_seq[:, p], term_seq[:, 1 - p], term_cu[:, p]).
  <game>/bfs_rank   [I] int32      the infostate's rank when infostates are numbered breadth-first by first visit
                                   (the order in which a cell's child infostates are added up)
  <game>/seq_map<p> [S_p, 2] int32 the reference's sequence id of player p -> (infostate row, action index); id 0
                                   (the empty sequence) -> (-1, -1)
  <game>/default_stepsize/<alpha>  MMDDilatedEnt(game, alpha).stepsize
  runs                             newline-joined run names; per run R (a list of segments, recorded after each):
  <R>/game                         the game string (bytes)
  <R>/iters, <R>/alpha, <R>/stepsize   [C] the segment's update_sequences() calls and the parameters they ran with
  <R>/t                            [C] update_sequences() calls so far
  <R>/x, <R>/avg_x, <R>/pi         [C, I, Amax] current and average sequences, get_policies()
  <R>/gap                          [C] get_gap() (nan where alpha = 0)
  <R>/nash_conv                    [C] exploitability.nash_conv of get_policies()
  <R>/min_seq                      [C] the smallest sequence value any iteration so far has held
  qre/x, qre/pi                    the kuhn_poker QRE at 1 / alpha = 10 of the reference's mmd_dilated_test.py
  qre/seq0, qre/seq1               ... as its two 13-vectors
  qre/x_after, qre/pi_after, qre/avg_x_after, qre/gap, qre/alpha, qre/stepsize
                                   one reference update from it (avg_x = x before), and the reference's gap AT it

Consumers: tests/test_mmd_goldens.py, tests/test_mmd_native.py (CPU), tests/test_z17_gpu_mmd.py (the HIP engine).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")

# name, game, segments (iterations, alpha, stepsize or None = the reference's default for that alpha)
RUNS = [
    ("kuhn_a0.1", "kuhn_poker", [(1, 0.1, None), (1, 0.1, None), (8, 0.1, None), (90, 0.1, None), (300, 0.1, None)]),
    ("kuhn_a0", "kuhn_poker", [(1, 0.0, 1.0), (9, 0.0, 1.0), (90, 0.0, 1.0)]),
    ("kuhn_a1", "kuhn_poker", [(100, 1.0, None)]),
    ("kuhn_anneal", "kuhn_poker", [(20, 0.5, None), (20, 0.1, None), (20, 0.02, 0.5)]),
    ("leduc_a0.05", "leduc_poker", [(1, 0.05, None), (9, 0.05, None), (20, 0.05, None)]),
    ("leduc_a0", "leduc_poker", [(20, 0.0, 2.0)]),
]

QRE = [  # mmd_dilated_test.py:32-41 (gambit's QRE of kuhn_poker at 1 / alpha = 10)
    np.array([1., 0.75364232, 0.64695966, 0.10668266, 0.24635768, 0.70309809, 0.25609184, 0.44700625, 0.29690191,
              0.47546799, 0.01290797, 0.46256001, 0.52453201]),
    np.array([1., 0.63415944, 0.36584056, 0.41154828, 0.58845172, 0.28438486, 0.71561514, 0.0620185, 0.9379815,
              0.65005434, 0.34994566, 0.79722767, 0.20277233]),
]


def reference_modules():
    """(pyspiel stand-in, mmd_dilated, exploitability) of the reference tree."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference_py)
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from open_spiel.python.algorithms import exploitability, mmd_dilated
    return pyspiel, mmd_dilated, exploitability


def layout(game):
    """One walk of the game: the infostate layout of make_xfp_vectors.py, and every terminal's last sequences."""
    info = {}   # key -> (player, legal, predecessor key or None, action taken there)
    terms = []  # ((key, action) or None per player, chance reach * returns, action sequence)
    first = {}  # key -> (depth, action sequence) of its first history in breadth-first order

    def walk(state, last, chance_reach, path):
        if state.is_terminal():
            terms.append((list(last), np.asarray(state.returns()) * chance_reach, path))
            return
        if state.is_chance_node():
            for action, prob in state.chance_outcomes():
                walk(state.child(action), last, prob * chance_reach, path + (action,))
            return
        player = state.current_player()
        key = state.information_state_string(player)
        legal = sorted(state.legal_actions())
        if key not in info:
            info[key] = (player, legal, last[player][0], last[player][1])
        first[key] = min(first.get(key, (len(path), path)), (len(path), path))
        for action in state.legal_actions(player):
            nxt = list(last)
            nxt[player] = (key, action)
            walk(state.child(action), nxt, chance_reach, path + (action,))

    walk(game.new_initial_state(), [(None, -1)] * game.num_players(), 1.0, ())
    terms.sort(key=lambda t: (len(t[2]), t[2]))   # level by level, a level by its action sequences (breadth-first order)
    keys = sorted(info)
    row = {k: i for i, k in enumerate(keys)}
    legal = [info[k][1] for k in keys]
    amax = max(len(l) for l in legal)
    player = np.array([info[k][0] for k in keys], np.int32)
    pred_info = np.array([-1 if info[k][2] is None else row[info[k][2]] for k in keys], np.int32)
    pred_action = np.array([-1 if info[k][2] is None else info[info[k][2]][1].index(info[k][3]) for k in keys], np.int32)

    def cell(seq):
        return -1 if seq[0] is None else row[seq[0]] * amax + legal[row[seq[0]]].index(seq[1])

    term_seq = np.array([[cell(last[0]), cell(last[1])] for last, _, _ in terms], np.int32)
    term_cu = np.array([cu for _, cu, _ in terms], np.float64)
    bfs_rank = np.zeros(len(keys), np.int32)
    for rank, k in enumerate(sorted(keys, key=lambda k: first[k])):
        bfs_rank[row[k]] = rank
    return keys, row, legal, amax, player, pred_info, pred_action, term_seq, term_cu, bfs_rank


def seq_map(mmd, player, row, legal):
    out = np.full((len(mmd.infoset_actions_to_seq[player]), 2), -1, np.int32)
    for isa_key, sid in mmd.infoset_actions_to_seq[player].items():
        if sid == 0:
            continue
        key, action = isa_key.split(" -=- ")
        out[sid] = (row[key], legal[row[key]].index(int(action)))
    return out


def to_table(seqs, maps, I, amax):
    out = np.zeros((I, amax))
    for p in range(2):
        for sid in range(1, len(seqs[p])):
            out[maps[p][sid, 0], maps[p][sid, 1]] = seqs[p][sid]
    return out


def policy_table(tabular, keys, legal, amax):
    out = np.zeros((len(keys), amax))
    for i, k in enumerate(keys):
        probs = tabular.policy_for_key(k)
        for a, action in enumerate(legal[i]):
            out[i, a] = probs[action]
    return out


def game_layout(pyspiel, mmd_dilated, game_string, cache={}):
    if game_string not in cache:
        game = pyspiel.load_game(game_string)
        lay = layout(game)
        probe = mmd_dilated.MMDDilatedEnt(game, 0.5)
        maps = [seq_map(probe, p, lay[1], lay[2]) for p in range(2)]
        cache[game_string] = (game, lay, maps)
    return cache[game_string]


def reference_run(mods, game_string, segments):
    pyspiel, mmd_dilated, exploitability = mods
    game, (keys, row, legal, amax, *_), maps = game_layout(pyspiel, mmd_dilated, game_string)
    I = len(keys)
    first_alpha, first_eta = segments[0][1], segments[0][2]
    mmd = mmd_dilated.MMDDilatedEnt(game, first_alpha, first_eta)
    out = {k: [] for k in ("iters", "alpha", "stepsize", "t", "x", "avg_x", "pi", "gap", "nash_conv", "min_seq")}
    t, min_seq = 0, min(s.min() for s in mmd.sequences)
    for iters, alpha, eta in segments:
        mmd.alpha = float(alpha)   # (the annealing run changes the attributes between calls)
        mmd.stepsize = eta if eta is not None else mmd_dilated.MMDDilatedEnt(game, alpha).stepsize
        for _ in range(iters):
            mmd.update_sequences()
            min_seq = min(min_seq, min(s.min() for s in mmd.sequences))
        t += iters
        pol = mmd.get_policies()
        out["iters"].append(iters); out["alpha"].append(alpha); out["stepsize"].append(mmd.stepsize); out["t"].append(t)
        out["x"].append(to_table(mmd.current_sequences(), maps, I, amax))
        out["avg_x"].append(to_table(mmd.get_avg_sequences(), maps, I, amax))
        out["pi"].append(policy_table(pol, keys, legal, amax))
        out["gap"].append(mmd.get_gap() if alpha > 0 else np.nan)
        out["nash_conv"].append(exploitability.nash_conv(game, pol, use_cpp_br=False))
        out["min_seq"].append(min_seq)
        print(f"{game_string} alpha={alpha} eta={mmd.stepsize} t={t} gap={out['gap'][-1]:.6g} "
              f"NashConv={out['nash_conv'][-1]:.6g} min_seq={min_seq:.3g}", flush=True)
    res = {k: np.array(v, np.int32 if k in ("iters", "t") else np.float64) for k, v in out.items()}
    res["game"] = np.frombuffer(game_string.encode(), np.uint8)
    return res


def qre_vectors(mods):
    pyspiel, mmd_dilated, _ = mods
    game, (keys, row, legal, amax, *_), maps = game_layout(pyspiel, mmd_dilated, "kuhn_poker")
    I = len(keys)
    mmd = mmd_dilated.MMDDilatedEnt(game, 1.0 / 10)
    mmd.sequences = [q.copy() for q in QRE]
    mmd.avg_sequences = [q.copy() for q in QRE]
    out = {"seq0": QRE[0], "seq1": QRE[1], "alpha": np.float64(mmd.alpha), "stepsize": np.float64(mmd.stepsize),
           "x": to_table(mmd.sequences, maps, I, amax), "pi": policy_table(mmd.get_policies(), keys, legal, amax),
           "gap": np.float64(mmd.get_gap())}
    mmd.update_sequences()
    out.update(x_after=to_table(mmd.sequences, maps, I, amax), avg_x_after=to_table(mmd.avg_sequences, maps, I, amax),
               pi_after=policy_table(mmd.get_policies(), keys, legal, amax))
    return out


def main(only=None, path=None, runs=None):
    """runs: another list in the form of RUNS (tests/golden/make_solver_variant_vectors.py); then `only` is taken as given."""
    mods = reference_modules()
    pyspiel, mmd_dilated, _ = mods
    out = {}
    if runs is not None:
        only = {r[0] for r in runs}
    runs = [r for r in (RUNS if runs is None else runs) if only is None or r[0] in only]
    for game_string in sorted({r[1] for r in runs}):
        game, (keys, row, legal, amax, player, pred_info, pred_action, term_seq, term_cu, bfs_rank), maps = \
            game_layout(pyspiel, mmd_dilated, game_string)
        g = game_string
        out[f"{g}/keys"] = np.frombuffer("\n".join(keys).encode(), np.uint8)
        out[f"{g}/nact"] = np.array([len(l) for l in legal], np.int32)
        out[f"{g}/legal"] = np.array([l + [0] * (amax - len(l)) for l in legal], np.int32)
        out[f"{g}/player"], out[f"{g}/pred_info"], out[f"{g}/pred_action"] = player, pred_info, pred_action
        out[f"{g}/term_seq"], out[f"{g}/term_cu"], out[f"{g}/bfs_rank"] = term_seq, term_cu, bfs_rank
        out[f"{g}/seq_map0"], out[f"{g}/seq_map1"] = maps
        for alpha in sorted({seg[1] for r in runs if r[1] == g for seg in r[2] if seg[2] is None}):
            out[f"{g}/default_stepsize/{alpha}"] = np.float64(mmd_dilated.MMDDilatedEnt(game, alpha).stepsize)
    for name, game_string, segments in runs:
        for k, v in reference_run(mods, game_string, segments).items():
            out[f"{name}/{k}"] = v
    out["runs"] = np.frombuffer("\n".join(r[0] for r in runs).encode(), np.uint8)
    if only is None:
        for k, v in qre_vectors(mods).items():
            out[f"qre/{k}"] = v
        path = path or os.path.join(ROOT, "tests", "golden", "mmd_vectors.npz")
    if path:
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    return out


if __name__ == "__main__":
    main()
