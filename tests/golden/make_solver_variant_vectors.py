#!/usr/bin/env python3
"""Golden runs of the tabular solvers on the accepted poker VARIANTS, produced by the recording functions of the
families' own makers (make_xfp_vectors.py, make_mmd_vectors.py, make_dcfr_vectors.py, make_efr_vectors.py: imported, not copied), i.e. by
RUNNING the reference's own Python over the genuine games (oracle/_ref/libspiel_ref.so through
oracle/pyspiel_over_capi.py).  Needs the reference tree (MMD and EFR need scipy):

    python tests/golden/make_solver_variant_vectors.py [layout] [dcfr] [xfp] [mmd] [efr] [action_value]      (no argument: all of them)

Games (GAMES below): G1 suit-isomorphic leduc, G2 leduc with action mapping, G3 leduc with player 1 to start, G4 all
three at once, G5 kuhn_poker(players=4).

Output, one file per family, each in the layout of the family's existing file (see the maker's docstring):

  tests/golden/variant_layout_vectors.npz   what the coverage assertions of tests/test_solver_variants_cpu.py read:
      <game>/histories       the number of nodes of the game tree (chance, decision and terminal)
      <game>/level_player    [D] the acting player of every history at depth d (-1 chance, -4 terminal only, -9 mixed)
      <game>/chance_rows     [R, K] the distinct chance distributions of the game (padded with 0), in order of first visit
      <game>/deals           [N, P] the private-card chance outcomes of every deal, <game>/deal_prob [N] its probability
      <game>/term_chance     [Z] the chance reach of every terminal history, level by level and a level by its action
                             sequences: the order of mmd_vectors.npz's term_seq / term_cu
      <game>/multi_pred      how many information states are reached by more than one (own infostate, own action): the
                             game as laid out has no perfect recall there, and the sequence form is not defined
  tests/golden/variant_dcfr_vectors.npz     sets D and L at 1, 2 and 10 iterations, G1-G5
  tests/golden/variant_xfp_vectors.npz      iterations 1..10 (every iteration: the device is fed the recorded best
                                            response where the iteration is not decisive), NashConv at 1, 2, 5, 10, G1-G5;
                                            and <game>/q [T, I, Amax], the counterfactual-weighted action values every
                                            best response maximised over (the optimality check of the device's choice)
  tests/golden/variant_mmd_vectors.npz      alpha 0.05 (default stepsize) and alpha 0 (stepsize 2) at 1, 10, 20, on G1 and
                                            G3.  Not G2 and G4: with action_mapping=True "fold" where there is nothing to
                                            call is "call", both lead to the same information state (multi_pred = 336 of
                                            936), mmd_dilated.py's sequences drop to 0 within ten iterations and its
                                            log(0) turns the run into NaN; MMDSolver refuses these strings.
  tests/golden/variant_efr_vectors.npz      `blind cf`, `informed cf`, `tips` (and `bhv` on G1) at 1, 2, 5 on G1, G3 and G5.
                                            Not G2 and G4: the regrets of "fold" against "call" where the two are one move
                                            are rounding noise (|R| ~ 1e-17) instead of 0 in efr.py's own run, no
                                            iteration passes make_efr_vectors.py's rule (smallest nonzero |R| >= 1e-9: no
                                            max(0, R) may turn on a rounding difference); EFRSolver refuses these strings.
                                            On G5 the checkpoints are 1, 3, 5: iteration 2 fails that rule and the maker
                                            moves the checkpoint on.
  tests/golden/variant_action_value_vectors.npz   the family's own cases (the uniform table, a random table, the table of
                                            exact zeros that plays only first actions; for the two-player games the
                                            vs-best-response form for each player) on G1-G5, with the flattened trees the
                                            host program reads.  With action mapping the first-action table's best
                                            responses tie exactly (ties > 0); the lower action is the recorded choice.

The existing *_vectors.npz are not touched (make_xfp_vectors.py's reference_run gained an optional argument; regenerated,
xfp_vectors.npz, dcfr_vectors.npz and mmd_vectors.npz come out byte for byte as committed).  Wall time, one
core each: layout 1 s, dcfr 21 s, xfp 63 s, mmd 17 s, efr 51 s, action_value 9 s.  Populations and ISMCTS are not
recorded on the variants: those entry points refuse the leduc parameters.  Consumers: tests/test_solver_variants_cpu.py, tests/test_z30_gpu_solver_variants.py.
"""
import importlib.util
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

GAMES = {
    "G1": "leduc_poker(suit_isomorphism=True)",
    "G2": "leduc_poker(action_mapping=True)",
    "G3": "leduc_poker(starting_player=1)",
    "G4": "leduc_poker(action_mapping=True,suit_isomorphism=True,starting_player=1)",
    "G5": "kuhn_poker(players=4)",
}
PERFECT_RECALL_TWO_PLAYER = ["G1", "G3"]
NO_ACTION_MAPPING = ["G1", "G3", "G5"]
DCFR_CHECKPOINTS = [1, 2, 10]
XFP_ITERATIONS, XFP_NASH_CONV = 10, [1, 2, 5, 10]
EFR_SETS, EFR_CHECKPOINTS = ["blind cf", "informed cf", "tips"], [1, 2, 5]
MMD_SEGMENTS = {"a0.05": [(1, 0.05, None), (9, 0.05, None), (10, 0.05, None)],
                "a0": [(1, 0.0, 2.0), (9, 0.0, 2.0), (10, 0.0, 2.0)]}


def maker(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save(family, out):
    path = os.path.join(HERE, f"variant_{family}_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays", flush=True)


def game_layout(game):
    """The coverage facts of one game, by one walk."""
    players = game.num_players()
    count = [0]
    levels, rows, deals, preds, terms = {}, [], [], {}, []

    def walk(state, depth, dealt, prob, last=None, path=()):
        last = last or [None] * players
        count[0] += 1
        if state.is_terminal():
            levels.setdefault(depth, set()).add(-4)
            terms.append((len(path), path, prob))
            return
        if state.is_chance_node():
            levels.setdefault(depth, set()).add(-1)
            outcomes = state.chance_outcomes()
            row = tuple(p for _, p in outcomes)
            if row not in rows:
                rows.append(row)
            for action, p in outcomes:
                now = dealt + (action,) if len(dealt) < players else dealt
                if len(dealt) < players and len(now) == players:
                    deals.append((now, prob * p))
                walk(state.child(action), depth + 1, now, p * prob, last, path + (action,))
            return
        player = state.current_player()
        levels.setdefault(depth, set()).add(player)
        key = state.information_state_string(player)
        preds.setdefault(key, set()).add(last[player])
        for action in state.legal_actions():
            nxt = list(last)
            nxt[player] = (key, action)
            walk(state.child(action), depth + 1, dealt, prob, nxt, path + (action,))

    walk(game.new_initial_state(), 0, (), 1.0)

    def owner(who):
        who = who - {-4} if len(who) > 1 else who
        return who.pop() if len(who) == 1 else -9

    width = max(len(r) for r in rows)
    terms.sort()
    return dict(histories=np.int64(count[0]), multi_pred=np.int32(sum(1 for v in preds.values() if len(v) > 1)),
                level_player=np.array([owner(set(levels[d])) for d in sorted(levels)], np.int32),
                chance_rows=np.array([list(r) + [0.0] * (width - len(r)) for r in rows], np.float64),
                term_chance=np.array([t[2] for t in terms], np.float64),
                deals=np.array([d for d, _ in deals], np.int32), deal_prob=np.array([p for _, p in deals], np.float64))


def record_layout():
    pyspiel = maker("make_xfp_vectors").reference_modules()[0]
    out = {}
    for game in GAMES.values():
        for name, value in game_layout(pyspiel.load_game(game)).items():
            out[f"{game}/{name}"] = value
        print(game, int(out[f"{game}/histories"]), "histories; levels", out[f"{game}/level_player"].tolist(), flush=True)
    save("layout", out)


def record_dcfr():
    gen = maker("make_dcfr_vectors")
    out = {}
    for game in GAMES.values():
        for name in ("D", "L"):
            keys, legal, tabs, _ = gen.reference_run(game, gen.SETS[name], DCFR_CHECKPOINTS)
            amax = max(len(l) for l in legal)
            out[f"{game}/keys"] = np.frombuffer("\n".join(keys).encode(), np.uint8)
            out[f"{game}/nact"] = np.array([len(l) for l in legal], np.int32)
            out[f"{game}/legal"] = np.array([l + [0] * (amax - len(l)) for l in legal], np.int32)
            for t, (reg, cum) in tabs.items():
                out[f"{game}/{name}/{t}/regrets"] = reg
                out[f"{game}/{name}/{t}/cum_policy"] = cum
            print(game, name, sorted(tabs), flush=True)
    save("dcfr", out)


def record_xfp():
    gen = maker("make_xfp_vectors")
    out = {}
    for game in GAMES.values():
        arrays, nash = gen.reference_run(game, XFP_ITERATIONS, XFP_NASH_CONV, action_values=True)
        for name, value in arrays.items():
            out[f"{game}/{name}"] = value
        for t, nc in nash.items():
            out[f"nash_conv/{game}/{t}"] = np.float64(nc)
    save("xfp", out)


def record_mmd():
    gen = maker("make_mmd_vectors")
    runs = [(f"{g}_{name}", GAMES[g], segments) for g in PERFECT_RECALL_TWO_PLAYER for name, segments in MMD_SEGMENTS.items()]
    gen.main(path=os.path.join(HERE, "variant_mmd_vectors.npz"), runs=runs)


def record_efr():
    gen = maker("make_efr_vectors")
    runs = [(GAMES[g], name, EFR_CHECKPOINTS) for g in NO_ACTION_MAPPING for name in EFR_SETS + (["bhv"] if g == "G1" else [])]
    gen.main(runs=runs, path=os.path.join(HERE, "variant_efr_vectors.npz"))


def record_action_value():
    sys.path.insert(0, HERE)
    gen = maker("make_action_value_vectors")
    gen.main(path=os.path.join(HERE, "variant_action_value_vectors.npz"), games=list(GAMES.values()), large=False)


FAMILIES = {"action_value": record_action_value, "efr": record_efr, "layout": record_layout, "dcfr": record_dcfr, "xfp": record_xfp, "mmd": record_mmd}


if __name__ == "__main__":
    for family in sys.argv[1:] or list(FAMILIES):
        started = time.time()
        FAMILIES[family]()
        print(f"{family}: {time.time() - started:.0f} s", flush=True)
