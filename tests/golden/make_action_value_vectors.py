#!/usr/bin/env python3
"""Golden per-infostate action values and reaches, produced by RUNNING the reference's own
open_spiel/python/algorithms/action_value.py (TreeWalkCalculator) and action_value_vs_best_response.py (Calculator),
imported unmodified from where they lie, over the genuine games (oracle/_ref/libspiel_ref.so through
oracle/pyspiel_over_capi.py).  Run in the build container (needs the reference tree):

    python tests/golden/make_action_value_vectors.py

Output: tests/golden/action_value_vectors.npz (np.savez_compressed).  Rows of [I] arrays are the infostate strings in
sorted order, columns the row's legal actions ascending (the legal-index layout), padding cells 0.

  seed                              the RandomState seed of the "random" policy table
  <game>/keys, nact, legal, player  the layout, as in xfp_vectors.npz
  <game>/num_players, num_distinct_actions
  <game>/max_members, histories     the most member histories any infostate has; H
  the flattened tree (the four small games): histories level by level, the children of a history next to each other
  in ascending action order
  <game>/nchild [H] uint8           the children of a history: the first history's are 1 .. nchild[0], the next one's
                                    follow, and so on (which gives every history's parent and first child)
  <game>/edge_action [H] int32      the action on the edge from the parent, -1 at the root
  <game>/kind   [H] int8            0 chance, 1 decision, 2 terminal
  <game>/actor  [H] int8            the acting player of a decision history, else -1
  <game>/info   [H] int32           its infostate row, else -1
  <game>/edge_prob [H]              the chance probability of the incoming edge (0 where the parent is no chance node)
  <game>/term_ret [terminals, P]    Returns() of the terminal histories, in history order
  <game>/mem_off [I + 1], mem       the member histories of every infostate in the DFS order the reference visits them
  cases                             newline-joined case names; per case C:
  <C>/game, <C>/policy              the game string and the policy kind (action_value_cases.policy_table)
  <C>/responder                     -1, or the player who best-responds (TabularBestResponse to the table)
  <C>/root_values [P], reach, cf_reach, chance_reach, player_reach [I], action_values, cf_reach_by_value [I, Amax],
  <C>/weighted_values [I, Amax, P]  the outputs of TreeWalkCalculator for the profile
  with a responder b:
  <C>/best_response_value           Calculator's `exploitability`
  <C>/best_index [I] int32          b's choice as an index among the legal actions, -1 at the other players' rows
  <C>/margin                        over b's infostates with positive counterfactual reach: the smallest difference
                                    between the summed value of the chosen action and of any other action (asserted
                                    >= 1e-9), but for
  <C>/ties                          how many of those infostates have an action whose value equals the chosen action's
                                    at every member history (the table that plays only first actions: kuhn_poker's
                                    card 2 wins 1 by passing and by betting): equal sums in any order of summation,
                                    and the lower action is chosen
  <C>/values_vs_br, counterfactual_reach_probs_vs_br, player_reach_probs_vs_br
                                    Calculator's other three fields for player 1 - b's rows (the rows where player == 1 - b),
                                    values_vs_br in the legal-index layout
  the large game (leduc_poker(players=3), 25 800 infostates) records, to stay a small file, its sorted keys as
  <game>/keys_sha256                the SHA-256 of the newline-joined keys (every game has it) and no keys,
  root_values whole, the [I] vectors whole for the uniform table and for the random table (incompressible) as
  <C>/<vector>_rows, <vector>_sum   rows 0, 4, 8, ... and the sum over all rows; of the tables
  <C>/<table>_rows                  rows 0, 16, 32, ... and
  <C>/<table>_colsum                the sum over all rows (np.sum(axis=0))

Consumers: tests/test_action_values_goldens.py, tests/test_action_values_native.py (CPU),
tests/test_z18_gpu_action_values.py (the HIP engine).
"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import action_value_cases as cases_mod  # noqa: E402

MARGIN = 1e-9


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
    from open_spiel.python import policy
    from open_spiel.python.algorithms import action_value, action_value_vs_best_response, best_response
    return pyspiel, policy, action_value, action_value_vs_best_response, best_response


class TabularBestResponseAdapter:
    """What Calculator asks of pyspiel.TabularBestResponse, over the reference's own best_response.BestResponsePolicy.
    An infostate that class does not list (none of its histories is reached counterfactually) answers its first legal
    action: best_response.cc's rule."""
    modules = None
    made = []

    class _DictPolicy:
        def __init__(self, table):
            self.table = table

        def action_probabilities(self, state, player_id=None):
            # (Calculator lists every action id, the illegal ones at probability 0: the legal ones only, as
            # TabularBestResponse reads its table)
            probs = dict(self.table[state.information_state_string()])
            return {a: probs[a] for a in state.legal_actions()}

    def __init__(self, game, player_id, tabular_policy):
        self.game, self.player_id = game, player_id
        self.set_policy(tabular_policy)
        TabularBestResponseAdapter.made.append(self)

    def set_policy(self, tabular_policy):
        best_response = TabularBestResponseAdapter.modules[4]
        self.br = best_response.BestResponsePolicy(self.game, self.player_id, self._DictPolicy(tabular_policy))

    def value_from_state(self, state):
        return self.br.value(state)

    def get_best_response_actions(self):
        br = self.br

        class Actions(dict):
            def __missing__(self, key):
                raise KeyError(key)

        return Actions({key: br.best_response_action(key) for key in br.infosets})

    def margin(self):
        """Over the infostates with positive counterfactual reach: (the smallest difference between the summed value of
        the chosen action and that of any action whose per-history values are not the chosen action's own, history by
        history; how many infostates have such a twin of the chosen action).  A twin ties in any order of summation:
        the chosen action is the lower of the two, here and in best_response.cc."""
        out, ties = np.inf, 0
        for key, infoset in self.br.infosets.items():
            if not any(cf_p > 0 for _, cf_p in infoset):
                continue
            legal = infoset[0][0].legal_actions(self.player_id)
            terms = {a: [self.br.q_value(s, a) for s, _ in infoset] for a in legal}
            total = {a: sum(cf_p * q for (_, cf_p), q in zip(infoset, terms[a])) for a in legal}
            best = self.br.best_response_action(key)
            twins = [a for a in legal if a != best and terms[a] == terms[best]]
            assert all(a > best for a in twins), (key, best, twins)
            ties += bool(twins)
            for a in legal:
                if a != best and a not in twins:
                    out = min(out, total[best] - total[a])
        return out, ties


def flatten(game, row):
    """The tree level by level; a history's children are consecutive, in ascending action order."""
    P = game.num_players()
    parent, edge_action, kind, actor, info, edge_prob, term_ret = [-1], [-1], [], [], [], [0.0], []
    level = [game.new_initial_state()]
    while level:
        nxt = []
        base = len(kind)
        for k, state in enumerate(level):
            h = base + k
            if state.is_terminal():
                kind.append(2); actor.append(-1); info.append(-1)
                term_ret.append(list(state.returns()))
                continue
            if state.is_chance_node():
                kind.append(0); actor.append(-1); info.append(-1)
                edges = sorted(state.chance_outcomes())
            else:
                p = state.current_player()
                kind.append(1); actor.append(p); info.append(row[state.information_state_string(p)])
                edges = [(a, 0.0) for a in sorted(state.legal_actions())]
            for a, pr in edges:
                parent.append(h); edge_action.append(a); edge_prob.append(pr)
                nxt.append(state.child(a))
        level = nxt
    H = len(kind)
    parent, kind = np.array(parent, np.int32), np.array(kind, np.int8)
    first_child, nchild = np.zeros(H, np.int64), np.zeros(H, np.int64)
    for h in range(H - 1, 0, -1):
        first_child[parent[h]] = h
        nchild[parent[h]] += 1
    members = [[] for _ in row]
    stack = [0]
    while stack:   # depth-first, children in ascending action order: the reference's visiting order
        h = stack.pop()
        if kind[h] == 1:
            members[info[h]].append(h)
        stack.extend(range(first_child[h] + nchild[h] - 1, first_child[h] - 1, -1))
    mem_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    return dict(nchild=nchild.astype(np.uint8), edge_action=np.array(edge_action, np.int32), kind=kind, actor=np.array(actor, np.int8),
                info=np.array(info, np.int32), edge_prob=np.array(edge_prob), term_ret=np.array(term_ret).reshape(-1, P),
                mem_off=mem_off, mem=np.array([h for m in members for h in m], np.int32))


def tabular(policy, game, base, keys, legal, table):
    pol = policy.TabularPolicy.__new__(policy.TabularPolicy)   # (a copy of `base` with its own array: the walk of the
    pol.__dict__.update(base.__dict__)                         # game behind the constructor is done once per game)
    pol.action_probability_array = np.zeros_like(base.action_probability_array)
    for i, k in enumerate(keys):
        for a, action in enumerate(legal[i]):
            pol.action_probability_array[base.state_lookup[k], action] = table[i, a]
    return pol


def outputs(walker, keys, legal, player, amax, P):
    """Every per-infostate quantity of a finished walk, in the legal-index layout."""
    I = len(keys)
    pairs = [(int(player[i]), k) for i, k in enumerate(keys)]
    stats = walker._get_tabular_statistics(pairs)
    out = dict(root_values=np.array(walker.root_values, np.float64),
               reach=np.array([walker.info_state_prob[k] for k in pairs]),
               cf_reach=np.array(stats.counterfactual_reach_probs, np.float64),
               chance_reach=np.array([walker.info_state_chance_prob[k] for k in pairs]),
               player_reach=np.array(stats.player_reach_probs, np.float64),
               action_values=np.zeros((I, amax)), cf_reach_by_value=np.zeros((I, amax)), weighted_values=np.zeros((I, amax, P)))
    for i, k in enumerate(pairs):
        for a, action in enumerate(legal[i]):
            out["action_values"][i, a] = stats.action_values[i][action]
            out["cf_reach_by_value"][i, a] = stats.sum_cfr_reach_by_action_value[i][action]
            out["weighted_values"][i, a] = walker.weighted_action_values[k][action]
    return out


def main(path=None, games=None, large=True):
    mods = reference_modules()
    pyspiel, policy, action_value, avbr, _ = mods
    TabularBestResponseAdapter.modules = mods
    pyspiel.TabularBestResponse = TabularBestResponseAdapter
    out, names = {}, []
    seed = 7
    games = list(games or cases_mod.SMALL_GAMES) + ([cases_mod.LARGE_GAME] if large else [])
    while True:   # raise the seed until every argmax of the random table is decided by MARGIN or more
        out, names, ok = {}, [], True
        for game_string in games:
            t0 = time.time()
            game = pyspiel.load_game(game_string)
            P = game.num_players()
            base = policy.TabularPolicy(game)
            keys = sorted(base.state_lookup)
            row = {k: i for i, k in enumerate(keys)}
            legal = [[a for a, on in enumerate(base.legal_actions_mask[base.state_lookup[k]]) if on] for k in keys]
            amax = max(len(l) for l in legal)
            player = np.zeros(len(keys), np.int32)
            for p, states in enumerate(base.states_per_player):
                for k in states:
                    player[row[k]] = p
            g = game_string
            joined = "\n".join(keys).encode()
            out[f"{g}/keys_sha256"] = np.frombuffer(hashlib.sha256(joined).digest(), np.uint8)
            if game_string != cases_mod.LARGE_GAME:
                out[f"{g}/keys"] = np.frombuffer(joined, np.uint8)
            out[f"{g}/nact"] = np.array([len(l) for l in legal], np.int32)
            out[f"{g}/legal"] = np.array([l + [0] * (amax - len(l)) for l in legal], np.int32)
            out[f"{g}/player"] = player
            out[f"{g}/num_players"], out[f"{g}/num_distinct_actions"] = np.int32(P), np.int32(game.num_distinct_actions())
            small = game_string != cases_mod.LARGE_GAME
            if small:
                tree = flatten(game, row)
                for name, value in tree.items():
                    out[f"{g}/{name}"] = value
                out[f"{g}/max_members"] = np.int32(np.diff(tree["mem_off"]).max())
                out[f"{g}/histories"] = np.int32(len(tree["kind"]))
            print(f"{g}: {len(keys)} infostates, layout in {time.time() - t0:.1f} s", flush=True)
            walker = action_value.TreeWalkCalculator(game)
            calculator = avbr.Calculator(game) if P == 2 else None
            for kind in cases_mod.POLICIES if small else cases_mod.POLICIES[:2]:
                table = cases_mod.policy_table(kind, out[f"{g}/nact"], amax, seed)
                pol = tabular(policy, game, base, keys, legal, table)
                responders = [-1] + ([0, 1] if P == 2 and kind != "uniform" else [])
                for b in responders:
                    t0 = time.time()
                    name = f"{g}/{kind}" + (f"/br{b}" if b >= 0 else "")
                    rec = dict(game=np.frombuffer(g.encode(), np.uint8), policy=np.frombuffer(kind.encode(), np.uint8),
                               responder=np.int32(b))
                    if b < 0:
                        walker.compute_all_states_action_values([pol] * P)
                        res = outputs(walker, keys, legal, player, amax, P)
                    else:
                        ret = calculator(1 - b, pol, [k for i, k in enumerate(keys) if player[i] == 1 - b])
                        adapter = calculator._best_responder[1 - b]
                        res = outputs(calculator._action_value_calculator, keys, legal, player, amax, P)
                        actions = adapter.get_best_response_actions()
                        rec["best_response_value"] = np.float64(ret.exploitability)
                        rec["best_index"] = np.array([legal[i].index(actions.get(k, legal[i][0])) if player[i] == b else -1
                                                      for i, k in enumerate(keys)], np.int32)
                        margin, ties = adapter.margin()
                        rec["margin"], rec["ties"] = np.float64(margin), np.int32(ties)
                        rows = [i for i in range(len(keys)) if player[i] == 1 - b]
                        rec["values_vs_br"] = np.array([[ret.values_vs_br[n][action] for action in legal[i]] + [0.0] * (amax - len(legal[i]))
                                                        for n, i in enumerate(rows)])
                        rec["counterfactual_reach_probs_vs_br"] = np.array(ret.counterfactual_reach_probs_vs_br, np.float64)
                        rec["player_reach_probs_vs_br"] = np.array(ret.player_reach_probs_vs_br, np.float64)
                        if rec["margin"] < MARGIN:
                            print(f"{name}: margin {rec['margin']:.3g} < {MARGIN}", flush=True)
                            ok = False
                            assert kind == "random", (name, rec["margin"])   # (no seed to raise)
                    if small:
                        rec.update(res)
                    else:
                        for k, val in res.items():
                            if k in cases_mod.TABLES:
                                rec[f"{k}_rows"] = val[::cases_mod.ROW_STRIDE]
                                rec[f"{k}_colsum"] = val.sum(axis=0)
                            elif k in cases_mod.VECTORS and kind == "random":
                                rec[f"{k}_rows"] = val[::cases_mod.VECTOR_STRIDE]
                                rec[f"{k}_sum"] = val.sum()
                            else:
                                rec[k] = val
                    for k, val in rec.items():
                        out[f"{name}/{k}"] = val
                    names.append(name)
                    print(f"{name}: root {res['root_values']}" + (f" br {float(rec['best_response_value']):.6g} margin {float(rec['margin']):.3g}" if b >= 0 else "")
                          + f" ({time.time() - t0:.1f} s)", flush=True)
                    if not ok:
                        break
                if not ok:
                    break
            if not ok:
                break
        if ok:
            break
        seed += 1
        print("raising the seed to", seed, flush=True)
    out["seed"] = np.int32(seed)
    out["cases"] = np.frombuffer("\n".join(names).encode(), np.uint8)
    path = path or os.path.join(ROOT, "tests", "golden", "action_value_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    return out


if __name__ == "__main__":
    main()
