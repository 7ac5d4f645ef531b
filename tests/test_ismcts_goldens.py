"""tests/golden/ismcts_vectors.npz on its own (no engine): the trees the reference's ismcts.py built under the scripted
random_state (tests/golden/make_ismcts_vectors.py) are trees of an IS-MCTS search, the conditions that make them
comparable bit for bit hold, every knob value appears with every game, and the restated resampler — the one piece of the
pinning that is not the reference's own code — is uniform over the deals consistent with the searcher's information."""
import itertools
import os

import numpy as np
import pytest

import ismcts_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return ic.load_cases()


def test_file_is_small_and_covers_every_knob_with_every_game(cases):
    assert os.path.getsize(ic.GOLDEN) < 1 << 20
    for game in ic.GAMES:
        mine = [c for c in cases if c["game"] == game]
        assert len(mine) >= 20
        for knob, values in ic.KNOBS.items():
            assert {c[knob] for c in mine} == set(values), (game, knob)
    assert {c["game"] for c in cases} == set(ic.GAMES)
    # leduc roots cover both rounds, facing a raise, and the raise cap (only fold and call left)
    for game in ic.GAMES[2:]:
        roots = {(c["nodes"][0][1]) for c in cases if c["game"] == game}
        assert any("[Round 1]" in k for k in roots) and any("[Round 2]" in k for k in roots)
    # cases of one (game, knobs, seed) sit at distinct stream indices below 257, so that they can share a launch
    groups = {}
    for c in cases:
        groups.setdefault((c["game"], c["seed"]) + tuple(c[k] for k in ic.KNOBS), []).append(c["index"])
    assert all(len(set(v)) == len(v) and max(v) <= 256 for v in groups.values())
    assert any(256 in v for v in groups.values())


def test_trees_are_consistent(cases):
    for c in cases:
        nodes = c["nodes"]
        actions = 2 if c["game"].startswith("kuhn") else 3
        assert len(nodes) >= 1 and len(nodes) <= c["max_simulations"]   # a simulation creates at most one node
        assert nodes[0][2] == c["max_simulations"] - 1                  # the first simulation only evaluates the root
        assert len({(n[0], n[1]) for n in nodes}) == len(nodes)         # one node per (player, information state)
        for player, key, total, visits, sums, rank in nodes:
            assert total == visits.sum() and (visits >= 0).all()
            expanded = rank >= 0
            assert sorted(rank[expanded]) == list(range(expanded.sum())) and not expanded[actions:].any()
            assert (visits[~expanded] == 0).all() and (sums[~expanded] == 0).all()
            assert (visits[expanded] >= 1).all()                        # a child is visited when it is created
            ic.node_ident(c["game"], player, key)                       # the key parses
        if c["status"] == 0:
            policy = c["policy"][:actions]
            assert abs(policy.sum() - 1.0) < 1e-12 and (policy >= 0).all() and np.isnan(c["policy"][actions:]).all()
            assert policy[c["sampled_action"]] > 0
            assert (policy[nodes[0][5][:actions] < 0] == 0).all()       # never expanded: appended with 0
        else:
            assert c["status"] == 1 and c["max_simulations"] == 1 and np.isnan(c["policy"]).all() and c["sampled_action"] == -1
        assert c["draws"] >= c["max_simulations"]


def test_the_tolerance_margin_holds(cases):
    """No selection had a child within 1e-9 of the candidate threshold max - 1e-5: a last-bit difference of log() between
    two machines cannot change a candidate set."""
    assert min(c["margin"] for c in cases) >= 1e-9
    assert any(np.isfinite(c["margin"]) for c in cases)


class _Uniforms:
    """A `uniform` callable that replays a fixed list of draws and reports when it runs out."""

    def __init__(self, values):
        self.values, self.used = values, 0

    def __call__(self):
        if self.used == len(self.values):
            raise IndexError
        self.used += 1
        return self.values[self.used - 1]


@pytest.mark.parametrize("game,history,player", [
    ("kuhn_poker", [1, 0], 0), ("kuhn_poker(players=3)", [2, 0, 3, 0], 1),
    ("leduc_poker", [2, 4, 1, 1, 3], 0), ("leduc_poker(players=3)", [0, 6, 3, 2, 1, 1], 2),
])
def test_restated_resampler_is_uniform_over_the_consistent_deals(reference, game, history, player):
    """The rejection loops, enumerated exactly over u.  A draw with d outcomes left cuts [0, 1) into d equal cells; the
    midpoint of a cell stands for it.
    (a) Every sequence of draws in which each is accepted at once ends in a different deal, the deals reached are exactly
        the deals consistent with the searcher's card (and the public card), and each sequence has the same probability
        (the product of 1 / d over its draws: d depends on the position of the draw only).
    (b) A barred cell, put before any draw of such a sequence, changes nothing but the number of draws consumed — the loop
        draws again — and the barred cells of a draw are the same number whatever was accepted before (the other players'
        cards are never barred), so the rejections multiply every deal's probability by the same geometric factor.
    (a) and (b) together: the deals are equally likely."""
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference)
    g = pyspiel.load_game(game)
    state = g.new_initial_state()
    for a in history:
        state.apply_action(a)
    players = g.num_players()
    key = state.information_state_string(player)
    barred = {history[player]}
    if game.startswith("leduc"):
        barred.add(ic.public_card(g, history))

    def finish(draws):
        u = _Uniforms(list(draws))
        out = ic.resample(state, player, u)
        assert u.used == len(draws)
        assert out.information_state_string(player) == key and out.history()[players:] == state.history()[players:]
        return tuple(out.history()[:players])

    reached, barred_per_draw = {}, {}
    frontier = [()]
    while frontier:
        grown = []
        for prefix in frontier:
            outcomes = _outcomes_after(g, state, player, prefix)
            if outcomes is None:   # the prefix finishes the loop
                deal = finish(prefix)
                assert deal not in reached
                reached[deal] = prefix
                continue
            d = len(outcomes)
            n_barred = sum(o in barred for o in outcomes)
            assert barred_per_draw.setdefault(len(prefix), (d, n_barred)) == (d, n_barred)
            grown += [prefix + ((k + 0.5) / d,) for k, o in enumerate(outcomes) if o not in barred]
        frontier = grown
    cards = [c for c in range(g.max_chance_outcomes()) if c not in barred]
    deals = set()
    for others in itertools.permutations(cards, players - 1):
        deal = list(others)
        deal.insert(player, history[player])
        deals.add(tuple(deal))
    assert set(reached) == deals and len({len(p) for p in reached.values()}) == 1
    for deal, prefix in reached.items():   # (b): one and two rejected draws in front of every draw
        for at in range(len(prefix)):
            outcomes = _outcomes_after(g, state, player, prefix[:at])
            d = len(outcomes)
            for k, o in enumerate(outcomes):
                if o in barred:
                    u = (k + 0.5) / d
                    assert finish(prefix[:at] + (u,) + prefix[at:]) == deal
                    assert finish(prefix[:at] + (u, u) + prefix[at:]) == deal


def _outcomes_after(game, state, player, prefix):
    """The chance outcomes the clone offers at the draw that follows the draws `prefix` (None: they finish the loop),
    by the loop written out once more with a `uniform` that stops there."""
    left = list(prefix)
    history = list(state.history())
    players = game.num_players()
    mine = history[player]
    barred = {mine, ic.public_card(game, history)} if str(game).startswith("leduc") else {mine}
    clone = game.new_initial_state()
    for p in range(players):
        action = mine
        if p != player:
            while action in barred:
                outcomes, probs = zip(*clone.chance_outcomes())
                if not left:
                    return list(outcomes)
                action = ic.cdf_scan(outcomes, probs, left.pop(0))
        clone.apply_action(action)
    assert not left
    return None
