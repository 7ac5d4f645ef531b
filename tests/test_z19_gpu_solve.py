"""Exhaustive enumeration and retrograde solve on the device (osg_solve_*; Game.solve / SolvedGame) against
tests/golden/solve_vectors.npz — what the reference's own value_iteration.py and get_all_states.py give
(tests/golden/make_solve_vectors.py).

No tolerance anywhere: the number of positions per level and in total, the SET of State::ToString() strings (compared
string by string where the goldens keep them, by SHA-256 of the sorted strings for the cases with 10^4 .. 10^5
positions) and every value are compared for equality.  A canonical key that is too fine shows as too many positions,
one that is too coarse as too few."""
import numpy as np
import pytest

import solve_cases as sc

pytestmark = pytest.mark.gpu

GEOMETRY = {"hex3x4": ("hex", 3, 4), "c4_4x4": ("connect_four", 4, 4), "c4_4x4k3": ("connect_four", 4, 4),
            "c4_3x5k3": ("connect_four", 3, 5), "c4_8x8_d6": ("connect_four", 8, 8), "hex6_d3": ("hex", 6, 6)}
LARGEST = "c4_4x4"   # 161 029 positions


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


_solved = {}


def solved(ctx, case):
    """One solve per golden case, shared by the tests and left unchanged."""
    if case not in _solved:
        import open_spiel_amd as osa
        _solved[case] = osa.Game(sc.field(case, "game")).solve(
            ctx, depth_limit=int(sc.field(case, "depth_limit")), include_terminals=bool(sc.field(case, "include_terminals")))
    return _solved[case]


def strings_of(s, case):
    if case not in GEOMETRY:
        return s.state_strings()   # osg_state_string, one call per position
    kind, rows, cols = GEOMETRY[case]
    out = sc.render_strings(kind, s.states.raw_words(), rows, cols)
    for i in range(0, s.n, 997):   # the host renderer prints what osg_state_string prints
        assert out[i] == s.states.state_string(i)
    return out


def check_enumeration(s, case):
    counts = sc.field(case, "level_counts")
    assert s.n == sc.field(case, "count")
    assert np.diff(s.level_offsets.cpu().numpy()).tolist() == counts.tolist()
    assert s.num_levels == len(counts)
    strings = strings_of(s, case)
    order = sorted(range(s.n), key=strings.__getitem__)
    ordered = [strings[i] for i in order]
    want = sc.keys(case)
    if want is not None:
        assert ordered == want
    assert sc.sha256_of(ordered) == sc.field(case, "keys_sha256")
    lv = np.repeat(np.arange(len(counts)), counts)
    assert [sc.stones(t) for t in strings[::53]] == lv[::53].tolist()
    return order


# ---- (a) ----
@pytest.mark.parametrize("case", ["ttt", "hex2", "hex3", "hex3x4", "c4_4x4", "c4_4x4k3", "c4_3x5k3"])
def test_positions_and_values_equal_the_reference(ctx, case):
    s = solved(ctx, case)
    order = check_enumeration(s, case)
    values = s.values.cpu().numpy()
    assert values.dtype == np.float64 and np.isin(values, (-1.0, 0.0, 1.0)).all()
    assert (values[order] == sc.field(case, "values").astype(np.float64)).all()
    assert values[0] == sc.field(case, "root_value")
    assert s.num_terminals == sc.field(case, "level_terminals").sum()
    assert s.num_edges == sc.field(case, "level_children").sum()
    assert int(s.edge_off[-1]) == s.num_edges


def edge_parents(s):
    import torch
    counts = s.edge_off[1:] - s.edge_off[:-1]
    return torch.repeat_interleave(torch.arange(s.n, device=counts.device), counts), counts


# ---- (b) ----
@pytest.mark.parametrize("case,stride", [("ttt", 1), (LARGEST, 7)])
def test_edges_lead_to_the_child_that_applying_the_action_gives(ctx, case, stride):
    import torch
    s = solved(ctx, case)
    parent, counts = edge_parents(s)
    legal = s.states.legal_actions_mask_bits()
    popcount = sum(((legal >> b) & 1).sum(dim=1) for b in range(32))
    assert (popcount == counts).all()   # every legal action has an edge ...
    a = s.edge_action.long()
    assert (((legal[parent, a >> 5] >> (a & 31)) & 1) == 1).all()   # ... which is legal ...
    inner = torch.ones_like(a, dtype=torch.bool)
    inner[s.edge_off[:-1][counts > 0]] = False
    assert (a[1:] > a[:-1])[inner[1:]].all()   # ... in ascending order
    keep = (parent % stride) == 0
    children = s.states.gather(parent[keep])
    children.apply_actions(s.edge_action[keep])
    assert (s.lookup(children) == s.edge_child[keep]).all()
    assert (s.edge_child >= 0).all()


# ---- (c) ----
@pytest.mark.parametrize("case", ["ttt", "hex3", LARGEST])
def test_optimal_mask_and_distance(ctx, case):
    import torch
    s = solved(ctx, case)
    parent, counts = edge_parents(s)
    legal, opt = s.states.legal_actions_mask_bits(), s.optimal_mask
    terminal = s.states.is_terminal()
    assert ((opt & ~legal) == 0).all()
    assert ((opt != 0).any(dim=1) == ~terminal).all()
    a = s.edge_action.long()
    chosen = ((opt[parent, a >> 5] >> (a & 31)) & 1) == 1
    assert (chosen == (s.values[s.edge_child] == s.values[parent])).all()
    # distance: 0 at terminal positions; else 1 + the nearest end among the optimal children where the mover wins,
    # the farthest where the mover loses or draws
    level = torch.repeat_interleave(torch.arange(s.num_levels, device=parent.device), s.level_offsets[1:] - s.level_offsets[:-1])
    mover_sign = 1.0 - 2.0 * (level % 2).double()   # player 0 moves on the even levels (and maximises)
    win = s.values * mover_sign > 0
    child_d = s.distance[s.edge_child].long()
    big = 1 << 20
    near = torch.full((s.n,), big, dtype=torch.int64, device=parent.device).scatter_reduce(
        0, parent[chosen], child_d[chosen], "amin")
    far = torch.full((s.n,), -1, dtype=torch.int64, device=parent.device).scatter_reduce(
        0, parent[chosen], child_d[chosen], "amax")
    want = torch.where(terminal, torch.zeros_like(near), 1 + torch.where(win, near, far))
    assert (s.distance.long() == want).all()
    assert (s.distance[terminal] == 0).all() and (s.distance[~terminal] > 0).all()


# ---- (d) ----
@pytest.mark.parametrize("case", ["ttt", LARGEST])
def test_alpha_beta_search_agrees_at_every_position(ctx, case):
    s = solved(ctx, case)
    value, best, _, status = s.states.alpha_beta_search(maximizing_player=0, max_nodes=1 << 24)
    assert (status == 0).all()
    assert (value == s.values).all()
    terminal = s.states.is_terminal()
    assert (best[terminal] == -1).all()
    b = best[~terminal].long()
    assert (((s.optimal_mask[~terminal, b >> 5] >> (b & 31)) & 1) == 1).all()


# ---- (e) ----
def test_lookup(ctx):
    import torch
    import open_spiel_amd as osa
    s = solved(ctx, "ttt")
    perm = torch.randperm(s.n, generator=torch.Generator().manual_seed(5)).to(ctx.device)
    assert (s.lookup(s.states.gather(perm)) == perm).all()
    odd = osa.StateBatch(ctx, "tic_tac_toe", 3)
    odd.set_cells(0, "xx.......")   # two more x than o: no play reaches it
    odd.set_cells(1, "xo.......")
    odd.set_cells(2, "xxxoo.o..")   # o moved after x's line was complete
    got = s.lookup(odd).cpu().tolist()
    strings = s.state_strings()
    assert got[0] == -1 and strings[got[1]] == "xo.\n...\n..." and got[2] == -1
    for wide in ("c4_8x8_d6", "hex6_d3"):   # the two-word keys
        w = solved(ctx, wide)
        pick = torch.arange(0, w.n, 11, device=ctx.device)
        assert (w.lookup(w.states.gather(pick)) == pick).all()


# ---- (f) and the two-word key ----
@pytest.mark.parametrize("case", ["ttt_d3", "ttt_noterm", "ttt_d5", "c4_8x8_d6", "hex6_d3"])
def test_limits_give_the_reference_counts(ctx, case):
    s = solved(ctx, case)
    check_enumeration(s, case)
    assert s.num_terminals == sc.field(case, "level_terminals").sum()
    assert s.num_edges == sc.field(case, "level_children").sum()
    dropped = int((s.edge_child < 0).sum())
    assert dropped > 0
    if case == "ttt_d3":   # every child of the 252 positions at the limit is a running game one ply too deep
        assert dropped == 1512


# ---- (g) ----
def test_max_states_is_a_clean_refusal(ctx):
    import open_spiel_amd as osa
    for cap in (1, 100, 5477):
        with pytest.raises(osa.OsgError, match="osg error -2.*max_states"):
            osa.Game("tic_tac_toe").solve(ctx, max_states=cap)
    s = osa.Game("tic_tac_toe").solve(ctx, max_states=5478)
    assert s.n == 5478 and float(s.values[0]) == 0.0


# ---- (h) ----
@pytest.mark.parametrize("game,why", [("kuhn_poker", "chance"), ("leduc_poker", "chance"), ("hex(swap=true)", "swap"),
                                      ("hex(board_size=12)", "128 cells"), ("hex(board_size=9)", "128 bits"),
                                      ("hex(board_size=3,string_rep=explicit)", "explicit")])
def test_unserved_games_are_refused_with_a_message(ctx, game, why):
    import open_spiel_amd as osa
    with pytest.raises(osa.OsgError, match="osg error -2.*" + why):
        osa.Game(game).solve(ctx)
    assert osa.Game("hex(board_size=2)").solve(ctx).n == 32


# ---- (i) ----
def test_mirror_value_iteration_and_get_all_states():
    """pyspiel_hip.value_iteration (algorithms::ValueIteration of the host mirror) returns the golden dict;
    get_all_states keeps returning the 5 478 positions of tic_tac_toe under the same keys."""
    import open_spiel_amd
    pyspiel = open_spiel_amd.pyspiel_hip
    for case in ("ttt", "hex3"):
        game = pyspiel.load_game(sc.field(case, "game"))
        values = pyspiel.value_iteration(game, -1, 0.01)
        assert sorted(values) == sc.keys(case)
        assert [values[k] for k in sc.keys(case)] == sc.field(case, "values").astype(np.float64).tolist()
    limited = pyspiel.value_iteration(pyspiel.load_game("tic_tac_toe"), 3, 0.01)
    assert sorted(limited) == sc.keys("ttt_d3") and set(limited.values()) == {0.0}
    states = pyspiel.get_all_states(pyspiel.load_game("tic_tac_toe"), -1, True, False)
    assert sorted(states) == sc.keys("ttt")
    assert all(str(st) == k for k, st in list(states.items())[::97])
    with pytest.raises(Exception, match="perfect information|chance"):
        pyspiel.value_iteration(pyspiel.load_game("kuhn_poker"), -1, 0.01)
