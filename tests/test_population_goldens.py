"""tests/golden/population_vectors.npz checked against itself and against tests/golden/action_value_vectors.npz: what
the reference's own expected_game_score.py and policy_aggregator.py left there (tests/golden/make_population_vectors.py)
obeys the identities of the quantities, and holds the cases the device tests rely on."""
import numpy as np
import pytest

import action_value_cases as avc
import population_cases as pc


@pytest.fixture(scope="module")
def v():
    return pc.load()


@pytest.fixture(scope="module")
def av():
    return avc.load()


def _aggregates(v, game):
    """(name, weights, rows of the aggregate, their row indices)."""
    for name in pc.weights_of(v, game):
        if game == pc.LARGE_GAME:
            rows = v[f"{game}/aggregate/{name}_rows"]
            yield name, v[f"{game}/weights/{name}"], rows, np.arange(len(v[f"{game}/nact"]))[::pc.ROW_STRIDE]
        else:
            rows = v[f"{game}/aggregate/{name}"]
            yield name, v[f"{game}/weights/{name}"], rows, np.arange(len(rows))


def test_the_cases_are_the_ones_the_generator_lists(v, av):
    assert int(v["seed"]) == int(av["seed"]) and float(v["epsilon"]) == pc.EPSILON == 1e-40
    for g in pc.GAMES:
        P = int(v[f"{g}/num_players"])
        assert tuple(pc.kinds_of(v, g)) == pc.RECORDED_KINDS[g]
        assert tuple(pc.weights_of(v, g)) == pc.RECORDED_WEIGHTS[g]
        assert np.array_equal(v[f"{g}/profiles"], pc.recorded_profiles(g, P))
        assert v[f"{g}/returns"].shape == (len(v[f"{g}/profiles"]), P)
        for name, w, _, _ in _aggregates(v, g):
            assert np.array_equal(w, pc.weight_matrix(name, P, len(pc.RECORDED_KINDS[g])))
            np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    assert [len(v[f"{g}/profiles"]) for g in pc.GAMES] == [16, 64, 32, 16, 4]


def test_the_layout_is_the_action_values(v, av):
    for g in pc.GAMES:
        for name in ("keys_sha256", "nact", "player", "num_players"):
            assert np.array_equal(v[f"{g}/{name}"], av[f"{g}/{name}"]), (g, name)
        assert int(v[f"{g}/amax"]) == av[f"{g}/legal"].shape[1]


def test_the_seeded_weights_hold_one_exact_zero_per_player_at_different_tables(v):
    for g in ("kuhn_poker", "leduc_poker", "kuhn_poker(players=3)", pc.LARGE_GAME):
        w = v[f"{g}/weights/seeded"]
        zeros = [tuple(np.nonzero(row == 0.0)[0]) for row in w]
        assert all(len(z) == 1 for z in zeros) and len(set(zeros)) == len(w), (g, zeros)


def test_a_profile_of_one_table_is_that_tables_root_values(v, av):
    seen = 0
    for g in pc.GAMES:
        kinds, profiles = pc.kinds_of(v, g), v[f"{g}/profiles"]
        for m, profile in enumerate(profiles):
            if len(set(profile)) == 1 and f"{g}/{kinds[profile[0]]}/root_values" in av:
                np.testing.assert_allclose(v[f"{g}/returns"][m], av[f"{g}/{kinds[profile[0]]}/root_values"], rtol=0, atol=pc.TOLERANCE)
                seen += 1
    assert seen == 3 * 3 + 2 + 2   # uniform, random, first on three games; uniform, random on kuhn_poker(players=5) and the large game


def test_returns_are_zero_sum(v):
    for g in pc.GAMES:
        assert np.abs(v[f"{g}/returns"].sum(axis=1)).max() <= pc.TOLERANCE, g


def test_every_aggregated_row_sums_to_one(v):
    for g in pc.GAMES:
        nact = v[f"{g}/nact"]
        for name, _, rows, index in _aggregates(v, g):
            np.testing.assert_allclose(rows.sum(axis=1), 1.0, rtol=0, atol=pc.TOLERANCE, err_msg=f"{g}/{name}")
            assert (rows >= 0).all() and (rows[np.arange(rows.shape[1])[None, :] >= nact[index][:, None]] == 0).all()
        if g == pc.LARGE_GAME:
            assert abs(v[f"{g}/aggregate/seeded_colsum"].sum() - len(nact)) <= pc.colsum_tolerance(len(nact))


def test_one_hot_weights_give_back_the_named_table_where_it_reaches(v, av):
    """Player p plays table (p + 1) mod K alone: the aggregate is that table at p's rows the table reaches (own reach
    > 0, recorded with the action values), and uniform through epsilon at the others."""
    checked_unreached = 0
    for g in pc.SMALL_GAMES:
        kinds, stack = pc.kinds_of(v, g), pc.recorded_stack(v, g)
        player, nact = v[f"{g}/player"], v[f"{g}/nact"]
        got = v[f"{g}/aggregate/onehot"]
        named = (player + 1) % len(kinds)
        for i in range(len(player)):
            kind = kinds[named[i]]
            reached = av[f"{g}/{kind}/player_reach"][i] > 0 if kind == "first" else True
            if reached:
                np.testing.assert_allclose(got[i], stack[named[i], i], rtol=0, atol=pc.TOLERANCE)
            else:
                np.testing.assert_allclose(got[i, :nact[i]], 1.0 / nact[i], rtol=0, atol=pc.TOLERANCE)
                checked_unreached += 1
    assert checked_unreached > 0


def test_uniform_weights_average_the_rows_at_first_decisions(v):
    """At a player's first decisions (no own action before them) the aggregate is the plain average of the tables' rows."""
    g = "kuhn_poker"
    stack, got = pc.recorded_stack(v, g), v[f"{g}/aggregate/uniform"]
    keys = avc.keys_of(avc.load(), g)
    first = [i for i, k in enumerate(keys) if len(k) == 1]   # player 0 with a card and no betting yet
    assert len(first) == 3
    np.testing.assert_allclose(got[first], stack[:, first].mean(axis=0), rtol=0, atol=pc.TOLERANCE)
