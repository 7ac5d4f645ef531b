"""The edge list (tests/edge_games.py) on the CPU: it covers every class it was derived for, the device library
describes every string it serves as the oracle does and refuses the others with the limit in words, and the oracle — which judges the device in
tests/test_z26_gpu_edge_games.py — equals the genuine reference build on every string: description, seeded playouts
bit for bit, strings and off-turn queries (the checks of tests/test_oracle_vs_reference.py, which pins only its own
two dozen strings)."""
import pytest

import edge_games as eg
import test_oracle_vs_reference as ovr


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import open_spiel_amd
    return open_spiel_amd


def playouts_for(og):
    """How many seeded playouts the record of every ply's tensors of every player allows (about 80 MB at most)."""
    per = (og.max_game_length + og.max_chance_nodes_in_history + 1) * og.num_players * \
          (og.observation_tensor_size + og.information_state_tensor_size)
    return max(4, min(60, 20_000_000 // per))


def test_the_list_covers_every_class():
    """Classes are computed from the strings; a class that loses its game fails here.  Every class has a game the parser
    SERVES, so that it runs on the device, but the three that no served board can have: those have a refused one."""
    covered = set()
    for g in eg.EDGE_GAMES:
        covered |= eg.classes_of(g)
    missing = [c for c in eg.REQUIRED if c not in covered and c not in eg.UNSERVABLE]
    assert not missing, missing
    refused = set()
    for g in eg.REFUSED:
        refused |= eg.classes_of(g)
    assert set(eg.UNSERVABLE) <= refused and not set(eg.UNSERVABLE) & covered
    assert len(set(eg.EDGE_GAMES)) == len(eg.EDGE_GAMES) and 55 <= len(eg.EDGE_GAMES) <= 70 and len(eg.REFUSED) == 10
    assert not set(eg.EDGE_GAMES) & set(eg.REFUSED)
    # no x_in_row above rows + columns (larger values are described only, below)
    for g in eg.EDGE_GAMES + eg.REFUSED:
        if g.startswith("connect_four"):
            R, C, K, _ = eg.c4_geometry(g)
            assert K <= R + C and (R + 1) * C <= eg.C4_MAX_BITS and C <= eg.C4_MAX_COLS
            assert eg.c4_served(R, C, K) == (g in eg.EDGE_GAMES)
        elif g.startswith("hex"):
            C, R, swap, plain, _ = eg.hex_geometry(g)
            assert C <= eg.HEX_MAX_COLS and C * R + swap <= eg.HEX_MAX_CELLS and (not swap or C <= R) and (not plain or C == R)
    assert len(eg.RULES_ONLY) == 2 and len(eg.SOLVABLE) >= 6


def test_unservable_classes_have_no_served_board():
    """Over every connect_four geometry that fits the bitboards and every x_in_row up to rows + columns: a board with
    one of eg.UNSERVABLE's classes is beyond the shift limit."""
    seen = set()
    for C in range(1, eg.C4_MAX_COLS + 1):
        for R in range(1, eg.C4_MAX_BITS // C):
            if (R + 1) * C not in (64, 128):
                continue
            for K in (max(R, C), max(R, C) + 1):
                hit = eg.classes_of(eg.c4(R, C, K)) & set(eg.UNSERVABLE)
                seen |= hit
                assert not (hit and eg.c4_served(R, C, K)), (R, C, K)
    assert seen == set(eg.UNSERVABLE)


@pytest.mark.parametrize("game", eg.REFUSED)
def test_boards_beyond_the_shift_limit_are_refused_with_the_limit_in_words(built, game):
    """The line test's largest shift would reach the width of the board's word: OSG_ERR_UNSUPPORTED, and the message
    gives the shift and the limit."""
    R, C, K, _ = eg.c4_geometry(game)
    k_dev = min(K, max(R, C) + 1)
    reach, limit = (2 if k_dev == 4 else k_dev - 1) * (R + 2), (128 if (R + 1) * C > 64 else 64) - 1
    assert reach > limit
    with pytest.raises(built.OsgError, match=f"osg error -2: connect_four: the line test of this board shifts by {reach} bits.*limit is {limit} "):
        built.describe(game)


def test_the_served_predicate_is_the_parsers(built):
    """eg.c4_served, which sorts the list into served and refused strings, against parse_game over every geometry that
    fits the bitboards and every x_in_row up to two beyond the longest side."""
    checked = 0
    for C in range(1, eg.C4_MAX_COLS + 1):
        for R in range(1, eg.C4_MAX_BITS // C):
            for K in range(1, max(R, C) + 3):
                try:
                    built.describe(eg.c4(R, C, K))
                    accepted = True
                except built.OsgError:
                    accepted = False
                assert accepted == eg.c4_served(R, C, K), (R, C, K)
                checked += 1
    assert checked > 5000


@pytest.mark.parametrize("game", eg.SERVED + eg.C4_HUGE_K)
def test_device_description_matches_the_oracle(built, oracle, game):
    """osg_game_describe (no device needed) against the oracle: the assertions of tests/test_abi.py."""
    d = built.describe(game)
    og = oracle.Game(game)
    assert d.num_distinct_actions == og.num_distinct_actions
    assert d.max_chance_outcomes == og.max_chance_outcomes
    assert d.num_players == og.num_players
    assert d.obs_size == og.observation_tensor_size
    assert d.info_size == og.information_state_tensor_size
    assert d.max_game_length == og.max_game_length
    assert d.max_chance_nodes == og.max_chance_nodes_in_history
    assert (d.min_utility, d.max_utility) == (og.min_utility, og.max_utility)
    assert [d.obs_shape[i] for i in range(d.obs_rank)] == og.observation_tensor_shape()
    assert d.canonical.decode() == str(og)
    assert d.mask_words == og.mask_words


def test_layout_words_follow_the_limits(built):
    """state_words at the layout switches: two / four connect_four words at 64 / 65 bits; hex 4 * NW words where the meta
    word folds (cells <= 32 * NW - 5), one more where it does not; the swap id opens a plane word at a multiple of 32."""
    for g in eg.SERVED:
        d = built.describe(g)
        if g.startswith("connect_four"):
            R, C, _, _ = eg.c4_geometry(g)
            assert d.state_words == (4 if (R + 1) * C > eg.C4_NARROW_BITS else 2), g
        elif g.startswith("hex"):
            C, R, swap, _, _ = eg.hex_geometry(g)
            nw = eg.hex_plane_words(C * R, swap)
            assert d.state_words == (4 * nw if C * R <= 32 * nw - 5 else 4 * nw + 1), g
            assert d.mask_words == (C * R + swap + 31) // 32, g


def test_unservable_sizes_are_refused_without_overflow(built):
    """Dimensions are bounded one by one before their product is formed."""
    for bad in ["connect_four(rows=2147483647,columns=1)", "connect_four(rows=128,columns=1)", "connect_four(rows=1,columns=33)",
                "connect_four(rows=64,columns=2)", "connect_four(rows=65535,columns=65537)",
                "hex(board_size=65536)", "hex(num_cols=1,num_rows=385)", "hex(num_cols=16,num_rows=24,swap=True)",
                "hex(num_cols=32,num_rows=2)", "hex(num_cols=2,num_rows=2147483647)"]:
        with pytest.raises(built.OsgError, match="osg error -2"):     # OSG_ERR_UNSUPPORTED
            built.describe(bad)


@pytest.mark.parametrize("game", eg.EDGE_GAMES + eg.REFUSED)
def test_oracle_description_matches_the_reference(oracle, reference, game):
    ovr.test_game_description_matches(oracle, reference, game, 0)


@pytest.mark.parametrize("game", eg.EDGE_GAMES + eg.REFUSED)
def test_oracle_playouts_are_bit_identical_to_the_reference(oracle, reference, game):
    ovr.test_seeded_playouts_are_bit_identical(oracle, reference, game, playouts_for(oracle.Game(game)))


@pytest.mark.parametrize("game", eg.EDGE_GAMES + eg.REFUSED)
def test_oracle_strings_and_offturn_queries_match_the_reference(oracle, reference, game):
    ovr.test_strings_and_offturn_queries_match_along_playouts(oracle, reference, game, 48)


@pytest.mark.parametrize("game", eg.C4_HUGE_K)
def test_no_line_exists_above_the_longest_side(oracle, reference, game):
    """x_in_row above max(rows, columns): the reference accepts the game and never finds a line — every playout fills
    the board and is a draw (the device plays such a game as x_in_row = max(rows, columns) + 1: no line either)."""
    for impl in (oracle, reference):
        g = impl.Game(game)
        rec = g.random_playouts(3, 20)
        assert (rec["returns"] == 0).all() and rec["terminal"][:, -1].all()
        assert ((rec["actions"] >= 0).sum(axis=1) == g.max_game_length).all()
