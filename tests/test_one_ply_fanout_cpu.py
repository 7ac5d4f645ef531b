"""The one-ply fan-out tables (tests/one_ply_fanout.py) on the CPU: the oracle's tables are the reference build's, call
for call; the positions reach the edges the device test is there for (asserted from the tables alone); and the
comparators the device test uses report a mismatch for every kind of wrong answer they are meant to catch."""
import numpy as np
import pytest

import one_ply_fanout as F

_TABLES = {}


def table(oracle, game):
    """The oracle's table of a game, built once and shared (read-only)."""
    if game not in _TABLES:
        _TABLES[game] = F.build_fanout(oracle, game)
    return _TABLES[game]


def popcount(mask_words):
    return np.unpackbits(np.ascontiguousarray(mask_words).view(np.uint8), axis=1).sum(axis=1)


def has_bit(mask_words, a):
    return (mask_words[:, a >> 5] >> np.uint32(a & 31)) & 1 != 0


@pytest.mark.parametrize("game", F.ALL_GAMES)
def test_oracle_tables_equal_the_reference_builds(oracle, reference, game):
    ours, theirs = table(oracle, game), F.build_fanout(reference, game)
    assert F.tables_equal(ours, theirs) == []
    assert ours["K"] > 0 and len(ours["child_pos"]) > 0


@pytest.mark.parametrize("game", F.ALL_GAMES)
def test_positions_cover_the_edges(oracle, game):
    t = table(oracle, game)
    live = t["term"] == 0
    width = max(t["A"], t["C"])
    count = popcount(t["mask"])
    assert (~live).any(), "a terminal position"
    assert (live & (count > 0) & (count < width)).any(), "a position whose legal set is a strict subset of the id range"
    # every position and every id is in: nothing is sampled away
    assert t["K"] == len(t["hist"]) and len(t["child_pos"]) == int(count.sum())
    if t["poker"]:
        chance = live & (t["cur"] == -1)
        assert (chance & (t["moves"] == 0)).any(), "a chance node of the private deal"
        if game.startswith("leduc"):
            assert (chance & (t["moves"] > 0)).any(), "a chance node of the public deal"
    if game.startswith("connect_four"):
        assert (live & (count < t["A"])).any(), "a running game with a full column"
        assert (live & (count == 1)).any(), "a running game with exactly one open column"
        assert (t["source"] == F.KIND_DRAW).any() and (t["source"] == F.KIND_LAST_CELL).any()
    if game.startswith("leduc") and "action_mapping" not in game:
        node = live & (t["cur"] >= 0)
        fold, call, rais = (has_bit(t["mask"], a) for a in (0, 1, 2))
        assert (node & ~fold).any() and (node & ~rais).any() and (node & fold & call & rais).any()
    if game.startswith("leduc") and "action_mapping" in game:
        node = live & (t["cur"] >= 0)
        assert node.any() and (count[node] == 3).all()
    if "swap=True" in game:
        first = live & (t["hist_len"] == 1)
        assert first.any() and has_bit(t["mask"], t["A"] - 1)[first].all(), "the swap action after the first move"
        assert not has_bit(t["mask"], t["A"] - 1)[t["hist_len"] != 1].any()
    if game in F.FOLDED_HEX:
        assert (live & (t["hist_len"] >= 16)).any() and (live & (t["hist_len"] >= 1)).any()
        assert 32 * t["W"] - t["A"] >= 5, "the ids of the meta bits lie inside the mask words"


def test_position_and_row_counts(oracle):
    """Every ply of every playout is a position (plus the row after the last action) and every byte a row: the sizes
    the device test works with, printed for the record."""
    for game in F.ALL_GAMES:
        t = table(oracle, game)
        og = oracle.Game(game)
        n = F.num_playouts(og, game)
        plies = int((og.random_playouts(F.SEEDS[game], n)["actions"] >= 0).sum())
        from_playouts = int((t["source"] == 0).sum())
        assert from_playouts == plies + 2 * n, game
        assert 1 <= n <= 16 and (game in F.GAMES_32BIT_ONLY or n == min(max(256 // (og.max_plies + 1), 1), 16))
        print(f"{game}: {n} playouts, {t['K']} positions ({from_playouts} from the playouts), {256 * t['K']} step rows, "
              f"{len(t['child_pos'])} children, {len(F.apply_rows(t)[0])} apply rows, "
              f"{len(F.env_rows(t, False, False)[0])} / {len(F.env_rows(t, True, False)[0])} environment rows")


# ---- the comparators notice what they are there to notice ---------------------------------------------------------
def _cmb(t):
    """compact_mask_bytes as the library defines it: 1 or 2 bytes where the ids fit, else the mask words."""
    width = max(t["A"], t["C"])
    return 1 if width <= 8 else 2 if width <= 16 else 4 * t["W"]


SENSITIVITY_GAMES = ["connect_four", "hex(board_size=9)", "kuhn_poker(players=3)", "leduc_poker", "hex(board_size=14,swap=True)"]


@pytest.mark.parametrize("game", SENSITIVITY_GAMES)
def test_comparators_accept_the_tables_own_answer(oracle, game):
    t = table(oracle, game)
    cmb = _cmb(t)
    for extra in (0, 1, 2):
        pos, act = F.step_rows(t, extra)
        assert F.compare_step(t, pos, act, F.ideal_step(t, pos, act, cmb), cmb) == []
    pos, ids = F.apply_rows(t)
    assert F.compare_apply(t, pos, ids, F.ideal_apply(t, pos, ids)) == []
    e = F.expected_apply(t, pos, ids)
    # the only accepted rows are the plain ids of the legal set: one per child
    assert int(e["legal"].sum()) == len(t["child_pos"]) and e["count"] == len(pos) - len(t["child_pos"]) - t["K"]


@pytest.mark.parametrize("game", SENSITIVITY_GAMES)
def test_one_legal_bit_flipped_is_reported(oracle, game):
    t = table(oracle, game)
    cmb = _cmb(t)
    pos, act = F.step_rows(t)
    # (a) a position's legal set loses an action: the device model refuses it
    wrong = F.copy_table(t)
    c = len(t["child_pos"]) // 2
    k, a = int(t["child_pos"][c]), int(t["child_act"][c])
    wrong["mask"][k, a >> 5] ^= np.uint32(1 << (a & 31))
    wrong["child_index"][k, a] = -1
    out = F.compare_step(t, pos, act, F.ideal_step(wrong, pos, act, cmb), cmb)
    assert any(m.startswith("status byte") for m in out) and any("not changed by a legal action" in m for m in out)
    # (b) one bit of one successor mask
    wrong = F.copy_table(t)
    c = int(np.nonzero(t["child_term"] == 0)[0][0])
    wrong["child_mask"][c, 0] ^= np.uint32(1)
    out = F.compare_step(t, pos, act, F.ideal_step(wrong, pos, act, cmb), cmb)
    assert len(out) == 1 and out[0].startswith("successor mask: 1 row(s)")
    got = dict(cur=wrong["child_cur"], term=wrong["child_term"], rets=wrong["child_rets"], mask=wrong["child_mask"])
    out = F.compare_children(t, np.arange(len(t["child_pos"])), got)
    assert len(out) == 1 and out[0].startswith("child mask: 1 row(s)")


@pytest.mark.parametrize("game", SENSITIVITY_GAMES)
def test_an_illegal_row_marked_changed_is_reported(oracle, game):
    t = table(oracle, game)
    cmb = _cmb(t)
    pos, act = F.step_rows(t)
    got = F.ideal_step(t, pos, act, cmb)
    row = int(np.nonzero(got["unchanged"] & (act != 255))[0][7])
    got["unchanged"] = got["unchanged"].copy()
    got["unchanged"][row] = False
    out = F.compare_step(t, pos, act, got, cmb)
    assert out == [f"record changed by a refused or skipped action: 1 row(s), first row {row} = position {pos[row]}, action {act[row]}"]
    pos, ids = F.apply_rows(t)
    got = F.ideal_apply(t, pos, ids)
    row = int(np.nonzero(got["unchanged"])[0][-1])
    got["unchanged"] = got["unchanged"].copy()
    got["unchanged"][row] = False
    assert len(F.compare_apply(t, pos, ids, got)) == 1


@pytest.mark.parametrize("game", SENSITIVITY_GAMES)
def test_a_count_off_by_one_is_reported(oracle, game):
    t = table(oracle, game)
    pos, ids = F.apply_rows(t)
    for delta in (-1, 1):
        got = F.ideal_apply(t, pos, ids)
        got["count"] += delta
        out = F.compare_apply(t, pos, ids, got)
        assert len(out) == 1 and out[0].startswith("illegal count")


@pytest.mark.parametrize("game", ["kuhn_poker", "kuhn_poker(players=10)", "leduc_poker(players=3)"])
def test_the_poker_terminal_code_is_checked(oracle, game):
    t = table(oracle, game)
    cmb = _cmb(t)
    pos, act = F.step_rows(t)
    got = F.ideal_step(t, pos, act, cmb)
    rows = np.nonzero(got["status"] == 0x87)[0]          # a legal action that ends the game
    assert len(rows) > 0 and (got["status"][got["status"] >= 0x80] & 7 == 7).all()
    got["status"] = got["status"].copy()
    got["status"][rows[0]] = 0x80
    out = F.compare_step(t, pos, act, got, cmb)
    assert len(out) == 1 and out[0].startswith("status byte: 1 row(s)")


@pytest.mark.parametrize("game", SENSITIVITY_GAMES)
def test_an_aliasing_id_accepted_is_reported(oracle, game):
    t = table(oracle, game)
    pos, ids = F.apply_rows(t)
    for fold in (lambda a: a & 0xFF, lambda a: a & 0xFFFF, lambda a: a & 0x7FFFFFFF, lambda a: np.where(a < -1, a + 256, a)):
        out = F.compare_apply(t, pos, ids, F.ideal_apply(t, pos, ids, fold))
        assert any(m.startswith("illegal count") for m in out), out
        assert any(m.startswith("record not changed by a legal action") or m.startswith("record changed") for m in out), out
    # through the byte-wide step: a device that tests the legal set modulo the mask width
    cmb = _cmb(t)
    pos, act = F.step_rows(t)
    width = 32 * t["W"]
    if width < 255:
        out = F.compare_step(t, pos, act, F.ideal_step(t, pos, act, cmb, fold=lambda a: a % width), cmb)
        assert any(m.startswith("status byte") for m in out)


def test_env_expectation_follows_the_tables(oracle):
    """expected_env on a game without chance is read off the tables: spot-check it against the oracle's own states."""
    t = table(oracle, "connect_four(rows=5,columns=6,x_in_row=3)")
    og = oracle.Game(t["game"])
    for compact in (False, True):
        pos, ids = F.env_rows(t, compact, odd=True)
        assert len(pos) & 1
        want = F.expected_env(t, og, pos, ids, None)
        for r in range(0, len(pos), 97):
            s = F.state_at(og, t["hist"][pos[r], :t["hist_len"][pos[r]]])
            if ids[r] in s.legal_actions():
                s.apply_action(int(ids[r]))
            assert want["type"][r] == (F.LAST if s.is_terminal() else F.MID) and want["cur"][r] == s.current_player()
            assert want["rew"][r].tolist() == (s.returns() if s.is_terminal() else [0.0, 0.0])
        got = dict(want, reset=want["type"] == F.LAST)
        assert F.compare_env(pos, ids, want, got) == []
        got["count"] += 1
        assert len(F.compare_env(pos, ids, want, got)) == 1
