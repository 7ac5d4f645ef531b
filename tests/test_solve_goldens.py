"""tests/golden/solve_vectors.npz is self-consistent: counts add up, the recorded strings hash to the recorded digest,
the root value is the value of the initial position's string, tic_tac_toe has the 5 478 states of the reference's own
get_all_states_test, and the cases hit the shapes at which the enumeration kernels can go wrong."""
import numpy as np
import pytest

import solve_cases as sc

EXPECTED = ["ttt", "hex2", "hex3", "hex3x4", "c4_4x4", "c4_4x4k3", "c4_3x5k3"]
GAMES = {"ttt": "tic_tac_toe", "hex2": "hex(board_size=2)", "hex3": "hex(board_size=3)",
         "hex3x4": "hex(num_rows=3,num_cols=4)", "c4_4x4": "connect_four(rows=4,columns=4)",
         "c4_4x4k3": "connect_four(rows=4,columns=4,x_in_row=3)", "c4_3x5k3": "connect_four(rows=3,columns=5,x_in_row=3)"}


def test_every_case_of_the_issue_is_recorded():
    assert sc.solve_cases() == EXPECTED
    for c in EXPECTED:
        assert sc.field(c, "game") == GAMES[c]
    assert sc.enum_cases() == ["ttt_d3", "ttt_noterm", "ttt_d5", "c4_8x8_d6", "hex6_d3"]


@pytest.mark.parametrize("case", EXPECTED + ["ttt_d3", "ttt_noterm", "ttt_d5", "c4_8x8_d6", "hex6_d3"])
def test_counts_add_up(case):
    counts, terms = sc.field(case, "level_counts"), sc.field(case, "level_terminals")
    assert counts.sum() == sc.field(case, "count")
    assert counts[0] == 1 and (terms <= counts).all()
    k = sc.keys(case)
    if k is not None:
        assert len(k) == sc.field(case, "count") and k == sorted(k) and len(set(k)) == len(k)
        assert sc.sha256_of(k) == sc.field(case, "keys_sha256")
        assert np.bincount([sc.stones(s) for s in k], minlength=len(counts)).tolist() == counts.tolist()
    if not sc.field(case, "include_terminals"):
        assert terms.sum() == 0


@pytest.mark.parametrize("case", EXPECTED)
def test_values_and_root(case):
    values = sc.field(case, "values")
    assert values.dtype == np.int8 and len(values) == sc.field(case, "count")
    assert np.isin(values, (-1, 0, 1)).all()
    k = sc.keys(case)
    if k is not None:
        root = [i for i, s in enumerate(k) if sc.stones(s) == 0]
        assert len(root) == 1 and values[root[0]] == sc.field(case, "root_value")
    # known answers: tic_tac_toe is a draw, the first player wins hex, 4 x 4 connect_four is a draw
    assert sc.field(case, "root_value") == {"ttt": 0, "c4_4x4": 0}.get(case, sc.field(case, "root_value"))
    if case.startswith("hex"):
        assert sc.field(case, "root_value") == 1


def test_tic_tac_toe_counts():
    assert sc.field("ttt", "count") == 5478           # get_all_states_test.cc
    assert sc.field("ttt_d3", "count") == 1 + 9 + 72 + 252
    assert sc.field("ttt_noterm", "count") == 5478 - sc.field("ttt", "level_terminals").sum()
    # a terminal position one ply below the limit is listed (get_all_states.cc:36-48), the others there are not
    assert sc.field("ttt_d5", "level_counts")[6] == sc.field("ttt", "level_terminals")[6]


def test_cases_hit_the_shapes_the_kernels_can_go_wrong_at():
    """One-state level (the root), child counts that are no multiple of the workgroup size (256), a last level of
    terminal positions only, levels whose merged duplicates outnumber a wavefront many times over, a two-word key.
    A single run of equal keys is as long as the position has parents, at most the stones of the player who moved
    last (6 in these games), so a run longer than 64 keys cannot occur in any served game; what the cases do hit is
    levels where the runs of duplicates, taken together, span many wavefronts and straddle their boundaries."""
    for case in EXPECTED:
        counts, children, terms = (sc.field(case, n) for n in ("level_counts", "level_children", "level_terminals"))
        assert counts[0] == 1
        assert terms[-1] == counts[-1] and children[-1] == 0
        assert any(c % 256 for c in children[:-1])
    for case in ("ttt", "hex3x4", "c4_4x4"):
        counts, children = sc.field(case, "level_counts"), sc.field(case, "level_children")
        assert (children[:-1] - counts[1:]).max() > 64 * 16
    # (rows + 1) * columns = 72 bits: the two-word bitboard and the two-word key
    assert sc.field("c4_8x8_d6", "game") == "connect_four(rows=8,columns=8)" and sc.field("c4_8x8_d6", "depth_limit") == 6
    # 36 cells: two words per hex plane, a key of the full 128 bits
    assert sc.field("hex6_d3", "game") == "hex(board_size=6)" and sc.field("hex6_d3", "level_counts").tolist() == [1, 36, 1260, 21420]
