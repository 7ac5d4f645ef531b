"""tests/golden/action_value_vectors.npz checked against itself: what the reference's own action_value.py and
action_value_vs_best_response.py left there (tests/golden/make_action_value_vectors.py) obeys the identities of the
quantities, and holds the cases the device tests rely on."""
import hashlib

import numpy as np
import pytest

import action_value_cases as avc


@pytest.fixture(scope="module")
def v():
    return avc.load()


def _small_cases(v):
    return [c for g in avc.SMALL_GAMES for c in avc.case_names(v, g)]


def test_the_cases_are_the_ones_the_generator_lists(v):
    names = avc.case_names(v)
    want = []
    for g in avc.SMALL_GAMES:
        for kind in avc.POLICIES:
            want.append(f"{g}/{kind}")
            if g in avc.TWO_PLAYER and kind != "uniform":
                want += [f"{g}/{kind}/br0", f"{g}/{kind}/br1"]
    want += [f"{avc.LARGE_GAME}/uniform", f"{avc.LARGE_GAME}/random"]
    assert names == want
    for g in avc.SMALL_GAMES:
        joined = "\n".join(avc.keys_of(v, g)).encode()
        assert bytes(v[f"{g}/keys_sha256"]) == hashlib.sha256(joined).digest()
        assert avc.keys_of(v, g) == sorted(avc.keys_of(v, g))


def test_uniform_root_values_are_the_known_ones(v):
    known = {"kuhn_poker": [0.125, -0.125], "leduc_poker": [-0.078125, 0.078125],
             "kuhn_poker(players=3)": [0.234375, -0.046875, -0.1875],
             avc.LARGE_GAME: [-0.15861304, -0.01909722, 0.17771026]}
    for g, want in known.items():
        np.testing.assert_allclose(v[f"{g}/uniform/root_values"], want, rtol=0, atol=5e-9)


def test_policy_weighted_values_add_up_to_the_value_mass(v):
    """sum_a pi[i, a] * weighted[i, a, q] is the infostate's value mass sum_h reach(h) * v_q(h).  For the acting player it
    equals reach[i] * sum_a pi[i, a] * q[i, a]; and over the rows of player 0's first decision in kuhn_poker (one card,
    no betting yet: every deal passes through exactly one of them) the masses add up to the root values."""
    for c in _small_cases(v):
        game = bytes(v[f"{c}/game"]).decode()
        if int(v[f"{c}/responder"]) >= 0:
            continue
        pol = avc.case_policy(v, c)
        player, reach = v[f"{game}/player"], v[f"{c}/reach"]
        w = v[f"{c}/weighted_values"]
        mass = np.einsum("ia,iaq->iq", pol, w)                    # [I, P]: sum_h reach(h) v_q(h)
        own = mass[np.arange(len(player)), player]
        q = v[f"{c}/action_values"]
        np.testing.assert_allclose((pol * q).sum(axis=1) * reach, own, rtol=0, atol=1e-12)
        if game.startswith("kuhn_poker"):   # the rows of player 0's first decision: a single card, no betting yet
            first = [i for i, k in enumerate(avc.keys_of(v, game)) if player[i] == 0 and len(k) == 1]
            assert len(first) == int(v[f"{game}/num_players"]) + 1
            np.testing.assert_allclose(mass[first].sum(axis=0), v[f"{c}/root_values"], rtol=0, atol=1e-12)


def test_reach_is_player_reach_times_counterfactual_reach(v):
    for c in _small_cases(v):
        np.testing.assert_allclose(v[f"{c}/reach"], v[f"{c}/player_reach"] * v[f"{c}/cf_reach"], rtol=0, atol=1e-12)
    c = f"{avc.LARGE_GAME}/uniform"
    np.testing.assert_allclose(v[f"{c}/reach"], v[f"{c}/player_reach"] * v[f"{c}/cf_reach"], rtol=0, atol=1e-12)
    c = f"{avc.LARGE_GAME}/random"
    np.testing.assert_allclose(v[f"{c}/reach_rows"], v[f"{c}/player_reach_rows"] * v[f"{c}/cf_reach_rows"], rtol=0, atol=1e-12)


def test_root_values_are_zero_sum(v):
    for c in avc.case_names(v):
        assert abs(v[f"{c}/root_values"].sum()) <= 1e-12, c


def test_the_responder_gets_its_best_response_value(v):
    seen = 0
    for c in avc.case_names(v):
        b = int(v[f"{c}/responder"])
        if b < 0:
            continue
        seen += 1
        game = bytes(v[f"{c}/game"]).decode()
        assert abs(float(v[f"{c}/best_response_value"]) - v[f"{c}/root_values"][b]) <= 1e-12, c
        player, best, nact = v[f"{game}/player"], v[f"{c}/best_index"], v[f"{game}/nact"]
        assert ((best >= 0) == (player == b)).all() and (best < nact).all()
        # Calculator's own three fields are the walk's, at the rows of the player who plays the table
        rows = player == 1 - b
        assert np.array_equal(v[f"{c}/values_vs_br"], v[f"{c}/action_values"][rows])
        assert np.array_equal(v[f"{c}/counterfactual_reach_probs_vs_br"], v[f"{c}/cf_reach"][rows])
        assert np.array_equal(v[f"{c}/player_reach_probs_vs_br"], v[f"{c}/player_reach"][rows])
    assert seen == 8


def test_an_infostate_has_more_members_than_a_wavefront_has_lanes(v):
    g = "kuhn_poker(players=5)"
    counts = np.diff(v[f"{g}/mem_off"])
    assert int(v[f"{g}/max_members"]) == counts.max() == 120   # more than 64, and no multiple of 64
    assert counts.max() > 64 and counts.max() % 64 != 0


def test_leduc_has_rows_whose_legal_actions_are_not_the_first_ids(v):
    legal, nact = v["leduc_poker/legal"], v["leduc_poker/nact"]
    kinds = {tuple(legal[i, :nact[i]]) for i in range(len(nact))}
    assert (0, 1) in kinds and (1, 2) in kinds and (0, 1, 2) in kinds
    assert int(v["leduc_poker/num_distinct_actions"]) == 3


def test_recorded_argmax_margins(v):
    """Every argmax is decided by 1e-9 or more; where an action ties with the chosen one it does so history by history
    (`ties`), in any order of summation."""
    for c in avc.case_names(v):
        if int(v[f"{c}/responder"]) >= 0:
            assert float(v[f"{c}/margin"]) >= 1e-9, c
            assert int(v[f"{c}/ties"]) >= 0


def test_flattened_tree_is_consistent(v):
    for g in avc.SMALL_GAMES:
        nchild, kind, info = v[f"{g}/nchild"], v[f"{g}/kind"], v[f"{g}/info"]
        H = int(v[f"{g}/histories"])
        assert len(nchild) == H == 1 + nchild.sum()
        assert ((kind == 2) == (nchild == 0)).all() and (kind == 2).sum() == len(v[f"{g}/term_ret"])
        mem, mem_off = v[f"{g}/mem"], v[f"{g}/mem_off"]
        assert sorted(mem) == list(np.nonzero(kind == 1)[0])
        for i in range(len(mem_off) - 1):
            assert (info[mem[mem_off[i]:mem_off[i + 1]]] == i).all()
    assert int(v["kuhn_poker/histories"]) == 58 and int(v["leduc_poker/histories"]) == 9457
