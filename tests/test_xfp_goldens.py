"""tests/golden/xfp_vectors.npz (the trajectories of the reference's own fictitious_play.py, tests/golden/make_xfp_vectors.py)
against a NumPy restatement of the averaging pass: the reach chain over pred_info / pred_action, multiplied root to leaf
from 1.0, and the update expression in the reference's order of operations.  Reaches and the next policy must come out
bit for bit, for every recorded iteration of the three games: this pins the arithmetic order the kernels implement
(open_spiel_amd/csrc/osg_xfp.h).  It also asserts what is known about ties between best-response actions, which decides
which iterations the device tests may run freely."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = {"kuhn_poker": (12, 120), "kuhn_poker(players=3)": (48, 40), "leduc_poker": (936, 25)}
# kuhn_poker: the iterations up to 120 with an exact tie or a tie at rounding level between best-response actions
KUHN_INDECISIVE = [1, 2, 3, 4, 5, 8, 13, 21, 23, 25, 33, 42, 48, 52, 59, 65, 72, 96, 108]
DECISIVE_GAP = 1e-9


@pytest.fixture(scope="module")
def vectors():
    with np.load(os.path.join(ROOT, "tests", "golden", "xfp_vectors.npz")) as z:
        return {k: z[k] for k in z.files}


def chains(pred_info, pred_action):
    """Per infostate the (row, action index) pairs of the same player's earlier decisions, root to leaf."""
    out = []
    for i in range(len(pred_info)):
        chain, j = [], i
        while pred_info[j] >= 0:
            chain.append((int(pred_info[j]), int(pred_action[j])))
            j = pred_info[j]
        out.append(chain[::-1])
    return out


def reaches(chain_of, policy, best):
    avg, br = np.ones(len(chain_of)), np.ones(len(chain_of))
    for i, chain in enumerate(chain_of):
        a_reach, b_reach = 1.0, 1.0
        for row, a in chain:   # root to leaf, from 1.0
            a_reach = a_reach * float(policy[row, a])
            b_reach = b_reach * (1.0 if best[row] == a else 0.0)
        avg[i], br[i] = a_reach, b_reach
    return avg, br


def update(policy, nact, best, alpha, avg_reach, br_reach):
    new = np.zeros_like(policy)
    for i, n in enumerate(nact):
        for a in range(n):
            avg, br = float(policy[i, a]), 1.0 if best[i] == a else 0.0
            new[i, a] = avg + (alpha * br_reach[i] * (br - avg)) / ((1.0 - alpha) * avg_reach[i] + alpha * br_reach[i])
    return new


def uniform(nact, amax):
    return np.array([[1.0 / n if a < n else 0.0 for a in range(amax)] for n in nact])


@pytest.mark.parametrize("game", list(GAMES))
def test_layout(vectors, game):
    infostates, iterations = GAMES[game]
    keys = bytes(vectors[f"{game}/keys"]).decode().split("\n")
    assert len(keys) == infostates and keys == sorted(keys)
    nact, player = vectors[f"{game}/nact"], vectors[f"{game}/player"]
    pred_info, pred_action = vectors[f"{game}/pred_info"], vectors[f"{game}/pred_action"]
    assert vectors[f"{game}/policy"].shape == (iterations, infostates, nact.max())
    assert vectors[f"{game}/br"].shape == (iterations, infostates)
    assert ((vectors[f"{game}/br"] >= 0) & (vectors[f"{game}/br"] < nact[None, :])).all()
    has = pred_info >= 0
    assert (pred_action[~has] == -1).all() and (~has).sum() >= int(player.max()) + 1
    assert (player[pred_info[has]] == player[has]).all()              # own-player predecessor
    assert (pred_action[has] < nact[pred_info[has]]).all() and (pred_action[has] >= 0).all()


@pytest.mark.parametrize("game", list(GAMES))
def test_restatement_reproduces_every_recorded_iteration_bit_for_bit(vectors, game):
    infostates, iterations = GAMES[game]
    nact = vectors[f"{game}/nact"]
    chain_of = chains(vectors[f"{game}/pred_info"], vectors[f"{game}/pred_action"])
    policy = uniform(nact, nact.max())
    for t in range(1, iterations + 1):
        best = vectors[f"{game}/br"][t - 1]
        avg_reach, br_reach = reaches(chain_of, policy, best)
        assert np.array_equal(avg_reach, vectors[f"{game}/avg_reach"][t - 1]), (game, t)
        assert np.array_equal(br_reach, vectors[f"{game}/br_reach"][t - 1]), (game, t)
        policy = update(policy, nact, best, 1 / (t + 1), avg_reach, br_reach)
        want = vectors[f"{game}/policy"][t - 1]
        assert np.array_equal(policy, want), (game, t, float(np.abs(policy - want).max()))
        policy = want
    sums = vectors[f"{game}/policy"].sum(axis=2)
    assert np.abs(sums - 1.0).max() <= 1e-10   # the reference's own assertion (fictitious_play.py:239-240)


def test_ties_and_gaps_are_as_measured(vectors):
    """Which iterations are decisive: zero exact ties and a smallest gap >= 1e-9 between the best and the second-best
    counterfactual-weighted action value, over the infostates with non-zero counterfactual reach."""
    ties, gap = vectors["leduc_poker/ties"], vectors["leduc_poker/min_gap"]
    assert (ties == 0).all() and 4.55e-5 < gap.min() < 4.65e-5, (ties, gap.min())
    ties, gap = vectors["kuhn_poker(players=3)/ties"], vectors["kuhn_poker(players=3)/min_gap"]
    assert ties[0] == 3 and (ties[1:] == 0).all() and 9.2e-5 < gap[1:].min() < 9.35e-5, (ties, gap[1:].min())
    ties, gap = vectors["kuhn_poker/ties"], vectors["kuhn_poker/min_gap"]
    indecisive = [t + 1 for t in range(120) if ties[t] > 0 or gap[t] < DECISIVE_GAP]
    assert indecisive == KUHN_INDECISIVE
    for t in KUHN_INDECISIVE:   # an exact tie, or a gap of rounding size: nothing in between
        assert ties[t - 1] > 0 or gap[t - 1] < 1e-15, (t, ties[t - 1], gap[t - 1])
    decisive = [t for t in range(1, 121) if t not in KUHN_INDECISIVE]
    assert gap[np.array(decisive) - 1].min() > 1e-5
    for game in GAMES:   # every infostate is reached counterfactually: the average policy never loses support
        assert vectors[f"{game}/cf_nonzero"].all()


def test_reference_nash_conv(vectors):
    want = {"leduc_poker": {10: 2.3475, 20: 1.5545, 25: 1.2654}, "kuhn_poker(players=3)": {1: 1.0755, 40: 0.1342},
            "kuhn_poker": {1: 0.625, 30: 0.0833, 120: 0.0461}}
    for game, at in want.items():
        for t, value in at.items():
            assert abs(float(vectors[f"nash_conv/{game}/{t}"]) - value) < 5e-5, (game, t)
