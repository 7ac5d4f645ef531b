"""tests/golden/mmd_vectors.npz (the trajectories of the reference's own mmd_dilated.py, tests/golden/make_mmd_vectors.py)
checked against itself, and regenerated where the reference tree is present."""
import os
import sys

import numpy as np
import pytest

import mmd_cases

ROOT = mmd_cases.ROOT


@pytest.fixture(scope="module")
def v():
    return mmd_cases.load()


def test_file_is_small_and_complete(v):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mmd_vectors.npz")) < 300 * 1024
    assert mmd_cases.run_names(v) == ["kuhn_a0.1", "kuhn_a0", "kuhn_a1", "kuhn_anneal", "leduc_a0.05", "leduc_a0"]
    assert list(v["kuhn_a0.1/t"]) == [1, 2, 10, 100, 400] and list(v["kuhn_a0/t"]) == [1, 10, 100]
    assert list(v["kuhn_a1/t"]) == [100] and list(v["kuhn_anneal/t"]) == [20, 40, 60]
    assert list(v["leduc_a0.05/t"]) == [1, 10, 30] and list(v["leduc_a0/t"]) == [20]
    assert list(v["kuhn_anneal/alpha"]) == [0.5, 0.1, 0.02] and v["kuhn_anneal/stepsize"][2] == 0.5
    assert v["kuhn_poker/default_stepsize/0.1"] == pytest.approx(0.9, abs=1e-15)
    assert float(v["leduc_poker/default_stepsize/0.05"]) == 4.260355029585798
    assert v["kuhn_poker/legal"].shape == (12, 2) and v["leduc_poker/legal"].shape == (936, 3)


@pytest.mark.parametrize("game", mmd_cases.GAMES)
def test_layout_is_a_sequence_form(v, game):
    I, A = v[f"{game}/legal"].shape
    pred, act, player, rank = (v[f"{game}/{n}"] for n in ("pred_info", "pred_action", "player", "bfs_rank"))
    assert sorted(rank) == list(range(I))
    for i in range(I):
        if pred[i] >= 0:
            assert player[pred[i]] == player[i] and 0 <= act[i] < v[f"{game}/nact"][pred[i]] and rank[pred[i]] < rank[i]
    seq = v[f"{game}/term_seq"]
    assert seq.min() >= 0 and seq.max() < I * A          # both players act before every terminal of these games
    assert (player[seq[:, 0] // A] == 0).all() and (player[seq[:, 1] // A] == 1).all()
    assert np.abs(v[f"{game}/term_cu"].sum(axis=1)).max() <= 1e-15    # zero-sum
    for p in range(2):   # every sequence id maps to a distinct cell of that player's
        m = v[f"{game}/seq_map{p}"]
        assert tuple(m[0]) == (-1, -1) and (player[m[1:, 0]] == p).all()
        assert len({tuple(r) for r in m[1:]}) == len(m) - 1 == int(v[f"{game}/nact"][player == p].sum())


@pytest.mark.parametrize("run", ["kuhn_a0.1", "kuhn_a0", "kuhn_a1", "kuhn_anneal", "leduc_a0.05", "leduc_a0", "qre"])
def test_sequences_sum_to_their_parent(v, run):
    game = "kuhn_poker" if run == "qre" else bytes(v[f"{run}/game"]).decode()
    pred, act, nact = v[f"{game}/pred_info"], v[f"{game}/pred_action"], v[f"{game}/nact"]
    # (the QRE itself is 8-digit data, so only what the reference rebuilt from a policy is a sequence form to the last digit)
    tables = [v["qre/x_after"]] if run == "qre" else list(v[f"{run}/x"]) + list(v[f"{run}/avg_x"])
    for x in tables:
        parent = np.where(pred >= 0, x[np.maximum(pred, 0), np.maximum(act, 0)], 1.0)
        assert np.abs(x.sum(axis=1) - parent).max() <= 1e-14
        assert (x[np.arange(x.shape[1])[None, :] >= nact[:, None]] == 0).all()
    if run != "qre":
        for x, pi in zip(v[f"{run}/x"], v[f"{run}/pi"]):
            parent = np.where(pred >= 0, x[np.maximum(pred, 0), np.maximum(act, 0)], 1.0)
            assert np.abs(pi * parent[:, None] - x).max() <= 1e-15
            assert np.abs(pi.sum(axis=1) - 1).max() <= 1e-15


def test_gap_falls_and_nothing_rests_on_underflow(v):
    for run in ("kuhn_a0.1", "leduc_a0.05"):   # alpha > 0, constant parameters
        gap = v[f"{run}/gap"]
        assert (np.diff(gap) < 0).all() and gap[-1] >= 0, (run, gap)
    assert abs(v["kuhn_a1/gap"][0]) <= 1e-15
    assert np.isnan(v["kuhn_a0/gap"]).all() and np.isnan(v["leduc_a0/gap"]).all()
    for run in mmd_cases.run_names(v):
        assert v[f"{run}/min_seq"].min() > 1e-300, run
        assert (np.diff(v[f"{run}/min_seq"]) <= 0).all()


def test_the_qre_is_a_fixed_point_by_the_reference_bounds(v):
    """mmd_dilated_test.py:95-109: one update moves it by less than rtol 1e-6, and its gap is <= 1e-6."""
    np.testing.assert_allclose(v["qre/x_after"], v["qre/x"], rtol=1e-6, atol=0)
    assert abs(v["qre/gap"]) <= 1e-6
    for p in range(2):
        m = v[f"kuhn_poker/seq_map{p}"]
        assert np.array_equal(v["qre/x"][m[1:, 0], m[1:, 1]], v[f"qre/seq{p}"][1:]) and v[f"qre/seq{p}"][0] == 1.0


def test_regenerated_kuhn_run_equals_the_file(v):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        pytest.skip("needs the reference sources")
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_mmd_vectors
    fresh = make_mmd_vectors.main(only=["kuhn_a0.1"])
    for k in [k for k in fresh if k.startswith(("kuhn_a0.1/", "kuhn_poker/"))]:
        if k == "kuhn_poker/default_stepsize/0.1" or not k.startswith("kuhn_poker/default_stepsize/"):
            # (the reference's BLAS may sum in another order on another CPU: floats within the bound, the rest equal)
            if fresh[k].dtype == np.float64:
                np.testing.assert_allclose(fresh[k], v[k], rtol=0, atol=mmd_cases.TOLERANCE, equal_nan=True, err_msg=k)
            else:
                assert np.array_equal(fresh[k], v[k]), k
