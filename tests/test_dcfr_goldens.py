"""tests/golden/dcfr_vectors.npz (tests/golden/make_dcfr_vectors.py): every checkpoint the device tests compare against
is there, with consistent shapes and keys; and, where the reference sources are present, re-running the reference's own
discounted_cfr.py reproduces a sample of the checkpoints exactly and satisfies the reference's own literal
(discounted_cfr_test.py:27-37)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_dcfr_vectors", os.path.join(GOLDEN, "make_dcfr_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _generator()


@pytest.fixture(scope="module")
def vectors():
    path = os.path.join(GOLDEN, "dcfr_vectors.npz")
    assert os.path.getsize(path) < 313277, "the file must stay below the largest golden there was before it"
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _keys(vectors, game):
    return bytes(vectors[f"{game}/keys"]).decode().split("\n")


def test_every_listed_checkpoint_is_recorded(gen, vectors):
    want = {
        ("kuhn_poker", "D"): [1, 2, 3, 5, 10, 100, 101, 1000, 1001],
        ("kuhn_poker", "L"): [1, 2, 3, 5, 10], ("kuhn_poker", "X"): [1, 2, 3, 5, 10],
        ("kuhn_poker(players=3)", "D"): [1, 2, 3, 5, 10, 100, 101],
        ("kuhn_poker(players=3)", "L"): [1, 2, 3, 5, 10], ("kuhn_poker(players=3)", "X"): [1, 2, 3, 5, 10],
        ("leduc_poker", "D"): [1, 2, 3, 5, 10, 50, 51, 100, 101],
        ("leduc_poker", "L"): [1, 5, 10], ("leduc_poker", "X"): [1, 5, 10],
    }
    assert {(g, n): cps for g, n, cps in gen.RUNS} == want
    assert gen.SETS == {"D": (1.5, 0, 2), "L": (1, 1, 1), "X": (1.5, 0.5, 3)}
    assert gen.STEPS == {"kuhn_poker": [100, 1000], "kuhn_poker(players=3)": [100], "leduc_poker": [50, 100]}
    tables = set()
    for (game, name), checkpoints in want.items():
        for t in checkpoints:
            for what in ("regrets", "cum_policy"):
                assert f"{game}/{name}/{t}/{what}" in vectors, (game, name, t, what)
                tables.add(f"{game}/{name}/{t}/{what}")
    meta = {f"{g}/{m}" for g in gen.INFOSTATES for m in ("keys", "nact", "legal")}
    assert set(vectors) == tables | meta | {"nash_conv/kuhn_poker/300", "nash_conv/leduc_poker/100"}
    assert sum(1 for k in tables if k.startswith("leduc_poker/") and k.endswith("/regrets")) == 15


@pytest.mark.parametrize("game,infostates,amax", [("kuhn_poker", 12, 2), ("kuhn_poker(players=3)", 48, 2), ("leduc_poker", 936, 3)])
def test_shapes_and_keys_are_consistent(vectors, game, infostates, amax):
    keys = _keys(vectors, game)
    assert len(keys) == infostates == len(set(keys)) and keys == sorted(keys)
    nact, legal = vectors[f"{game}/nact"], vectors[f"{game}/legal"]
    assert nact.shape == (infostates,) and legal.shape == (infostates, amax) and nact.max() == amax and nact.min() >= 1
    for i in range(infostates):
        row = legal[i, :nact[i]].tolist()
        assert row == sorted(set(row)) and not legal[i, nact[i]:].any()
    pad = np.arange(amax)[None, :] >= nact[:, None]
    for k, v in vectors.items():
        if k.startswith(game + "/") and k.endswith(("/regrets", "/cum_policy")):
            assert v.shape == (infostates, amax) and v.dtype == np.float64 and np.isfinite(v).all(), k
            assert not v[pad].any(), k
            if k.endswith("/cum_policy"):
                assert (v >= 0).all(), k


def test_recorded_tables_are_discounted_tables(vectors):
    """Cheap sanity of the content itself: after iteration 1 every regret was multiplied by 1/2 whatever the exponents
    (1**x / (1**x + 1)), so the three parameter sets agree at T = 1 and differ afterwards; the cumulative policy of a
    row sums to the weighted reach it accumulated, which grows with gamma."""
    for game in ("kuhn_poker", "kuhn_poker(players=3)", "leduc_poker"):
        d1, l1, x1 = (vectors[f"{game}/{n}/1/regrets"] for n in "DLX")
        assert np.array_equal(d1, l1) and np.array_equal(d1, x1)
        assert np.array_equal(vectors[f"{game}/D/1/cum_policy"], vectors[f"{game}/L/1/cum_policy"])
        assert not np.array_equal(vectors[f"{game}/D/5/regrets"], vectors[f"{game}/L/5/regrets"])
        assert vectors[f"{game}/X/10/cum_policy"].sum() > vectors[f"{game}/D/10/cum_policy"].sum() > vectors[f"{game}/L/10/cum_policy"].sum()
    assert 1.3e-3 < float(vectors["nash_conv/kuhn_poker/300"]) < 1.5e-3     # the issue's table: 1.39e-3
    assert 0.0150 < float(vectors["nash_conv/leduc_poker/100"]) < 0.0160    # 0.0155


@pytest.fixture(scope="module")
def reference_gen(gen, reference):
    if not reference.sources_present():
        pytest.skip("needs the reference sources")
    return gen


@pytest.mark.parametrize("game,name,checkpoints", [
    ("kuhn_poker", "D", [1, 10, 100, 101]), ("kuhn_poker", "L", [3, 10]), ("kuhn_poker(players=3)", "X", [2, 5]),
    ("leduc_poker", "D", [1, 2]),
])
def test_rerunning_the_reference_reproduces_the_checkpoints(reference_gen, vectors, game, name, checkpoints):
    keys, legal, tabs, _ = reference_gen.reference_run(game, reference_gen.SETS[name], checkpoints)
    assert keys == _keys(vectors, game)
    assert [len(l) for l in legal] == vectors[f"{game}/nact"].tolist()
    for t in checkpoints:
        assert np.array_equal(tabs[t][0], vectors[f"{game}/{name}/{t}/regrets"]), (game, name, t)
        assert np.array_equal(tabs[t][1], vectors[f"{game}/{name}/{t}/cum_policy"]), (game, name, t)


def test_the_reference_literal_holds_on_its_own_run(reference_gen, vectors):
    """discounted_cfr_test.py:27-37: 300 iterations of DCFRSolver on kuhn_poker, the average policy's value within 1e-3
    of (-1/18, 1/18); the same run passes through the recorded checkpoints and ends at the recorded NashConv."""
    pyspiel, discounted_cfr, exploitability, expected_game_score = reference_gen.reference_modules()
    game = pyspiel.load_game("kuhn_poker")
    solver = discounted_cfr.DCFRSolver(game)
    keys, legal = reference_gen.layout(solver)
    for t in range(1, 301):
        solver.evaluate_and_update_policy()
        if t in (5, 101):
            reg, cum = reference_gen.tables(solver, keys, legal)
            assert np.array_equal(reg, vectors[f"kuhn_poker/D/{t}/regrets"])
            assert np.array_equal(cum, vectors[f"kuhn_poker/D/{t}/cum_policy"])
    average_policy = solver.average_policy()
    values = expected_game_score.policy_value(game.new_initial_state(), [average_policy] * 2)
    np.testing.assert_allclose(values, [-1 / 18, 1 / 18], atol=1e-3)
    assert exploitability.nash_conv(game, average_policy, use_cpp_br=False) == float(vectors["nash_conv/kuhn_poker/300"])
