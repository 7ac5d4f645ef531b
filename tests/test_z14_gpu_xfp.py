"""Extensive-form fictitious play on the device (osg_xfp_iterate / osg_xfp_update / osg_xfp_reaches; XFPSolver) against
the trajectories the reference's own fictitious_play.py left in tests/golden/xfp_vectors.npz
(tests/golden/make_xfp_vectors.py).

Pin for the policy table: |device - reference| <= 1e-12, the project's pin for CFR tables (tests/test_gpu_cfr.py);
probabilities are <= 1, so it is absolute.  The order of operations is fixed (open_spiel_amd/csrc/osg_xfp.h), so bit
identity is the expectation; every test prints the worst deviation it saw, and whether it was 0, before it asserts.

The trajectory depends on argmax decisions.  A run that computes its own best responses is compared only over
iterations for which the goldens record zero exact ties and a smallest gap >= 1e-9 between the best and the second-best
action value (asserted from the file first); any other iteration is fed the reference's best response through update()."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = 1e-12
DECISIVE_GAP = 1e-9
KUHN3 = "kuhn_poker(players=3)"

# the form each general_kernel= value must take on each game, as osg_cfr_last_kernel names it
FORMS = {
    "kuhn_poker": [({}, "k_xfp_small"), (dict(general_kernel=True), "k_xfp<k_policy_eval>"),
                   (dict(general_kernel="grid"), "k_xfp<k_geval>")],
    KUHN3: [({}, "k_xfp_small"), (dict(general_kernel=True), "k_xfp<k_policy_eval>"),
            (dict(general_kernel="grid"), "k_xfp<k_geval>")],
    "leduc_poker": [({}, "k_xfp<k_eval_jobs>"), (dict(general_kernel=True), "k_xfp<k_policy_eval>"),
                    (dict(general_kernel="grid"), "k_xfp<k_geval>")],
}


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


@pytest.fixture(scope="module")
def vectors():
    with np.load(os.path.join(ROOT, "tests", "golden", "xfp_vectors.npz")) as z:
        return {k: z[k] for k in z.files}


class Golden:
    """The goldens of one game in the device solver's row order."""

    def __init__(self, vectors, solver, game):
        dev = solver.tables()
        keys = bytes(vectors[f"{game}/keys"]).decode().split("\n")
        where = {k: i for i, k in enumerate(keys)}
        assert sorted(dev["keys"]) == keys
        self.order = np.array([where[k] for k in dev["keys"]])
        self.nact = dev["nact"]
        assert np.array_equal(self.nact, vectors[f"{game}/nact"][self.order])
        self.used = np.arange(dev["legal"].shape[1])[None, :] < self.nact[:, None]
        assert np.array_equal(dev["legal"][self.used], vectors[f"{game}/legal"][self.order][self.used])
        self.v, self.game = vectors, game

    def policy(self, t):
        if t == 0:
            return np.where(self.used, 1.0 / self.nact[:, None], 0.0)
        return self.v[f"{self.game}/policy"][t - 1][self.order]

    def best(self, t):
        return self.v[f"{self.game}/br"][t - 1][self.order]

    def cf_nonzero(self, t):
        return self.v[f"{self.game}/cf_nonzero"][t - 1][self.order]

    def reaches(self, t):
        return self.v[f"{self.game}/avg_reach"][t - 1][self.order], self.v[f"{self.game}/br_reach"][t - 1][self.order]

    def assert_decisive(self, iterations):
        for t in iterations:
            ties, gap = self.v[f"{self.game}/ties"][t - 1], self.v[f"{self.game}/min_gap"][t - 1]
            assert ties == 0 and gap >= DECISIVE_GAP, (self.game, t, ties, gap)


def _set_iteration(solver, t):
    from open_spiel_amd import _abi
    _abi.check(_abi.lib().osg_cfr_set_iteration(solver._h, t))


def _policy(solver):
    return solver.tables()["cur_policy"]


def _pin(got, want, what, worst):
    d = float(np.abs(got - want).max())
    worst.append(d)
    assert d <= PIN, (what, d)


def _report(what, worst):
    print(f"xfp {what}: worst |device - reference| = {max(worst):.3g} over {len(worst)} checkpoints; "
          f"bit-identical: {max(worst) == 0.0}")


@pytest.mark.parametrize("kwargs,form", FORMS["leduc_poker"])
def test_leduc_from_the_initial_table(ctx, vectors, kwargs, form):
    """1. leduc_poker, iterations 1..25 with the device's own best responses."""
    import open_spiel_amd as osa
    s = osa.XFPSolver(ctx, "leduc_poker", **kwargs)
    g = Golden(vectors, s, "leduc_poker")
    g.assert_decisive(range(1, 26))
    assert np.array_equal(_policy(s), g.policy(0))
    worst = []
    for t in range(1, 26):
        best, _ = s.best_responses()
        reached = g.cf_nonzero(t)
        assert np.array_equal(best[reached], g.best(t)[reached]), ("best response", t, form)
        s.iteration()
        assert s.iterations == t and s.last_kernel() == form
        _pin(_policy(s), g.policy(t), ("leduc_poker", form, t), worst)
        if t in (10, 20, 25):
            nc, want = s.nash_conv(), float(vectors[f"nash_conv/leduc_poker/{t}"])
            print(f"xfp leduc_poker {form} T={t}: NashConv {nc!r}, reference {want!r}, difference {abs(nc - want):.3g}")
            assert abs(nc - want) <= 1e-9, (t, nc, want)
    _report(f"leduc_poker {form} 1..25", worst)


def test_kuhn3_first_iteration_fed_then_free(ctx, vectors):
    """2. kuhn_poker(players=3): iteration 1 has exact ties and takes the reference's best response; 2..40 run freely.
    The fused and the general forms, bit-identical with each other."""
    import open_spiel_amd as osa
    tables = {}
    for kwargs, form in FORMS[KUHN3]:
        s = osa.XFPSolver(ctx, KUHN3, **kwargs)
        g = Golden(vectors, s, KUHN3)
        g.assert_decisive(range(2, 41))
        worst = []
        s.update(g.best(1))
        assert s.iterations == 1 and s.last_kernel() == "k_xfp_update"
        _pin(_policy(s), g.policy(1), (KUHN3, form, 1), worst)
        tables[form] = [_policy(s)]
        for t in range(2, 41):
            s.iteration()
            assert s.iterations == t and s.last_kernel() == form
            tables[form].append(_policy(s))
            _pin(tables[form][-1], g.policy(t), (KUHN3, form, t), worst)
        nc, want = s.nash_conv(), float(vectors[f"nash_conv/{KUHN3}/40"])
        print(f"xfp {KUHN3} {form} T=40: NashConv {nc!r}, reference {want!r}")
        assert abs(nc - want) <= 1e-9
        _report(f"{KUHN3} {form} 1..40", worst)
    first = FORMS[KUHN3][0][1]
    for form in tables:
        for t, (a, b) in enumerate(zip(tables[first], tables[form]), 1):
            assert np.array_equal(a, b), (first, form, t)


def test_kuhn_every_iteration_with_the_reference_best_response(ctx, vectors):
    """3a. kuhn_poker: all 120 iterations through update(golden best response): the averaging arithmetic alone."""
    import open_spiel_amd as osa
    s = osa.XFPSolver(ctx, "kuhn_poker")
    g = Golden(vectors, s, "kuhn_poker")
    worst = []
    for t in range(1, 121):
        s.update(g.best(t))
        assert s.iterations == t
        _pin(_policy(s), g.policy(t), ("kuhn_poker update", t), worst)
    nc, want = s.nash_conv(), float(vectors["nash_conv/kuhn_poker/120"])
    print(f"xfp kuhn_poker T=120: NashConv {nc!r}, reference {want!r}")
    assert abs(nc - want) <= 1e-9
    _report("kuhn_poker update 1..120", worst)


@pytest.mark.parametrize("kwargs,form", FORMS["kuhn_poker"])
def test_kuhn_free_steps_where_the_best_response_is_decisive(ctx, vectors, kwargs, form):
    """3b. kuhn_poker: single free steps t - 1 -> t for t = 10, 20, 100 and a free run 14..20 from the reference's policy
    after 13."""
    import open_spiel_amd as osa
    s = osa.XFPSolver(ctx, "kuhn_poker", **kwargs)
    g = Golden(vectors, s, "kuhn_poker")
    g.assert_decisive([10, 20, 100] + list(range(14, 21)))
    worst = []
    for t in (10, 20, 100):
        s.load_tables(cur_policy=g.policy(t - 1))
        _set_iteration(s, t - 1)
        best, _ = s.best_responses()
        assert np.array_equal(best[g.cf_nonzero(t)], g.best(t)[g.cf_nonzero(t)]), ("best response", t)
        s.iteration()
        assert s.iterations == t and s.last_kernel() == form
        _pin(_policy(s), g.policy(t), ("kuhn_poker step", form, t), worst)
    s.load_tables(cur_policy=g.policy(13))
    _set_iteration(s, 13)
    for t in range(14, 21):
        s.iteration()
        _pin(_policy(s), g.policy(t), ("kuhn_poker run from 13", form, t), worst)
    assert s.iterations == 20
    _report(f"kuhn_poker {form} free steps", worst)


@pytest.mark.parametrize("game,at", [("kuhn_poker", [1, 7, 10, 100]), (KUHN3, [1, 2, 17, 40]), ("leduc_poker", [1, 2, 13, 25])])
def test_reaches_equal_the_golden_vectors(ctx, vectors, game, at):
    """4a. reaches() on the reference's policy of t - 1: with the reference's best response, and — where iteration t is
    decisive — with the device's own."""
    import open_spiel_amd as osa
    s = osa.XFPSolver(ctx, game)
    g = Golden(vectors, s, game)
    worst = []
    for t in at:
        s.load_tables(cur_policy=g.policy(t - 1))
        _set_iteration(s, t - 1)
        want_avg, want_br = g.reaches(t)
        before = _policy(s)
        avg, br = s.reaches(g.best(t))
        _pin(avg, want_avg, (game, "avg_reach", t), worst)
        assert np.array_equal(br, want_br), (game, "br_reach", t)
        if vectors[f"{game}/ties"][t - 1] == 0 and vectors[f"{game}/min_gap"][t - 1] >= DECISIVE_GAP:
            avg, br = s.reaches()
            _pin(avg, want_avg, (game, "avg_reach, own best response", t), worst)
            assert np.array_equal(br, want_br), (game, "br_reach, own best response", t)
        assert s.iterations == t - 1 and np.array_equal(_policy(s), before)   # a diagnostic: nothing moved
    _report(f"{game} reaches", worst)


@pytest.mark.parametrize("game", ["kuhn_poker", KUHN3, "leduc_poker"])
def test_batched_iterations_and_forms_are_bit_identical(ctx, game):
    """4b. iterate(k) equals k x iteration(); every form that serves the game gives the same bits (free runs of the
    device against itself: ties resolve the same way in every form)."""
    import open_spiel_amd as osa
    k = 30 if game != "leduc_poker" else 6
    tables = {}
    for kwargs, form in FORMS[game]:
        one, many = osa.XFPSolver(ctx, game, **kwargs), osa.XFPSolver(ctx, game, **kwargs)
        for _ in range(k):
            one.iteration()
        many.iterate(k)
        assert one.iterations == many.iterations == k and many.last_kernel() == form
        tables[form] = _policy(many)
        assert np.array_equal(_policy(one), tables[form]), (game, form)
        t = many.tables()
        assert not t["regrets"].any() and not t["cum_policy"].any()   # regrets and cum_policy are not touched
        many.iterate(0)
        assert many.iterations == k
    first = FORMS[game][0][1]
    for form, table in tables.items():
        assert np.array_equal(tables[first], table), (game, first, form)
    assert np.abs(tables[first].sum(axis=1) - 1.0).max() <= 1e-12


def test_refusals_and_reset(ctx, vectors):
    """5. What osg_xfp_iterate refuses, the out-of-range best response, and reset()."""
    import open_spiel_amd as osa
    from open_spiel_amd import _abi
    lib = _abi.lib()
    best0 = np.zeros(12, np.int32)

    def calls(solver):
        avg, br = np.zeros(12), np.zeros(12)
        return [lambda: lib.osg_xfp_iterate(solver._h, 1), lambda: lib.osg_xfp_update(solver._h, best0.ctypes.data),
                lambda: lib.osg_xfp_reaches(solver._h, None, avg.ctypes.data, br.ctypes.data)]

    for kwargs, code, why in [(dict(mccfr=True), -1, "MCCFR"), (dict(mccfr="outcome"), -1, "MCCFR"),
                              (dict(replicas=4), -2, "replicas"), (dict(discounting=(1.5, 0, 2), linear_averaging=True), -1, "discount")]:
        s = osa.TabularSolver(ctx, "kuhn_poker", **kwargs)
        before = s.tables()["cur_policy"].copy()
        for call in calls(s):
            assert call() == code, (kwargs, code)
            assert why in lib.osg_last_error().decode(), (kwargs, lib.osg_last_error().decode())
        assert s.iteration == 0 and np.array_equal(s.tables()["cur_policy"], before)
    assert lib.osg_xfp_iterate(None, 1) == -1 and lib.osg_xfp_update(None, None) == -1

    s = osa.XFPSolver(ctx, "kuhn_poker")
    g = Golden(vectors, s, "kuhn_poker")
    s.update(g.best(1))
    s.update(g.best(2))
    before = _policy(s)
    for bad_row, bad in [(3, 2), (0, -1), (11, 7)]:
        best = g.best(3).copy()
        best[bad_row] = bad
        with pytest.raises(osa.OsgError, match="osg error -1.*osg_xfp_update.*out of range"):
            s.update(best)
        with pytest.raises(osa.OsgError, match="osg error -1.*osg_xfp_reaches.*out of range"):
            s.reaches(best)
        assert s.iterations == 2 and np.array_equal(_policy(s), before)   # table and counter untouched
    with pytest.raises(osa.OsgError, match="one per information state"):
        s.update(np.zeros(5, np.int32))
    with pytest.raises(osa.OsgError, match="fictitious play"):
        s.evaluate_and_update_policy()
    with pytest.raises(osa.OsgError, match="osg_xfp_iterate: bad argument"):
        s.iterate(-1)
    s.update(g.best(3))   # still usable after the refusals
    assert np.abs(_policy(s) - g.policy(3)).max() <= PIN
    s.reset()
    assert s.iterations == 0 and np.array_equal(_policy(s), g.policy(0))
    tables = s.average_policy_tables()
    assert len(tables) == 2 and sum(len(t) for t in tables) == 12 and tables[0]["0"] == {0: 0.5, 1: 0.5}
    assert s.average_policy()["0"] == [(0, 0.5), (1, 0.5)]


def test_leduc3_smoke(ctx):
    """6. leduc_poker(players=3), on the device alone (the reference takes hours there): 3 iterations."""
    import open_spiel_amd as osa
    s = osa.XFPSolver(ctx, "leduc_poker(players=3)")
    s.iterate(2)
    s.iteration()
    assert s.iterations == 3 and s.last_kernel() == "k_xfp<k_geval>"
    policy = _policy(s)
    rows = np.abs(policy.sum(axis=1) - 1.0).max()
    print(f"xfp leduc_poker(players=3): {s.num_infostates} infostates, worst |row sum - 1| = {rows:.3g}")
    assert rows <= 1e-12 and (policy >= 0).all()
    ev = s.evaluate_policy("current")
    assert np.isfinite(ev["nash_conv"]) and ev["nash_conv"] > 0
    assert s.nash_conv() == ev["nash_conv"]
    best, values = s.best_responses()
    assert best.shape == (s.num_infostates,) and (best >= 0).all() and (best < s.tables()["nact"]).all()
    assert np.array_equal(values, ev["best_response_values"])
