"""The device tabular solvers on the accepted poker variants against the reference's own runs recorded in
tests/golden/variant_*_vectors.npz (tests/golden/make_solver_variant_vectors.py):

  G1 leduc_poker(suit_isomorphism=True)   G2 leduc_poker(action_mapping=True)   G3 leduc_poker(starting_player=1)
  G4 leduc_poker(action_mapping=True,suit_isomorphism=True,starting_player=1)   G5 kuhn_poker(players=4)

One test per (family, game, kernel form); every comparator and bound is the one of the family's own device test, imported
or restated from it, none new:
  DCFR / LCFR   |device - reference| <= 1e-12 of the table's scale, tests/test_z13_gpu_dcfr.py
  XFP           |device - reference| <= 1e-12, NashConv within 1e-9, tests/test_z14_gpu_xfp.py
  MMD           mmd_cases.TOLERANCE, NashConv within 1e-10, tests/test_z17_gpu_mmd.py
  EFR           deviation tables exact, R and the three policies within efr_cases.TOLERANCE, tests/test_z27_gpu_efr.py
  action values every output within action_value_cases.TOLERANCE, the best responder's choice equal,
                tests/test_z18_gpu_action_values.py
and the forms that serve a game agree with each other bit for bit.  last_kernel() is asserted in every test, so the form
each game takes is on record (FORMS below; G2's 44 527 histories run k_cfr_small<global> where the default game's 9 457
run k_cfr_split, and k_xfp<k_policy_eval> where the default game runs k_xfp<k_eval_jobs>).

Ties: with action_mapping=True "fold" where there is nothing to call is "call", so G2 and G4 have hundreds of exactly
tied best-response actions in EVERY iteration.  XFP is compared there with the reference's best response fed in at every
iteration; free-running only over the iterations the golden marks decisive; and the device's own best responses are
checked for optimality on every game: at every infostate the RECORDED action value (<game>/q of the golden) of the action
the device chose is within the bound of the recorded maximum, whichever tied action it picked.

MMD refuses G2 and G4 (no sequence form: fold and call lead to the same information state of the player who chose; the
reference's own run ends in NaN) and G5 (four players).  EFR refuses G2 and G4 (an information state has several own
histories there, and the regrets between fold and call are rounding noise in the reference's run, so no iteration of
it passes the golden maker's own admission rule).  Populations (profile_returns, payoff_tensors, aggregate_policies,
PSROSolver) and ISMCTS have no recorded run of the reference on the leduc parameters and refuse G1-G4.  The refusals
are pinned with their messages.

Best responses: XFPSolver.best_responses() IS osg_cfr_best_response; action_values(responder=...) is the device side
of action_values_vs_best_response; both are checked for optimality against recorded action values, ties included.
PSROSolver's oracle is refused with PSROSolver on G1-G4.

With OSG_SOLVER_VARIANTS_PROFILE=<path> set, the largest deviation and the form taken per (family, game, form) are
written there at the end of the module (profiles/solver_variants.txt is such a run).  The whole file takes about
4 s on an MI355X (91 tests, measured; 1.8 s of it the context)."""
import os

import numpy as np
import pytest

import efr_cases
import mmd_cases
from test_xfp_goldens import DECISIVE_GAP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G1 = "leduc_poker(suit_isomorphism=True)"
G2 = "leduc_poker(action_mapping=True)"
G3 = "leduc_poker(starting_player=1)"
G4 = "leduc_poker(action_mapping=True,suit_isomorphism=True,starting_player=1)"
G5 = "kuhn_poker(players=4)"
NAMES = {G1: "G1", G2: "G2", G3: "G3", G4: "G4", G5: "G5"}
HISTORIES = {G1: 1939, G2: 44527, G3: 9457, G4: 8992, G5: 7886}
PIN = 1e-12           # tests/test_z13_gpu_dcfr.py (of the table's scale) and tests/test_z14_gpu_xfp.py (absolute)
SETS = {"D": (1.5, 0, 2), "L": (1, 1, 1)}
CHECKPOINTS = [1, 2, 10]

# the form every general_kernel= value that changes it takes on each game, as osg_cfr_last_kernel names it
DCFR_FORMS = {
    G1: [({}, "k_cfr_small<global, dcfr>"), (dict(general_kernel="grid"), "k_gcfr<dcfr>"), (dict(general_kernel=True), "k_cfr<dcfr>")],
    G2: [({}, "k_cfr_small<global, dcfr>"), (dict(general_kernel="grid"), "k_gcfr<dcfr>"), (dict(general_kernel=True), "k_cfr<dcfr>"),
         (dict(general_kernel="sub"), "k_cfr_sub<dcfr>")],
    G3: [({}, "k_cfr_split<dcfr>"), (dict(general_kernel="path"), "k_cfr_small<global, dcfr>"), (dict(general_kernel="grid"), "k_gcfr<dcfr>"),
         (dict(general_kernel=True), "k_cfr<dcfr>"), (dict(general_kernel="sub"), "k_cfr_sub<dcfr>")],
    G4: [({}, "k_cfr_small<global, dcfr>"), (dict(general_kernel="grid"), "k_gcfr<dcfr>"), (dict(general_kernel=True), "k_cfr<dcfr>"),
         (dict(general_kernel="sub"), "k_cfr_sub<dcfr>")],
    G5: [({}, "k_cfr_split<dcfr>"), (dict(general_kernel="path"), "k_cfr_small<global, dcfr>"), (dict(general_kernel="grid"), "k_gcfr<dcfr>"),
         (dict(general_kernel=True), "k_cfr<dcfr>"), (dict(general_kernel="sub"), "k_cfr_sub<dcfr>")],
}
XFP_FORMS = {
    G1: [({}, "k_xfp<k_policy_eval>"), (dict(general_kernel="grid"), "k_xfp<k_geval>")],
    G2: [({}, "k_xfp<k_policy_eval>"), (dict(general_kernel="grid"), "k_xfp<k_geval>")],
    G3: [({}, "k_xfp<k_eval_jobs>"), (dict(general_kernel=True), "k_xfp<k_policy_eval>"), (dict(general_kernel="grid"), "k_xfp<k_geval>")],
    G4: [({}, "k_xfp<k_eval_jobs>"), (dict(general_kernel=True), "k_xfp<k_policy_eval>"), (dict(general_kernel="grid"), "k_xfp<k_geval>")],
    G5: [({}, "k_xfp<k_eval_jobs>"), (dict(general_kernel=True), "k_xfp<k_policy_eval>"), (dict(general_kernel="grid"), "k_xfp<k_geval>")],
}
MMD_FORMS = [({}, "k_mmd_small"), (dict(general_kernel=True), "k_mmd")]


def _cases(forms):
    return [pytest.param(g, kw, f, id=f"{NAMES[g]}-{f}") for g, per_game in forms.items() for kw, f in per_game]


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


def _load(family):
    with np.load(os.path.join(ROOT, "tests", "golden", f"variant_{family}_vectors.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dcfr():
    return _load("dcfr")


@pytest.fixture(scope="module")
def xfp():
    return _load("xfp")


@pytest.fixture(scope="module")
def mmd():
    return _load("mmd")


@pytest.fixture(scope="module")
def efr():
    return _load("efr")


@pytest.fixture(scope="module")
def profile():
    """{(family, game, form): (largest deviation, what it is of)}; written out when the module is done."""
    lines = {}
    yield lines
    path = os.environ.get("OSG_SOLVER_VARIANTS_PROFILE")
    if path:
        with open(path, "w") as f:
            f.write("family game form: largest |device - reference| (of what; the bound)\n")
            for (family, game, form), (worst, what) in sorted(lines.items(), key=lambda kv: (kv[0][0], NAMES[kv[0][1]], kv[0][2])):
                f.write(f"{family} {NAMES[game]} {form}: {worst:.3g} ({what})\n")


def _order(v, dev, game):
    """Row of the goldens for every row of the device solver; the layouts must agree."""
    keys = bytes(v[f"{game}/keys"]).decode().split("\n")
    where = {k: i for i, k in enumerate(keys)}
    assert sorted(dev["keys"]) == keys
    order = np.array([where[k] for k in dev["keys"]])
    assert np.array_equal(dev["nact"], v[f"{game}/nact"][order])
    used = np.arange(dev["legal"].shape[1])[None, :] < dev["nact"][:, None]
    assert np.array_equal(dev["legal"][used], v[f"{game}/legal"][order][used])
    return order


# ---- DCFR / LCFR --------------------------------------------------------------------------------------------------------
def _deviation(got, want):
    """tests/test_z13_gpu_dcfr.py: largest |got - want| as a fraction of the table's scale max(1, max |want|)."""
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def _dcfr_run(ctx, game, name, kwargs, form):
    import open_spiel_amd as osa
    s = osa.TabularSolver(ctx, game, linear_averaging=True, discounting=SETS[name], **kwargs)
    assert s.num_histories == HISTORIES[game]
    out = []
    for t in CHECKPOINTS:
        s.evaluate_and_update_policy(t - s.iteration)
        assert s.iteration == t and s.last_kernel() == form
        out.append(s.tables())
    return out


@pytest.fixture(scope="module")
def dcfr_runs(ctx):
    """The tables of (game, set, form) at the checkpoints, computed once and shared by the comparisons."""
    cache = {}

    def get(game, name, kwargs, form):
        if (game, name, form) not in cache:
            cache[(game, name, form)] = _dcfr_run(ctx, game, name, kwargs, form)
        return cache[(game, name, form)]
    return get


@pytest.mark.parametrize("game,kwargs,form", _cases(DCFR_FORMS))
def test_dcfr_and_lcfr_match_the_reference_tables(dcfr, dcfr_runs, profile, game, kwargs, form):
    worst = 0.0
    for name in SETS:
        for t, dev in zip(CHECKPOINTS, dcfr_runs(game, name, kwargs, form)):
            order = _order(dcfr, dev, game)
            d_reg = _deviation(dev["regrets"], dcfr[f"{game}/{name}/{t}/regrets"][order])
            d_cum = _deviation(dev["cum_policy"], dcfr[f"{game}/{name}/{t}/cum_policy"][order])
            print(f"dcfr {NAMES[game]} {name} T={t} {form}: regrets {d_reg:.3g} cum_policy {d_cum:.3g} of the scale")
            worst = max(worst, d_reg, d_cum)
            assert d_reg <= PIN, (game, name, t, form, d_reg)
            assert d_cum <= PIN, (game, name, t, form, d_cum)
    profile[("dcfr", game, form)] = (worst, f"regrets and cum_policy, sets D and L at T = 1, 2, 10, of the table's scale; bound {PIN}")


@pytest.mark.parametrize("game", list(DCFR_FORMS), ids=lambda g: NAMES[g])
def test_dcfr_forms_agree_bit_for_bit(dcfr_runs, game):
    (kw0, first), rest = DCFR_FORMS[game][0], DCFR_FORMS[game][1:]
    for name in SETS:
        want = dcfr_runs(game, name, kw0, first)
        for kwargs, form in rest:
            for t, a, b in zip(CHECKPOINTS, want, dcfr_runs(game, name, kwargs, form)):
                for table in ("regrets", "cum_policy", "cur_policy"):
                    np.testing.assert_array_equal(a[table], b[table], err_msg=f"{game} {name} T={t}: {first} vs {form}: {table}")


# ---- XFP ----------------------------------------------------------------------------------------------------------------
def _optimal(best, q, nact, reached, what):
    """The device's choice is a maximiser of the RECORDED action values q [I, Amax] (the counterfactual-weighted values
    the reference's best response maximised over), at every reached infostate, whichever tied action it is."""
    assert ((best >= 0) & (best < nact)).all(), what
    assert reached.all() and np.isfinite(q[np.arange(q.shape[1])[None, :] < nact[:, None]]).all(), what
    top = np.nanmax(q, axis=1)
    gap = float((top - q[np.arange(len(best)), best]).max())
    assert gap <= PIN, (what, gap)
    return gap


@pytest.mark.parametrize("game,kwargs,form", _cases(XFP_FORMS))
def test_xfp_matches_the_reference_run(ctx, xfp, profile, game, kwargs, form):
    """Iterations 1..10.  A decisive iteration (no exact tie, smallest gap >= DECISIVE_GAP) runs freely and the device's own
    best response must be the recorded one; any other is fed the recorded best response through update(), after the
    device's own best response was checked to be a maximiser."""
    import open_spiel_amd as osa
    s = osa.XFPSolver(ctx, game, **kwargs)
    assert s.num_histories == HISTORIES[game]
    dev = s.tables()
    order = _order(xfp, dev, game)
    nact = dev["nact"]
    used = np.arange(dev["legal"].shape[1])[None, :] < nact[:, None]
    assert np.array_equal(dev["cur_policy"], np.where(used, 1.0 / nact[:, None], 0.0))
    worst, free, tie_rows = 0.0, 0, 0
    for t in range(1, 11):
        decisive = xfp[f"{game}/ties"][t - 1] == 0 and xfp[f"{game}/min_gap"][t - 1] >= DECISIVE_GAP
        want_best = xfp[f"{game}/br"][t - 1][order]
        reached = xfp[f"{game}/cf_nonzero"][t - 1][order]
        best, _ = s.best_responses()
        _optimal(best, xfp[f"{game}/q"][t - 1][order], nact, reached, (game, form, t))
        tie_rows += int((best[reached] != want_best[reached]).sum())
        if decisive:
            assert np.array_equal(best[reached], want_best[reached]), ("best response", game, form, t)
            s.iteration()
            assert s.last_kernel() == form
            free += 1
        else:
            s.update(want_best)
            assert s.last_kernel() == "k_xfp_update"
        assert s.iterations == t
        d = float(np.abs(s.tables()["cur_policy"] - xfp[f"{game}/policy"][t - 1][order]).max())
        worst = max(worst, d)
        assert d <= PIN, (game, form, t, d)
        if t in (1, 2, 5, 10):
            nc, want = s.nash_conv(), float(xfp[f"nash_conv/{game}/{t}"])
            assert abs(nc - want) <= 1e-9, (game, form, t, nc, want)
    assert free == {G1: 10, G2: 0, G3: 10, G4: 0, G5: 9}[game]
    assert tie_rows == 0 or free < 10   # (only an exact tie can be resolved differently from the reference)
    # the evaluation kernel of this form ran in every iteration (best_responses()); a fed game still launches it freely once
    if free == 0:
        s.iteration()
        assert s.last_kernel() == form and s.iterations == 11
    print(f"xfp {NAMES[game]} {form}: worst |device - reference| = {worst:.3g}; {free} free iterations, "
          f"{tie_rows} tied infostates resolved differently from the reference")
    profile[("xfp", game, form)] = (worst, f"policy, iterations 1..10, {free} of them free-running; bound {PIN}")


@pytest.mark.parametrize("game", list(XFP_FORMS), ids=lambda g: NAMES[g])
def test_xfp_forms_agree_bit_for_bit(ctx, game):
    """Free runs of the device against itself: ties resolve the same way in every form."""
    import open_spiel_amd as osa
    tables = {}
    for kwargs, form in XFP_FORMS[game]:
        s = osa.XFPSolver(ctx, game, **kwargs)
        s.iterate(4)
        assert s.last_kernel() == form and s.iterations == 4
        best, values = s.best_responses()
        tables[form] = (s.tables()["cur_policy"], best, values)
    first = XFP_FORMS[game][0][1]
    for form, got in tables.items():
        for a, b in zip(tables[first], got):
            assert np.array_equal(a, b), (game, first, form)


# ---- MMD ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs,form", MMD_FORMS, ids=[f for _, f in MMD_FORMS])
@pytest.mark.parametrize("game", [G1, G3], ids=lambda g: NAMES[g])
def test_mmd_matches_the_reference_run(ctx, mmd, profile, game, kwargs, form):
    """x, avg_x, pi, get_gap() and nash_conv() at every checkpoint of both runs (alpha 0.05 at the default stepsize, and
    alpha 0), as tests/test_z17_gpu_mmd.py compares them."""
    import open_spiel_amd as osa
    worst = {}
    for run in mmd_cases.run_names(mmd, game):
        def stepsize(c):   # None where the segment ran with the reference's default
            key = f"{game}/default_stepsize/{mmd[f'{run}/alpha'][c]}"
            return None if key in mmd and mmd[key] == mmd[f"{run}/stepsize"][c] else float(mmd[f"{run}/stepsize"][c])

        s = osa.MMDSolver(ctx, game, float(mmd[f"{run}/alpha"][0]), stepsize(0), **kwargs)
        back = np.argsort(_order(mmd, s.tables(), game))
        for c in range(len(mmd[f"{run}/t"])):
            alpha = float(mmd[f"{run}/alpha"][c])
            s.set_params(alpha, stepsize(c))
            assert abs(s.stepsize[0] - mmd[f"{run}/stepsize"][c]) <= mmd_cases.TOLERANCE
            s.iterate(int(mmd[f"{run}/iters"][c]))
            assert s.last_kernel() == form and s.iteration == mmd[f"{run}/t"][c]
            t = s.tables()
            got = dict(x=s.current_sequences()[back], avg_x=s.get_avg_sequences()[back], pi=t["cur_policy"][back])
            for name, table in got.items():
                worst[name] = max(worst.get(name, 0.0), float(np.abs(table - mmd[f"{run}/{name}"][c]).max()))
            if alpha > 0:
                worst["gap"] = max(worst.get("gap", 0.0), abs(s.get_gap() - mmd[f"{run}/gap"][c]))
            worst["nash_conv"] = max(worst.get("nash_conv", 0.0), abs(s.nash_conv() - mmd[f"{run}/nash_conv"][c]))
    print(f"mmd {NAMES[game]} {form}: worst |device - reference| " + " ".join(f"{k} {d:.3g}" for k, d in worst.items()))
    for name, d in worst.items():
        assert d <= (1e-10 if name == "nash_conv" else mmd_cases.TOLERANCE), (game, form, name, d)
    tables = max(d for k, d in worst.items() if k != "nash_conv")
    profile[("mmd", game, form)] = (tables, f"x, avg_x, pi and the gap, alpha 0.05 and 0 at T = 1, 10, 20; bound {mmd_cases.TOLERANCE}")


@pytest.mark.parametrize("game", [G1, G3], ids=lambda g: NAMES[g])
def test_mmd_forms_agree_bit_for_bit(ctx, game):
    import open_spiel_amd as osa
    for alpha, eta in ((0.05, None), (0.0, 2.0)):
        got = []
        for kwargs, form in MMD_FORMS:
            s = osa.MMDSolver(ctx, game, alpha, eta, **kwargs)
            s.iterate(10)
            assert s.last_kernel() == form
            got.append((s.current_sequences(), s.get_avg_sequences(), s.tables()["cur_policy"]))
        for a, b in zip(*got):
            assert np.array_equal(a, b), (game, alpha)


@pytest.mark.parametrize("game,why", [(G2, "action_mapping=True has no sequence form"), (G4, "action_mapping=True has no sequence form"),
                                      (G5, "two-player zero-sum games only, this game has 4 players")],
                         ids=["G2", "G4", "G5"])
@pytest.mark.parametrize("kwargs", [{}, dict(general_kernel=True)], ids=["resident", "general"])
def test_mmd_refuses_what_it_cannot_serve(ctx, game, why, kwargs):
    """OSG_ERR_UNSUPPORTED (-2) with a message that names the parameter, from every MMD entry point, in both forms."""
    import open_spiel_amd as osa
    from open_spiel_amd import _abi
    with pytest.raises(osa.OsgError, match="osg error -2: .*" + why):
        osa.MMDSolver(ctx, game, 0.05, **kwargs)
    with pytest.raises(osa.OsgError, match="osg error -2: .*" + why):
        osa.MMDSolver(ctx, game, 0.0, 2.0, **kwargs)
    s = osa.TabularSolver(ctx, game, **kwargs)
    before = s.tables()
    one = np.array([0.05]), np.array([1.0])
    lib = _abi.lib()
    assert lib.osg_mmd_set_params(s._h, 1, one[0].ctypes.data, one[1].ctypes.data) == -2 and why.encode() in lib.osg_last_error()
    assert lib.osg_mmd_iterate(s._h, 1) == -2 and why.encode() in lib.osg_last_error()
    after = s.tables()
    assert all(np.array_equal(before[k], after[k]) for k in ("regrets", "cum_policy", "cur_policy")) and s.iteration == 0
    s.evaluate_and_update_policy(1)   # still the CFR solver it was
    assert s.iteration == 1


# ---- EFR ----------------------------------------------------------------------------------------------------------------
EFR_FORMS = [("resident", "k_efr_resident"), ("levels", "k_efr")]
EFR_RUNS = [(g, d) for g in (G1,) for d in ("blind cf", "informed cf", "tips", "bhv")] + \
           [(g, d) for g in (G3, G5) for d in ("blind cf", "informed cf", "tips")]
_efr_runs = {}


def _efr_trajectory(ctx, v, r, form):
    """tests/test_z27_gpu_efr.py's _trajectory: the device's state at every checkpoint of run r, in the golden's order."""
    import open_spiel_amd as osa
    if (r, form) not in _efr_runs:
        _, game, name = efr_cases.runs(v)[r]
        s = osa.EFRSolver(ctx, game, name, form=form)
        assert s.num_histories == HISTORIES[game]
        dev_tables = s.tables()
        where = {k: i for i, k in enumerate(dev_tables["keys"])}
        keys = efr_cases.keys_of(v, r)
        assert sorted(keys) == sorted(dev_tables["keys"])
        rows = np.array([where[k] for k in keys])
        assert np.array_equal(dev_tables["nact"][rows], v[f"r{r}/nact"])
        dev = s.deviations()
        off = dev["offsets"]
        out, done = [], 0
        for upto in v[f"r{r}/checkpoints"]:
            s.evaluate_and_update_policy(int(upto) - done)
            done = int(upto)
            assert s.iteration == done and s.last_kernel() == dict(EFR_FORMS)[form]
            state, t = s.regret_state(), s.tables()
            R = np.concatenate([state[off[i]:off[i + 1]] for i in rows])
            y = state[s.num_deviations:].reshape(-1, efr_cases.MAX_KEYS)[rows]
            out.append((R, y, t["cur_policy"][rows], t["cum_policy"][rows], t["avg_policy"][rows]))
        _efr_runs[(r, form)] = (rows, dev, out)
    return _efr_runs[(r, form)]


@pytest.mark.parametrize("form", [f for f, _ in EFR_FORMS])
@pytest.mark.parametrize("r", range(len(EFR_RUNS)), ids=[f"{NAMES[g]}-{d}".replace(" ", "_") for g, d in EFR_RUNS])
def test_efr_tables_exact_and_every_checkpoint(ctx, efr, profile, r, form):
    _, game, name = efr_cases.runs(efr)[r]
    assert (game, name) == EFR_RUNS[r]
    rows, dev, out = _efr_trajectory(ctx, efr, r, form)
    off = dev["offsets"]
    assert np.array_equal((off[1:] - off[:-1])[rows], efr[f"r{r}/dev_count"])
    pick = np.concatenate([np.arange(off[i], off[i + 1]) for i in rows])
    none = efr[f"r{r}/dev_weights_none"]
    assert np.array_equal(dev["target"][pick], efr[f"r{r}/dev_target"]) and np.array_equal(dev["source"][pick], efr[f"r{r}/dev_source"])
    assert np.array_equal(dev["weights_none"][pick], none) and np.array_equal(dev["weights"][pick], efr[f"r{r}/dev_weights"])
    assert np.array_equal(dev["memory"][pick][none == 0], efr[f"r{r}/dev_memory"][none == 0])
    largest = 0.0
    for c, (R, _, cur, cum, avg) in enumerate(out):
        for k, mine in (("R", R), ("cur", cur), ("cum", cum), ("avg", avg)):
            want = efr[f"r{r}/R"][c] if k == "R" else efr_cases.by_legal(efr, r, efr[f"r{r}/{k}"][c])
            largest = max(largest, float(np.max(np.abs(mine - want))))
    print(f"efr {NAMES[game]} | {name} [{form}]: largest deviation {largest:.3g} (bound {efr_cases.TOLERANCE:.3g})")
    assert largest <= efr_cases.TOLERANCE
    key = ("efr", game, dict(EFR_FORMS)[form])
    profile[key] = (max(largest, profile.get(key, (0.0, ""))[0]),
                    f"R, current, cumulative and average policy, every recorded deviation set and checkpoint; bound {efr_cases.TOLERANCE}")


@pytest.mark.parametrize("r", range(len(EFR_RUNS)), ids=[f"{NAMES[g]}-{d}".replace(" ", "_") for g, d in EFR_RUNS])
def test_efr_forms_agree_bit_for_bit(ctx, efr, r):
    resident, levels = (_efr_trajectory(ctx, efr, r, f)[2] for f, _ in EFR_FORMS)
    for c in range(len(resident)):
        for a, b in zip(resident[c], levels[c]):
            assert np.array_equal(a, b), ("the two forms differ", EFR_RUNS[r], c)


@pytest.mark.parametrize("game", [G2, G4], ids=["G2", "G4"])
@pytest.mark.parametrize("name", ["blind cf", "tips"])
def test_efr_refuses_action_mapping(ctx, game, name):
    import open_spiel_amd as osa
    for form in (None, "resident", "levels"):
        with pytest.raises(osa.OsgError, match="osg error -2: .*action_mapping=True gives an information state several own histories"):
            osa.EFRSolver(ctx, game, name, form=form)


# ---- ISMCTS -------------------------------------------------------------------------------------------------------------
def test_ismcts_refuses_four_player_kuhn(ctx):
    """kuhn_poker(players=4) is the first size the search refuses: from the batch entry point and from ISMCTSBot at the
    first decision node (after the four deals), with the message that names the served player counts."""
    import open_spiel_amd as osa
    batch = osa.StateBatch(ctx, G5, 2)
    for card in (0, 1, 2, 3):
        batch.apply_actions(np.array([card, card], np.int32))
    with pytest.raises(osa.OsgError, match="osg error -2: .*kuhn_poker and leduc_poker are searched with 2 or 3 players"):
        batch.ismcts_search(max_simulations=4)
    state = osa.pyspiel_hip.load_game(G5).new_initial_state()
    for card in (0, 1, 2, 3):
        state.apply_action(card)
    bot = osa.ISMCTSBot(G5, 2.0, 8, ctx=ctx)
    with pytest.raises(osa.OsgError, match="osg error -2: .*kuhn_poker and leduc_poker are searched with 2 or 3 players"):
        bot.step(state)


def test_ismcts_refuses_the_leduc_parameters(ctx):
    """The search leans on what each leduc parameter changes (rank-keyed nodes and the resampler's "never my rank" with
    suit_isomorphism, tied children with action_mapping, the owner of the first level with starting_player) and no run of
    the reference on them is recorded: osg_ismcts_search and ISMCTSBot refuse them, naming the parameter."""
    import open_spiel_amd as osa
    for game, names in ((G1, "suit_isomorphism=True"), (G2, "action_mapping=True"), (G3, "starting_player != 0"), (G4, "suit_isomorphism=True")):
        batch = osa.StateBatch(ctx, game, 2)
        for card in (0, 1):
            batch.apply_actions(np.array([card, card + 1], np.int32))
        with pytest.raises(osa.OsgError, match="osg error -2: osg_ismcts_search: leduc_poker is searched with its default rules; " + names):
            batch.ismcts_search(max_simulations=4)
        state = osa.pyspiel_hip.load_game(game).new_initial_state()
        for card in (0, 1):
            state.apply_action(card)
        with pytest.raises(osa.OsgError, match="osg error -2: .*" + names):
            osa.ISMCTSBot(game, 2.0, 8, ctx=ctx).step(state)
    # the default rules are searched as before
    batch = osa.StateBatch(ctx, "leduc_poker", 2)
    for card in (0, 1):
        batch.apply_actions(np.array([card, card + 1], np.int32))
    assert batch.ismcts_search(max_simulations=4)["status"].cpu().numpy().tolist() == [0, 0]


# ---- populations and PSRO -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,names", [(G1, "suit_isomorphism=True"), (G2, "action_mapping=True"), (G3, "starting_player != 0"),
                                        (G4, "suit_isomorphism=True")], ids=["G1", "G2", "G3", "G4"])
def test_populations_and_psro_refuse_the_leduc_parameters(ctx, game, names):
    """No run of the reference's policy_value / PolicyAggregator on the leduc parameters is recorded: profile_returns,
    payoff_tensors, aggregate_policies and PSROSolver (whose constructor evaluates its first profile) refuse them."""
    import open_spiel_amd as osa
    from open_spiel_amd.psro import PSROSolver
    s = osa.TabularSolver(ctx, game)
    t = s.tables()
    stack = np.stack([t["cur_policy"], t["cur_policy"]])
    message = "osg error -2: .*leduc_poker populations are served with its default rules; " + names
    with pytest.raises(osa.OsgError, match=message):
        s.profile_returns(stack, np.array([[0, 1]], np.int32))
    with pytest.raises(osa.OsgError, match=message):
        s.payoff_tensors(stack)
    with pytest.raises(osa.OsgError, match=message):
        s.aggregate_policies(stack, np.full((2, 2), 0.5))
    with pytest.raises(osa.OsgError, match=message):
        PSROSolver(ctx, game)
    s.evaluate_and_update_policy(1)   # the solver itself is what it was
    assert s.iteration == 1


def test_populations_serve_four_player_kuhn_as_before(ctx):
    import open_spiel_amd as osa
    s = osa.TabularSolver(ctx, G5)
    t = s.tables()
    ret = s.profile_returns(np.stack([t["cur_policy"]]), np.zeros((1, 4), np.int32))
    assert ret.shape == (1, 4) and abs(ret.sum()) <= 1e-12   # zero-sum


# ---- action values ----------------------------------------------------------------------------------------------------------
import hashlib  # noqa: E402

import action_value_cases as avc  # noqa: E402

AV_FORMS = [({}, "k_qvalues_small"), (dict(general_kernel="grid"), "k_qvalues")]
AV_OUTPUTS = ("root_values",) + avc.VECTORS + avc.TABLES
_av_results = {}


@pytest.fixture(scope="module")
def av():
    return _load("action_value")


def _av_run(ctx, av, game, kwargs, kernel):
    """Every recorded case of the game through action_values("table", ...): {case: outputs}, rows in the goldens' order."""
    import open_spiel_amd as osa
    if (game, kernel) not in _av_results:
        s = osa.TabularSolver(ctx, game, **kwargs)
        assert s.num_histories == HISTORIES[game] == int(av[f"{game}/histories"])
        dev = s.tables()
        keys = sorted(dev["keys"])
        assert bytes(av[f"{game}/keys_sha256"]) == hashlib.sha256("\n".join(keys).encode()).digest()
        order = _order(av, dev, game)
        back = np.argsort(order)
        out = {}
        for case in avc.case_names(av, game):
            b = int(av[f"{case}/responder"])
            got = s.action_values("table", avc.case_policy(av, case)[order], responder=None if b < 0 else b)
            assert s.last_eval_kernel() == kernel
            out[case] = {k: (np.asarray(x) if k in ("root_values", "best_response_value") else np.asarray(x)[back]) for k, x in got.items()}
        _av_results[(game, kernel)] = out
    return _av_results[(game, kernel)]


@pytest.mark.parametrize("kwargs,kernel", AV_FORMS, ids=[k for _, k in AV_FORMS])
@pytest.mark.parametrize("game", list(NAMES), ids=lambda g: NAMES[g])
def test_action_values_match_the_reference(ctx, av, profile, game, kwargs, kernel):
    """tests/test_z18_gpu_action_values.py's comparison: every output within action_value_cases.TOLERANCE, the best
    responder's choice equal to the recorded one; and the choice is a maximiser of the RECORDED action values at every
    infostate the responder reaches counterfactually, whichever tied action it is."""
    results = _av_run(ctx, av, game, kwargs, kernel)
    assert len(results) == (3 if game == G5 else 7)
    worst = 0.0
    for case, got in results.items():
        for name in AV_OUTPUTS:
            d = float(np.abs(got[name] - av[f"{case}/{name}"]).max())
            worst = max(worst, d)
            assert d <= avc.TOLERANCE, (case, kernel, name, d)
        b = int(av[f"{case}/responder"])
        if b >= 0:
            d = abs(float(got["best_response_value"]) - float(av[f"{case}/best_response_value"]))
            worst = max(worst, d)
            assert d <= avc.TOLERANCE, (case, kernel, "best_response_value", d)
            best = got["best_index"]
            assert np.array_equal(best, av[f"{case}/best_index"]), (case, kernel)
            mine = (av[f"{game}/player"] == b) & (av[f"{case}/cf_reach"] > 0)
            q = np.where(np.arange(av[f"{game}/legal"].shape[1])[None, :] < av[f"{game}/nact"][:, None], av[f"{case}/action_values"], -np.inf)
            gap = float((q.max(axis=1) - q[np.arange(len(best)), np.maximum(best, 0)])[mine].max())
            assert gap <= avc.TOLERANCE, (case, kernel, "the device's choice is not a maximiser", gap)
    print(f"action values {NAMES[game]} {kernel}: worst |device - reference| = {worst:.3g}")
    profile[("action_values", game, kernel)] = (worst, f"every output of every case (uniform, random and first-action tables, "
                                                       f"vs best response for each player); bound {avc.TOLERANCE}")


@pytest.mark.parametrize("game", list(NAMES), ids=lambda g: NAMES[g])
def test_action_value_forms_agree_bit_for_bit(ctx, av, game):
    small, wide = (_av_run(ctx, av, game, kw, k) for kw, k in AV_FORMS)
    for case in small:
        assert sorted(small[case]) == sorted(wide[case])
        for name in small[case]:
            assert np.array_equal(small[case][name], wide[case][name]), (case, name)
