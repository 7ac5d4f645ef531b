"""Extensive-form regret minimization on the device (osg_efr_* in include/osg_abi.h; EFRSolver) against the runs the
reference's own efr.py left in tests/golden/efr_vectors.npz (tests/golden/make_efr_vectors.py).

Every golden run in both kernel forms: the deviation tables equal the reference's exactly, and R per deviation, the
current, cumulative and average policy agree at every checkpoint within efr_cases.TOLERANCE (100 x the measured largest
deviation of the host program from the reference; efr_cases' docstring).  The device has one order
for every sum (open_spiel_amd/csrc/osg_efr.h), so the two forms, a split call, a checkpoint round trip and the host
program (tests/native/efr_host_test.cpp, the same header on the CPU) are compared with array_equal.  Every test prints
the worst deviation it saw before it asserts."""
import subprocess

import numpy as np
import pytest

import efr_cases as ec

pytestmark = pytest.mark.gpu

FORMS = [("resident", "k_efr_resident"), ("levels", "k_efr")]
INVALID, UNSUPPORTED = "osg error -1: ", "osg error -2: "


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


@pytest.fixture(scope="module")
def v():
    return ec.load()


def _solver(ctx, game, name, form=None, **kw):
    import open_spiel_amd as osa
    return osa.EFRSolver(ctx, game, name, form=form, **kw)


def _rows(v, r, solver):
    """The device row of every golden row."""
    dev = solver.tables()
    where = {k: i for i, k in enumerate(dev["keys"])}
    keys = ec.keys_of(v, r)
    assert sorted(keys) == sorted(dev["keys"])
    rows = np.array([where[k] for k in keys])
    assert np.array_equal(dev["nact"][rows], v[f"r{r}/nact"])
    return rows


def _golden_order(v, r, solver, rows, dev):
    """(R [D] in the golden's deviation order, y [I, 16], current, cumulative, average) of the device."""
    state, t = solver.regret_state(), solver.tables()
    off = dev["offsets"]
    R = np.concatenate([state[off[i]:off[i + 1]] for i in rows])
    y = state[solver.num_deviations:].reshape(-1, ec.MAX_KEYS)[rows]
    return R, y, t["cur_policy"][rows], t["cum_policy"][rows], t["avg_policy"][rows]


_runs = {}


def _trajectory(ctx, v, r, form):
    """The device's state at every checkpoint of golden run r in the given form (computed once per module)."""
    if (r, form) not in _runs:
        _, game, name = ec.runs(v)[r]
        s = _solver(ctx, game, name, form)
        rows, dev = _rows(v, r, s), s.deviations()
        out, done = [], 0
        for upto in v[f"r{r}/checkpoints"]:
            s.evaluate_and_update_policy(int(upto) - done)
            done = int(upto)
            assert s.iteration == done and s.last_kernel() == dict(FORMS)[form]
            out.append(_golden_order(v, r, s, rows, dev))
        _runs[(r, form)] = (s, rows, dev, out)
    return _runs[(r, form)]


@pytest.mark.parametrize("form", [f for f, _ in FORMS])
@pytest.mark.parametrize("r", range(len(ec.run_ids())), ids=ec.run_ids())
def test_every_run_tables_exact_and_every_checkpoint(ctx, v, r, form):
    _, game, name = ec.runs(v)[r]
    s, rows, dev, out = _trajectory(ctx, v, r, form)
    off = dev["offsets"]
    assert np.array_equal((off[1:] - off[:-1])[rows], v[f"r{r}/dev_count"])
    pick = np.concatenate([np.arange(off[i], off[i + 1]) for i in rows])
    none = v[f"r{r}/dev_weights_none"]
    assert np.array_equal(dev["target"][pick], v[f"r{r}/dev_target"]) and np.array_equal(dev["source"][pick], v[f"r{r}/dev_source"])
    assert np.array_equal(dev["weights_none"][pick], none) and np.array_equal(dev["weights"][pick], v[f"r{r}/dev_weights"])
    assert np.array_equal(dev["memory"][pick][none == 0], v[f"r{r}/dev_memory"][none == 0])
    counts = s.deviation_counts()
    assert counts["total"] == len(none) and counts["max_per_infostate"] == v[f"r{r}/dev_count"].max()
    assert counts["memory"] == v[f"r{r}/dev_weights"].shape[1]
    # the cells whose product is memreach, and the y slots, against the restatement's tables
    lay = ec.layout(v, r, game)
    T = ec.build_tables(lay, ec.TYPES.index(name))
    A = s.amax
    want_cells = np.full((len(none), T["L"]), -1, np.int64)
    for k in range(len(none)):
        for j in range(T["L"]):
            if (T["mask"][k] >> j) & 1:
                col = (T["cols"][k] >> (4 * j)) & 0xF
                want_cells[k, j] = -2 if col == ec.ZERO_COL else rows[T["own_info"][T["info"][k]][j]] * A + col
    assert np.array_equal(dev["cells"][pick], want_cells) and np.array_equal(dev["y_slot"][pick], T["slot"])
    largest = 0.0
    for c, (R, _, cur, cum, avg) in enumerate(out):
        for k, mine in (("R", R), ("cur", cur), ("cum", cum), ("avg", avg)):
            want = v[f"r{r}/R"][c] if k == "R" else ec.by_legal(v, r, v[f"r{r}/{k}"][c])
            d = float(np.max(np.abs(mine - want)))
            largest = max(largest, d)
            print(f"{game} | {name} [{form}] iteration {v[f'r{r}/checkpoints'][c]} {k}: {d:.3g}")
    print(f"largest deviation {largest:.3g} (bound {ec.TOLERANCE:.3g})")
    assert largest <= ec.TOLERANCE
    regrets = s.return_cumulative_regret()
    assert np.array_equal(np.concatenate([regrets[k] for k in ec.keys_of(v, r)]), out[-1][0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ec.build_host_test(str(tmp_path_factory.mktemp("efr") / "efr_host_test"))


@pytest.mark.parametrize("r", range(len(ec.run_ids())), ids=ec.run_ids())
def test_forms_and_host_program_give_the_same_bits(ctx, v, r, exe, tmp_path):
    lay = ec.write_case(v, r, tmp_path / "case.bin")
    p = subprocess.run([exe, "run", str(tmp_path / "case.bin"), repr(ec.TOLERANCE), str(tmp_path / "state.bin")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-500:]
    host = ec.read_host_state(v, r, lay, tmp_path / "state.bin")
    resident, levels = (_trajectory(ctx, v, r, f)[3] for f, _ in FORMS)
    D = len(v[f"r{r}/dev_target"])
    for c in range(len(host)):
        for a, b in zip(resident[c], levels[c]):
            assert np.array_equal(a, b), "the two forms differ"
        R, y, cur, cum, _ = resident[c]
        worst = max(float(np.max(np.abs(R - host[c][0][:D]))), float(np.max(np.abs(cur - host[c][1]))), float(np.max(np.abs(cum - host[c][2]))))
        print(f"checkpoint {c}: device against the host program {worst:.3g}")
        assert np.array_equal(R, host[c][0][:D]) and np.array_equal(y, host[c][0][D:].reshape(-1, ec.MAX_KEYS))
        assert np.array_equal(cur, host[c][1]) and np.array_equal(cum, host[c][2])


@pytest.mark.parametrize("form", [f for f, _ in FORMS])
@pytest.mark.parametrize("game,name", [("kuhn_poker", "csps"), ("leduc_poker", "cfps")])
def test_split_calls_and_checkpoint_round_trip(ctx, form, game, name):
    a, b, c = (_solver(ctx, game, name, form) for _ in range(3))
    a.evaluate_and_update_policy(5)
    b.evaluate_and_update_policy(3)
    t = b.tables()
    c.load_regret_state(b.regret_state())
    c.load_tables(cum_policy=t["cum_policy"], cur_policy=t["cur_policy"])
    c.set_iteration(b.iteration)
    b.evaluate_and_update_policy(2)
    c.evaluate_and_update_policy(2)
    ta = a.tables()
    for other in (b, c):
        assert other.iteration == 5
        assert np.array_equal(a.regret_state(), other.regret_state())
        to = other.tables()
        assert np.array_equal(ta["cur_policy"], to["cur_policy"]) and np.array_equal(ta["cum_policy"], to["cum_policy"])
    a.reset()
    assert a.iteration == 0 and not a.regret_state().any() and not a.tables()["cum_policy"].any()


@pytest.mark.parametrize("game,form", [("leduc_poker", "levels"), ("kuhn_poker(players=3)", None)])
def test_blind_cf_is_simultaneous_cfr(ctx, game, form):
    import open_spiel_amd as osa
    efr = _solver(ctx, game, "blind cf", form)
    cfr = osa.TabularSolver(ctx, game, alternating_updates=False, linear_averaging=False, regret_matching_plus=False)
    efr.evaluate_and_update_policy(4)
    cfr.evaluate_and_update_policy(4)
    if form == "levels":
        assert efr.last_kernel() == "k_efr" and efr.depths > 1
    te, tc = efr.tables(), cfr.tables()
    assert te["keys"] == tc["keys"]
    for k in ("cur_policy", "cum_policy", "avg_policy"):
        d = float(np.max(np.abs(te[k] - tc[k])))
        print(f"{game} {k}: EFR blind cf against the device CFR {d:.3g}")
        assert d <= ec.TOLERANCE
    off = efr.deviations()["offsets"]
    R = efr.regret_state()[:efr.num_deviations]
    for i in range(efr.num_infostates):   # blind cf: deviation a of an infostate is "play a", CFR's regret of a
        assert np.max(np.abs(R[off[i]:off[i + 1]] - tc["regrets"][i, :tc["nact"][i]])) <= ec.TOLERANCE


def test_nash_conv_of_the_kuhn_tips_average(ctx, v):
    r = [q for q, g, d in ec.runs(v) if (g, d) == ("kuhn_poker", "tips")][0]
    s, rows, _, out = _trajectory(ctx, v, r, "resident")
    assert v[f"r{r}/checkpoints"][-1] == 20
    table = np.zeros((s.num_infostates, s.amax))
    table[rows] = ec.by_legal(v, r, v[f"r{r}/avg"][-1])
    want = s.evaluate_policy("table", table)["nash_conv"]
    got = s.nash_conv()
    print(f"NashConv of the tips average after 20 iterations: {got!r}, of the golden average policy {want!r}")
    assert abs(got - want) <= ec.TOLERANCE and 0 < got < 0.5
    assert s.action_values()["action_values"].shape == (s.num_infostates, s.amax)


def test_refusals(ctx):
    import open_spiel_amd as osa
    from open_spiel_amd import _abi
    with pytest.raises(ValueError, match="Unsupported Deviation Set Passed              As Constructor Argument"):
        _solver(ctx, "kuhn_poker", "blind")
    with pytest.raises(osa.OsgError) as e:
        _solver(ctx, "kuhn_poker", "blind cf", replicas=2)
    assert str(e.value).startswith(UNSUPPORTED) and "replicas" in str(e.value)
    plain = osa.TabularSolver(ctx, "kuhn_poker", alternating_updates=False)
    assert _abi.lib().osg_efr_iterate(plain._h, 1) == -1
    assert b"osg_efr_set_deviations comes first" in _abi.lib().osg_last_error()
    assert _abi.lib().osg_efr_set_deviations(plain._h, 9, 0) == -1 and _abi.lib().osg_efr_set_deviations(plain._h, 2, 3) == -1
    plain.evaluate_and_update_policy(1)   # (a refused call changed nothing: still a CFR solver)
    s = _solver(ctx, "kuhn_poker", "tips")
    with pytest.raises(osa.OsgError) as e:
        osa.TabularSolver.evaluate_and_update_policy(s, 1)
    assert str(e.value).startswith(INVALID)
    with pytest.raises(osa.OsgError):
        s.evaluate_and_update_policy_cfr_br()


@pytest.mark.parametrize("game", ["kuhn_poker(players=4)", "kuhn_poker(players=5)"])
def test_more_players_build_and_keep_policies_normalised(ctx, game):
    """(3-player leduc is exercised by tools/probe_efr.py only: its creation alone exceeds a few seconds)"""
    s = _solver(ctx, game, "tips")
    s.evaluate_and_update_policy(3)
    t = s.tables()
    used = np.arange(s.amax)[None, :] < t["nact"][:, None]
    assert np.all(np.abs(np.where(used, t["cur_policy"], 0).sum(axis=1) - 1) <= 1e-12) and np.isfinite(s.nash_conv())
