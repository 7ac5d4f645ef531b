"""Magnetic mirror descent on the device (osg_mmd_* in include/osg_abi.h; MMDSolver) against the trajectories the
reference's own mmd_dilated.py left in tests/golden/mmd_vectors.npz (tests/golden/make_mmd_vectors.py).

Bound for x, avg_x, pi and the gap: |device - reference| <= 1e-12 absolute.  The reference sums its payoff products
through BLAS in no fixed order; reordering them moves its own trajectory by at most 3.3e-15 over these runs, and the
bound leaves room for exp and log that differ from libm's by an ulp or two per call over up to 400 steps.  NashConv of
the current policy: within 1e-10 of the recorded value.  The device itself has one order for every sum
(open_spiel_amd/csrc/osg_mmd.h), so everything device-against-device is compared with array_equal.  Every test prints
the worst deviation it saw before it asserts.  The annealing run (set_params between calls) is one of the runs of
test_every_run_and_checkpoint."""
import numpy as np
import pytest

import mmd_cases

pytestmark = pytest.mark.gpu

PIN = mmd_cases.TOLERANCE
FORMS = [({}, "k_mmd_small"), (dict(general_kernel=True), "k_mmd")]
RUNS = ["kuhn_a0.1", "kuhn_a0", "kuhn_a1", "kuhn_anneal", "leduc_a0.05", "leduc_a0"]
INVALID, UNSUPPORTED = "osg error -1: ", "osg error -2: "


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


@pytest.fixture(scope="module")
def v():
    return mmd_cases.load()


def _order(v, solver, game):
    """Row of the goldens for every row of the device solver."""
    dev = solver.tables()
    keys = mmd_cases.keys_of(v, game)
    where = {k: i for i, k in enumerate(keys)}
    assert sorted(dev["keys"]) == keys
    order = np.array([where[k] for k in dev["keys"]])
    assert np.array_equal(dev["nact"], v[f"{game}/nact"][order])
    used = np.arange(dev["legal"].shape[1])[None, :] < dev["nact"][:, None]
    assert np.array_equal(dev["legal"][used], v[f"{game}/legal"][order][used])
    return order


def _state(s):
    t = s.tables()
    return s.current_sequences(), t["cum_policy"], t["cur_policy"], s.iteration


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


def _set_iteration(s, t):
    from open_spiel_amd import _abi
    _abi.check(_abi.lib().osg_cfr_set_iteration(s._h, t))


def _run(ctx, v, run, kwargs, form):
    """The run through MMDSolver: [(x, avg_x, pi, gap)] per checkpoint in the goldens' row order, each pinned."""
    import open_spiel_amd as osa
    game = bytes(v[f"{run}/game"]).decode()

    def stepsize(c):   # None where the segment ran with the reference's default
        key = f"{game}/default_stepsize/{v[f'{run}/alpha'][c]}"
        return None if key in v and v[key] == v[f"{run}/stepsize"][c] else float(v[f"{run}/stepsize"][c])

    s = osa.MMDSolver(ctx, game, float(v[f"{run}/alpha"][0]), stepsize(0), **kwargs)
    order = _order(v, s, game)
    back = np.argsort(order)
    out, worst = [], {}
    for c in range(len(v[f"{run}/t"])):
        alpha = float(v[f"{run}/alpha"][c])
        s.set_params(alpha, stepsize(c))
        assert abs(s.stepsize[0] - v[f"{run}/stepsize"][c]) <= PIN
        s.iterate(int(v[f"{run}/iters"][c]))
        assert s.last_kernel() == form and s.iteration == v[f"{run}/t"][c]
        t = s.tables()
        got = dict(x=s.current_sequences()[back], avg_x=s.get_avg_sequences()[back], pi=t["cur_policy"][back])
        assert np.array_equal(got["avg_x"], t["cum_policy"][back])
        gap = s.get_gap() if alpha > 0 else float("nan")
        out.append((got["x"], got["avg_x"], got["pi"], gap))
        for name, table in got.items():
            worst[name] = max(worst.get(name, 0.0), float(np.abs(table - v[f"{run}/{name}"][c]).max()))
        if alpha > 0:
            worst["gap"] = max(worst.get("gap", 0.0), abs(gap - v[f"{run}/gap"][c]))
        worst["nash_conv"] = max(worst.get("nash_conv", 0.0), abs(s.nash_conv() - v[f"{run}/nash_conv"][c]))
    print(f"mmd {run} {form}: worst |device - reference| " + " ".join(f"{k} {d:.3g}" for k, d in worst.items()))
    for name, d in worst.items():
        assert d <= (1e-10 if name == "nash_conv" else PIN), (run, form, name, d)
    return out


@pytest.mark.parametrize("kwargs,form", FORMS)
@pytest.mark.parametrize("run", RUNS)
def test_every_run_and_checkpoint(ctx, v, run, kwargs, form):
    """1. and 4.: x, avg_x, pi, get_gap() and nash_conv() at every recorded checkpoint, in both forms."""
    _run(ctx, v, run, kwargs, form)


@pytest.mark.parametrize("game", mmd_cases.GAMES)
def test_device_against_the_host_program(ctx, v, game, tmp_path):
    """The header's functions on the CPU (tests/native/mmd_host_test.cpp) and in the kernels: the same tables up to the
    device's exp and log, well inside the bound."""
    import subprocess
    exe = mmd_cases.build_host_test(str(tmp_path / "mmd_host_test"))
    listed = mmd_cases.write_cases(v, game, tmp_path / "cases.bin")
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), repr(PIN), str(tmp_path / "tables.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]
    host = mmd_cases.read_host_tables(v, game, listed, tmp_path / "tables.bin")
    for run in mmd_cases.run_names(v, game):
        worst = 0.0
        for c, dev in enumerate(_run(ctx, v, run, {}, "k_mmd_small")):
            for k in range(3):
                worst = max(worst, float(np.abs(dev[k] - host[(run, c)][k]).max()))
            if not np.isnan(dev[3]):
                worst = max(worst, abs(dev[3] - host[(run, c)][3]))
        print(f"mmd {run}: worst |device - host program| = {worst:.3g}; bit-identical: {worst == 0.0}")
        assert worst <= PIN


@pytest.mark.parametrize("game,alpha", [("kuhn_poker", 0.1), ("kuhn_poker", 0.0), ("leduc_poker", 0.05)])
def test_bit_identity(ctx, v, game, alpha):
    """2. iterate(10) against ten iterate(1); resident against general form; a run repeated after reset(); a checkpoint
    restored into a fresh solver and continued against the uninterrupted run."""
    import open_spiel_amd as osa
    eta = 1.0 if alpha == 0 else None
    a = osa.MMDSolver(ctx, game, alpha, eta)
    start = _state(a)
    assert np.array_equal(start[0], start[1]) and start[3] == 0   # avg_x = x of the uniform policy
    a.iterate(10)
    whole = _state(a)
    assert whole[3] == 10 and np.isfinite(whole[0]).all()
    b = osa.MMDSolver(ctx, game, alpha, eta)
    for _ in range(10):
        b.update_sequences()
    assert _same(_state(b), whole), "iterate(10) != 10 x iterate(1)"
    g = osa.MMDSolver(ctx, game, alpha, eta, general_kernel=True)
    g.iterate(4)
    mid = _state(g)
    g.iterate(6)
    assert g.last_kernel() == "k_mmd" and a.last_kernel() == "k_mmd_small"
    assert _same(_state(g), whole), "general form != resident form"
    if alpha > 0:
        assert a.get_gap() == g.get_gap()
    a.reset()
    assert _same(_state(a), start)
    a.iterate(10)
    assert _same(_state(a), whole), "a run repeated after reset() differs"
    for kwargs in ({}, dict(general_kernel=True)):
        r = osa.MMDSolver(ctx, game, alpha, eta, **kwargs)
        r.load_tables(cum_policy=mid[1], cur_policy=mid[2])
        _set_iteration(r, 4)
        r.iterate(6)
        assert _same(_state(r), whole), f"a restored checkpoint continues differently ({kwargs})"


def _replica_params(n):
    return 0.05 * np.arange(n), 0.3 + 0.01 * np.arange(n)   # replica 0 has alpha = 0


@pytest.fixture(scope="module")
def single_runs(ctx):
    """Replica r's parameters on a solver of its own, 10 + 15 iterations: computed once per r, shared by the counts."""
    import open_spiel_amd as osa
    cache, solver = {}, []

    def get(r):
        if r not in cache:
            alpha, eta = _replica_params(r + 1)
            if not solver:
                solver.append(osa.MMDSolver(ctx, "kuhn_poker", 0.0, 1.0))
            s = solver[0]
            s.set_params(alpha[r], eta[r])
            s.reset()
            s.iterate(10)
            s.iterate(15)
            cache[r] = (_state(s), s.get_gap() if alpha[r] > 0 else None)
        return cache[r]
    return get


@pytest.mark.parametrize("replicas", [1, 3, 65])
def test_replicas(ctx, single_runs, replicas):
    """3. Every replica runs with its own (alpha, stepsize), one workgroup each; its tables equal a single solver's."""
    import open_spiel_amd as osa
    alpha, eta = _replica_params(replicas)
    s = osa.MMDSolver(ctx, "kuhn_poker", alpha, eta, replicas=replicas)
    s.iterate(10)
    s.iterate(15)
    assert s.last_kernel() == "k_mmd_small"
    for r in range(replicas):
        s.select_replica(r)
        want, gap = single_runs(r)
        assert _same(_state(s), want), f"replica {r} of {replicas}"
        if gap is None:
            with pytest.raises(osa.OsgError, match=INVALID + ".*alpha = 0"):
                s.get_gap()
        else:
            assert s.get_gap() == gap
    if replicas > 1:
        with pytest.raises(osa.OsgError, match=UNSUPPORTED + ".*replicas"):
            osa.MMDSolver(ctx, "kuhn_poker", alpha, eta, replicas=replicas, general_kernel=True)


@pytest.mark.parametrize("kwargs,form", FORMS)
def test_qre_fixed_point(ctx, v, kwargs, form):
    """5. The kuhn_poker QRE at 1 / alpha = 10 (mmd_dilated_test.py:95-109): one update stays within rtol 1e-6, gap <= 1e-6."""
    import open_spiel_amd as osa
    s = osa.MMDSolver(ctx, "kuhn_poker", float(v["qre/alpha"]), **kwargs)
    order = _order(v, s, "kuhn_poker")
    s.load_tables(cum_policy=v["qre/x"][order], cur_policy=v["qre/pi"][order])
    gap = s.get_gap()
    s.update_sequences()
    x, pi = s.current_sequences(), s.tables()["cur_policy"]
    used = v["qre/x"][order] > 0
    print(f"mmd qre {form}: gap {gap:.3g} (reference {float(v['qre/gap']):.3g}), worst relative move "
          f"{float(np.abs(x[used] / v['qre/x'][order][used] - 1).max()):.3g}")
    assert s.last_kernel() == form and s.iteration == 1
    assert abs(gap) <= 1e-6
    np.testing.assert_allclose(x, v["qre/x"][order], rtol=1e-6, atol=0)
    np.testing.assert_allclose(pi, v["qre/pi"][order], rtol=1e-6, atol=0)


def test_refusals(ctx):
    """6. Every refusal with its error code; the tables and the counter are bit-unchanged after each."""
    import open_spiel_amd as osa
    from open_spiel_amd import _abi
    lib = _abi.lib()
    with pytest.raises(osa.OsgError, match=UNSUPPORTED + ".*3 players"):
        osa.MMDSolver(ctx, "kuhn_poker(players=3)", 0.1)
    with pytest.raises(osa.OsgError, match=INVALID + ".*alpha"):
        osa.MMDSolver(ctx, "kuhn_poker", -1.0)
    one = np.array([0.1]), np.array([0.5])
    m = osa.TabularSolver(ctx, "kuhn_poker", mccfr=True)
    before = m.tables()
    assert lib.osg_mmd_set_params(m._h, 1, one[0].ctypes.data, one[1].ctypes.data) == -1 and b"MCCFR" in lib.osg_last_error()
    d = osa.DCFRSolver(ctx, "kuhn_poker")
    assert lib.osg_mmd_set_params(d._h, 1, one[0].ctypes.data, one[1].ctypes.data) == -1 and b"discount" in lib.osg_last_error()
    fresh = osa.TabularSolver(ctx, "kuhn_poker")
    assert lib.osg_mmd_iterate(fresh._h, 1) == -1 and b"osg_mmd_set_params" in lib.osg_last_error()
    assert all(np.array_equal(before[k], m.tables()[k]) for k in ("regrets", "cum_policy", "cur_policy"))
    fresh.evaluate_and_update_policy(1)   # (not in MMD mode: CFR still runs)

    s = osa.MMDSolver(ctx, "kuhn_poker", 0.0, 1.0)
    s.iterate(3)
    state, params = _state(s), (s.alpha.copy(), s.stepsize.copy())
    regrets = s.tables()["regrets"]
    two = np.array([0.1, 0.2])
    refused = [
        (INVALID + ".*alpha", lambda: s.set_params(-1.0, 0.5)),
        (INVALID + ".*stepsize", lambda: s.set_params(0.1, float("nan"))),
        (INVALID + ".*stepsize", lambda: s.set_params(0.1, -0.5)),
        (INVALID + ".*alpha", lambda: s.set_params(float("inf"), 0.5)),
        (INVALID + ".*2 parameter pairs for 1 replicas", lambda: _abi.check(lib.osg_mmd_set_params(s._h, 2, two.ctypes.data, two.ctypes.data))),
        (INVALID + ".*alpha = 0", s.get_gap),
        (INVALID + ".*mirror-descent mode", lambda: _abi.check(lib.osg_cfr_iterate(s._h, 1))),
        (INVALID + ".*mirror-descent mode", lambda: _abi.check(lib.osg_cfr_br_iterate(s._h, 1))),
        (INVALID + ".*mirror-descent mode", lambda: _abi.check(lib.osg_xfp_iterate(s._h, 1))),
        ("MMDSolver", s.evaluate_and_update_policy),
        ("MMDSolver", s.evaluate_and_update_policy_cfr_br),
    ]
    for pattern, call in refused:
        with pytest.raises(osa.OsgError, match=pattern):
            call()
        assert _same(_state(s), state) and np.array_equal(s.tables()["regrets"], regrets), pattern
        assert np.array_equal(s.alpha, params[0]) and np.array_equal(s.stepsize, params[1])
    # a refused set_params left the device's parameters alone too: the run continues as one that was never disturbed
    s.iterate(2)
    u = osa.MMDSolver(ctx, "kuhn_poker", 0.0, 1.0)
    u.iterate(5)
    assert _same(_state(s), _state(u))


@pytest.mark.parametrize("kwargs,form", FORMS)
def test_leduc_run_ends_with_finite_normalised_tables(ctx, kwargs, form):
    """7. leduc_poker, 30 iterations: finite tables, every row sums to 1 within 1e-15 * nact; the accessors agree."""
    import open_spiel_amd as osa
    s = osa.MMDSolver(ctx, "leduc_poker", 0.05, **kwargs)
    assert abs(s.stepsize[0] - 4.260355029585798) <= PIN
    s.iterate(30)
    assert s.last_kernel() == form
    t = s.tables()
    x, avg = s.current_sequences(), s.get_avg_sequences()
    for table in (t["cur_policy"], t["avg_policy"], x, avg):
        assert np.isfinite(table).all() and (table >= 0).all()
    for name in ("cur_policy", "avg_policy"):
        d = np.abs(t[name].sum(axis=1) - 1.0)
        print(f"mmd leduc {form}: worst |row sum - 1| of {name} = {float(d.max()):.3g}")
        assert (d <= 1e-15 * t["nact"]).all()
    pol, avg_pol = s.get_policies(), s.get_avg_policies()
    i = 17
    assert [p for _, p in pol[t["keys"][i]]] == list(t["cur_policy"][i, :t["nact"][i]])
    assert [p for _, p in avg_pol[t["keys"][i]]] == list(t["avg_policy"][i, :t["nact"][i]])
    assert s.exploitability() == pytest.approx(s.nash_conv() / 2, abs=1e-15)
