"""Per-infostate action values and reaches on the device (osg_cfr_action_values in include/osg_abi.h;
TabularSolver.action_values) against what the reference's own action_value.py and action_value_vs_best_response.py left
in tests/golden/action_value_vectors.npz (tests/golden/make_action_value_vectors.py).

Bound for every output against the reference: |device - reference| <= 1e-12 absolute (action_value_cases.TOLERANCE).
The device has one order for every sum (open_spiel_amd/csrc/osg_action_values.h), so everything device-against-device
is compared with array_equal.  Every test prints the worst deviation it saw before it asserts."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import action_value_cases as avc

pytestmark = pytest.mark.gpu

PIN = avc.TOLERANCE
SMALL, GENERAL = ({}, "k_qvalues_small"), (dict(general_kernel="grid"), "k_qvalues")
# kuhn_poker(players=5) (116 437 histories) and leduc_poker(players=3) take the launch-per-level form by themselves
FORMS = [("kuhn_poker", SMALL), ("kuhn_poker", GENERAL), ("kuhn_poker(players=3)", SMALL), ("kuhn_poker(players=3)", GENERAL),
         ("kuhn_poker(players=5)", ({}, "k_qvalues")), ("leduc_poker", SMALL), ("leduc_poker", GENERAL),
         (avc.LARGE_GAME, ({}, "k_qvalues"))]
OUTPUTS = ("root_values",) + avc.VECTORS + avc.TABLES
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


@pytest.fixture(scope="module")
def v():
    return avc.load()


@pytest.fixture(scope="module")
def solvers(ctx, v):
    """(solver, order) per (game, form), made once: order[device row] = the goldens' row."""
    import open_spiel_amd as osa
    made = {}

    def get(game, kwargs=()):
        key = (game, tuple(sorted(dict(kwargs).items())))
        if key not in made:
            s = osa.TabularSolver(ctx, game, **dict(kwargs))
            dev = s.tables()
            keys = sorted(dev["keys"])
            assert bytes(v[f"{game}/keys_sha256"]) == hashlib.sha256("\n".join(keys).encode()).digest()
            where = {k: i for i, k in enumerate(keys)}
            order = np.array([where[k] for k in dev["keys"]])
            assert np.array_equal(dev["nact"], v[f"{game}/nact"][order])
            used = np.arange(dev["legal"].shape[1])[None, :] < dev["nact"][:, None]
            assert np.array_equal(dev["legal"][used], v[f"{game}/legal"][order][used])
            made[key] = (s, order)
        return made[key]
    return get


def _responder(v, case):
    b = int(v[f"{case}/responder"])
    return None if b < 0 else b


def _same(a, b):
    assert sorted(a) == sorted(b)
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def _to_numpy(res):
    return {k: (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)) for k, x in res.items()}


def _check_case(v, case, got, order):
    """Every recorded output of the case against the device's, rows brought into the goldens' order."""
    back = np.argsort(order)
    worst = {}
    for name in OUTPUTS:
        dev = got[name] if name == "root_values" else got[name][back]
        if f"{case}/{name}" in v:
            worst[name] = float(np.abs(dev - v[f"{case}/{name}"]).max())
        else:   # the large game: rows and sums
            stride = avc.ROW_STRIDE if name in avc.TABLES else avc.VECTOR_STRIDE
            total = "colsum" if name in avc.TABLES else "sum"
            worst[name + "_rows"] = float(np.abs(dev[::stride] - v[f"{case}/{name}_rows"]).max())
            worst[name + "_" + total] = float(np.abs(dev.sum(axis=0) - v[f"{case}/{name}_{total}"]).max())
    b = _responder(v, case)
    if b is not None:
        worst["best_response_value"] = abs(float(got["best_response_value"]) - float(v[f"{case}/best_response_value"]))
        assert np.array_equal(got["best_index"][back], v[f"{case}/best_index"]), case
    print(f"action values {case}: worst |device - reference| " + " ".join(f"{k} {d:.3g}" for k, d in worst.items()))
    for name, d in worst.items():
        assert d <= PIN, (case, name, d)


@pytest.mark.parametrize("game,form", FORMS)
def test_every_case(solvers, v, game, form):
    """Every case of the fixture through osg_cfr_action_values with which = 2, in every form the game can take."""
    kwargs, kernel = form
    s, order = solvers(game, kwargs)
    cases = avc.case_names(v, game)
    assert len(cases) == (2 if game == avc.LARGE_GAME else 7 if game in avc.TWO_PLAYER else 3)
    for case in cases:
        table = avc.case_policy(v, case)[order]
        got = s.action_values("table", table, responder=_responder(v, case))
        assert s.last_eval_kernel() == kernel
        _check_case(v, case, got, order)


@pytest.mark.parametrize("game", ["kuhn_poker", "kuhn_poker(players=3)", "leduc_poker"])
def test_the_two_forms_and_two_runs_give_the_same_bits(solvers, v, game):
    (small, order), (general, order_g) = solvers(game), solvers(game, dict(general_kernel="grid"))
    assert np.array_equal(order, order_g)
    for case in avc.case_names(v, game):
        table, b = avc.case_policy(v, case)[order], _responder(v, case)
        first = small.action_values("table", table, responder=b)
        assert small.last_eval_kernel() == "k_qvalues_small"
        again = small.action_values("table", table, responder=b)
        wide = general.action_values("table", table, responder=b)
        assert general.last_eval_kernel() == "k_qvalues"
        assert _same(first, again), f"{case}: two runs differ"
        assert _same(first, wide), f"{case}: the resident and the launch-per-level form differ"


def test_more_members_than_lanes_twice_the_same_bits(solvers, v):
    """kuhn_poker(players=5): infostates of 120 members, a full chunk of 64 and a partial one of 56."""
    s, order = solvers("kuhn_poker(players=5)")
    table = avc.case_policy(v, "kuhn_poker(players=5)/random")[order]
    first, again = s.action_values("table", table), s.action_values("table", table)
    assert s.last_eval_kernel() == "k_qvalues" and _same(first, again)


@pytest.mark.parametrize("game,kwargs", [("kuhn_poker", {}), ("leduc_poker", {}), ("leduc_poker", dict(general_kernel="grid")),
                                         ("kuhn_poker(players=5)", {})])
def test_device_pointers_give_the_host_pointers_bits(ctx, solvers, v, game, kwargs):
    import torch
    s, order = solvers(game, kwargs)
    for kind in ("random", "first"):
        table = avc.case_policy(v, f"{game}/{kind}")[order]
        for b in ([None, 0, 1] if game in avc.TWO_PLAYER else [None]):
            host = s.action_values("table", table, responder=b)
            dev = s.action_values("table", torch.from_numpy(table).to(ctx.device), responder=b, device=True)
            assert all(isinstance(x, torch.Tensor) and x.device == ctx.device for x in dev.values())
            assert dev["action_values"].dtype == torch.float64
            ctx.synchronize()
            assert _same(host, _to_numpy(dev)), (game, kind, b)


@pytest.mark.parametrize("game,kwargs", [("kuhn_poker", {}), ("leduc_poker", {}), ("leduc_poker", dict(general_kernel="grid"))])
def test_the_solvers_own_tables(ctx, game, kwargs):
    """which = average / current after 10 CFR iterations equals which = table on the tables read back."""
    import open_spiel_amd as osa
    s = osa.TabularSolver(ctx, game, **kwargs)
    s.evaluate_and_update_policy(10)
    t = s.tables()
    for which, name in (("average", "avg_policy"), ("current", "cur_policy")):
        for b in (None, 1):
            assert _same(s.action_values(which, responder=b), s.action_values("table", t[name], responder=b)), (which, b)
    assert not np.array_equal(t["avg_policy"], t["cur_policy"])


def test_the_selected_replica(ctx):
    import open_spiel_amd as osa
    s = osa.TabularSolver(ctx, "kuhn_poker", replicas=3, random_initial_regrets=True, seed=11)
    s.evaluate_and_update_policy(5)
    seen = []
    for r in (0, 2):
        s.select_replica(r)
        t = s.tables()
        for which, name in (("average", "avg_policy"), ("current", "cur_policy")):
            assert _same(s.action_values(which), s.action_values("table", t[name])), (r, which)
        seen.append(s.action_values("current")["action_values"])
    assert not np.array_equal(seen[0], seen[1])


@pytest.mark.parametrize("game", ["kuhn_poker", "kuhn_poker(players=3)", "leduc_poker", "kuhn_poker(players=5)"])
def test_root_values_are_the_expected_returns(solvers, v, game):
    s, order = solvers(game)
    for kind in avc.POLICIES:
        table = avc.case_policy(v, f"{game}/{kind}")[order]
        d = np.abs(s.action_values("table", table)["root_values"] - s.evaluate_policy("table", table)["expected_returns"]).max()
        print(f"action values {game}/{kind}: |root_values - expected_returns| = {d:.3g}")
        assert d <= PIN


@pytest.mark.parametrize("game,kwargs", [("kuhn_poker", {}), ("leduc_poker", {}), ("leduc_poker", dict(general_kernel="grid"))])
def test_the_argmax_is_osg_cfr_best_responses(solvers, v, game, kwargs):
    from open_spiel_amd import _abi
    s, order = solvers(game, kwargs)
    player = v[f"{game}/player"][order]
    for kind in ("random", "first"):
        table = np.ascontiguousarray(avc.case_policy(v, f"{game}/{kind}")[order])
        best, values = np.zeros(s.num_infostates, np.int32), np.zeros(2)
        _abi.check(_abi.lib().osg_cfr_best_response(s._h, 2, table.ctypes.data, best.ctypes.data, values.ctypes.data))
        for b in (0, 1):
            got = s.action_values("table", table, responder=b)
            assert np.array_equal(got["best_index"], np.where(player == b, best, -1))
            assert got["best_response_value"] == values[b]


@pytest.mark.parametrize("game", ["kuhn_poker", "kuhn_poker(players=3)", "leduc_poker"])
def test_player_reach_is_fictitious_plays_average_reach(ctx, solvers, v, game):
    """osg_xfp_reaches multiplies the owner's probabilities root to leaf from 1.0 at the infostate's first member
    history (osg_xfp.h), the order of qv_member_reach: compared bit for bit."""
    import open_spiel_amd as osa
    s, order = solvers(game)
    x = osa.XFPSolver(ctx, game)
    for kind in ("random", "first"):
        table = avc.case_policy(v, f"{game}/{kind}")[order]
        x.load_tables(cur_policy=table)
        avg_reach, _ = x.reaches()
        assert np.array_equal(s.action_values("table", table)["player_reach"], avg_reach), (game, kind)


def test_both_layouts(ctx, solvers, v):
    import torch
    s, order = solvers("leduc_poker")
    table = avc.case_policy(v, "leduc_poker/random")[order]
    t = s.tables()
    legal = s.action_values("table", table)
    wide = s.action_values("table", table, layout="action_id")
    wide_dev = _to_numpy(s.action_values("table", torch.from_numpy(table).to(ctx.device), device=True, layout="action_id"))
    assert _same(wide, wide_dev)
    differ = 0
    for name in ("action_values", "cf_reach_by_value"):
        assert wide[name].shape == (s.num_infostates, 3)
        for i in range(s.num_infostates):
            ids = list(t["legal"][i, :t["nact"][i]])
            assert np.array_equal(wide[name][i, ids], legal[name][i, :len(ids)])
            assert all(wide[name][i, a] == 0 for a in range(3) if a not in ids)
            differ += ids != list(range(len(ids)))
    assert differ > 0   # rows whose legal set is {1, 2}
    for name in set(legal) - {"action_values", "cf_reach_by_value"}:
        assert np.array_equal(wide[name], legal[name])
    with pytest.raises(Exception, match="layout"):
        s.action_values("table", table, layout="dense")


@pytest.mark.parametrize("game", avc.TWO_PLAYER)
def test_action_values_vs_best_response(solvers, v, game):
    """Calculator's four fields for both players, random and first-action tables."""
    s, order = solvers(game)
    legal, nact = v[f"{game}/legal"], v[f"{game}/nact"]
    for kind in ("random", "first"):
        table = avc.case_policy(v, f"{game}/{kind}")[order]
        for player in (0, 1):
            case = f"{game}/{kind}/br{1 - player}"
            got = s.action_values_vs_best_response(player, "table", table)
            rows = order[got["rows"]]            # the goldens' rows, in the device's order of the player's infostates
            assert sorted(rows) == list(np.nonzero(v[f"{game}/player"] == player)[0])
            at = np.argsort(np.argsort(rows))    # position of each among the goldens' (ascending) rows of the player
            worst = abs(got["exploitability"] - float(v[f"{case}/best_response_value"]))
            worst = max(worst, np.abs(got["counterfactual_reach_probs_vs_br"] - v[f"{case}/counterfactual_reach_probs_vs_br"][at]).max())
            worst = max(worst, np.abs(got["player_reach_probs_vs_br"] - v[f"{case}/player_reach_probs_vs_br"][at]).max())
            for n, i in enumerate(rows):
                want = np.zeros(int(v[f"{game}/num_distinct_actions"]))
                want[legal[i, :nact[i]]] = v[f"{case}/values_vs_br"][at[n], :nact[i]]
                worst = max(worst, np.abs(got["values_vs_br"][n] - want).max())
            print(f"action values vs best response {case}: worst |device - reference| = {worst:.3g}")
            assert worst <= PIN


def test_refusals_write_nothing(ctx, solvers, v):
    """Every refusal of osg_cfr_action_values with its code; the canary-filled outputs stay as they were."""
    import open_spiel_amd as osa
    from open_spiel_amd import _abi
    lib = _abi.lib()
    s, order = solvers("kuhn_poker")
    three, _ = solvers("kuhn_poker(players=3)")
    I, A, P = s.num_infostates, s.amax, 2
    table = np.ascontiguousarray(avc.case_policy(v, "kuhn_poker/random")[order])
    table3 = np.ascontiguousarray(avc.case_policy(v, "kuhn_poker(players=3)/random"))

    def outputs(I, A, P):
        shapes = dict(root_values=(P,), action_values=(I, A), cf_reach=(I,), player_reach=(I,), reach=(I,), chance_reach=(I,),
                      cf_reach_by_value=(I, A), weighted_values=(I, A, P), best_response_value=(1,))
        arrays = {k: np.full(shape, -777.25) for k, shape in shapes.items()}
        arrays["best_index"] = np.full(I, -777, np.int32)
        return arrays, _abi.ActionValuesOut(**{k: a.ctypes.data for k, a in arrays.items()})

    arrays, out = outputs(I, A, P)
    arrays3, out3 = outputs(three.num_infostates, three.amax, 3)
    refused = [
        (INVALID, b"null", lambda: lib.osg_cfr_action_values(None, 2, table.ctypes.data, -1, 1, C.byref(out))),
        (INVALID, b"null", lambda: lib.osg_cfr_action_values(s._h, 2, table.ctypes.data, -1, 1, None)),
        (INVALID, b"which_policy", lambda: lib.osg_cfr_action_values(s._h, 3, table.ctypes.data, -1, 1, C.byref(out))),
        (INVALID, b"which_policy", lambda: lib.osg_cfr_action_values(s._h, -1, table.ctypes.data, -1, 1, C.byref(out))),
        (INVALID, b"needs policy", lambda: lib.osg_cfr_action_values(s._h, 2, None, -1, 1, C.byref(out))),
        (INVALID, b"responder", lambda: lib.osg_cfr_action_values(s._h, 2, table.ctypes.data, 2, 1, C.byref(out))),
        (INVALID, b"responder", lambda: lib.osg_cfr_action_values(s._h, 2, table.ctypes.data, -2, 1, C.byref(out))),
        (INVALID, b"responder", lambda: lib.osg_cfr_action_values(three._h, 2, table3.ctypes.data, 3, 1, C.byref(out3))),
        (UNSUPPORTED, b"2-player", lambda: lib.osg_cfr_action_values(three._h, 2, table3.ctypes.data, 0, 1, C.byref(out3))),
        (UNSUPPORTED, b"2-player", lambda: lib.osg_cfr_action_values(three._h, 1, None, 2, 1, C.byref(out3))),
    ]
    for code, word, call in refused:
        assert call() == code and word in lib.osg_last_error(), (code, word, lib.osg_last_error())
        ctx.synchronize()
        for a in list(arrays.values()) + list(arrays3.values()):
            assert (a == (-777 if a.dtype == np.int32 else -777.25)).all(), word
    with pytest.raises(osa.OsgError, match="2-player"):
        three.action_values_vs_best_response(0)
    # and an accepted call writes every one of them; without a responder its two outputs stay
    assert lib.osg_cfr_action_values(s._h, 2, table.ctypes.data, -1, 1, C.byref(out)) == 0
    assert all((a != -777.25).all() for k, a in arrays.items() if k not in ("best_index", "best_response_value"))
    assert (arrays["best_index"] == -777).all() and arrays["best_response_value"][0] == -777.25
    assert lib.osg_cfr_action_values(s._h, 2, table.ctypes.data, 0, 1, C.byref(out)) == 0
    assert (arrays["best_index"] != -777).all() and arrays["best_response_value"][0] != -777.25
    partial = _abi.ActionValuesOut(root_values=arrays["root_values"].ctypes.data)   # any member may be NULL
    assert lib.osg_cfr_action_values(s._h, 2, table.ctypes.data, -1, 1, C.byref(partial)) == 0
