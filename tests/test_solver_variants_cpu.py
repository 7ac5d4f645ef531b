"""The tabular solvers on the accepted poker variants, the parts that need no device: tests/golden/variant_*_vectors.npz
(tests/golden/make_solver_variant_vectors.py: the families' own makers run over leduc_poker with suit_isomorphism,
action_mapping and starting_player=1, all three at once, and kuhn_poker(players=4)).

1. Coverage by construction: the recorded layouts hold what makes each variant a variant (unequal chance rows and pair
   deals, three legal actions at every decision, player 1 on the first decision level, a tree beyond 9 457 histories).
2. The families' existing host programs and NumPy restatements over the new files, with the families' own comparators
   and bounds (imported from test_xfp_goldens.py / mmd_cases.py, not copied): the XFP averaging pass bit for bit in
   Python floats and through open_spiel_amd/csrc/osg_xfp.h, the MMD iterations through osg_mmd.h within
   mmd_cases.TOLERANCE, the EFR iterations through osg_efr.h (efr_cases.build_host_test) within efr_cases.TOLERANCE, and a
   re-run of the reference's discounted_cfr.py against the DCFR tables.
3. Sensitivity: a recorded array perturbed the way the variant could go wrong is rejected by the same comparator.

action_mapping=True: "fold" where there is nothing to call is "call"; both actions lead to the same information state of
the player who took them, so an information state has more than one own (infostate, action) predecessor and the game
as laid out has no sequence form.  The reference's mmd_dilated.py runs into log(0) = NaN there within ten iterations;
in its efr.py the regrets between the two tied moves are rounding noise, and no iteration passes the golden maker's
admission rule.  MMDSolver and EFRSolver refuse such strings (tests/test_z30_gpu_solver_variants.py), and no MMD or EFR
run of them is recorded."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import action_value_cases as avc
import efr_cases
import mmd_cases
import test_xfp_goldens as xfp_restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
G1 = "leduc_poker(suit_isomorphism=True)"
G2 = "leduc_poker(action_mapping=True)"
G3 = "leduc_poker(starting_player=1)"
G4 = "leduc_poker(action_mapping=True,suit_isomorphism=True,starting_player=1)"
G5 = "kuhn_poker(players=4)"
GAMES = [G1, G2, G3, G4, G5]
INFOSTATES = {G1: 288, G2: 936, G3: 936, G4: 288, G5: 160}
LARGEST_FIXTURE = 791154   # tests/golden/action_value_vectors.npz


def _load(family):
    path = os.path.join(GOLDEN, f"variant_{family}_vectors.npz")
    assert os.path.getsize(path) < LARGEST_FIXTURE, path
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def layout():
    return _load("layout")


@pytest.fixture(scope="module")
def xfp():
    return _load("xfp")


@pytest.fixture(scope="module")
def dcfr():
    return _load("dcfr")


@pytest.fixture(scope="module")
def mmd():
    return _load("mmd")


@pytest.fixture(scope="module")
def efr():
    return _load("efr")


@pytest.fixture(scope="module")
def av():
    return _load("action_value")


# ---- 1. coverage by construction ----------------------------------------------------------------------------------------
def test_suit_isomorphic_chance_rows_are_unequal_and_change_after_each_deal(layout):
    rows = layout[f"{G1}/chance_rows"]
    assert rows.shape[1] == 3   # K = 3 outcomes
    unequal = [r for r in rows if len(set(r[r > 0].tolist())) > 1]
    assert len(unequal) >= 6 and len(rows) >= 8, rows          # 1/3 each only before the first card
    assert np.abs(rows.sum(axis=1) - 1.0).max() <= 1e-15
    for game in (G2, G3, G5):                                  # the other games deal uniformly
        for r in layout[f"{game}/chance_rows"]:
            assert len(set(r[r > 0].tolist())) == 1, (game, r)


def test_suit_isomorphic_leduc_has_pair_deals(layout):
    deals, prob = layout[f"{G1}/deals"], layout[f"{G1}/deal_prob"]
    assert deals.shape == (9, 2)
    pairs = deals[:, 0] == deals[:, 1]
    assert pairs.sum() == 3
    assert abs(prob.sum() - 1.0) <= 1e-15
    assert np.allclose(prob[pairs], 1 / 15) and np.allclose(prob[~pairs], 2 / 15)   # unequal deal weights
    plain = layout[f"{G3}/deals"]
    assert plain.shape == (30, 2) and not (plain[:, 0] == plain[:, 1]).any()         # card ids: no deal repeats one


@pytest.mark.parametrize("game", [G2, G4])
def test_action_mapping_gives_every_decision_three_actions(xfp, dcfr, game):
    for v in (xfp, dcfr):
        assert (v[f"{game}/nact"] == 3).all()
        assert np.array_equal(v[f"{game}/legal"], np.tile([0, 1, 2], (INFOSTATES[game], 1)))   # legal index = action id
    assert (xfp[f"{G3}/nact"] == 2).any() and (xfp[f"{G3}/nact"] == 3).any()                   # unlike the default rules


@pytest.mark.parametrize("game", [G2, G4])
def test_action_mapping_ties_fold_with_call(xfp, layout, game):
    """Fold (0) where there is nothing to call is call (1): infostates whose two recorded action values (the
    counterfactual-weighted values XFP's best response maximised over) are bit-equal, in every iteration."""
    q = xfp[f"{game}/q"]
    assert q.shape == (10, INFOSTATES[game], 3) and np.isfinite(q).all()
    tied = q[:, :, 0].view(np.uint64) == q[:, :, 1].view(np.uint64)
    assert tied[0].sum() >= 1 and (tied == tied[0]).all()   # the same infostates in every iteration: those with nothing to call
    on_top = tied & (q[:, :, 0] >= q[:, :, 2])              # ... and where the tie is the maximum, the argmax has an exact tie
    print(game, "infostates with fold == call:", int(tied[0].sum()), "of them on top per iteration:", on_top.sum(axis=1))
    assert (on_top.sum(axis=1) >= 1).all() and (on_top.sum(axis=1) <= xfp[f"{game}/ties"]).all()
    for other in (G1, G3):
        o = xfp[f"{other}/q"]
        assert not (o[:, :, 0].view(np.uint64) == o[:, :, 1].view(np.uint64)).any()
    assert (xfp[f"{game}/ties"] >= 88).all(), xfp[f"{game}/ties"]
    assert int(layout[f"{game}/multi_pred"]) == {G2: 336, G4: 102}[game]
    for other in (G1, G3, G5):
        assert int(layout[f"{other}/multi_pred"]) == 0
    assert (xfp[f"{G1}/ties"] == 0).all() and (xfp[f"{G3}/ties"] == 0).all()


def test_starting_player_one_owns_the_first_decision_level(layout, xfp):
    for game, first in ((G3, 1), (G4, 1), (G1, 0), (G2, 0)):
        levels = layout[f"{game}/level_player"]
        assert levels[:2].tolist() == [-1, -1] and levels[2] == first and levels[3] == 1 - first, (game, levels)
    # and in the infostate layout: the infostates without an own predecessor that are nobody's reply are player 1's
    keys = bytes(xfp[f"{G3}/keys"]).decode().split("\n")
    opening = [i for i, k in enumerate(keys) if "[Round1: ]" in k and "[Round 1]" in k]
    assert len(opening) == 6 and (xfp[f"{G3}/player"][opening] == 1).all()


def test_action_mapped_tree_is_beyond_the_default_leduc_tree(layout):
    assert int(layout[f"{G3}/histories"]) == 9457           # what the LDS-resident forms were sized on
    assert int(layout[f"{G2}/histories"]) == 44527 > 9457
    assert [int(layout[f"{g}/histories"]) for g in (G1, G4, G5)] == [1939, 8992, 7886]


@pytest.mark.parametrize("game", GAMES)
def test_layouts_agree_between_the_families(xfp, dcfr, mmd, game):
    keys = bytes(xfp[f"{game}/keys"]).decode().split("\n")
    assert len(keys) == INFOSTATES[game] and keys == sorted(keys)
    for v in (dcfr,) + ((mmd,) if f"{game}/keys" in mmd else ()):
        for name in ("keys", "nact", "legal"):
            assert np.array_equal(v[f"{game}/{name}"], xfp[f"{game}/{name}"]), (game, name)
    assert (f"{game}/keys" in mmd) == (game in (G1, G3))


# ---- 2. host programs and restatements ----------------------------------------------------------------------------------
def _xfp_restate(v, game, policy_of=lambda want: want):
    """test_xfp_goldens.py's restatement over one game: the first (iteration, array) that is not bit-equal, or None."""
    nact = v[f"{game}/nact"]
    chain_of = xfp_restatement.chains(v[f"{game}/pred_info"], v[f"{game}/pred_action"])
    policy = xfp_restatement.uniform(nact, nact.max())
    for t in range(1, len(v[f"{game}/br"]) + 1):
        best = v[f"{game}/br"][t - 1]
        avg_reach, br_reach = xfp_restatement.reaches(chain_of, policy, best)
        if not np.array_equal(avg_reach, v[f"{game}/avg_reach"][t - 1]):
            return t, "avg_reach"
        if not np.array_equal(br_reach, v[f"{game}/br_reach"][t - 1]):
            return t, "br_reach"
        policy = xfp_restatement.update(policy, nact, best, 1 / (t + 1), avg_reach, br_reach)
        if not np.array_equal(policy, v[f"{game}/policy"][t - 1]):
            return t, "policy"
    return None


@pytest.mark.parametrize("game", GAMES)
def test_xfp_restatement_reproduces_every_recorded_iteration_bit_for_bit(xfp, game):
    assert xfp[f"{game}/policy"].shape == (10, INFOSTATES[game], xfp[f"{game}/nact"].max())
    assert _xfp_restate(xfp, game) is None
    assert np.abs(xfp[f"{game}/policy"].sum(axis=2) - 1.0).max() <= 1e-10
    assert xfp[f"{game}/cf_nonzero"].all()
    for t in (1, 2, 5, 10):
        assert np.isfinite(xfp[f"nash_conv/{game}/{t}"])


def test_xfp_decisive_iterations_are_as_recorded(xfp):
    """Which iterations the device may run freely (tests/test_z30_gpu_solver_variants.py): zero exact ties and a smallest
    gap of xfp_restatement.DECISIVE_GAP or more.  With action mapping none is."""
    decisive = {g: [t + 1 for t in range(10) if xfp[f"{g}/ties"][t] == 0 and xfp[f"{g}/min_gap"][t] >= xfp_restatement.DECISIVE_GAP]
                for g in GAMES}
    assert decisive == {G1: list(range(1, 11)), G2: [], G3: list(range(1, 11)), G4: [], G5: list(range(2, 11))}
    for g in (G1, G3, G5):   # nothing at rounding level: a gap is an exact tie or beyond 1e-5
        assert xfp[f"{g}/min_gap"].min() > 1e-5


@pytest.fixture(scope="module")
def xfp_exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("xfp") / "xfp_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "xfp_host_test.cpp"), "-o", path])
    return path


def _xfp_host(exe, v, game, path):
    """tests/native/xfp_host_test.cpp over one game (the input file of tests/test_xfp_native.py)."""
    T, I, A = v[f"{game}/policy"].shape
    with open(path, "wb") as f:
        f.write(np.array([I, A, int(v[f"{game}/player"].max()) + 1, T], np.int32).tobytes())
        for name in ("nact", "player", "pred_info", "pred_action"):
            f.write(np.ascontiguousarray(v[f"{game}/{name}"], np.int32).tobytes())
        for t in range(T):
            f.write(np.ascontiguousarray(v[f"{game}/br"][t], np.int32).tobytes())
            for name in ("avg_reach", "br_reach", "policy"):
                f.write(np.ascontiguousarray(v[f"{game}/{name}"][t], np.float64).tobytes())
    return subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("game", GAMES)
def test_xfp_header_functions_reproduce_every_recorded_iteration(xfp_exe, xfp, tmp_path, game):
    r = _xfp_host(xfp_exe, xfp, game, tmp_path / "cases.bin")
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.startswith(f"ok: 10 iterations, {INFOSTATES[game]} infostates, {int(xfp[f'{game}/nact'].sum()) * 10} cells")


@pytest.fixture(scope="module")
def mmd_exe(tmp_path_factory):
    return mmd_cases.build_host_test(str(tmp_path_factory.mktemp("mmd") / "mmd_host_test"))


def _mmd_host(exe, v, game, tmp_path):
    listed = mmd_cases.write_cases(v, game, tmp_path / "cases.bin")
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), repr(mmd_cases.TOLERANCE), str(tmp_path / "tables.bin")],
                       capture_output=True, text=True, timeout=120)
    return listed, r


@pytest.mark.parametrize("game", [G1, G3])
def test_mmd_header_functions_reproduce_every_recorded_checkpoint(mmd_exe, mmd, tmp_path, game):
    assert len(mmd_cases.run_names(mmd, game)) == 2
    for run in mmd_cases.run_names(mmd, game):
        assert mmd[f"{run}/t"].tolist() == [1, 10, 20] and np.isfinite(mmd[f"{run}/x"]).all()
    listed, r = _mmd_host(mmd_exe, mmd, game, tmp_path)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.rstrip().endswith(f"ok: {len(listed)} runs")
    assert r.stdout.count("largest deviation") == len(listed) == 2 and "FAILED" not in r.stdout


def test_mmd_is_not_recorded_where_the_sequence_form_is_undefined(mmd, layout):
    recorded = {bytes(mmd[f"{r}/game"]).decode() for r in mmd_cases.run_names(mmd)}
    assert recorded == {G1, G3}
    assert all(int(layout[f"{g}/multi_pred"]) == 0 for g in recorded)
    assert all(int(layout[f"{g}/multi_pred"]) > 0 for g in (G2, G4))


@pytest.mark.parametrize("game", GAMES)
def test_dcfr_tables_are_consistent_discounted_tables(dcfr, game):
    """tests/test_dcfr_goldens.py's checks of shape and content on the variant file."""
    I, amax = dcfr[f"{game}/legal"].shape
    nact = dcfr[f"{game}/nact"]
    pad = np.arange(amax)[None, :] >= nact[:, None]
    for name in "DL":
        for t in (1, 2, 10):
            for what in ("regrets", "cum_policy"):
                v = dcfr[f"{game}/{name}/{t}/{what}"]
                assert v.shape == (I, amax) and v.dtype == np.float64 and np.isfinite(v).all() and not v[pad].any()
            assert (dcfr[f"{game}/{name}/{t}/cum_policy"] >= 0).all()
    assert np.array_equal(dcfr[f"{game}/D/1/regrets"], dcfr[f"{game}/L/1/regrets"])      # 1/2 whatever the exponents
    assert np.array_equal(dcfr[f"{game}/D/1/cum_policy"], dcfr[f"{game}/L/1/cum_policy"])
    assert not np.array_equal(dcfr[f"{game}/D/10/regrets"], dcfr[f"{game}/L/10/regrets"])
    assert dcfr[f"{game}/D/10/cum_policy"].sum() > dcfr[f"{game}/L/10/cum_policy"].sum()
    if game != G5:   # after ten iterations every infostate of the leduc variants has been updated: no row is still zero
        assert (np.abs(dcfr[f"{game}/D/10/regrets"]).max(axis=1) > 0).all()


@pytest.mark.parametrize("game,name", [(G1, "D"), (G4, "L"), (G5, "D")])
def test_rerunning_the_reference_reproduces_the_dcfr_checkpoints(reference, dcfr, game, name):
    if not reference.sources_present():
        pytest.skip("needs the reference sources")
    spec = importlib.util.spec_from_file_location("make_dcfr_vectors", os.path.join(GOLDEN, "make_dcfr_vectors.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    keys, legal, tabs, _ = gen.reference_run(game, gen.SETS[name], [1, 2])
    assert "\n".join(keys).encode() == bytes(dcfr[f"{game}/keys"])
    for t in (1, 2):
        assert np.array_equal(tabs[t][0], dcfr[f"{game}/{name}/{t}/regrets"]), (game, name, t)
        assert np.array_equal(tabs[t][1], dcfr[f"{game}/{name}/{t}/cum_policy"]), (game, name, t)


EFR_RUNS = [(g, d) for g in (G1,) for d in ("blind cf", "informed cf", "tips", "bhv")] + \
           [(g, d) for g in (G3, G5) for d in ("blind cf", "informed cf", "tips")]


@pytest.fixture(scope="module")
def efr_exe(tmp_path_factory):
    return efr_cases.build_host_test(str(tmp_path_factory.mktemp("efr") / "efr_host_test"))


def _efr_host(exe, v, r, tmp_path):
    efr_cases.write_case(v, r, tmp_path / "case.bin")
    return subprocess.run([exe, "run", str(tmp_path / "case.bin"), repr(efr_cases.TOLERANCE), str(tmp_path / "state.bin")],
                          capture_output=True, text=True, timeout=120)


def test_efr_runs_are_the_listed_ones(efr, layout):
    assert [(g, d) for _, g, d in efr_cases.runs(efr)] == EFR_RUNS
    for r, game, _ in efr_cases.runs(efr):
        assert efr[f"r{r}/checkpoints"].tolist() == ([1, 3, 5] if game == G5 else [1, 2, 5])   # (2 -> 3: the maker's |R| >= 1e-9 rule)
        assert float(efr[f"r{r}/min_abs_R"]) >= 1e-9 and float(efr[f"r{r}/min_z"]) >= 1e-9
        assert len(efr[f"tree/{game}/parent"]) == int(layout[f"{game}/histories"])
    # the first decision level of G3 is player 1's in the recorded tree too
    tree = {k: efr[f"tree/{G3}/{k}"] for k in ("parent", "kind", "info")}
    first = [h for h in range(len(tree["kind"])) if tree["kind"][h] == 1 and tree["parent"][tree["parent"][tree["parent"][h]]] == -1]
    r3 = [r for r, g, _ in efr_cases.runs(efr) if g == G3][0]
    assert len(first) == 30 and (efr[f"r{r3}/player"][tree["info"][first]] == 1).all()
    assert (efr[f"r{r3}/own_len"][tree["info"][first]] == 0).all()


@pytest.mark.parametrize("r", range(len(EFR_RUNS)), ids=[f"{g}-{d}".replace(" ", "_") for g, d in EFR_RUNS])
def test_efr_header_functions_reproduce_every_recorded_checkpoint(efr_exe, efr, tmp_path, r):
    p = _efr_host(efr_exe, efr, r, tmp_path)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert p.stdout.rstrip().endswith("ok: 3 checkpoints")
    assert "largest deviation" in p.stdout and "FAILED" not in p.stdout and "deviation tables" in p.stdout


# ---- 3. sensitivity -----------------------------------------------------------------------------------------------------
def _default(family):
    with np.load(os.path.join(GOLDEN, f"{family}_vectors.npz")) as z:
        return {k: z[k] for k in z.files}


def test_xfp_comparator_rejects_level_zero_owned_by_player_zero(xfp, xfp_exe, tmp_path):
    """starting_player=1 run through the layout that numbers the levels from player 0 (the default game's own-predecessor
    chains, tests/golden/xfp_vectors.npz): the restatement and the host program both stop matching the recorded run."""
    default = _default("xfp")
    assert default["leduc_poker/pred_info"].shape == xfp[f"{G3}/pred_info"].shape
    assert not np.array_equal(default["leduc_poker/pred_info"], xfp[f"{G3}/pred_info"])
    v = dict(xfp)
    for name in ("pred_info", "pred_action", "player"):
        v[f"{G3}/{name}"] = default[f"leduc_poker/{name}"]
    assert _xfp_restate(v, G3) is not None
    r = _xfp_host(xfp_exe, v, G3, tmp_path / "default_layout.bin")
    assert r.returncode != 0 and not r.stdout.startswith("ok:")


def test_mmd_comparator_rejects_uniform_chance_weights(mmd_exe, mmd, layout, tmp_path):
    """Suit-isomorphic leduc with every terminal's chance weight replaced by the mean weight: the host program's
    comparison with the recorded run fails."""
    chance = layout[f"{G1}/term_chance"]
    cu = mmd[f"{G1}/term_cu"]
    assert chance.shape == (len(cu),) and len(np.unique(chance)) > 1     # unequal weights are in the record
    u = cu[:, 0] / chance                                               # the layout's terminals are MMD's, in its order:
    assert np.abs(u - np.round(u)).max() <= 1e-12 and np.abs(u).max() == 13   # whole chips, up to the full stakes
    assert np.array_equal(cu[:, 0], -cu[:, 1])
    v = dict(mmd)
    v[f"{G1}/term_cu"] = np.round(np.stack([u, -u], axis=1)) * chance.mean()
    _, r = _mmd_host(mmd_exe, v, G1, tmp_path)
    assert r.returncode != 0 and "FAILED" in r.stdout, r.stdout[-2000:]


def test_xfp_comparator_rejects_the_other_tied_action(xfp, xfp_exe, tmp_path):
    """The argmax moved from fold to call where the two tie (action mapping): the averaged policy differs, so which tied
    action the reference takes is part of the record."""
    v = dict(xfp)
    br = v[f"{G2}/br"].copy()
    row = int(np.flatnonzero(br[0] == 0)[0])   # an infostate whose recorded best response is action 0 (fold)
    br[0, row] = 1
    v[f"{G2}/br"] = br
    assert _xfp_restate(v, G2) is not None
    r = _xfp_host(xfp_exe, v, G2, tmp_path / "tied.bin")
    assert r.returncode != 0 and not r.stdout.startswith("ok:")


def test_efr_comparator_rejects_uniform_chance_weights(efr_exe, efr, tmp_path):
    """Suit-isomorphic leduc with every chance row made uniform (1 / its number of outcomes): the host program's run no
    longer meets the recorded checkpoints within efr_cases.TOLERANCE."""
    v = dict(efr)
    parent, kind, prob = (v[f"tree/{G1}/{k}"] for k in ("parent", "kind", "prob"))
    under_chance = np.flatnonzero((parent >= 0) & (kind[np.maximum(parent, 0)] == 0))
    siblings = np.bincount(parent[under_chance], minlength=len(parent))
    flat = prob.copy()
    flat[under_chance] = 1.0 / siblings[parent[under_chance]]
    assert np.abs(flat - prob).max() > 0.1
    v[f"tree/{G1}/prob"] = flat
    efr_cases._cache.pop(("layout", G1), None)   # (the layout is cached per game)
    try:
        p = _efr_host(efr_exe, v, 0, tmp_path)
    finally:
        efr_cases._cache.pop(("layout", G1), None)
    assert p.returncode != 0 and "FAILED" in p.stdout, p.stdout[-2000:]


def test_efr_comparator_rejects_level_zero_owned_by_player_zero(efr_exe, efr, tmp_path):
    """starting_player=1 with the owners exchanged (every infostate given to the other player, as a layout that numbers
    the levels from player 0 would): the deviation tables or the checkpoints stop matching."""
    v = dict(efr)
    r = [r for r, g, d in efr_cases.runs(efr) if g == G3 and d == "informed cf"][0]
    v[f"r{r}/player"] = (1 - v[f"r{r}/player"]).astype(np.int8)
    efr_cases._cache.pop(("layout", G3), None)   # (the layout is cached per game)
    try:
        p = _efr_host(efr_exe, v, r, tmp_path)
    finally:
        efr_cases._cache.pop(("layout", G3), None)
    assert p.returncode != 0 or "FAILED" in p.stdout, p.stdout[-2000:]


# ---- DCFR: a restatement of discounted_cfr.py over the recorded trees -----------------------------------------------------
def _dcfr_restatement(efr, dcfr, game, params, iterations, prob=None, owner=None):
    """_DCFRSolver(alternating, linear averaging, no RM+, *params) in Python floats over the tree variant_efr_vectors.npz
    records for the game (depth first, children in action order: the reference's visiting order), every sum in the
    reference's order; returns {t: (regrets, cum_policy)} in the DCFR goldens' layout.  prob / owner replace the chance
    probabilities / the owner of every information state (the sensitivity cases)."""
    r = [r for r, g, _ in efr_cases.runs(efr) if g == game][0]
    tree = {k: efr[f"tree/{game}/{k}"] for k in ("parent", "kind", "prob", "info", "returns")}
    prob = tree["prob"] if prob is None else prob
    owner = efr[f"r{r}/player"].astype(int) if owner is None else owner
    H, P = len(tree["kind"]), tree["returns"].shape[1]
    kids = [[] for _ in range(H)]
    for h in range(1, H):
        kids[tree["parent"][h]].append(h)
    where = {k: i for i, k in enumerate(bytes(dcfr[f"{game}/keys"]).decode().split("\n"))}
    row = np.array([where[k] for k in efr_cases.keys_of(efr, r)])      # the goldens' row of a tree infostate
    nact = efr[f"r{r}/nact"]
    assert np.array_equal(nact, dcfr[f"{game}/nact"][row])
    I = len(nact)
    reg = [[0.0] * n for n in nact]
    cum = [[0.0] * n for n in nact]
    pol = [[1.0 / n] * n for n in nact]
    alpha, beta, gamma = params
    kind, info, returns = tree["kind"], tree["info"], tree["returns"]

    def walk(h, reach, player, t):
        if kind[h] == 2:
            return [float(x) for x in returns[h]]
        if kind[h] == 0:
            value = [0.0] * P
            for c in kids[h]:
                nxt = list(reach)
                nxt[-1] = nxt[-1] * float(prob[c])
                child = walk(c, nxt, player, t)
                value = [v + float(prob[c]) * u for v, u in zip(value, child)]
            return value
        if all(x == 0 for x in reach[:-1]):
            return [0.0] * P
        i = int(info[h])
        cp = int(owner[i])
        value, children = [0.0] * P, []
        for a, c in enumerate(kids[h]):
            nxt = list(reach)
            nxt[cp] = nxt[cp] * pol[i][a]
            child = walk(c, nxt, player, t)
            value = [v + pol[i][a] * u for v, u in zip(value, child)]
            children.append(child)
        if cp != player:
            return value
        before = after = 1.0
        for x in reach[:cp]:
            before = before * x
        for x in reach[cp + 1:]:
            after = after * x
        cf = before * after
        for a in range(len(children)):
            reg[i][a] = reg[i][a] + cf * (children[a][cp] - value[cp])
            cum[i][a] = cum[i][a] + reach[cp] * pol[i][a] * (t ** gamma)
        return value

    out = {}
    for t in range(1, iterations + 1):
        for player in range(P):
            walk(0, [1.0] * (P + 1), player, t)
            for i in range(I):
                if owner[i] == player:
                    for a in range(nact[i]):
                        reg[i][a] = reg[i][a] * ((t ** alpha / (t ** alpha + 1)) if reg[i][a] >= 0 else (t ** beta / (t ** beta + 1)))
            for i in range(I):   # cfr._update_current_policy: regret matching of every infostate
                total = 0.0
                for x in reg[i]:
                    total = total + (x if x > 0 else 0.0)
                pol[i] = [(x if x > 0 else 0.0) / total for x in reg[i]] if total > 0 else [1.0 / nact[i]] * nact[i]
        tabs = np.zeros((2,) + dcfr[f"{game}/D/1/regrets"].shape)
        for i in range(I):
            tabs[0, row[i], :nact[i]], tabs[1, row[i], :nact[i]] = reg[i], cum[i]
        out[t] = (tabs[0], tabs[1])
    return out


def _dcfr_deviation(got, want):
    """tests/test_z13_gpu_dcfr.py's comparator: the largest difference as a fraction of the table's scale (bound 1e-12)."""
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


DCFR_SETS = {"D": (3 / 2, 0, 2), "L": (1, 1, 1)}


def _dcfr_worst(tabs, dcfr, game, name):
    return max(_dcfr_deviation(tabs[t][k], dcfr[f"{game}/{name}/{t}/{what}"]) for t in (1, 2) for k, what in enumerate(("regrets", "cum_policy")))


@pytest.mark.parametrize("name", list(DCFR_SETS))
@pytest.mark.parametrize("game", [G1, G3, G5])
def test_dcfr_restatement_reproduces_the_recorded_tables(efr, dcfr, game, name):
    worst = _dcfr_worst(_dcfr_restatement(efr, dcfr, game, DCFR_SETS[name], 2), dcfr, game, name)
    print(f"dcfr restatement {game} {name}: worst deviation {worst:.3g} of the table's scale at T = 1, 2")
    assert worst <= 1e-12


def test_dcfr_comparator_rejects_uniform_chance_weights(efr, dcfr):
    parent, kind, prob = (efr[f"tree/{G1}/{k}"] for k in ("parent", "kind", "prob"))
    under_chance = np.flatnonzero((parent >= 0) & (kind[np.maximum(parent, 0)] == 0))
    flat = prob.copy()
    flat[under_chance] = 1.0 / np.bincount(parent[under_chance], minlength=len(parent))[parent[under_chance]]
    assert _dcfr_worst(_dcfr_restatement(efr, dcfr, G1, DCFR_SETS["D"], 2, prob=flat), dcfr, G1, "D") > 1e-12


def test_dcfr_comparator_rejects_level_zero_owned_by_player_zero(efr, dcfr):
    """Alternating updates visit player 0 first: with the owners exchanged the first pass updates the wrong half."""
    r = [r for r, g, _ in efr_cases.runs(efr) if g == G3][0]
    swapped = 1 - efr[f"r{r}/player"].astype(int)
    assert _dcfr_worst(_dcfr_restatement(efr, dcfr, G3, DCFR_SETS["D"], 2, owner=swapped), dcfr, G3, "D") > 1e-12


# ---- action values --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def av_exe(tmp_path_factory):
    return avc.build_host_test(str(tmp_path_factory.mktemp("av") / "action_values_host_test"))


def _av_host(exe, v, game, tmp_path):
    listed = avc.write_cases(v, game, tmp_path / "cases.bin")
    return listed, subprocess.run([exe, str(tmp_path / "cases.bin"), repr(avc.TOLERANCE)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("game", GAMES)
def test_action_value_header_functions_reproduce_every_recorded_case(av_exe, av, layout, tmp_path, game):
    assert int(av[f"{game}/histories"]) == int(layout[f"{game}/histories"])
    listed, r = _av_host(av_exe, av, game, tmp_path)
    assert len(listed) == (3 if game == G5 else 7)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.rstrip().endswith(f"ok: {len(listed)} cases")
    assert r.stdout.count("largest deviation") == len(listed) and "FAILED" not in r.stdout
    assert r.stdout.count("agree bit for bit") == len(listed)


@pytest.mark.parametrize("game", [G2, G4])
def test_recorded_action_values_tie_fold_with_call(av, game):
    """In every case of the action-mapped games there are infostates whose fold and call values are bit-equal, and the
    best responders' recorded choices have exact ties (the lower action is the recorded one)."""
    for case in avc.case_names(av, game):
        q = av[f"{case}/action_values"]
        tied = (q[:, 0].view(np.uint64) == q[:, 1].view(np.uint64)) & (av[f"{case}/cf_reach"] > 0)
        assert tied.sum() >= 1, case
    assert max(int(av[f"{c}/ties"]) for c in avc.case_names(av, game) if int(av[f"{c}/responder"]) >= 0) > 0
    for other in (G1, G3):
        q = av[f"{other}/random/action_values"]
        assert not (q[:, 0].view(np.uint64) == q[:, 1].view(np.uint64)).any()


def test_action_value_comparator_rejects_the_other_tied_action(av_exe, av, tmp_path):
    v = dict(av)
    case = [c for c in avc.case_names(av, G2) if int(av[f"{c}/responder"]) == 0 and int(av[f"{c}/ties"]) > 0][0]
    best = v[f"{case}/best_index"].copy()
    q = av[f"{case}/action_values"]
    rows = np.flatnonzero((best == 0) & (q[:, 0] == q[:, 1]) & (av[f"{case}/cf_reach"] > 0))
    assert len(rows) >= 1
    best[rows[0]] = 1
    v[f"{case}/best_index"] = best
    _, r = _av_host(av_exe, v, G2, tmp_path)
    assert r.returncode != 0 or "FAILED" in r.stdout, r.stdout[-1500:]


def test_action_value_comparator_rejects_uniform_chance_weights(av_exe, av, tmp_path):
    v = dict(av)
    parent, _ = avc.tree_links(av[f"{G1}/nchild"])
    kind, prob = av[f"{G1}/kind"], av[f"{G1}/edge_prob"]
    under_chance = np.flatnonzero((parent >= 0) & (kind[np.maximum(parent, 0)] == 0))
    flat = prob.copy()
    flat[under_chance] = 1.0 / av[f"{G1}/nchild"][parent[under_chance]]
    assert np.abs(flat - prob).max() > 0.1
    v[f"{G1}/edge_prob"] = flat
    _, r = _av_host(av_exe, v, G1, tmp_path)
    assert r.returncode != 0 or "FAILED" in r.stdout, r.stdout[-1500:]


def test_mmd_comparator_rejects_level_zero_owned_by_player_zero(mmd_exe, mmd, tmp_path):
    """starting_player=1 with the terminal payoffs handed to the sequences as if player 0 owned the first level: every
    terminal keeps its two last sequences and gets the other player's chance-weighted payoff.  (Exchanging sequences AND
    payoffs together changes nothing: the terminal lists are filed by the cell's owner, not by a level number.)"""
    v = dict(mmd)
    v[f"{G3}/term_seq"] = np.ascontiguousarray(mmd[f"{G3}/term_seq"][:, ::-1])
    v[f"{G3}/term_cu"] = np.ascontiguousarray(mmd[f"{G3}/term_cu"][:, ::-1])
    _, r = _mmd_host(mmd_exe, v, G3, tmp_path)
    assert r.returncode == 0 and "FAILED" not in r.stdout
    v[f"{G3}/term_seq"] = mmd[f"{G3}/term_seq"]
    _, r = _mmd_host(mmd_exe, v, G3, tmp_path)
    assert r.returncode != 0 or "FAILED" in r.stdout, r.stdout[-1500:]
