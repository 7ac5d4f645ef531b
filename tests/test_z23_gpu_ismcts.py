"""Batched information-set MCTS on the device (osg_ismcts_search; StateBatch.ismcts_search; ISMCTSBot) against
tests/golden/ismcts_vectors.npz — trees that the reference's own ismcts.py built under a random_state scripted from the
device's counter stream (tests/golden/make_ismcts_vectors.py).

No tolerance anywhere.  Every golden case is searched at row `index - index_offset` of batches of 1, 63, 64, 65 and 257
roots whose other rows hold other roots of the game, and everything is compared for equality, doubles bit for bit: status,
policy, sampled action, draws consumed, and the whole tree — every node in creation order with its player, information
state string, total visits and per action visits, return sum and expansion rank.  (The one transcendental in the search,
log() in the UCT term, only decides candidate sets, and the goldens assert a margin of 1e-9 around every decision.)"""
import ctypes as C

import numpy as np
import pytest

import ismcts_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


@pytest.fixture(scope="module")
def cases():
    return ic.load_cases()


@pytest.fixture(scope="module")
def groups(cases):
    """Cases that share a game, the knobs and the seed: one launch can hold them at their own rows."""
    out = {}
    for c in cases:
        out.setdefault((c["game"], c["seed"]) + tuple(c[k] for k in ic.KNOBS), []).append(c)
    return list(out.values())


def _roots_of(cases, game):
    seen = []
    for c in cases:
        if c["game"] == game and c["history"] not in seen:
            seen.append(c["history"])
    return seen


def _batch(ctx, game, histories):
    import open_spiel_amd as osa
    batch = osa.StateBatch(ctx, game, len(histories))
    for t in range(max(len(h) for h in histories)):
        batch.apply_actions(np.array([h[t] if t < len(h) else -1 for h in histories], np.int32))
    return batch


def _knobs(c, **over):
    kw = dict(uct_c=c["uct_c"], max_simulations=c["max_simulations"], n_rollouts=c["n_rollouts"],
              max_world_samples=c["max_world_samples"], final_policy_type=c["final_policy_type"],
              puct=c["child_selection_policy"] == 2, seed=c["seed"])
    kw.update(over)
    return kw


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _check_case(c, out, row, tree=None):
    A = 2 if c["game"].startswith("kuhn") else 3
    host = {k: v.cpu().numpy() for k, v in out.items() if k not in ("trees", "draws")}
    root = c["nodes"][0]
    where = (c["game"], c["index"], c["max_simulations"])
    assert host["status"][row] == c["status"], where
    assert host["sampled_action"][row] == c["sampled_action"], where
    assert host["nodes"][row] == len(c["nodes"]), where
    assert _same_bits(host["policy"][row], c["policy"][:A]), where
    assert (host["child_visits"][row] == root[3][:A]).all() and (host["expansion_rank"][row] == root[5][:A]).all(), where
    assert _same_bits(host["child_return_sum"][row], root[4][:A]), where
    if tree is not None:
        assert int(out["draws"][row]) == c["draws"], where
        assert len(tree["key"]) == len(c["nodes"])
        for i, (player, key, total, visits, sums, rank) in enumerate(c["nodes"]):
            assert (tree["player"][i], tree["key"][i], tree["total_visits"][i]) == (player, key, total), (where, i)
            assert (tree["visits"][i] == visits).all() and (tree["rank"][i] == rank).all(), (where, i)
            assert _same_bits(tree["return_sum"][i], sums), (where, i)


@pytest.mark.parametrize("size", ic.BATCH_SIZES)
def test_every_golden_case_at_its_row(ctx, cases, groups, size):
    checked = 0
    for group in groups:
        game = group[0]["game"]
        fill = _roots_of(cases, game)
        by_offset = {}
        for c in group:
            by_offset.setdefault(c["index"] - c["index"] % size, []).append(c)
        for offset, members in by_offset.items():
            rows = {c["index"] - offset: c for c in members}
            batch = _batch(ctx, game, [rows[r]["history"] if r in rows else fill[(7 * r + 3) % len(fill)] for r in range(size)])
            out = batch.ismcts_search(**_knobs(group[0], index_offset=offset, want_tree=sorted(rows)))
            for row, c in rows.items():
                _check_case(c, out, row, out["trees"][row])
                checked += 1
    assert checked == len(cases)


def _leduc_group(groups):
    return max((g for g in groups if g[0]["game"] == "leduc_poker(players=3)" and g[0]["max_simulations"] == 50), key=len)


def _all_outputs(batch, **kw):
    out = batch.ismcts_search(**kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_split_batches_repeated_calls_and_host_outputs_agree(ctx, cases, groups):
    import open_spiel_amd as osa
    from open_spiel_amd import _abi
    group = _leduc_group(groups)
    game, n, k = group[0]["game"], 257, 100
    fill = _roots_of(cases, game)
    histories = [fill[(5 * r + 1) % len(fill)] for r in range(n)]
    whole = _all_outputs(_batch(ctx, game, histories), **_knobs(group[0]))
    assert (whole["status"] == 0).all() and (whole["nodes"] > 1).all()
    again = _all_outputs(_batch(ctx, game, histories), **_knobs(group[0]))
    low = _all_outputs(_batch(ctx, game, histories[:k]), **_knobs(group[0]))
    high = _all_outputs(_batch(ctx, game, histories[k:]), **_knobs(group[0], index_offset=k))
    for name, value in whole.items():
        assert value.tobytes() == again[name].tobytes(), name                                   # two identical calls
        assert value.tobytes() == np.concatenate([low[name], high[name]]).tobytes(), name        # [0, k) and [k, n)
    # host pointers (on_host = 1) against the device tensors
    c = group[0]
    cfg = _abi.IsmctsCfg(c["uct_c"], c["max_simulations"], c["n_rollouts"], c["max_world_samples"], c["final_policy_type"],
                         c["child_selection_policy"], 0, c["seed"], 0)
    batch = _batch(ctx, game, histories)
    A = 3
    host = dict(policy=np.empty((n, A)), sampled_action=np.empty(n, np.int32), child_visits=np.empty((n, A), np.int32),
                child_return_sum=np.empty((n, A)), expansion_rank=np.empty((n, A), np.int32), nodes=np.empty(n, np.int32),
                status=np.empty(n, np.uint8))
    _abi.check(osa.lib().osg_ismcts_search(batch._h, C.byref(cfg), *[a.ctypes.data for a in host.values()], 1))
    for name, value in whole.items():
        assert value.tobytes() == host[name].tobytes(), name


def test_capacity_edges(ctx, cases):
    """max_nodes = K (the nodes the case builds) finishes with the reference's tree; K - 1 stops with status 2."""
    for game in ic.GAMES:
        c = max((c for c in cases if c["game"] == game), key=lambda c: len(c["nodes"]))
        k = len(c["nodes"])
        batch = _batch(ctx, game, [c["history"]])
        out = batch.ismcts_search(**_knobs(c, index_offset=c["index"], max_nodes=k, want_tree=[0]))
        _check_case(c, out, 0, out["trees"][0])
        out = batch.ismcts_search(**_knobs(c, index_offset=c["index"], max_nodes=k - 1, want_tree=[0]))
        assert out["status"].cpu()[0] == 2 and out["nodes"].cpu()[0] == k - 1 and out["sampled_action"].cpu()[0] == -1
        assert np.isnan(out["policy"].cpu().numpy()).all()
        tree = out["trees"][0]   # what was built before the table filled is the reference's tree so far
        assert [(p, key) for p, key in zip(tree["player"], tree["key"])] == [(n[0], n[1]) for n in c["nodes"][:k - 1]]


def test_single_action_rows_consume_nothing(ctx, cases):
    """Neither game has a decision node with one legal action under its rules (kuhn_poker always offers pass and bet;
    leduc_poker's raise cap is only reached facing a raise, where fold and call remain), so the row is made from a capped
    leduc_poker root by raising the mover's ante to the stakes in the raw record: only `call` is left."""
    game = "leduc_poker"
    capped = next(c for c in cases if c["game"] == game and _legal(c) == [0, 1])
    other = next(c for c in cases if c["game"] == game and c is not capped)
    batch = _batch(ctx, game, [other["history"], capped["history"], other["history"]])
    words = batch.raw_words()
    w0 = int(words[0, 1])
    mover, stakes = (w0 & 7) - 1, (w0 >> 8) & 15
    w0 = (w0 & ~(15 << (42 + 4 * mover))) | (stakes << (42 + 4 * mover))
    words[0, 1] = w0
    batch.load_raw_words(words)
    assert int(batch.legal_actions_mask_bits().cpu()[1, 0]) == 2
    out = batch.ismcts_search(**_knobs(other, want_tree=[0, 1]))
    assert out["status"].cpu()[1] == 0 and out["nodes"].cpu()[1] == 0 and int(out["draws"][1]) == 0
    assert out["policy"].cpu().numpy()[1].tolist() == [0.0, 1.0, 0.0] and out["sampled_action"].cpu()[1] == 1
    assert len(out["trees"][1]["key"]) == 0
    assert out["nodes"].cpu()[0] >= 1 and int(out["draws"][0]) > 0


def _legal(c):
    """The legal actions of a leduc_poker golden root, from its information state: fold only facing a raise, raise below
    the cap of two raises in the round."""
    _, _, pub, r1, r2 = ic.node_ident(c["game"], c["nodes"][0][0], c["nodes"][0][1])
    moves = r2 if pub >= 0 else r1
    return ([0] if 2 in moves else []) + [1] + ([2] if sum(m == 2 for m in moves) < 2 else [])


def test_refusals(ctx):
    import open_spiel_amd as osa
    with pytest.raises(osa.OsgError, match="kuhn_poker and leduc_poker"):
        osa.StateBatch(ctx, "hex(board_size=3)", 4).ismcts_search(max_simulations=4)
    with pytest.raises(osa.OsgError, match="2 or 3 players"):
        _batch(ctx, "leduc_poker(players=4)", [[0, 1, 2, 3]] * 2).ismcts_search(max_simulations=4)
    decision, chance, terminal = [0, 1], [0], [0, 1, 0, 0]
    with pytest.raises(osa.OsgError, match="root 5 is a chance node"):
        _batch(ctx, "kuhn_poker", [decision] * 5 + [chance, decision, chance]).ismcts_search(max_simulations=4)
    with pytest.raises(osa.OsgError, match="root 3 is terminal"):
        _batch(ctx, "kuhn_poker", [decision] * 3 + [terminal, chance]).ismcts_search(max_simulations=4)
    for bad in (dict(max_simulations=0), dict(n_rollouts=0), dict(final_policy_type=4), dict(max_nodes=(1 << 24) + 1)):
        with pytest.raises(osa.OsgError):
            _batch(ctx, "kuhn_poker", [decision]).ismcts_search(**bad)
    for unsupported in (dict(evaluator=object()), dict(use_observation_string=True), dict(allow_inconsistent_action_sets=True)):
        with pytest.raises(ValueError):
            osa.ISMCTSBot("kuhn_poker", 2.0, 10, ctx=ctx, **unsupported)
    with pytest.raises(ValueError):
        osa.ISMCTSBot("kuhn_poker", 2.0, 10, ctx=ctx).set_resampler(lambda s, p: s)


def test_bot_on_a_mirror_state_equals_the_golden_case(ctx, cases):
    import open_spiel_amd as osa
    pyspiel = osa.pyspiel_hip
    for game in ic.GAMES:
        for c in [c for c in cases if c["game"] == game and c["status"] == 0][:3]:
            state = pyspiel.load_game(game).new_initial_state()
            for a in c["history"]:
                state.apply_action(a)
            bot = osa.ISMCTSBot(game, c["uct_c"], c["max_simulations"], max_world_samples=c["max_world_samples"] or -1,
                                seed=c["seed"], final_policy_type=osa.ISMCTSFinalPolicyType(c["final_policy_type"]),
                                child_selection_policy=osa.ChildSelectionPolicy(c["child_selection_policy"]),
                                n_rollouts=c["n_rollouts"], index=c["index"], ctx=ctx)
            policy, action = bot.step_with_policy(state)
            rank = c["nodes"][0][5]
            legal = state.legal_actions()
            order = sorted((a for a in legal if rank[a] >= 0), key=lambda a: rank[a]) + [a for a in legal if rank[a] < 0]
            assert [a for a, _ in policy] == order and action == c["sampled_action"]
            assert _same_bits(np.array([p for _, p in policy]), c["policy"][order])
            assert bot.index == c["index"] + 1
        # a chance node: the reference's invalid-action answers
        bot = osa.ISMCTSBot(game, 2.0, 10, ctx=ctx)
        assert bot.step(pyspiel.load_game(game).new_initial_state()) == -1
