"""Deep CFR on the device (osg_cfr_infostate_tensors, osg_reservoir_*, osg_deep_cfr_traverse / _staged in
include/osg_abi.h; open_spiel_amd.deep_cfr) against the goldens the reference's own deep_cfr.py produced
(tests/golden/make_deep_cfr_vectors.py), the NumPy restatement (tests/deep_cfr_cases.py) and, independently of both, the
counterfactual regrets TabularSolver.action_values gives for the same strategy table.

The goldens and the restatement number the infostates in order of first depth-first visit, the solver level by level:
rows are compared after mapping the device's indices through the infostate strings.

Measured on an MI355X (profiles/deep_cfr_probe.txt): every comparison with the goldens and the restatement is exact; in the
statistical test the largest |mean - regret| is 0.0045 (player 0) and 0.0034 (player 1) against the Hoeffding bound 0.194."""
import numpy as np
import pytest

import deep_cfr_cases as dc
import sampling_stats as st

pytestmark = pytest.mark.gpu

GAMES = ("kuhn_poker", "kuhn_poker(players=3)", "leduc_poker")


@pytest.fixture(scope="module")
def osa():
    import open_spiel_amd
    return open_spiel_amd


@pytest.fixture(scope="module")
def ctx(osa):
    return osa.Context(0)


@pytest.fixture(scope="module")
def solvers(osa, ctx):
    """game -> (solver, tree, gold_of_dev [I], dev_of_gold [I])."""
    cache = {}

    def get(game):
        if game not in cache:
            solver = osa.TabularSolver(ctx, game, mccfr=True)
            keys, _, _ = dc.golden_game(game)
            index = {k: i for i, k in enumerate(keys)}
            gold_of_dev = np.array([index[k] for k in solver.tables()["keys"]], np.int64)
            assert sorted(gold_of_dev.tolist()) == list(range(len(keys)))
            cache[game] = (solver, dc.golden_tree(game), gold_of_dev, np.argsort(gold_of_dev))
        return cache[game]

    return get


def _device_table(torch, ctx, advantages, gold_of_dev):
    return torch.from_numpy(np.ascontiguousarray(advantages[gold_of_dev], np.float32)).to(ctx.device)


def _staged(solver, gold_of_dev):
    s = solver.deep_cfr_staged()
    rows = {}
    for k in ("adv", "strat"):
        info = s[k + "_info"].cpu().numpy()
        rows[k] = (s[k + "_offsets"].cpu().numpy(), gold_of_dev[info].astype(np.int32), s[k + "_values"].cpu().numpy())
    return rows["adv"], rows["strat"], s["draws"].cpu().numpy(), s["bounds"]


def _state(buf, gold_of_dev):
    info, it, vals = buf.filled()
    return buf.add_calls, gold_of_dev[info.cpu().numpy()].astype(np.int32), it.cpu().numpy(), vals.cpu().numpy()


@pytest.mark.parametrize("game", GAMES)
def test_infostate_tensors_are_the_recorded_ones(solvers, game):
    solver, tree, gold_of_dev, dev_of_gold = solvers(game)
    _, tensors, player = dc.golden_game(game)
    host = solver.infostate_tensors(device=False)
    assert host.shape == tensors.shape and host.dtype == np.float32
    assert np.array_equal(host[dev_of_gold], tensors)
    assert np.array_equal(solver.infostate_tensors().cpu().numpy(), host)
    assert np.array_equal(solver.infostate_players()[dev_of_gold], player)


@pytest.mark.parametrize("r", range(len(dc.golden_runs())))
def test_traverse_reproduces_every_recorded_step(osa, ctx, solvers, r):
    import torch
    meta, steps = dc.golden_run(r)
    solver, tree, gold_of_dev, _ = solvers(meta["game"])
    P, A = meta["players"], tree.num_actions
    buffers = [osa.ReservoirBuffer(ctx, A, meta["capacity"], meta["res_seed"], b) for b in range(P + 1)]
    before = solver.tables()["regrets"].copy()
    for s, step in enumerate(steps):
        T = len(step["draws"])
        counts = solver.deep_cfr_traverse(_device_table(torch, ctx, step["advantages"], gold_of_dev), step["player"], step["iteration"],
                                          meta["seed"], T, step["first"], buffers[step["player"]], buffers[P])
        adv, strat, draws, bounds = _staged(solver, gold_of_dev)
        assert counts == (len(step["adv"][1]), len(step["strat"][1]))
        assert dc.same_rows(adv, step["adv"]), (r, s)                 # the rows per trajectory and their order
        assert dc.same_rows(strat, step["strat"]), (r, s)
        assert np.array_equal(draws, step["draws"])
        assert bounds == tuple(max(b, 1) for b in dc.row_bounds(tree, step["player"]))
        for b, want in step["buffers"].items():
            assert dc.same_buffer(_state(buffers[b], gold_of_dev), want), (r, s, b)
        for b, buf in enumerate(buffers):
            assert (b in step["buffers"]) == (buf.add_calls > 0)
    assert np.array_equal(solver.tables()["regrets"], before)        # the solver's tables are not touched


def _synthetic_call(osa, ctx, torch, solvers, game, seed, calls, capacity=37):
    """calls: [(first, count)] against one pair of buffers -> per call (adv, strat, draws), and the buffers' states."""
    solver, tree, gold_of_dev, _ = solvers(game)
    A = tree.num_actions
    adv = dc.synthetic_advantages(tree, seed)
    player = seed % tree.num_players
    table = _device_table(torch, ctx, adv, gold_of_dev)
    bufs = [osa.ReservoirBuffer(ctx, A, capacity, 77, b) for b in range(2)]
    mine = [dc.Reservoir(capacity, A, 77, b) for b in range(2)]
    out = []
    for first, count in calls:
        solver.deep_cfr_traverse(table, player, 3, seed, count, first, bufs[0], bufs[1])
        got = _staged(solver, gold_of_dev)
        want = dc.run_step(tree, adv, player, 3, seed, first, count, mine[0], mine[1])
        out.append((got, want))
    return tree, out, [_state(b, gold_of_dev) for b in bufs], [m.state() for m in mine]


@pytest.mark.parametrize("count", dc.BATCH_SIZES)
@pytest.mark.parametrize("game", GAMES)
def test_synthetic_tables_equal_the_restatement(osa, ctx, solvers, game, count):
    import torch
    tree, out, got_bufs, want_bufs = _synthetic_call(osa, ctx, torch, solvers, game, 40 + count, [(1000 + count, count)])
    (adv, strat, draws, _), want = out[0]
    A = tree.num_actions
    assert dc.same_rows(adv, dc.flatten([w[0] for w in want], A))
    assert dc.same_rows(strat, dc.flatten([w[1] for w in want], A))
    assert np.array_equal(draws, np.array([w[2] for w in want], np.int32))
    for g, w in zip(got_bufs, want_bufs):
        assert dc.same_buffer(g, w)


def test_two_consecutive_calls_equal_one(osa, ctx, solvers):
    import torch
    game = "leduc_poker"
    _, one, one_bufs, want_bufs = _synthetic_call(osa, ctx, torch, solvers, game, 9, [(50, 65)])
    _, two, two_bufs, _ = _synthetic_call(osa, ctx, torch, solvers, game, 9, [(50, 22), (72, 43)])
    whole = one[0][0]
    for k in (0, 1):
        assert np.array_equal(whole[k][1], np.concatenate([two[0][0][k][1], two[1][0][k][1]]))
        assert np.array_equal(whole[k][2].view(np.uint32), np.concatenate([two[0][0][k][2], two[1][0][k][2]]).view(np.uint32))
    assert np.array_equal(whole[2], np.concatenate([two[0][0][2], two[1][0][2]]))
    for a, b, w in zip(one_bufs, two_bufs, want_bufs):
        assert dc.same_buffer(a, b) and dc.same_buffer(a, w)


@pytest.mark.parametrize("capacity,calls", [(1, (5, 3)), (7, (40, 33)), (100, (60, 70)), (64, (64, 1, 300))])
def test_append_is_the_sequential_appends(osa, ctx, capacity, calls):
    """capacity 1; a capacity below one call's rows (several rows of a call meet in a slot); add_calls crossing the
    capacity inside a call; a call that ends exactly at the capacity; later calls continuing."""
    import torch
    A = 3
    rng = np.random.default_rng(capacity)
    buf = osa.ReservoirBuffer(ctx, A, capacity, 123, 4)
    mine = dc.Reservoir(capacity, A, 123, 4)
    assert len(buf) == 0 and buf.add_calls == 0
    for it, m in enumerate(calls, start=1):
        info = rng.integers(0, 1000, m).astype(np.int32)
        vals = rng.standard_normal((m, A)).astype(np.float32)
        buf.append(torch.from_numpy(info).to(ctx.device), it, torch.from_numpy(vals).to(ctx.device))
        mine.append_many(info, it, vals)
        got = buf.filled()
        assert dc.same_buffer((buf.add_calls, got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()), mine.state())
        assert len(buf) == len(mine)
    m = min(5, len(mine))
    slots = buf.sample_slots(m, 31, 2)
    want = mine.sample(31, 2, m)
    assert np.array_equal(slots.cpu().numpy(), want) and len(set(want.tolist())) == m and want.max() < len(mine)
    info, it, vals = buf.rows(slots)
    assert np.array_equal(info.cpu().numpy(), mine.info[want]) and np.array_equal(it.cpu().numpy(), mine.iteration[want])
    assert np.array_equal(vals.cpu().numpy().view(np.uint32), mine.values[want].view(np.uint32))
    with pytest.raises(ValueError):
        buf.sample_slots(len(mine) + 1, 31, 2)
    buf.clear()
    assert len(buf) == 0 and buf.add_calls == 0


def test_several_rows_of_one_call_meet_in_one_slot():
    """The case the append test is there for exists in its inputs: with capacity 7, the 33 rows of the second call hit
    some slot more than once."""
    mine = dc.Reservoir(7, 1, 123, 4)
    for n in range(40):
        mine.append(n, 1, [0.0])
    first = len(mine.writes)
    for n in range(33):
        mine.append(n, 2, [0.0])
    writes = [w for w in mine.writes[first:] if w >= 0]
    assert len(writes) > len(set(writes))


def test_sampled_advantages_average_to_the_counterfactual_regrets(osa, ctx, solvers):
    """Independent of the restatement: on leduc_poker with a fixed synthetic table, the per-infostate sum of the
    traverser's advantage rows over N trajectories, divided by N, against sum_h cf_reach(h) (Q(h, a) - V(h)) from
    TabularSolver.action_values with the same strategy table.  A trajectory visits an infostate of the traverser at most
    once and a row entry is a difference of two values in [min_utility, max_utility]: |X| <= c = max - min, a range of
    2 c, Hoeffding at delta = 1e-9 over all compared entries."""
    import torch
    game = "leduc_poker"
    solver, tree, gold_of_dev, dev_of_gold = solvers(game)
    desc = osa.describe(game)
    c = desc.max_utility - desc.min_utility
    I, A = tree.num_infostates, tree.num_actions
    adv = dc.synthetic_advantages(tree, 2024)
    table_gold, _ = dc.strategy_table(tree, adv)                      # by action id, golden order
    tab = solver.tables()
    legal, nact = tab["legal"], tab["nact"]
    table_dev = table_gold[gold_of_dev]
    by_legal = np.where(legal >= 0, np.take_along_axis(table_dev, np.clip(legal, 0, None), 1), 0.0)
    av = solver.action_values(which="table", table=by_legal)
    q = av["cf_reach_by_value"]                                       # [I, Amax] by legal index
    regret = q - (by_legal * q).sum(1, keepdims=True)
    N, chunk = 1 << 20, 1 << 18      # the bound falls as 1 / sqrt(N): 0.194 here, under either player's largest regret
    players = solver.infostate_players()
    worst = 0.0
    for player in range(2):
        total = torch.zeros((I, A), dtype=torch.float64, device=ctx.device)
        for first in range(0, N, chunk):
            solver.deep_cfr_traverse(_device_table(torch, ctx, adv, gold_of_dev), player, 1, 0xC0FFEE, chunk, player * N + first)
            s = solver.deep_cfr_staged()
            total.index_add_(0, s["adv_info"].long(), s["adv_values"].double())
        mean_by_id = (total / N).cpu().numpy()
        mean = np.where(legal >= 0, np.take_along_axis(mean_by_id, np.clip(legal, 0, None), 1), 0.0)
        rows = players == player
        cells = int(nact[rows].sum())
        bound = st.hoeffding_bound(N, 2 * c, m=2 * cells)
        err = np.abs(mean - regret)[rows][legal[rows] >= 0]
        print(f"player {player}: {cells} entries, largest |mean - regret| {err.max():.4f}, bound {bound:.4f}, "
              f"largest |regret| {np.abs(regret[rows]).max():.3f}")
        worst = max(worst, float(err.max() / bound))
        assert err.max() <= bound
        assert np.abs(mean[~rows]).max() == 0.0                       # only the traverser's infostates get advantage rows
        # the check has something to see: rows of zeros (and so rows of the wrong sign) would miss the bound at the
        # player's largest regret (0.43 and 0.23 by action_values; N is chosen for that)
        assert np.abs(regret[rows]).max() > bound
    print(f"worst ratio to the bound {worst:.3f}")


def test_solver_runs_the_references_loop(osa, ctx, solvers):
    import torch
    game = "kuhn_poker"
    _, tree, gold_of_dev, _ = solvers(game)
    solver = osa.DeepCFRSolver(ctx, game, policy_network_layers=(8,), advantage_network_layers=(8,), num_iterations=3,
                               num_traversals=16, learning_rate=1e-2, batch_size_advantage=8, batch_size_strategy=8,
                               memory_capacity=40, seed=5)
    steps = []
    solver.step_callback = lambda it, p, table: steps.append((it, p, table.cpu().numpy().copy()))
    net, losses, policy_loss = solver.solve()
    assert net is solver._policy_network and set(losses) == {0, 1} and all(len(v) == 3 for v in losses.values())
    assert policy_loss is not None and np.isfinite(policy_loss)
    assert [(it, p) for it, p, _ in steps] == [(it, p) for it in (1, 2, 3) for p in (0, 1)]
    # the restatement's replay of the same steps, from the tables the networks gave
    from open_spiel_amd import deep_cfr
    res_seed = (5 ^ deep_cfr.RESERVOIR_SALT) & dc.M64
    mine = [dc.Reservoir(40, tree.num_actions, res_seed, b) for b in range(3)]
    dev_of_gold = np.argsort(gold_of_dev)
    for it, p, table in steps:
        dc.run_step(tree, table[dev_of_gold], p, it, 5, ((it - 1) * 2 + p) * 16, 16, mine[p], mine[2])
    bufs = solver.advantage_buffers + [solver.strategy_buffer]
    assert [b.add_calls for b in bufs] == [m.add_calls for m in mine]
    assert all(b.add_calls > 40 for b in bufs)
    for b, m in zip(bufs, mine):
        assert dc.same_buffer(_state(b, gold_of_dev), m.state())
    table = solver.policy_table()
    legal = solver.tabular.tables()["legal"]
    assert table.shape == legal.shape and (table >= 0).all() and (table[legal < 0] == 0).all()
    assert np.abs(table.sum(1) - 1.0).max() < 1e-12
    conv = solver.nash_conv()
    print(f"kuhn_poker after 3 iterations of 16 traversals: NashConv {conv:.4f}")
    assert np.isfinite(conv) and conv >= -1e-12
