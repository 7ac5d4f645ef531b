"""NFSP on the device (osg_transition_ring_*, osg_nfsp_collect / _staged in include/osg_abi.h; open_spiel_amd.nfsp)
against the goldens the reference's own nfsp.py and dqn.py produced (tests/golden/make_nfsp_vectors.py), the NumPy
restatement (tests/nfsp_cases.py) and, independently of both, the reaches and returns TabularSolver.action_values and
profile_returns give for the same behavioural tables.

The goldens and the restatement number the infostates in order of first depth-first visit, the solver level by level:
rows are compared after mapping the device's indices through the infostate strings.

Measured on an MI355X (profiles/nfsp_probe.txt): every comparison with the goldens and the restatement is exact; in the
statistical test (2^18 leduc_poker episodes) the largest |supervised rows / N - expectation| over the 936 infostates is
0.00087 against the Hoeffding bound 0.00734, and the largest |mean terminal reward - expectation| 0.0024 against 0.1909."""
import math

import numpy as np
import pytest

import deep_cfr_cases as dc
import nfsp_cases as nc
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
            keys, _, _ = nc.golden_game(game)
            index = {k: i for i, k in enumerate(keys)}
            gold_of_dev = np.array([index[k] for k in solver.tables()["keys"]], np.int64)
            assert sorted(gold_of_dev.tolist()) == list(range(len(keys)))
            cache[game] = (solver, nc.golden_tree(game), gold_of_dev, np.argsort(gold_of_dev))
        return cache[game]

    return get


def _device_table(torch, ctx, table, gold_of_dev):
    return torch.from_numpy(np.ascontiguousarray(table[gold_of_dev], np.float32)).to(ctx.device)


def _gold(gold_of_dev, info):
    return np.where(info >= 0, gold_of_dev[np.clip(info, 0, None)], -1).astype(np.int32)


def _staged(solver, gold_of_dev):
    s = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in solver.nfsp_staged().items()}
    ring = (s["ring_offsets"], _gold(gold_of_dev, s["ring_info"]), s["ring_action"], s["ring_reward"], _gold(gold_of_dev, s["ring_next"]),
            s["ring_final"])
    sl = (s["sl_offsets"], _gold(gold_of_dev, s["sl_info"]), s["sl_probs"])
    return dict(draws=s["draws"], modes=s["modes"], ring=ring, sl=sl), s["bounds"]


def _ring_state(ring, gold_of_dev):
    info, action, reward, nxt, final = (t.cpu().numpy() for t in ring.filled())
    return ring.entry_index, _gold(gold_of_dev, info), action, reward, _gold(gold_of_dev, nxt), final


def _res_state(buf, gold_of_dev):
    info, _, vals = buf.filled()
    return buf.add_calls, _gold(gold_of_dev, info.cpu().numpy()), vals.cpu().numpy()


def _buffers(osa, ctx, P, A, ring_cap, res_cap, res_seed):
    from open_spiel_amd.nfsp import TransitionRing
    return [TransitionRing(ctx, ring_cap) for _ in range(P)], [osa.ReservoirBuffer(ctx, A, res_cap, res_seed, p) for p in range(P)]


@pytest.mark.parametrize("r", range(len(nc.golden_runs())))
def test_collect_reproduces_every_recorded_chunk(osa, ctx, solvers, r):
    import torch
    meta, chunks = nc.golden_run(r)
    solver, tree, gold_of_dev, _ = solvers(meta["game"])
    P, A = meta["players"], tree.num_actions
    rings, reservoirs = _buffers(osa, ctx, P, A, meta["ring_capacity"], meta["res_capacity"], meta["res_seed"])
    q, avg = _device_table(torch, ctx, meta["q"], gold_of_dev), _device_table(torch, ctx, meta["avg"], gold_of_dev)
    before = solver.tables()["regrets"].copy()
    steps = np.zeros((P, 2), np.int64)
    for c, chunk in enumerate(chunks):
        totals = solver.nfsp_collect(q, avg, meta["eps"], meta["anticipatory"], meta["seed"], len(chunk["draws"]), chunk["first"],
                                     rings, reservoirs)
        got, bounds = _staged(solver, gold_of_dev)
        assert nc.same_chunk(got, chunk), (r, c)                          # the rows per episode, their order, draws, modes
        assert np.array_equal(totals, nc.totals(chunk, P))
        steps += totals[:, 2:]
        assert np.array_equal(steps[:, 0], chunk["dqn_steps"]) and np.array_equal(steps[:, 1], chunk["nfsp_steps"])
        assert bounds == tuple(nc.row_bound(tree, p) for p in range(P))
        for p in range(P):
            assert nc.same_ring(_ring_state(rings[p], gold_of_dev), chunk["rings"][p]), (r, c, p)
            assert nc.same_reservoir(_res_state(reservoirs[p], gold_of_dev), chunk["reservoirs"][p]), (r, c, p)
    assert np.array_equal(solver.tables()["regrets"], before)            # the solver's tables are not touched


def _synthetic(osa, ctx, torch, solvers, game, seed, calls, ring_cap=11, res_cap=9, ties=False, eps=0.25, anticipatory=0.6, skip=None):
    """calls: [(first, count)] against one set of buffers -> per call (got chunk, wanted chunk, totals), the buffers'
    states on the device and in the restatement.  skip: a player whose buffers are NULL."""
    solver, tree, gold_of_dev, _ = solvers(game)
    P, A = tree.num_players, tree.num_actions
    q, avg = nc.synthetic_tables(tree, seed, ties)
    e, a = np.linspace(eps, eps + 0.2, P), np.linspace(anticipatory, anticipatory - 0.2, P)
    rings, reservoirs = _buffers(osa, ctx, P, A, ring_cap, res_cap, 77)
    mine = ([nc.Ring(ring_cap) for _ in range(P)], [dc.Reservoir(res_cap, A, 77, p) for p in range(P)])
    if skip is not None:
        rings[skip] = reservoirs[skip] = mine[0][skip] = mine[1][skip] = None
    dq, davg = _device_table(torch, ctx, q, gold_of_dev), _device_table(torch, ctx, avg, gold_of_dev)
    out = []
    for first, count in calls:
        totals = solver.nfsp_collect(dq, davg, e, a, seed, count, first, rings, reservoirs)
        got, _ = _staged(solver, gold_of_dev)
        want = nc.flatten_chunk(nc.run_chunk(tree, q, avg, e, a, seed, first, count, *mine), P, A)
        out.append((got, want, totals))
    got_state = [(None if r is None else _ring_state(r, gold_of_dev), None if b is None else _res_state(b, gold_of_dev))
                 for r, b in zip(rings, reservoirs)]
    want_state = [(None if r is None else r.state(), None if b is None else nc.reservoir_state(b)) for r, b in zip(*mine)]
    return tree, out, got_state, want_state


def _same_states(a, b):
    return all((x[0] is None and y[0] is None) or (nc.same_ring(x[0], y[0]) and nc.same_reservoir(x[1], y[1])) for x, y in zip(a, b))


@pytest.mark.parametrize("count", nc.EPISODE_COUNTS)
@pytest.mark.parametrize("game", GAMES)
def test_synthetic_tables_equal_the_restatement(osa, ctx, solvers, game, count):
    """1, 63, 64, 65 and 257 episodes (a lane, a wave less one, a wave, a wave and one, more than a block) from a
    non-zero first episode, into buffers smaller than one call's rows."""
    import torch
    tree, out, got_state, want_state = _synthetic(osa, ctx, torch, solvers, game, 40 + count, [(1000 + count, count)])
    got, want, totals = out[0]
    assert nc.same_chunk(got, want)
    assert np.array_equal(totals, nc.totals(want, tree.num_players))
    assert _same_states(got_state, want_state)


def test_two_consecutive_calls_equal_one(osa, ctx, solvers):
    import torch
    game = "leduc_poker"
    tree, one, one_state, want_state = _synthetic(osa, ctx, torch, solvers, game, 9, [(50, 65)])
    _, two, two_state, _ = _synthetic(osa, ctx, torch, solvers, game, 9, [(50, 22), (72, 43)])
    whole, head, tail = one[0][0], two[0][0], two[1][0]
    assert np.array_equal(whole["draws"], np.concatenate([head["draws"], tail["draws"]]))
    assert np.array_equal(whole["modes"], np.concatenate([head["modes"], tail["modes"]]))
    P = tree.num_players
    for key, same in (("ring", nc.same_ring_rows), ("sl", nc.same_sl_rows)):
        for p in range(P):                                           # player p's rows of the whole = its rows of the two parts
            def part(chunk, p=p, key=key):
                E = len(chunk["draws"])
                lo, hi = chunk[key][0][p * E], chunk[key][0][(p + 1) * E]
                return tuple(col[lo:hi] for col in chunk[key][1:])
            joined = tuple(np.concatenate([x, y]) for x, y in zip(part(head), part(tail)))
            assert same((np.zeros(0),) + part(whole), (np.zeros(0),) + joined)
    assert np.array_equal(one[0][2], two[0][2] + two[1][2])
    assert _same_states(one_state, two_state) and _same_states(one_state, want_state)      # bit-identical in every buffer


@pytest.mark.parametrize("ring_cap,res_cap", [(1, 1), (3, 2)])
def test_tiny_capacities(osa, ctx, solvers, ring_cap, res_cap):
    """Ring capacity 1, and capacities far below one call's rows: every slot is fought over by many rows of the call."""
    import torch
    _, out, got_state, want_state = _synthetic(osa, ctx, torch, solvers, "kuhn_poker", 21, [(0, 65), (65, 64)], ring_cap, res_cap)
    assert all(nc.same_chunk(g, w) for g, w, _ in out)
    assert out[0][2][:, 0].min() > 2 * ring_cap
    assert _same_states(got_state, want_state)


def test_null_buffers_for_one_player(osa, ctx, solvers):
    import torch
    _, out, got_state, want_state = _synthetic(osa, ctx, torch, solvers, "kuhn_poker(players=3)", 5, [(7, 65)], skip=1)
    assert nc.same_chunk(out[0][0], out[0][1]) and out[0][2][1, 0] > 0           # the rows are staged and counted all the same
    assert got_state[1] == (None, None) and _same_states(got_state, want_state)
    solver, tree, gold_of_dev, _ = solvers("kuhn_poker")
    q, avg = nc.synthetic_tables(tree, 1)
    totals = solver.nfsp_collect(_device_table(torch, ctx, q, gold_of_dev), _device_table(torch, ctx, avg, gold_of_dev), 0.1, 0.5, 3, 10)
    assert totals[:, 0].min() >= 10                                                # no buffers at all


def test_a_tie_in_q_goes_to_the_first_legal_id(osa, ctx, solvers):
    """A table built with equal entries: every legal entry of a row equal (illegal ids larger), equal after a smaller
    first one, or a single maximum at the last legal id; epsilon below 0 and anticipatory above 1 make every decision
    greedy."""
    import torch
    tree, out, _, _ = _synthetic(osa, ctx, torch, solvers, "leduc_poker", 7, [(0, 257)], 64, 64, ties=True, eps=-0.5, anticipatory=1.2)
    got, want, _ = out[0]
    assert nc.same_chunk(got, want) and (got["modes"] == 3).all()
    seen = set()
    for i, row in zip(got["sl"][1], got["sl"][2]):
        legal = tree.legal[int(i)]
        assert row[nc.tie_pick(int(i), legal)] == 1.0 and row.sum() == 1.0
        seen.add((int(i) % 3, len(legal)))
    assert {(0, 2), (0, 3), (1, 2), (1, 3)} <= seen


@pytest.mark.parametrize("capacity,calls", [(1, (5, 3)), (7, (40, 33)), (64, (64, 1, 300))])
def test_ring_append_is_the_sequential_appends(ctx, capacity, calls):
    """Capacity 1; a capacity below one call's rows (the ring wraps several times inside the call); a call that ends
    exactly at the capacity; later calls continuing."""
    import torch
    from open_spiel_amd.nfsp import TransitionRing
    rng = np.random.default_rng(capacity)
    ring, mine = TransitionRing(ctx, capacity), nc.Ring(capacity)
    assert len(ring) == 0 and ring.entry_index == 0
    for m in calls:
        cols = [rng.integers(0, 1000, m).astype(np.int32), rng.integers(0, 3, m).astype(np.int32), rng.standard_normal(m).astype(np.float32),
                rng.integers(-1, 1000, m).astype(np.int32), rng.integers(0, 2, m).astype(np.uint8)]
        ring.append(*[torch.from_numpy(c).to(ctx.device) for c in cols])
        for row in zip(*cols):
            mine.append(row)
        got = (ring.entry_index,) + tuple(t.cpu().numpy() for t in ring.filled())
        assert nc.same_ring(got, mine.state()) and len(ring) == len(mine)
    m = min(5, len(mine))
    slots = ring.sample_slots(m, 31, 2)
    want = mine.sample(31, 2, m)
    assert np.array_equal(slots.cpu().numpy(), want) and len(set(want.tolist())) == m
    rows = ring.rows(slots)
    assert all(np.array_equal(t.cpu().numpy(), c[want]) for t, c in zip(rows, mine.cols))
    with pytest.raises(ValueError):
        ring.sample_slots(len(mine) + 1, 31, 2)
    ring.clear()
    assert len(ring) == 0 and ring.entry_index == 0


@pytest.mark.parametrize("game", ["tic_tac_toe", "leduc_poker(players=4)"])
def test_a_game_the_solvers_do_not_serve_is_refused(osa, ctx, game):
    with pytest.raises(osa.OsgError, match="osg error -2"):
        osa.NFSPSolver(ctx, game, [8], 100, 0.1)


def test_supervised_rows_and_rewards_average_to_their_expectations(osa, ctx, solvers):
    """Independent of the restatement: leduc_poker with frozen random tables, N = 2^18 episodes.  A player in
    BEST_RESPONSE mode plays eps / n + (1 - eps) [greedy] at every infostate and in AVERAGE_POLICY mode the average
    table; with w(m) the probability of the mode profile m, the expected supervised rows per episode at infostate i of
    player p are sum_m w(m) [m_p = BR] reach_m(i) (the reaches from action_values for the profile's behavioural table)
    and the expected terminal reward of p is sum_m w(m) returns_m[p] (profile_returns).  An episode visits an infostate
    at most once (a count in [0, 1], range 1) and a reward lies in [min_utility, max_utility]; Hoeffding at
    delta = 1e-9 over all compared cells."""
    import torch
    game = "leduc_poker"
    solver, tree, gold_of_dev, _ = solvers(game)
    desc = osa.describe(game)
    P, A, I = tree.num_players, tree.num_actions, tree.num_infostates
    q, avg = nc.synthetic_tables(tree, 2024)
    eps, ant = np.array([0.3, 0.2]), np.array([0.6, 0.35])
    legal = solver.tables()["legal"]                                   # [I, Amax] device order, -1 padded
    players = solver.infostate_players()
    q_dev, avg_dev = q[gold_of_dev], avg[gold_of_dev]
    by_legal = lambda t: np.where(legal >= 0, np.take_along_axis(t.astype(np.float64), np.clip(legal, 0, None), 1), 0.0)   # noqa: E731
    nact = (legal >= 0).sum(1)
    greedy = np.zeros((I, legal.shape[1]))
    values = np.where(legal >= 0, np.take_along_axis(q_dev, np.clip(legal, 0, None), 1), -np.inf)
    greedy[np.arange(I), values.argmax(1)] = 1.0
    e_row = eps[players][:, None]
    br_table = np.where(legal >= 0, e_row / nact[:, None] + (1 - e_row) * greedy, 0.0)
    avg_table = by_legal(avg_dev)
    avg_table = avg_table / avg_table.sum(1, keepdims=True)
    expect_rows, expect_ret = np.zeros(I), np.zeros(P)
    profiles = [(a, b) for a in (0, 1) for b in (0, 1)]                # 0: BEST_RESPONSE, 1: AVERAGE_POLICY
    returns = solver.profile_returns(np.stack([br_table, avg_table]), np.array(profiles))
    for m, ret in zip(profiles, returns):
        w = np.prod([ant[p] if m[p] == 0 else 1 - ant[p] for p in range(P)])
        table = np.where((np.array(m)[players] == 0)[:, None], br_table, avg_table)
        reach = solver.action_values(which="table", table=table)["reach"]
        expect_rows += w * reach * (np.array(m)[players] == 0)
        expect_ret += w * ret
    N, chunk = 1 << 18, 1 << 16
    dq, davg = (torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(ctx.device) for t in (q_dev, avg_dev))
    rows = torch.zeros(I, dtype=torch.int64, device=ctx.device)
    reward = torch.zeros(P, dtype=torch.float64, device=ctx.device)
    finals = torch.zeros(P, dtype=torch.int64, device=ctx.device)
    for first in range(0, N, chunk):
        solver.nfsp_collect(dq, davg, eps, ant, 0xC0FFEE, chunk, first)
        s = solver.nfsp_staged()
        rows += torch.bincount(s["sl_info"].long(), minlength=I)
        off = s["ring_offsets"]
        for p in range(P):
            lo, hi = int(off[p * chunk]), int(off[(p + 1) * chunk])
            last = s["ring_final"][lo:hi] != 0
            reward[p] += (s["ring_reward"][lo:hi].double() * last).sum()
            finals[p] += last.sum()
    assert finals.cpu().tolist() == [N] * P                             # every player ends every leduc episode with a transition
    mean_rows = rows.cpu().numpy() / N
    bound_rows = st.hoeffding_bound(N, 1.0, m=I + P)
    bound_ret = st.hoeffding_bound(N, desc.max_utility - desc.min_utility, m=I + P)
    err_rows = np.abs(mean_rows - expect_rows)
    err_ret = np.abs(reward.cpu().numpy() / N - expect_ret)
    print(f"{I} infostates: largest |rows / N - expectation| {err_rows.max():.5f}, bound {bound_rows:.5f}, largest expectation "
          f"{expect_rows.max():.4f}; rewards: largest |mean - expectation| {err_ret.max():.4f}, bound {bound_ret:.4f}, "
          f"expected returns {expect_ret}")
    assert err_rows.max() <= bound_rows and err_ret.max() <= bound_ret
    # the check has something to see: player 0's six first infostates are reached in every episode with its card, an
    # expectation of anticipatory[0] / 6 = 0.1 each — rows dropped or doubled there would miss the bound thirteen times over
    assert np.sort(expect_rows)[-6:].min() > 10 * bound_rows


@pytest.mark.parametrize("game", GAMES)
def test_the_solvers_tables_respect_the_legal_ids(osa, ctx, solvers, game):
    """The average table is a distribution over exactly the legal ids (leduc_poker has rows [0, 1] of a width of 3), and
    policy_table() has it by legal index."""
    tabular, tree, gold_of_dev, _ = solvers(game)
    solver = osa.NFSPSolver(ctx, game, [8], 100, 0.1, tabular=tabular)
    q, avg = (t.cpu().numpy() for t in solver.tables())
    legal = tabular.tables()["legal"]
    mask = np.zeros(avg.shape, bool)
    for i, row in enumerate(legal):
        mask[i, row[row >= 0]] = True
        assert mask[i].tolist() == [a in tree.legal[gold_of_dev[i]] for a in range(avg.shape[1])]
    assert q.shape == avg.shape == mask.shape and np.isfinite(q).all()
    assert (avg[mask] > 0).all() and (avg[~mask] == 0).all() and np.abs(avg.sum(1) - 1).max() < 1e-6
    table = solver.policy_table("average")
    by_id = np.where(legal >= 0, np.take_along_axis(avg.astype(np.float64), np.clip(legal, 0, None), 1), 0.0)
    assert np.abs(table - by_id / by_id.sum(1, keepdims=True)).max() < 1e-12
    greedy = solver.policy_table("best_response")
    values = np.where(legal >= 0, np.take_along_axis(q, np.clip(legal, 0, None), 1), -np.inf)
    assert (greedy.sum(1) == 1).all() and (greedy.argmax(1) == values.argmax(1)).all()


def test_solver_runs_the_stated_schedule(osa, ctx, solvers):
    import torch
    game = "kuhn_poker"
    _, tree, gold_of_dev, dev_of_gold = solvers(game)
    E, L, U = 50, 16, 40
    solver = osa.NFSPSolver(ctx, game, [8], 60, 0.3, batch_size=8, min_buffer_size_to_learn=16, learn_every=L, replay_buffer_capacity=50,
                            update_target_network_every=U, epsilon_start=0.5, epsilon_end=0.1, epsilon_decay_duration=200,
                            episodes_per_step=E, seed=5)
    from open_spiel_amd import deep_cfr
    mine = ([nc.Ring(50) for _ in range(2)], [dc.Reservoir(60, tree.num_actions, (5 ^ deep_cfr.RESERVOIR_SALT) & dc.M64, p) for p in range(2)])
    dqn_steps, nfsp_steps = np.zeros(2, np.int64), np.zeros(2, np.int64)
    for k in range(4):
        q, avg = (t.cpu().numpy()[dev_of_gold] for t in solver.tables())
        eps = solver.epsilons()
        want_eps = [0.1 + (0.5 - 0.1) * math.exp(-1.0 * min(int(t), 200) / 200) for t in dqn_steps]
        assert eps == want_eps                                                       # the schedule at the DQN counter
        before = [list(u) for u in solver.updates]
        totals = solver.step()
        want = nc.flatten_chunk(nc.run_chunk(tree, q, avg, eps, [0.3, 0.3], 5, k * E, E, *mine), 2, tree.num_actions)
        assert np.array_equal(totals, nc.totals(want, 2))
        for p in range(2):
            d0, n0 = int(dqn_steps[p]), int(nfsp_steps[p])
            d1, n1 = d0 + int(totals[p, 2]), n0 + int(totals[p, 3])
            made = [a - b for a, b in zip(solver.updates[p], before[p])]
            sl = n1 // L - n0 // L
            assert made[1] == sl and made[2] == d1 // U - d0 // U
            assert d1 // L - d0 // L <= made[0] <= d1 // L - d0 // L + sl             # + those that fell in AVERAGE_POLICY episodes
            assert nc.same_ring(_ring_state(solver.replay_buffers[p], gold_of_dev), mine[0][p].state())
            assert nc.same_reservoir(_res_state(solver.reservoir_buffers[p], gold_of_dev), nc.reservoir_state(mine[1][p]))
        dqn_steps += totals[:, 2]
        nfsp_steps += totals[:, 3]
        assert solver.dqn_steps == dqn_steps.tolist() and solver.nfsp_steps == nfsp_steps.tolist()
    assert solver.episodes == 4 * E and all(u[0] > 0 and u[1] > 0 and u[2] > 0 for u in solver.updates)
    assert all(np.isfinite(sl) and np.isfinite(rl) for sl, rl in solver.loss)
    legal = solver.tabular.tables()["legal"]
    for mode in ("average", "best_response"):
        table = solver.policy_table(mode)
        assert table.shape == legal.shape and (table >= 0).all() and (table[legal < 0] == 0).all()
        assert np.abs(table.sum(1) - 1.0).max() < 1e-12
    conv = solver.nash_conv()
    print(f"kuhn_poker after {4 * E} episodes: NashConv of the average policy {conv:.4f}, of the greedy policy {solver.nash_conv('best_response'):.4f}")
    assert np.isfinite(conv) and conv >= -1e-12
