"""The NumPy restatement of the NFSP arithmetic (tests/nfsp_cases.py) against the goldens the reference's own nfsp.py and
dqn.py produced (tests/golden/make_nfsp_vectors.py): every recorded row, its position, every draw count, every mode,
every ring and reservoir slot and every counter, bit for bit.  Each comparator is shown to reject a perturbed record."""
import os

import numpy as np
import pytest

import deep_cfr_cases as dc
import nfsp_cases as nc

RUNS = list(range(len(nc.golden_runs())))


def _replay(r):
    meta, chunks = nc.golden_run(r)
    tree = nc.golden_tree(meta["game"])
    rings, reservoirs = nc.new_buffers(meta, tree.num_actions)
    for chunk in chunks:
        eps = nc.run_chunk(tree, meta["q"], meta["avg"], meta["eps"], meta["anticipatory"], meta["seed"], chunk["first"],
                           len(chunk["draws"]), rings, reservoirs)
        yield meta, tree, chunk, eps, rings, reservoirs


@pytest.mark.parametrize("r", RUNS)
def test_the_restatement_reproduces_every_recorded_chunk(r):
    done = 0
    steps = None
    for meta, tree, chunk, eps, rings, reservoirs in _replay(r):
        P, A = meta["players"], tree.num_actions
        if steps is None:
            steps = np.zeros((P, 2), np.int64)
        got = nc.flatten_chunk(eps, P, A)
        assert chunk["first"] == done * meta["episodes"] and len(chunk["draws"]) == meta["episodes"]
        assert np.array_equal(got["modes"], chunk["modes"]), (r, done)
        assert np.array_equal(got["draws"], chunk["draws"]), (r, done)
        assert nc.same_ring_rows(got["ring"], chunk["ring"]), (r, done)
        assert nc.same_sl_rows(got["sl"], chunk["sl"]), (r, done)
        tot = nc.totals(got, P)
        steps += tot[:, 2:]
        assert np.array_equal(steps[:, 0], chunk["dqn_steps"]) and np.array_equal(steps[:, 1], chunk["nfsp_steps"])
        for p in range(P):
            assert nc.same_ring(rings[p].state(), chunk["rings"][p]), (r, done, p)
            assert nc.same_reservoir(nc.reservoir_state(reservoirs[p]), chunk["reservoirs"][p]), (r, done, p)
            bound = nc.row_bound(tree, p)
            E = meta["episodes"]
            assert np.diff(chunk["ring"][0][p * E:(p + 1) * E + 1]).max() <= bound
            assert np.diff(chunk["sl"][0][p * E:(p + 1) * E + 1]).max() <= bound
        done += 1
    assert done == meta["chunks"]


def test_the_goldens_cover_what_they_are_for():
    """Recomputed from the file alone."""
    games = {run.split("|")[0] for run in nc.golden_runs()}
    assert games == {"kuhn_poker", "kuhn_poker(players=3)", "leduc_poker"}
    wrapped = twice = bound_met = mixed = 0
    pure_dqn = pure_average = 0
    for r in RUNS:
        meta, chunks = nc.golden_run(r)
        tree = nc.golden_tree(meta["game"])
        P, E, q = meta["players"], meta["episodes"], meta["q"]
        modes = np.concatenate([c["modes"] for c in chunks])
        per_player = [set((((modes >> p) & 1) != 0).tolist()) for p in range(P)]
        explored = greedy = 0
        for c in chunks:
            _, info, probs = c["sl"]
            for i, row in zip(info, probs):
                legal = tree.legal[int(i)]
                if len(legal) > 1 and (row[legal] == row[legal[0]]).all():
                    explored += 1
                else:
                    assert row.max() == 1.0 and int(np.argmax(row)) == legal[nc.greedy(q[int(i)], legal)]
                    greedy += len(legal) > 1
        ant = float(meta["anticipatory"][0])
        if ant == 1.0:
            pure_dqn += all(m == {True} for m in per_player) and all(len(c["sl"][1]) == len(c["ring"][1]) for c in chunks)
        elif ant == 0.0:
            pure_average += all(m == {False} for m in per_player) and all(len(c["sl"][1]) == 0 for c in chunks)
        else:
            assert all(m == {True, False} for m in per_player), (r, per_player)     # both modes occur for every player
            assert explored > 0 and greedy > 0                                      # and both branches of the rule
            mixed += 1
        entry, calls = [0] * P, [0] * P
        for c in chunks:
            for p in range(P):
                wrapped += c["rings"][p][0] - entry[p] > 2 * meta["ring_capacity"]
                entry[p] = c["rings"][p][0]
                add_calls = c["reservoirs"][p][0]
                writes = [dc.reservoir_slot(meta["res_seed"], p, n, meta["res_capacity"]) for n in range(calls[p], add_calls)]
                writes = [w for w in writes if w >= 0]
                twice += max([writes.count(w) for w in set(writes)], default=0) >= 2
                calls[p] = add_calls
                bound_met += int(np.diff(c["ring"][0][p * E:(p + 1) * E + 1]).max() == nc.row_bound(tree, p))
    assert mixed >= 3 and pure_dqn == 1 and pure_average == 1
    assert wrapped >= 3 and twice >= 3
    assert bound_met > 0          # the row bound is exact: some episode reaches it
    assert os.path.getsize(nc.GOLDEN) < max(os.path.getsize(os.path.join(os.path.dirname(nc.GOLDEN), f))
                                            for f in os.listdir(os.path.dirname(nc.GOLDEN)) if f != os.path.basename(nc.GOLDEN))


def test_the_probs_row_is_what_numpy_gives():
    """probs = np.zeros(A); probs[legal] = 1 / len(legal) (or probs[action] = 1); probs / probs.sum(); float32."""
    for A in (2, 3, 4):
        for n in range(1, A + 1):
            legal = list(range(A - n, A))
            probs = np.zeros(A)
            probs[legal] = 1.0 / n
            want = np.asarray(probs / probs.sum(), dtype=np.float32)
            assert nc.probs_row(legal, A, None).tobytes() == want.tobytes()
            for k in range(n):
                probs = np.zeros(A)
                probs[legal[k]] = 1.0
                assert nc.probs_row(legal, A, k).tobytes() == np.asarray(probs / probs.sum(), dtype=np.float32).tobytes()


def test_greedy_is_the_first_maximum_as_argmax_is():
    rng = np.random.default_rng(3)
    for k in range(500):
        A = int(rng.integers(2, 5))
        legal = sorted(rng.choice(A, int(rng.integers(1, A + 1)), replace=False).tolist())
        q = rng.integers(-2, 3, A).astype(np.float32)                      # many ties
        assert nc.greedy(q, legal) == int(np.argmax(q[legal]))


def test_the_ring_rule():
    ring = nc.Ring(5)
    for n in range(13):
        ring.append((n, 0, 0.0, -1, 1))
    assert ring.entry_index == 13 and len(ring) == 5
    assert ring.cols[0].tolist() == [10, 11, 12, 8, 9] and ring.writes == [n % 5 for n in range(13)]
    slots = ring.sample(4, 1, 3)
    assert len(set(slots.tolist())) == 3 and np.array_equal(slots, ring.sample(4, 1, 3))
    # of m rows appended in one go, row r stays iff r + capacity >= m
    for cap, m in ((1, 4), (5, 3), (5, 5), (5, 17)):
        ring = nc.Ring(cap)
        for n in range(m):
            ring.append((n, 0, 0.0, -1, 1))
        assert sorted(ring.cols[0][:len(ring)].tolist()) == [r for r in range(m) if r + cap >= m]


# ---- the comparators reject perturbed records ---------------------------------------------------------------------------
def _a_chunk():
    for meta, tree, chunk, eps, rings, reservoirs in _replay(0):
        return meta, tree, chunk, nc.flatten_chunk(eps, meta["players"], tree.num_actions), rings, reservoirs


def test_the_row_comparators_reject_a_swapped_row_a_moved_offset_and_a_flipped_mode():
    meta, tree, chunk, got, _, _ = _a_chunk()
    assert nc.same_chunk(got, chunk)
    off, info, action, reward, nxt, final = got["ring"]
    k = next(k for k in range(len(info) - 1) if (info[k], action[k], nxt[k]) != (info[k + 1], action[k + 1], nxt[k + 1]))
    swapped = [c.copy() for c in got["ring"]]
    for c in swapped[1:]:
        c[[k, k + 1]] = c[[k + 1, k]]
    assert not nc.same_ring_rows(tuple(swapped), chunk["ring"])                     # a row out of order
    moved = off.copy()
    j = next(j for j in range(1, len(off) - 1) if off[j] > off[j - 1])
    moved[j] -= 1
    assert not nc.same_ring_rows((moved,) + got["ring"][1:], chunk["ring"])          # a row in the neighbouring episode
    ulp = reward.copy()
    ulp[final != 0] = np.nextafter(ulp[final != 0], np.float32(np.inf))
    assert not nc.same_ring_rows((off, info, action, ulp, nxt, final), chunk["ring"])
    flipped = dict(got, modes=got["modes"] ^ np.where(np.arange(len(got["modes"])) == 3, 1, 0).astype(np.int32))
    assert not nc.same_chunk(flipped, chunk)                                         # a flipped mode
    assert not nc.same_chunk(dict(got, draws=got["draws"] + (np.arange(len(got["draws"])) == 0)), chunk)
    so, si, sp = got["sl"]
    assert len(si) > 1
    other = sp.copy()
    other[0] = other[0][::-1] if other[0][0] != other[0][-1] else other[0] + np.float32(1e-7)
    assert not nc.same_sl_rows((so, si, other), chunk["sl"])
    assert not nc.same_sl_rows((so, np.roll(si, 1), sp), chunk["sl"]) or len(set(si.tolist())) == 1


def test_the_buffer_comparators_reject_a_slot_off_by_one_and_a_wrong_count():
    meta, tree, chunk, _, rings, reservoirs = _a_chunk()
    got, want = rings[0].state(), chunk["rings"][0]
    assert nc.same_ring(got, want) and len(got[1]) >= 2
    assert not nc.same_ring((got[0] + 1,) + got[1:], want)
    rolled = (got[0],) + tuple(np.roll(c, 1) for c in got[1:])
    assert any(not np.array_equal(a, b) for a, b in zip(rolled[1:], got[1:]))
    assert not nc.same_ring(rolled, want)                                             # every row one slot off
    p = next(p for p in range(meta["players"]) if len(chunk["reservoirs"][p][1]) >= 2)
    got, want = nc.reservoir_state(reservoirs[p]), chunk["reservoirs"][p]
    assert nc.same_reservoir(got, want)
    assert not nc.same_reservoir((got[0] - 1, got[1], got[2]), want)
    rolled = (got[0], np.roll(got[1], 1), np.roll(got[2], 1, axis=0))
    if not (np.array_equal(rolled[1], got[1]) and np.array_equal(rolled[2], got[2])):
        assert not nc.same_reservoir(rolled, want)
    ulp = got[2].copy()
    ulp[0, 0] = np.nextafter(ulp[0, 0], np.float32(np.inf))
    assert not nc.same_reservoir((got[0], got[1], ulp), want)
