"""The NFSP arithmetic (open_spiel_amd/csrc/osg_nfsp.h, host + device) driven on the CPU by
tests/native/nfsp_host_test.cpp and held against the goldens and the NumPy restatement (tests/nfsp_cases.py), bit for
bit.  The program is stand-alone; it is built once plain and once with the address and undefined-behaviour sanitizers
and run as its own binary."""
import numpy as np
import pytest

import deep_cfr_cases as dc
import nfsp_cases as nc

GAMES = ("kuhn_poker", "kuhn_poker(players=3)", "leduc_poker")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("nfsp_io"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return nc.build_host_test(str(tmp_path_factory.mktemp("nfsp") / "nfsp_host_test"))


@pytest.fixture(scope="module")
def sanitized_exe(tmp_path_factory):
    return nc.build_host_test(str(tmp_path_factory.mktemp("nfsp_san") / "nfsp_host_test_san"),
                              extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"))


@pytest.mark.parametrize("r", range(len(nc.golden_runs())))
def test_the_program_reproduces_every_recorded_chunk(exe, workdir, r):
    meta, chunks = nc.golden_run(r)
    tree = nc.golden_tree(meta["game"])
    P = meta["players"]
    rings, reservoirs = nc.new_buffers(meta, tree.num_actions)
    steps = np.zeros((P, 2), np.int64)
    for c, chunk in enumerate(chunks):
        got, bounds, tot = nc.host_chunk(exe, workdir, tree, meta["q"], meta["avg"], meta["eps"], meta["anticipatory"], meta["seed"],
                                         chunk["first"], len(chunk["draws"]), rings, reservoirs, name=f"g{r}_{c}")
        assert nc.same_chunk(got, chunk), (r, c)
        assert bounds.tolist() == [nc.row_bound(tree, p) for p in range(P)]
        assert np.array_equal(tot, nc.totals(chunk, P))
        steps += tot[:, 2:]
        assert np.array_equal(steps[:, 0], chunk["dqn_steps"]) and np.array_equal(steps[:, 1], chunk["nfsp_steps"])
        for p in range(P):
            assert nc.same_ring(rings[p].state(), chunk["rings"][p]), (r, c, p)
            assert nc.same_reservoir(nc.reservoir_state(reservoirs[p]), chunk["reservoirs"][p]), (r, c, p)


def _synthetic(exe, workdir, game, calls, seed, ring_cap, res_cap, name, ties=False, anticipatory=0.6, eps=0.25):
    tree = nc.golden_tree(game)
    P, A = tree.num_players, tree.num_actions
    q, avg = nc.synthetic_tables(tree, seed, ties)
    e, a = np.linspace(eps, eps + 0.2, P), np.linspace(anticipatory, anticipatory - 0.2, P)
    mine = ([nc.Ring(ring_cap) for _ in range(P)], [dc.Reservoir(res_cap, A, 77, p) for p in range(P)])
    theirs = ([nc.Ring(ring_cap) for _ in range(P)], [dc.Reservoir(res_cap, A, 77, p) for p in range(P)])
    out = []
    for k, (first, count) in enumerate(calls):
        want = nc.flatten_chunk(nc.run_chunk(tree, q, avg, e, a, seed, first, count, *mine), P, A)
        got, _, tot = nc.host_chunk(exe, workdir, tree, q, avg, e, a, seed, first, count, *theirs, name=f"{name}_{k}")
        out.append((got, want, tot))
    return tree, q, out, mine, theirs


def _same_buffers(mine, theirs):
    return (all(nc.same_ring(a.state(), b.state()) for a, b in zip(mine[0], theirs[0]))
            and all(nc.same_reservoir(nc.reservoir_state(a), nc.reservoir_state(b)) for a, b in zip(mine[1], theirs[1])))


@pytest.mark.parametrize("game", GAMES)
def test_synthetic_tables_equal_the_restatement(exe, workdir, game):
    for k, count in enumerate(nc.EPISODE_COUNTS[:4]):
        tree, q, out, mine, theirs = _synthetic(exe, workdir, game, [(1000 * k, count)], 40 + k, 11, 9, f"syn{k}")
        got, want, tot = out[0]
        assert nc.same_chunk(got, want) and np.array_equal(tot, nc.totals(want, tree.num_players))
        assert _same_buffers(mine, theirs)


def test_a_tie_in_q_goes_to_the_first_legal_id(exe, workdir):
    """Every legal entry of a row equal (illegal ids larger), or equal after a smaller first one: with epsilon 0 and
    anticipatory 1 every supervised row is one-hot at the first legal id of the tie."""
    tree, q, out, mine, theirs = _synthetic(exe, workdir, "leduc_poker", [(0, 65)], 7, 64, 64, "ties", ties=True, anticipatory=1.2, eps=-0.5)
    got, want, _ = out[0]
    assert nc.same_chunk(got, want) and len(got["sl"][1]) > 100
    seen = set()
    for i, row in zip(got["sl"][1], got["sl"][2]):
        legal = tree.legal[int(i)]
        assert row[nc.tie_pick(int(i), legal)] == 1.0 and row.sum() == 1.0
        seen.add((int(i) % 3, len(legal)))
    assert {(0, 2), (0, 3), (1, 2), (1, 3)} <= seen


def test_two_calls_continue_one(exe, workdir):
    tree, _, one, a_mine, a_theirs = _synthetic(exe, workdir, "kuhn_poker", [(100, 65)], 5, 9, 7, "whole")
    _, _, two, b_mine, b_theirs = _synthetic(exe, workdir, "kuhn_poker", [(100, 22), (122, 43)], 5, 9, 7, "parts")
    assert np.array_equal(one[0][0]["draws"], np.concatenate([two[0][0]["draws"], two[1][0]["draws"]]))
    assert np.array_equal(one[0][0]["modes"], np.concatenate([two[0][0]["modes"], two[1][0]["modes"]]))
    assert np.array_equal(one[0][2], two[0][2] + two[1][2])
    assert _same_buffers(a_theirs, b_theirs) and _same_buffers(a_theirs, a_mine)


def test_the_same_program_is_clean_under_the_sanitizers(sanitized_exe, exe, workdir):
    for game in GAMES:
        outs = []
        for which, name in ((sanitized_exe, "san"), (exe, "plain")):
            _, _, out, mine, theirs = _synthetic(which, workdir, game, [(0, 65), (65, 3)], 3, 1, 5, name)
            assert _same_buffers(mine, theirs)
            outs.append(out)
        for (a, _, ta), (b, _, tb) in zip(*outs):
            assert nc.same_chunk(a, b) and np.array_equal(ta, tb)
