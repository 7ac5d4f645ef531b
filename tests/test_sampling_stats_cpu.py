"""tests/sampling_stats.py on the CPU: the decision rules accept correct samples and reject stated defects at the N
of the GPU test each one guards (tests/test_z22_gpu_sampling_statistics.py quotes the smallest rejected defect as its
sensitivity), the exact references reproduce known answers, and the restated generator and keyed orders of
open_spiel_amd/csrc/osg_common.h stay within the rules themselves at N = 2^20 — the condition that makes the GPU
thresholds fair."""
import math

import numpy as np
import pytest

import sampling_stats as ss
from test_synth_batch_cpu import CounterRng

N_JOINT = 1 << 20     # the 49-cell joints of the GPU tests
N_ORDER = 1 << 18     # roots per search in the sibling-order tests
R_PLAYOUT = 4096      # rollouts per root


# ---------------------------------------------------------------------------------------------------------------
# the rules on correct samples
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells,n", [(49, N_JOINT), (24, N_ORDER), (6, N_ORDER), (120, N_JOINT), (300, N_ORDER)])
def test_chi_square_accepts_exact_draws(cells, n):
    rng = np.random.default_rng(1000 + cells)
    probs = np.full(cells, 1.0 / cells)
    for _ in range(5):
        z, _, d = ss.chi_square(rng.multinomial(n, probs), probs)
        assert d == cells - 1 and ss.accept(z)
    skew = np.arange(cells, 2 * cells, dtype=np.float64)   # unequal cells, the thinnest half the thickest
    skew /= skew.sum()
    assert ss.accept(ss.chi_square(rng.multinomial(n, skew), skew)[0])


def test_chi_square_refuses_thin_cells_and_flags_a_fit_that_is_too_good():
    with pytest.raises(AssertionError, match="thin cell"):
        ss.chi_square(np.full(100, 10), np.full(100, 0.01))
    z, x2, _ = ss.chi_square(np.full(300, 1000), np.full(300, 1.0 / 300))   # every count exactly as expected
    assert x2 < 1e-20 and z < -ss.Z_MAX and not ss.accept(z)


def test_wilson_hilferty_matches_known_quantiles():
    # chi-square quantiles from the standard tables: P[X^2_10 <= 18.307] = P[X^2_100 <= 124.342] = 0.95 (z = 1.645)
    assert abs(ss.wilson_hilferty(18.307, 10) - 1.645) < 0.01
    assert abs(ss.wilson_hilferty(124.342, 100) - 1.645) < 0.005
    assert abs(ss.wilson_hilferty(48.0, 48)) < 0.1   # the median of X^2_d is ~ d (1 - 2 / (9 d))^3


def test_bounds_solve_their_equations():
    n, var, c, m = 4096, 0.37, 2.0, 5478
    t = float(ss.bernstein_bound(n, var, c, m))
    assert abs(2 * math.exp(-n * t * t / (2 * var + 2 * c * t / 3)) - ss.DELTA / m) < 1e-6 * ss.DELTA / m
    h = ss.hoeffding_bound(n, c, m)
    assert abs(2 * math.exp(-2 * n * h * h / (c * c)) - ss.DELTA / m) < 1e-6 * ss.DELTA / m
    assert t < h   # the variance is below (c / 2)^2: Bernstein is the tighter one


HOEFFDING_CASES = [   # (N, M, all cells shifted by this multiple of the bound, one cell by this one): all in use on the GPU
    (4096, 4520, 0.6, 1.2), (4096, 3404, 0.7, 1.3), (4096, 3301, 0.7, 1.3),          # mean plies of the playouts
    (1 << 23, 48, 0.8, 1.4), (1 << 25, 192, 0.8, 1.3), (1 << 27, 4368, 0.6, 1.3),    # ES-MCCFR, the flat kernels
    (1 << 20, 48, 0.8, 1.4), (699040, 192, 0.8, 1.2), (1 << 20, 4368, 0.6, 1.3),     # ES-MCCFR, the split forms
    (1 << 26, 24, 0.9, 1.2), (1 << 26, 96, 0.8, 1.5),                                # OS-MCCFR
    (1 << 22, 48, 0.8, 1.4), (1 << 22, 192, 0.8, 1.2), (1 << 22, 4368, 0.6, 1.3),    # the general kernels, ES
    (1 << 22, 24, 0.9, 1.2), (1 << 22, 96, 0.8, 1.5)]                                # the general kernels, OS


@pytest.mark.parametrize("n,m,all_cells,one_cell", HOEFFDING_CASES)
def test_hoeffding_rule_accepts_exact_means_and_rejects_a_shift(n, m, all_cells, one_cell):
    """The Hoeffding rule at every (N, M) the GPU tests use it with, on a variable that takes the two ends of its
    range with equal probability — the largest variance the range allows; in units of the range, so c = 1.  M cells
    of N draws each (a binomial count), 16 seeded repetitions: the exact mean is accepted every time; every cell's
    mean shifted by `all_cells` x the bound is rejected every time, and so is ONE cell's mean shifted by `one_cell` x
    the bound — the smallest multiples (steps of 0.1) for which that holds.  (A variable of smaller variance is held
    closer to 1.0 x the bound from both sides: no draw carries it across.)"""
    bound = ss.hoeffding_bound(n, 1.0, m)

    def accepted(seed, shift_all=0.0, shift_one=0.0):
        p = np.full(m, 0.5 + shift_all * bound)
        p[m // 2] += shift_one * bound
        means = np.random.default_rng(700 + seed).binomial(n, p) / n
        return np.abs(means - 0.5).max() <= bound

    for seed in range(16):
        assert accepted(seed)
        assert not accepted(seed, shift_all=all_cells) and not accepted(seed, shift_one=one_cell)
    assert any(accepted(seed, shift_all=all_cells - 0.1) for seed in range(16))
    assert any(accepted(seed, shift_one=one_cell - 0.1) for seed in range(16))


def _playout_rows(rng, rows, shift=0.0, playouts=R_PLAYOUT, per_sample=1):
    """`rows` roots with returns in {-1, 0, 1}: exact means and variances of one sample (the mean of `per_sample`
    playouts), and sample means over `playouts` samples whose win probability is raised (and loss probability
    lowered) by shift / 2."""
    p = rng.dirichlet(np.ones(3), size=rows)            # P(-1), P(0), P(+1)
    p[: rows // 8] = np.array([0.0, 0.0, 1.0])          # decided positions: variance 0
    mu, var = p[:, 2] - p[:, 0], (p[:, 2] + p[:, 0] - (p[:, 2] - p[:, 0]) ** 2) / per_sample
    q = p.copy()
    live = (q[:, 0] > shift) & (q[:, 2] < 1 - shift)
    q[live, 0] -= shift / 2
    q[live, 2] += shift / 2
    draws = np.stack([rng.multinomial(playouts * per_sample, row) for row in q])
    return (draws[:, 2] - draws[:, 0]) / (playouts * per_sample), mu, var


@pytest.mark.parametrize("rows,shift", [(5478, 0.004), (4096, 0.005), (1000, 0.0075), (400, 0.01)])
def test_check_means_accepts_exact_draws_and_rejects_a_shared_shift(rows, shift):
    """The playout test's rule (`rows` roots of 4 096 playouts; 5 478 = tic_tac_toe): accepted on exact draws; a
    shift of every mean return by `shift` — at 5 478 roots a fifth of a row's own standard error — is rejected by
    the aggregate sum of z^2, where the per-row Bernstein bound (~0.1) cannot see it."""
    rng = np.random.default_rng(7)
    ok = ss.check_means(*_playout_rows(rng, rows), n=R_PLAYOUT, c=2.0)
    assert ok["ok"] and ok["exact"] and ok["worst"] < 1.0 and ss.accept(ok["z"])
    bad = ss.check_means(*_playout_rows(rng, rows, shift=shift), n=R_PLAYOUT, c=2.0)
    assert bad["worst"] < 1.0 and bad["z"] > ss.Z_MAX and not bad["ok"]
    # a decided position that does not come out exact fails whatever the rest does
    means, mu, var = _playout_rows(rng, 64)
    means[0] -= 1.0 / R_PLAYOUT
    assert not ss.check_means(means, mu, var, n=R_PLAYOUT, c=2.0)["ok"]


@pytest.mark.parametrize("children,visits", [(9, 7281), (4, 16384), (12, 5461)])
def test_search_value_rule_rejects_a_shared_shift(children, visits):
    """The search-value test's rule: `children` root children, each visited by 2^16 / children searches whose reward
    is the mean of 64 playouts.  Exact draws pass; every child's value shifted by 0.003 is rejected."""
    rng = np.random.default_rng(children)
    assert ss.check_means(*_playout_rows(rng, children, 0.0, visits, 64), n=visits, c=2.0)["ok"]
    assert not ss.check_means(*_playout_rows(rng, children, 0.003, visits, 64), n=visits, c=2.0)["ok"]


def test_check_means_rejects_one_row_beyond_its_bound():
    rng = np.random.default_rng(8)
    means, mu, var = _playout_rows(rng, 600)
    k = 599
    means[k] = mu[k] + 1.05 * float(ss.bernstein_bound(R_PLAYOUT, var[k], 2.0, int((var > 0).sum())))
    out = ss.check_means(means, mu, var, n=R_PLAYOUT, c=2.0)
    assert out["worst"] > 1.0 and not out["ok"]


# ---------------------------------------------------------------------------------------------------------------
# the rules reject stated defects, each at the N of the GPU test it guards
# ---------------------------------------------------------------------------------------------------------------
def _bumped(probs, cell, rel):
    p = np.array(probs, np.float64)
    p[cell] *= 1.0 + rel
    return p / p.sum()


@pytest.mark.parametrize("cells,n,rel", [(49, N_JOINT, 0.08), (7, N_JOINT, 0.03), (6, N_JOINT, 0.03),
                                         (12, N_JOINT, 0.04), (60, N_JOINT, 0.10), (120, N_JOINT, 0.15),
                                         (7, N_ORDER, 0.05), (9, N_ORDER, 0.06), (21, N_ORDER, 0.10),
                                         (25, N_ORDER, 0.10), (36, N_ORDER, 0.15), (300, N_ORDER, 0.60)])
def test_one_cell_raised_is_rejected(cells, n, rel):
    """One cell's probability raised by `rel` (relative): rejected; the same draw without the defect is accepted."""
    rng = np.random.default_rng(cells)
    probs = np.full(cells, 1.0 / cells)
    assert ss.accept(ss.chi_square(rng.multinomial(n, probs), probs)[0])
    assert ss.chi_square(rng.multinomial(n, _bumped(probs, cells // 3, rel)), probs)[0] > ss.Z_MAX


@pytest.mark.parametrize("k,n,rise", [(7, N_JOINT, 0.005), (4, N_ORDER // 2, 0.015), (7, N_ORDER // 2, 0.015),
                                      (9, N_ORDER // 2, 0.01), (25, N_ORDER // 2, 0.01)])
def test_neighbouring_rows_that_agree_too_often_are_rejected(k, n, rise):
    """P[row i + 1's draw equals row i's] raised from 1 / k by `rise` (absolute): the k x k joint is rejected
    (n pairs of rows: 2^20 in the one-ply joints, 2^17 = the pairs among the 2^18 roots of a search)."""
    rng = np.random.default_rng(50 + k)
    uniform = np.full((k, k), 1.0 / (k * k))
    joint = np.full((k, k), (1.0 - 1.0 / k - rise) / (k * k - k))
    np.fill_diagonal(joint, (1.0 / k + rise) / k)
    assert abs(joint.sum() - 1.0) < 1e-12
    assert ss.accept(ss.chi_square(rng.multinomial(n, uniform.ravel()), uniform)[0])
    assert ss.chi_square(rng.multinomial(n, joint.ravel()), uniform)[0] > ss.Z_MAX


@pytest.mark.parametrize("k,rel", [(3, 0.05), (4, 0.10)])
def test_one_preferred_permutation_is_rejected(k, rel):
    """One of the k! orders preferred by `rel` (relative) at N = 2^18 roots."""
    cells = math.factorial(k)
    rng = np.random.default_rng(k)
    probs = np.full(cells, 1.0 / cells)
    assert ss.accept(ss.chi_square(rng.multinomial(N_ORDER, probs), probs)[0])
    assert ss.chi_square(rng.multinomial(N_ORDER, _bumped(probs, 5, rel)), probs)[0] > ss.Z_MAX


def test_grouped_chi_square_rejects_one_preferred_child():
    """The one-ply rule (every non-terminal tic_tac_toe position 256 times): exact draws pass; the first child of
    every position preferred by 10 % (relative) is rejected (256 draws per position is a thin sample: the GPU test
    adds the counts by child rank, summed over the positions with the same number of children, which sees 3 % —
    the (7 .. 9)-cell rows of test_one_cell_raised_is_rejected)."""
    rng = np.random.default_rng(11)
    legal = rng.integers(2, 10, size=4520)
    for rel, verdict in ((0.0, True), (0.10, False)):
        counts, expected = [], []
        for k in legal:
            p = np.full(k, 1.0 / k)
            counts.append(rng.multinomial(256, _bumped(p, 0, rel)))
            expected.append(256 * p)
        z, _, d = ss.chi_square_grouped(np.concatenate(counts), np.concatenate(expected), legal.size)
        assert d == int((legal - 1).sum()) and ss.accept(z) == verdict


def test_two_sample_mean_z_rejects_a_shifted_win_rate():
    """The big-board rule: a recorded reference estimate of 2^16 single playouts against 2^14 searches whose value is
    the mean of 64 playouts after a random first move.  The same win rate passes; a win rate that differs by 0.02
    (a mean return by 0.04) is rejected."""
    rng = np.random.default_rng(19)
    first_move = rng.uniform(0.35, 0.75, 361)   # black's win rate after each first move
    rate = first_move.mean()
    for shift, verdict in ((0.0, True), (0.02, False)):
        ref_wins = rng.binomial(1 << 16, rate)
        ref_mean = 2.0 * ref_wins / (1 << 16) - 1.0
        moves = rng.integers(0, 361, 1 << 14)
        values = 2.0 * rng.binomial(64, first_move[moves] + shift) / 64.0 - 1.0
        z = ss.two_sample_mean_z(values.mean(), values.var(ddof=1), values.size, ref_mean, 1.0 - ref_mean ** 2, 1 << 16)
        assert ss.accept(z) == verdict, z


def test_recorded_random_play_rates_are_recorded_results_only():
    """tests/golden/random_play_rates.json (tests/golden/make_random_play_rates.py): counts per board, nothing else;
    black, who moves first, wins a little more than half of the random playouts on every board."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_play_rates.json"), encoding="utf-8") as f:
        rec = json.load(f)
    assert sorted(rec) == ["boards", "samples"] and isinstance(rec["samples"], str)
    assert sorted(rec["boards"]) == sorted(f"hex(board_size={b})" for b in (9, 13, 15, 19))
    for board in rec["boards"].values():
        assert sorted(board) == ["black_wins", "playouts"] and board["playouts"] == 1 << 16
        assert 0.5 < board["black_wins"] / board["playouts"] < 0.55


# ---------------------------------------------------------------------------------------------------------------
# random_play_moments on tic_tac_toe, edge table built from the oracle's states
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ttt_table(oracle):
    og = oracle.Game("tic_tac_toe")
    levels, states = [{str(og.new_initial_state()): 0}], [og.new_initial_state()]
    edges = []   # per position: list of child indices
    at = 0
    while at < len(states):
        level = {}
        first_new = len(states)
        for i in range(at, first_new):
            s = states[i]
            kids = []
            if not s.is_terminal():
                for a in s.legal_actions():
                    c = s.child(a)
                    key = str(c)
                    if key not in level:
                        level[key] = len(states)
                        states.append(c)
                    kids.append(level[key])
            edges.append(kids)
        at = first_new
        levels.append(level)
    edge_off = np.zeros(len(states) + 1, np.int64)
    edge_off[1:] = np.cumsum([len(k) for k in edges])
    edge_child = np.array([c for k in edges for c in k], np.int64)
    returns = np.array([s.returns()[0] if s.is_terminal() else 0.0 for s in states])
    return states, edges, edge_off, edge_child, returns


def test_random_play_moments_on_tic_tac_toe(ttt_table):
    states, edges, edge_off, edge_child, returns = ttt_table
    assert len(states) == 5478
    m1, m2, plies = ss.random_play_moments(edge_off, edge_child, returns)
    x_wins = ss.random_play_moments(edge_off, edge_child, (returns > 0).astype(float))[0]
    o_wins = ss.random_play_moments(edge_off, edge_child, (returns < 0).astype(float))[0]
    assert abs(x_wins[0] - 737 / 1260) <= 1e-15 and abs(o_wins[0] - 121 / 420) <= 1e-15
    assert abs(1.0 - x_wins[0] - o_wins[0] - 8 / 63) <= 1e-15
    assert abs(m1[0] - (737 / 1260 - 121 / 420)) <= 1e-15 and abs(m2[0] - (1 - 8 / 63)) <= 1e-15
    # a direct memoised recursion over the oracle's states, position by position
    memo = {}

    def direct(i):
        if i not in memo:
            if not edges[i]:
                memo[i] = (returns[i], returns[i] ** 2, 0.0)
            else:
                kids = [direct(c) for c in edges[i]]
                memo[i] = (sum(k[0] for k in kids) / len(kids), sum(k[1] for k in kids) / len(kids),
                           1.0 + sum(k[2] for k in kids) / len(kids))
        return memo[i]

    want = np.array([direct(i) for i in range(len(states))])
    assert np.abs(m1 - want[:, 0]).max() <= 1e-15 and np.abs(m2 - want[:, 1]).max() <= 1e-15
    assert np.abs(plies - want[:, 2]).max() <= 1e-14   # (values up to 9: a few ulp of 8)
    assert 5.0 <= plies[0] <= 9.0 and (plies[np.diff(edge_off) == 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# es_expected_deltas against one simultaneous-update iteration of the oracle's vanilla CFR from zero tables
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", ["kuhn_poker", "kuhn_poker(players=3)"])
def test_es_expected_deltas_equal_the_instantaneous_regrets_of_cfr(oracle, game):
    og = oracle.Game(game)
    solver = oracle.Solver(og, "cfr_simultaneous")
    solver.iterate(1)
    t = solver.tables()
    d_regret, d_policy = ss.es_expected_deltas(og)
    assert sorted(d_regret) == sorted(t["keys"])
    for key, nact, row in zip(t["keys"], t["nact"], t["regrets"]):
        assert np.abs(d_regret[key] - row[:nact]).max() <= 1e-12, key
        assert abs((d_regret[key] * 0.5).sum()) <= 1e-12   # regrets average to 0 under sigma (uniform: 2 actions)
    # the kSimple policy term: sigma(I, a) times the reach of everybody but the traverser.  In kuhn_poker every
    # infostate of player p holds (cards of the others) histories of equal chance reach; under the uniform policy
    # the total over an infostate's actions is the probability that a traversal of player p - 1 passes through I.
    total = sum(v.sum() for v in d_policy.values())
    assert total > 0 and all((v >= 0).all() and np.allclose(v, v[0]) for v in d_policy.values())


def test_es_expected_deltas_follow_the_table(oracle):
    """A non-uniform table: the regrets still average to 0 under sigma at every infostate, and an action with
    negative regret has sigma = 0, so its policy term vanishes."""
    og = oracle.Game("kuhn_poker")
    keys = sorted(ss.es_expected_deltas(og)[0])
    rng = np.random.default_rng(3)
    table = {k: rng.uniform(-1, 1, 2) for k in keys}
    d_regret, d_policy = ss.es_expected_deltas(og, table)
    for k in keys:
        sigma = ss.regret_matching(table[k])
        assert abs(sigma @ d_regret[k]) <= 1e-15
        assert ((sigma == 0) == (d_policy[k] == 0)).all() or d_policy[k].sum() == 0


# ---------------------------------------------------------------------------------------------------------------
# the restated streams themselves stay within the rules (N = 2^20)
# ---------------------------------------------------------------------------------------------------------------
SEED = 0x5A3D1E


def test_vectorised_restatement_equals_the_python_counter_rng():
    idx = np.array([0, 1, 2, 77, 1 << 33, (1 << 63) + 5], np.uint64)
    for seed, sub in ((0, 0), (SEED, 3), ((1 << 64) - 1, 1 << 40)):
        v = ss.VecRng(seed, idx, sub)
        first, second, third = v.next(), v.below(361), v.unit()
        for k, i in enumerate(idx.tolist()):
            r = CounterRng(seed, i, sub)
            assert int(first[k]) == r.next() and int(second[k]) == r.below(361) and float(third[k]) == r.unit()


def test_keyed_orders_equal_the_device_header(tmp_path):
    """The NumPy order_base / order_key / fill_base / fill_key against open_spiel_amd/csrc/osg_common.h itself,
    compiled for the host (tests/native/keyed_order_values.cpp prints the header's values for 20 (seed, root) pairs,
    8 action / cell ids and 5 sub-streams): the tests below speak about the functions the kernels run."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "keyed_order_values")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w",
                           "-I", os.path.join(root, "open_spiel_amd", "csrc"),
                           os.path.join(root, "tests", "native", "keyed_order_values.cpp"), "-o", exe])
    lines = [line.split() for line in subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()]
    seen = {"path_hash_root": 0, "order_base": 0, "order_key": 0, "fill_base": 0, "fill_key": 0}
    for name, *v in lines:
        v = [int(x) for x in v]
        seen[name] += 1
        if name == "path_hash_root":
            assert ss.PATH_HASH_ROOT == v[0]
        elif name == "order_base":
            assert int(ss.order_base(v[0], np.array([v[1]], np.uint64))[0]) == v[2]
        elif name == "order_key":
            base = ss.order_base(v[0], np.array([v[1]], np.uint64))
            assert int(ss.order_key(base, ss.PATH_HASH_ROOT, [v[2]])[0, 0]) == v[3]
        elif name == "fill_base":
            assert int(ss.fill_base(v[0], np.array([v[1]], np.uint64), np.array([v[2]], np.uint64))[0]) == v[3]
        else:
            base = ss.fill_base(v[0], np.array([v[1]], np.uint64), np.array([v[2]], np.uint64))
            assert int(ss.fill_key(base, [v[3]])[0, 0]) == v[4]
    assert seen == {"path_hash_root": 1, "order_base": 20, "order_key": 160, "fill_base": 100, "fill_key": 800}


def _orders(keys):
    return np.argsort(keys, axis=-1, kind="stable")


def _check_order_statistics(order, k, what):
    """first element (k cells), first ordered pair (k (k - 1) cells), and the full order where k! cells are not thin."""
    n = order.shape[0]
    out = {}
    out["first"] = ss.chi_square(ss.counts_of(order[:, 0], k), np.full(k, 1.0 / k))[0]
    pair = order[:, 0] * (k - 1) + order[:, 1] - (order[:, 1] > order[:, 0])
    out["pair"] = ss.chi_square(ss.counts_of(pair, k * (k - 1)), np.full(k * (k - 1), 1.0 / (k * (k - 1))))[0]
    if n / math.factorial(k) >= ss.MIN_EXPECTED:
        cells = math.factorial(k)
        out["order"] = ss.chi_square(ss.counts_of(ss.permutation_index(order), cells), np.full(cells, 1.0 / cells))[0]
    else:   # 9! = 362 880 orders would be thin at 2^20: the first three places (504 cells) instead
        rest = np.sort(order[:, :2], axis=1)
        third = order[:, 2] - (order[:, 2] > rest[:, 0]) - (order[:, 2] > rest[:, 1])
        cells = k * (k - 1) * (k - 2)
        out["triple"] = ss.chi_square(ss.counts_of(pair * (k - 2) + third, cells), np.full(cells, 1.0 / cells))[0]
    for name, z in out.items():
        assert ss.accept(z), (what, name, z)
    return out


@pytest.mark.parametrize("actions", [[0, 1, 2], [2, 5, 7], [0, 1, 2, 3], [1, 3, 4, 8], list(range(9)), list(range(7))])
def test_order_key_orders_siblings_uniformly(actions):
    roots = np.arange(N_JOINT, dtype=np.uint64) + np.uint64(12345)
    keys = ss.order_key(ss.order_base(SEED, roots), ss.PATH_HASH_ROOT, actions)
    assert keys.dtype == np.uint32 and ((keys & np.uint32(0xFF)) == np.asarray(actions, np.uint32)).all()
    order = _orders(keys)
    _check_order_statistics(order, len(actions), "order_key")
    # neighbouring roots: the first siblings of roots i and i + 1
    k = len(actions)
    joint = order[:-1, 0] * k + order[1:, 0]
    assert ss.accept(ss.chi_square(ss.counts_of(joint, k * k), np.full(k * k, 1.0 / (k * k)))[0])


@pytest.mark.parametrize("cells", [3, 4, 9])
def test_fill_key_orders_cells_uniformly(cells):
    roots = np.arange(1 << 10, dtype=np.uint64)[:, None]
    subs = np.arange(1 << 10, dtype=np.uint64)[None, :]
    keys = ss.fill_key(ss.fill_base(SEED, roots, subs).reshape(-1), np.arange(cells))
    assert ((keys & np.uint64(0xFF)) == np.arange(cells, dtype=np.uint64)).all() and int(keys.max()) < 1 << 40
    _check_order_statistics(_orders(keys), cells, "fill_key")


def _fisher_yates(rng, k, n):
    """expand_on_pool's shuffle (osg_mcts_lane.h): for i = k - 1 .. 1: swap(i, below(i + 1))."""
    order = np.tile(np.arange(k), (n, 1))
    rows = np.arange(n)
    for i in range(k - 1, 0, -1):
        j = rng.below(i + 1)
        order[rows, i], order[rows, j] = order[rows, j], order[rows, i].copy()
    return order


@pytest.mark.parametrize("k", [3, 4, 9])
def test_fisher_yates_on_below_is_uniform(k):
    order = _fisher_yates(ss.VecRng(SEED, np.arange(N_JOINT, dtype=np.uint64), 1), k, N_JOINT)
    assert (np.sort(order, axis=1) == np.arange(k)).all()
    _check_order_statistics(order, k, "fisher_yates")


@pytest.mark.parametrize("n", [2, 3, 7, 9, 81, 361])
def test_below_is_uniform(n):
    draws = ss.VecRng(SEED, np.arange(N_JOINT, dtype=np.uint64), 0).below(n)
    assert draws.min() == 0 and draws.max() == n - 1
    assert ss.accept(ss.chi_square(ss.counts_of(draws, n), np.full(n, 1.0 / n))[0])


@pytest.mark.parametrize("which", ["index", "sub", "seed"])
def test_first_draws_of_neighbouring_streams_are_independent(which):
    i = np.arange(N_JOINT, dtype=np.uint64)
    if which == "index":
        a, b = ss.VecRng(SEED, i, 0), ss.VecRng(SEED, i + np.uint64(1), 0)
    elif which == "sub":
        a, b = ss.VecRng(SEED, 5, i), ss.VecRng(SEED, 5, i + np.uint64(1))
    else:
        a, b = ss.VecRng(i, 5, 0), ss.VecRng(i + np.uint64(1), 5, 0)
    joint = a.below(7) * 7 + b.below(7)
    assert ss.accept(ss.chi_square(ss.counts_of(joint, 49), np.full(49, 1.0 / 49))[0])
    ua, ub = a.unit(), b.unit()   # and the second draws as uniforms: a 16 x 16 grid
    grid = (ua * 16).astype(np.int64) * 16 + (ub * 16).astype(np.int64)
    assert ss.accept(ss.chi_square(ss.counts_of(grid, 256), np.full(256, 1.0 / 256))[0])


def test_permutation_and_pair_indices():
    import itertools
    perms = np.array(list(itertools.permutations(range(4))))
    assert ss.permutation_index(perms).tolist() == list(range(24))
    pairs = [(a, b) for a in range(7) for b in range(a + 1, 7)]
    got = [int(ss.unordered_pair_index(np.int64(b), np.int64(a), 7)) for a, b in pairs]
    assert got == list(range(21))
