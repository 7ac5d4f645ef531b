"""The NumPy restatement of the Deep CFR arithmetic (tests/deep_cfr_cases.py) against the goldens the reference's own
deep_cfr.py produced (tests/golden/make_deep_cfr_vectors.py): every recorded row, draw count and buffer state, bit for
bit.  Each comparator is shown to reject a perturbed record."""
import numpy as np
import pytest

import deep_cfr_cases as dc

RUNS = list(range(len(dc.golden_runs())))


def _replay(r):
    meta, steps = dc.golden_run(r)
    tree = dc.golden_tree(meta["game"])
    buffers = dc.new_buffers(meta, tree.num_actions)
    P = meta["players"]
    for step in steps:
        T = len(step["draws"])
        out = dc.run_step(tree, step["advantages"], step["player"], step["iteration"], meta["seed"], step["first"], T,
                          buffers[step["player"]], buffers[P])
        yield meta, tree, step, out, buffers


@pytest.mark.parametrize("r", RUNS)
def test_the_restatement_reproduces_every_recorded_step(r):
    steps = 0
    for meta, tree, step, out, buffers in _replay(r):
        A = tree.num_actions
        assert step["first"] == ((step["iteration"] - 1) * meta["players"] + step["player"]) * meta["traversals"]
        assert dc.same_rows(dc.flatten([o[0] for o in out], A), step["adv"]), (r, steps)
        assert dc.same_rows(dc.flatten([o[1] for o in out], A), step["strat"]), (r, steps)
        assert np.array_equal(np.array([o[2] for o in out], np.int32), step["draws"])
        assert step["buffers"]
        for b, want in step["buffers"].items():
            assert dc.same_buffer(buffers[b].state(), want), (r, steps, b)
        for b, buf in enumerate(buffers):
            assert (b in step["buffers"]) == (buf.add_calls > 0)
        bound = dc.row_bounds(tree, step["player"])
        assert np.diff(step["adv"][0]).max() <= bound[0] and np.diff(step["strat"][0]).max() <= bound[1]
        steps += 1
    assert steps == meta["iterations"] * meta["players"]


def test_the_goldens_cover_what_they_are_for():
    branches, crossed, twice, bound_met = set(), 0, 0, 0
    for r in RUNS:
        meta, steps = dc.golden_run(r)
        tree = dc.golden_tree(meta["game"])
        calls = [0] * (meta["players"] + 1)
        for step in steps:
            _, branch = dc.strategy_table(tree, step["advantages"])
            branches |= {int(branch[i]) for i in np.concatenate([step["adv"][1], step["strat"][1]])}
            bound = dc.row_bounds(tree, step["player"])
            bound_met += int(np.diff(step["adv"][0]).max() == bound[0])
            for b, (add_calls, *_rest) in step["buffers"].items():
                writes = [dc.reservoir_slot(meta["res_seed"], b, n, meta["capacity"]) for n in range(calls[b], add_calls)]
                writes = [w for w in writes if w >= 0]
                twice += len(writes) != len(set(writes))
                crossed += calls[b] < meta["capacity"] < add_calls
                calls[b] = add_calls
    assert branches == {0, 1, 2}
    assert crossed >= 3 and twice >= 3
    assert bound_met > 0          # the advantage-row bound is exact: some trajectory reaches it


def test_the_dtype_rules_the_restatement_follows_hold_on_this_numpy():
    """The strategy rule's three branches exist because of how Python's max and NumPy's sum and division type their
    results; the goldens pin the outcome, this pins the facts on the installed NumPy."""
    x, y, zero = np.float32(0.3), np.float32(-0.2), np.float32(0.0)
    assert type(max(0., x)) is np.float32 and type(max(0., y)) is float and type(max(0., zero)) is float
    assert np.sum([x, x]).dtype == np.float32 and np.sum([x, max(0., y)]).dtype == np.float64
    assert (x / np.sum([x, x])).dtype == np.float32 and (x / np.sum([x, max(0., y)])).dtype == np.float64
    assert type(max(0., y) / np.sum([x, max(0., y)])) is np.float64
    three = [np.float32(0.1), np.float32(0.7), np.float32(1e-8)]                      # short float32 sums are sequential
    assert np.sum(three) == np.float32(np.float32(three[0] + three[1]) + three[2])
    assert max([2, 0, 1], key=lambda a: [5.0, 3.0, 5.0][a]) == 2 and max([0, 2], key=lambda a: [5.0, 3.0, 5.0][a]) == 0


def test_the_strategy_rule_against_an_array_formulation():
    """The restatement's scalar loops against whole-array NumPy on the same rule."""
    rng = np.random.default_rng(1)
    seen = set()
    for k in range(3000):
        A = int(rng.integers(2, 5))
        legal = np.sort(rng.choice(A, int(rng.integers(1, A + 1)), replace=False))
        raw = rng.standard_normal(A).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 3))
        if k % 4 == 0:
            raw = np.abs(raw)
        if k % 7 == 0:
            raw[legal[0]] = 0.0
        if k % 11 == 0:
            raw[legal] = np.float32(-0.5)
        want = np.zeros(A, np.float64)
        if (raw[legal] > 0).all():
            want[legal] = (raw[legal] / np.sum(raw[legal])).astype(np.float64)      # float32 throughout, widened last
        elif (raw[legal] > 0).any():
            clipped = np.where(raw[legal] > 0, raw[legal], 0).astype(np.float64)
            want[legal] = clipped / np.sum(clipped)
        else:
            want[legal[np.argmax(raw[legal])]] = 1.0                                   # argmax: the first maximum
        got, branch = dc.strategy(raw, [int(a) for a in legal], A)
        assert got.tobytes() == want.tobytes(), (k, raw, legal)
        seen.add(branch)
    assert seen == {0, 1, 2}


def test_choice_is_numpys_rule():
    rng = np.random.default_rng(2)
    for k in range(500):
        n = int(rng.integers(1, 9))
        p = rng.random(n)
        p[rng.integers(0, n)] *= k % 2
        p = p / p.sum() if p.sum() > 0 else np.full(n, 1.0 / n)
        u = np.random.RandomState(k).random_sample()
        assert dc.choice(list(p), u) == int(np.random.RandomState(k).choice(n, p=p))


def test_the_reservoir_rule_is_uniform_over_the_stream():
    """mulhi64(x, n + 1) < capacity with probability capacity / (n + 1): the kept fraction of a long stream."""
    cap, N = 64, 20000
    buf = dc.Reservoir(cap, 1, 9, 3)
    for n in range(N):
        buf.append(n, 1, [0.0])
    kept = np.sort(buf.info)
    assert len(set(kept)) == cap and buf.add_calls == N
    # a uniform sample of the stream: its mean position is N / 2 within 6 sigma of the mean of 64 uniform draws
    assert abs(kept.mean() - N / 2) < 6 * N / np.sqrt(12 * cap)
    slots = buf.sample(5, 7, 10)
    assert len(set(slots.tolist())) == 10 and slots.min() >= 0 and slots.max() < cap
    assert np.array_equal(slots, buf.sample(5, 7, 10)) and not np.array_equal(slots, buf.sample(6, 7, 10))


# ---- the comparators reject perturbed records ---------------------------------------------------------------------------
def _first_step_with_rows(min_rows=3):
    for r in RUNS:
        for meta, tree, step, out, buffers in _replay(r):
            if len(step["adv"][1]) >= min_rows and len(set(step["adv"][1][:2].tolist())) == 2:
                return tree, step, out, buffers
    raise AssertionError("no such step")


def test_the_row_comparator_rejects_a_swap_an_ulp_and_a_moved_offset():
    tree, step, out, _ = _first_step_with_rows()
    off, info, vals = dc.flatten([o[0] for o in out], tree.num_actions)
    assert dc.same_rows((off, info, vals), step["adv"])
    swapped_i, swapped_v = info.copy(), vals.copy()
    swapped_i[[0, 1]], swapped_v[[0, 1]] = info[[1, 0]], vals[[1, 0]]
    assert not dc.same_rows((off, swapped_i, swapped_v), step["adv"])             # a row out of order
    ulp = vals.copy()
    nz = np.argwhere(ulp != 0)[0]
    ulp[tuple(nz)] = np.nextafter(ulp[tuple(nz)], np.float32(np.inf))
    assert not dc.same_rows((off, info, ulp), step["adv"])                        # a float32 off by one ulp
    moved = off.copy()
    inner = np.nonzero(np.diff(off) > 0)[0]
    if len(off) > 2:
        moved[1] += 1 if moved[1] < moved[2] or len(inner) == 0 else -1
        assert not dc.same_rows((moved, info, vals), step["adv"])                 # a row in the neighbouring trajectory
    signed = vals.copy()
    signed[vals == 0] = np.float32(-0.0)
    assert (vals == 0).any() and not dc.same_rows((off, info, signed), step["adv"])   # -0.0 is not +0.0


def test_the_buffer_comparator_rejects_a_wrong_slot_and_a_wrong_count():
    tree, step, out, buffers = _first_step_with_rows()
    b, want = next((b, w) for b, w in step["buffers"].items() if len(w[1]) >= 2)
    got = buffers[b].state()
    assert dc.same_buffer(got, want)
    add_calls, info, it, vals = got
    assert not dc.same_buffer((add_calls + 1, info, it, vals), want)
    rolled = (add_calls, np.roll(info, 1), np.roll(it, 1), np.roll(vals, 1, axis=0))
    if not (np.array_equal(rolled[1], info) and np.array_equal(rolled[3], vals)):
        assert not dc.same_buffer(rolled, want)                                   # every row one slot off
    other = it.copy()
    other[0] += 1
    assert not dc.same_buffer((add_calls, info, other, vals), want)
    ulp = vals.copy()
    ulp[0, 0] = np.nextafter(ulp[0, 0], np.float32(np.inf))
    assert not dc.same_buffer((add_calls, info, it, ulp), want)
