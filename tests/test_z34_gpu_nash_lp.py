"""The exact Nash meta-solver on the device (osg_nash_lp in include/osg_abi.h; open_spiel_amd.meta_solvers;
PSROSolver(meta_solver="nash_lp")) against the NumPy restatement of open_spiel_amd/csrc/osg_nash_lp.h (nash_lp_cases.solve:
array_equal, since both evaluate the one order the header fixes without fused multiply-adds) and against the certificate
of a Nash pair with HiGHS's value (nash_lp_cases.certify).

The generated sweep (nash_lp_cases.sweep) walks the kernel's layout edges: 64 columns (lane 0's second column), fewer
rows or columns than lanes, strides next to 32 and 64, more cells than threads, and LDS above the default cap.  Every
matrix of it, the ends of the fp64 range and the power-of-two multiples must equal the restatement, whose answers
tests/test_nash_lp_native.py certifies on the CPU, wherever the problem sits in a batch of 4096."""
import numpy as np
import pytest

import nash_lp_cases as nc

pytestmark = pytest.mark.gpu

SHAPES = sorted({A.shape for A in nc.CASES.values()})


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


def _same(out, k, want, what):
    x, y, v, pivots, status = want
    assert int(out["status"][k]) == status and int(out["pivots"][k]) == pivots, what
    assert np.array_equal(out["row"][k], x, equal_nan=True) and np.array_equal(out["col"][k], y, equal_nan=True), what
    assert np.array_equal(out["value"][k], v, equal_nan=True), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_is_the_restatement_wherever_a_problem_sits(ctx, shape):
    import torch
    import open_spiel_amd.meta_solvers as ms
    names = [n for n, A in nc.CASES.items() if A.shape == shape] * 3
    order = np.random.default_rng(shape[0] * 100 + shape[1]).permutation(len(names))
    names = [names[k] for k in order]
    batch = np.stack([nc.CASES[n] for n in names])
    out = ms.solve_zero_sum_matrix_games(ctx, batch)
    on_device = ms.solve_zero_sum_matrix_games(ctx, torch.as_tensor(batch, device=ctx.device), device=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in on_device.values())
    on_device = {k: v.cpu().numpy() for k, v in on_device.items()}
    for k, name in enumerate(names):
        _same(out, k, nc.restated(name), name)
        _same(on_device, k, nc.restated(name), name)
        nc.certify(nc.CASES[name], out["row"][k], out["col"][k], out["value"][k], out["status"][k], name)


def test_an_empty_batch_and_a_matrix_that_is_not_finite(ctx):
    import torch
    import open_spiel_amd.meta_solvers as ms
    assert ms.solve_zero_sum_matrix_games(ctx, np.zeros((0, 5, 7)))["row"].shape == (0, 5)
    assert ms.solve_zero_sum_matrix_games(ctx, torch.zeros((0, 5, 7), dtype=torch.float64, device=ctx.device), device=True)["col"].shape == (0, 7)
    batch = np.stack([nc.CASES["integers_33x17"]] * 4)
    batch[1, 32, 16] = np.nan
    batch[2, 0, 0] = np.inf
    out = ms.solve_zero_sum_matrix_games(ctx, batch)
    nan = (np.full(33, np.nan), np.full(17, np.nan), np.nan, 0, 1)
    for k, want in enumerate((nc.restated("integers_33x17"), nan, nan, nc.restated("integers_33x17"))):
        _same(out, k, want, k)
    with pytest.raises(ValueError):
        ms.solve_zero_sum_matrix_game(ctx, batch[1])


def test_refusals(ctx):
    import open_spiel_amd as osa
    import open_spiel_amd.meta_solvers as ms
    for shape in ((1, 65, 3), (2, 4, 0)):
        with pytest.raises(osa.OsgError, match=f"{shape[1]} rows and {shape[2]} columns"):
            ms.solve_zero_sum_matrix_games(ctx, np.zeros(shape))
    T = nc.CASES["rps"]
    with pytest.raises(NotImplementedError, match="nash_strategy solver works only for 2p zero-sum"):
        ms.nash_strategy(ctx, [np.zeros((2, 2, 2))] * 3)
    with pytest.raises(ValueError):
        ms.nash_strategy(ctx, [T, T])
    with pytest.raises(osa.OsgError):
        osa.PSROSolver(ctx, "kuhn_poker", meta_solver="nash_lp", meta_solver_kwargs=dict(iterations=10))
    with pytest.raises(osa.OsgError, match="nash_lp"):
        osa.PSROSolver(ctx, "kuhn_poker", meta_solver="nash")
    (p0, p1), joint = ms.nash_strategy(ctx, [T, -T], return_joint=True)
    assert np.array_equal(joint, np.outer(p0, p1)) and np.array_equal(p0, nc.restated("rps")[0])
    assert ms.solve_zero_sum_matrix_game(ctx, T)[2:] == (nc.restated("rps")[2], -nc.restated("rps")[2])


@pytest.mark.parametrize("game", ["kuhn_poker", "leduc_poker"])
def test_psro_with_the_device_nash_solver_is_psro_with_the_restatement(ctx, game):
    import open_spiel_amd as osa
    import open_spiel_amd.meta_solvers as ms
    on_device, on_host = osa.PSROSolver(ctx, game, meta_solver="nash_lp"), osa.PSROSolver(ctx, game, meta_solver=nc.meta_solver)
    for it in range(6):
        meta_game = on_device.meta_games()[0]
        on_device.iteration()
        on_host.iteration()
        got, want = on_device.last_meta_strategies(), on_host.last_meta_strategies()
        assert [len(w) for w in got] == [it + 1] * 2
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), it
        nc.certify(meta_game, got[0], got[1], ms.solve_zero_sum_matrix_game(ctx, meta_game)[2], 0, f"{game} iteration {it}")
    assert all(np.array_equal(a, b) for a, b in zip(on_device.meta_games(), on_host.meta_games()))
    assert all(np.array_equal(a, b) for a, b in zip(on_device.policies(), on_host.policies()))
    assert any(not np.allclose(w, 1.0 / len(w)) for w in got), "the meta-strategies stayed uniform"


# ---- the sweep ----
_SWEPT = {}


def _swept(m, n, family):
    if (m, n, family) not in _SWEPT:
        _SWEPT[m, n, family] = nc.solve(nc.sweep_matrix(m, n, family))
    return _SWEPT[m, n, family]


def _both_ways(ctx, batch):
    """The batch through host pointers and through device pointers."""
    import torch
    import open_spiel_amd.meta_solvers as ms
    on_device = ms.solve_zero_sum_matrix_games(ctx, torch.as_tensor(batch, device=ctx.device), device=True)
    return ms.solve_zero_sum_matrix_games(ctx, batch), {k: v.cpu().numpy() for k, v in on_device.items()}


def _without_pivots(ctx, batch):
    """osg_nash_lp with a null `pivots`, which the ABI allows and the Python wrapper never passes."""
    from open_spiel_amd._abi import check, lib
    B, rows, cols = batch.shape
    out = dict(row=np.empty((B, rows)), col=np.empty((B, cols)), value=np.empty(B), status=np.empty(B, np.int32))
    check(lib().osg_nash_lp(ctx._h, rows, cols, B, batch.ctypes.data, out["row"].ctypes.data, out["col"].ctypes.data,
                            out["value"].ctypes.data, None, out["status"].ctypes.data, 1))
    return out


@pytest.mark.parametrize("m", nc.SIDES)
def test_device_is_the_restatement_on_the_sweep(ctx, m):
    for n in nc.SIDES:
        families = nc.families(m, n)
        batch = np.stack([nc.sweep_matrix(m, n, f) for f in families])
        outs = _both_ways(ctx, batch)
        for k, family in enumerate(families):
            for out in outs:
                _same(out, k, _swept(m, n, family), f"{family} {m}x{n}")
        if n == m:
            bare = _without_pivots(ctx, batch)
            assert all(np.array_equal(bare[key], outs[0][key], equal_nan=True) for key in bare), f"{m}x{n}, pivots null"


def test_device_is_the_restatement_at_the_ends_of_the_range_and_on_power_of_two_multiples(ctx):
    extra = [(name, A) for name, A, _ in nc.range_cases()]
    extra += [(f"{name} * 2**{k}", np.ldexp(A, k)) for name, A in nc.scaling_matrices().items() for k in (0, *nc.SCALINGS)]
    for shape in sorted({A.shape for _, A in extra}):
        names, batch = zip(*[(name, A) for name, A in extra if A.shape == shape])
        for out in _both_ways(ctx, np.stack(batch)):
            for k, name in enumerate(names):
                _same(out, k, nc.solve(batch[k]), name)
    for name, A in nc.scaling_matrices().items():   # device against device: the same bits, the value's exponent moved
        out = _both_ways(ctx, np.stack([np.ldexp(A, k) for k in (0, *nc.SCALINGS)]))[1]
        for at, k in enumerate(nc.SCALINGS, 1):
            assert all(np.array_equal(out[key][at], out[key][0]) for key in ("row", "col", "pivots", "status")), (name, k)
            assert out["value"][at] == np.ldexp(out["value"][0], k), (name, k)


@pytest.mark.parametrize("m", nc.SIDES)
def test_a_sweep_problems_bits_do_not_depend_on_its_place_among_4096(ctx, m):
    import torch
    import open_spiel_amd.meta_solvers as ms
    for n in nc.SIDES:
        families = nc.families(m, n)
        rng = np.random.default_rng(m * 100 + n)
        which = rng.permutation(np.arange(4096) % len(families))
        stack = torch.as_tensor(np.stack([nc.sweep_matrix(m, n, f) for f in families]), device=ctx.device)
        out = ms.solve_zero_sum_matrix_games(ctx, stack[torch.as_tensor(which, device=ctx.device)], device=True)
        places = np.sort(rng.choice(4096, 64, replace=False))
        out = {key: v[torch.as_tensor(places, device=ctx.device)].cpu().numpy() for key, v in out.items()}
        for k, place in enumerate(places):
            _same(out, k, _swept(m, n, families[which[place]]), f"{families[which[place]]} {m}x{n} at {place}")
