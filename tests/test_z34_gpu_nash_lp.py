"""The exact Nash meta-solver on the device (osg_nash_lp in include/osg_abi.h; open_spiel_amd.meta_solvers;
PSROSolver(meta_solver="nash_lp")) against the NumPy restatement of open_spiel_amd/csrc/osg_nash_lp.h (nash_lp_cases.solve:
array_equal, since both evaluate the one order the header fixes without fused multiply-adds) and against the certificate
of a Nash pair with HiGHS's value (nash_lp_cases.certify)."""
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
