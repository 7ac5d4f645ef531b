"""The fused policy-value forward on the device (osg_vpnet_forward; mcts.VPNetEvaluator(model, forward="fused")) against
the float64 restatement of test_vpnet_host.  The forward has no discontinuity in its outputs, so the comparison is a
rounding matter: the kernel's largest absolute deviation from float64 (prior and value together) may be at most 4 x that
of torch's float32 VPNetMLP.forward on the device for the same case — a different but equally long summation order.

Measured on an MI355X, in the order of CASES: fused 1.08e-8 4.80e-8 4.77e-8 1.04e-8 1.34e-8 2.33e-8; torch 1.90e-8 4.80e-8
4.77e-8 1.30e-8 1.49e-8 2.61e-8."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_vpnet_host import reference_forward

pytestmark = pytest.mark.gpu

# (O, W, depth, A, n; n in rows or as (tiles, extra) of the planner's R): depth 0 and one row; W padded, a partial tile;
# a second tile; O's tail, three mask words, three tiles; odd W; the widest form (R = 32) and four mask words.
CASES = [(27, 64, 0, 9, 1), (126, 40, 1, 7, (1, -1)), (126, 256, 1, 7, (1, 1)), (729, 256, 2, 81, (2, 3)), (225, 17, 3, 26, 67),
         (1089, 512, 1, 121, 33)]


@pytest.fixture(scope="module")
def osa():
    import open_spiel_amd
    import open_spiel_amd.alpha_zero   # noqa: F401 (and with it open_spiel_amd.mcts)
    return open_spiel_amd


@pytest.fixture(scope="module")
def ctx(osa):
    return osa.Context(0)


def _rows_per_workgroup(osa, ctx, shape):
    plan = (C.c_int64 * 8)()
    osa._abi.check(osa.lib().osg_vpnet_plan(ctx._h, *shape, plan))
    return int(plan[0])

def _fused(osa, ctx, shape, flat, obs, bits):
    O, W, D, A = shape
    n = obs.shape[0]
    prior = torch.full((n, A), float("nan"), dtype=torch.float64, device=ctx.device)
    value = torch.full((n, 2), float("nan"), dtype=torch.float64, device=ctx.device)
    osa._abi.check(osa.lib().osg_vpnet_forward(ctx._h, O, W, D, A, flat.data_ptr(), obs.data_ptr(), bits.data_ptr(), bits.shape[1], n,
                                               prior.data_ptr(), value.data_ptr()))
    ctx.synchronize()
    return prior.cpu().numpy(), value.cpu().numpy()


def _case(osa, ctx, case):
    """model, obs, legal [n, A] bool, bits [n, words] i32 on the device: 0 / 1 observations, row 0 without a legal action
    (n > 1), row 1 with one."""
    O, W, D, A, n = case
    if isinstance(n, tuple):
        n = n[0] * _rows_per_workgroup(osa, ctx, (O, W, D, A)) + n[1]
    torch.manual_seed(11)
    model = osa.alpha_zero.VPNetMLP(O, A, W, D).to(ctx.device)
    g = torch.Generator().manual_seed(7)
    obs = (torch.rand(n, O, generator=g) < 0.3).float().to(ctx.device)
    legal = torch.rand(n, A, generator=g) < 0.5
    legal[:, A - 1] |= ~legal.any(1)
    if n > 1:
        legal[0] = False
        legal[1] = torch.arange(A) == A // 2
    words = (A + 31) // 32
    padded = torch.zeros(n, 32 * words, dtype=torch.int64)
    padded[:, :A] = legal
    bits = (padded.reshape(n, words, 32) << torch.arange(32)).sum(2)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).to(ctx.device)
    return model, obs, legal.to(ctx.device), bits


def _deviations(want, prior, value, torch_policy, torch_value, legal):
    assert not np.isnan(prior).any() and not np.isnan(value).any()
    assert (prior[~legal] == 0.0).all() and np.array_equal(value[:, 1], -value[:, 0])
    assert np.abs(prior.sum(1) - legal.any(1)).max() < 1e-5          # 1 with a legal action, 0 without
    return (max(np.abs(prior - want[0]).max(), np.abs(value[:, 0] - want[1]).max()),
            max(np.abs(torch_policy * legal - want[0]).max(), np.abs(torch_value - want[1]).max()))


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_float64_within_four_times_torch_float32(osa, ctx, case):
    model, obs, legal, bits = _case(osa, ctx, case)
    shape = case[:4]
    prior, value = _fused(osa, ctx, shape, model.flat, obs, bits)
    with torch.no_grad():
        torch_policy, torch_value = model(obs, legal)
    want = reference_forward(model.flat.detach().cpu().numpy(), shape, obs.cpu().numpy(), legal.cpu().numpy())
    dev, torch_dev = _deviations(want, prior, value, torch_policy.cpu().numpy(), torch_value.cpu().numpy(), legal.cpu().numpy())
    print(f"vpnet case {case}: n {obs.shape[0]} fused dev {dev:.3e} torch dev {torch_dev:.3e}")
    assert dev <= 4 * torch_dev, (dev, torch_dev)


def test_a_rows_bits_do_not_depend_on_the_other_rows(osa, ctx):
    case = CASES[2]
    model, obs, legal, bits = _case(osa, ctx, case)
    R = _rows_per_workgroup(osa, ctx, case[:4])
    prior, value = _fused(osa, ctx, case[:4], model.flat, obs, bits)
    for row in (0, R - 1, R):
        alone = _fused(osa, ctx, case[:4], model.flat, obs[row:row + 1].contiguous(), bits[row:row + 1].contiguous())
        assert np.array_equal(alone[0][0], prior[row]) and np.array_equal(alone[1][0], value[row]), row


def test_the_fused_evaluator_through_the_public_path(osa, ctx):
    torch.manual_seed(13)
    model = osa.alpha_zero.VPNetMLP(126, 7, 64, 1).to(ctx.device)
    fused, plain = osa.mcts.VPNetEvaluator(model, forward="fused"), osa.mcts.VPNetEvaluator(model)
    batch = osa.StateBatch(ctx, "connect_four", 257)
    batch.random_steps(5, 30)
    everything = torch.ones(257, dtype=torch.bool, device=ctx.device)
    prior, value = fused.evaluate(batch, everything, everything)
    torch_prior, torch_value = plain.evaluate(batch, everything, everything)
    ctx.synchronize()
    legal = batch.legal_actions_bool().cpu().numpy()
    want = reference_forward(model.flat.detach().cpu().numpy(), (126, 64, 1, 7), batch.observation_tensor(-1).cpu().numpy(), legal)
    dev, torch_dev = _deviations(want, prior.cpu().numpy(), value.cpu().numpy(), torch_prior.cpu().numpy(), torch_value[:, 0].cpu().numpy(), legal)
    assert dev <= 4 * torch_dev, (dev, torch_dev)
    roots = osa.StateBatch(ctx, "connect_four", 64)
    roots.random_steps(9, 4)
    visits = [osa.mcts.search(roots, ev, max_simulations=8, puct=True)["child_visits"].sum(1).cpu() for ev in (fused, plain)]
    assert torch.equal(visits[0], visits[1]) and int(visits[0].min()) > 0
    with pytest.raises(ValueError, match='forward="torch"'):
        osa.mcts.VPNetEvaluator(osa.alpha_zero.VPNetMLP(126, 7, 513, 1).to(ctx.device), forward="fused")
