"""The wide fused Deep CFR learner on the device (osg_deep_cfr_learn_wide; DeepCFRSolver(learner="fused_wide")) against the
NumPy float64 restatement (tests/deep_cfr_learn_cases.py), with the helpers and the rules of test_z36_gpu_deep_cfr_learn:
dev(p) = max |p - p64| / max |p64| over the parameters kept, tolerance 8 x the largest dev of torch's float32 learner on
the cases of the same kind and U, smallest nonzero ReLU pre-activation of the reference above 100 x that tolerance.
After ONE update a parameter is p - lr sign(g) whatever g is, so at U = 1 Adam's first moment (0.1 g) is held to the
same rule against the reference's, torch's figure being 0.1 x its autograd gradient of the same batch.

Measured on an MI355X, in the order of CASES: wide dev 4.7e-8 9.2e-8 4.8e-8 6.4e-8 1.9e-7 | 1.5e-7 5.5e-8 6.0e-8 6.5e-8;
torch dev 4.7e-8 9.8e-8 4.8e-8 5.7e-8 1.6e-7 | 7.0e-8 5.5e-8 5.9e-8 6.0e-8.  First moment at U = 1: wide 3.2e-7 3.7e-7
1.5e-6 | 4.5e-7 3.4e-7 6.1e-7; torch 1.1e-7 3.0e-7 1.5e-6 | 6.8e-7 5.3e-7 2.9e-7.  Tolerances: kind 0 4.6e-7 (U = 1; m
1.2e-5) and 1.3e-6 (U = 3), kind 1 4.8e-7 (m 5.4e-6) and 5.6e-7; smallest margin 1.46e-4 (1.26e-4 is asked of it, at
(256, 256), U = 3); at most 0.04 % of a case's parameters left out.  Seed 1 meets both conditions in every case."""
import numpy as np
import pytest
import torch

import deep_cfr_learn_cases as lc
from test_z36_gpu_deep_cfr_learn import _fill, _flat, _job, _parts, _reference, _solver, ctx, osa, tabular  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

# (kind, game, hidden, B, U, seed).  One workgroup and one row; the smallest G > 1 with one row in the last workgroup
# (R = 64 for (20,)); the first width past the narrow form; widths that are no multiple of 16 in both places; the target
# at 8 workgroups, both kinds; two k-chunks per panel row and 64 workgroups.  seed: as in lc.CASES, the first from 1
# whose reference leaves out at most 1 % of the parameters and keeps its ReLU margin above 100 x the tolerance.
CASES = [
    (0, "kuhn_poker", (20,), 1, 1, 1), (0, "kuhn_poker", (20,), 65, 3, 1), (0, "leduc_poker", (200, 136), 50, 1, 1),
    (0, "leduc_poker", (256, 256), 256, 1, 1), (0, "leduc_poker", (256, 256), 256, 3, 1),
    (1, "kuhn_poker", (20,), 65, 3, 1), (1, "leduc_poker", (129,), 40, 1, 1), (1, "leduc_poker", (256, 256), 256, 1, 1),
    (1, "leduc_poker", (512,), 1024, 1, 1),
]


def _run_case(osa, ctx, tabular, case, learners=("torch", "fused_wide")):
    """Per learner (dev of the parameters, dev of Adam's m, last loss), then the reference's margin, share left out, loss."""
    kind, game, hidden, B, U, seed = case
    got = {}
    for learner in learners:
        s = _solver(osa, ctx, tabular, game, list(hidden), B, learner, seed)
        _fill(s, kind, seed, B + 16)
        net, memory, opt, loss_fn = _parts(s, kind)
        before = _flat(net)
        if learner == "torch":      # (the draw _train makes, made first on a counter of its own)
            slots = memory.sample_slots_many(B, s._seed ^ osa.deep_cfr.SAMPLE_SALT, np.arange(1, U + 1))
        loss = s._train(net, opt, loss_fn, memory, B, U)
        m = 0.1 * torch.cat([p.grad.reshape(-1) for p in net.parameters()]) if learner == "torch" else s._fused[net].m
        got[learner] = (_flat(net), m.cpu().numpy(), loss, before)
        assert np.array_equal(before, got["torch"][3]) and (learner == "torch" or torch.equal(slots, s.last_slots))
    ref = _reference(s, kind, slots, before)
    keep = ~ref[5]
    out = {k: (lc.dev(p, ref[0], keep), lc.dev(m, ref[1], keep), loss) for k, (p, m, loss, _) in got.items()}
    return out, ref[4], (~keep).mean(), ref[3][-1]


@pytest.fixture(scope="module")
def measured(osa, ctx, tabular):
    return [_run_case(osa, ctx, tabular, case) for case in CASES]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_wide_learner_against_the_float64_reference(measured, k):
    kind, U = CASES[k][0], CASES[k][4]
    same = [m[0]["torch"] for m, c in zip(measured, CASES) if (c[0], c[4]) == (kind, U)]
    tol, tol_m = 8 * max(t[0] for t in same), 8 * max(t[1] for t in same)
    out, margin, share, loss64 = measured[k]
    print(f"case {CASES[k]}: torch dev {out['torch'][0]:.3e} (m {out['torch'][1]:.3e}), wide dev {out['fused_wide'][0]:.3e} (m {out['fused_wide'][1]:.3e}), "
          f"tolerance {tol:.3e} (m {tol_m:.3e}), margin {margin:.3e}, left out {share:.4f}, loss {out['fused_wide'][2]:.8g} against {loss64:.8g}")
    assert share <= 0.01 and margin > 100 * tol
    assert out["fused_wide"][0] <= tol and (U > 1 or out["fused_wide"][1] <= tol_m)
    assert abs(out["fused_wide"][2] - loss64) <= 1e-4 * abs(loss64)


def _launch(ctx, pairs):
    from open_spiel_amd._abi import DeepCfrLearnJob, check, lib
    check(lib().osg_deep_cfr_learn_wide(ctx._h, (DeepCfrLearnJob * len(pairs))(*[job for job, _ in pairs]), len(pairs)))
    ctx.synchronize()
    return [[b.cpu().numpy() for b in bufs] for _, bufs in pairs]


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_moments_and_step_count_carry_across_calls(osa, ctx, tabular):
    s = _solver(osa, ctx, tabular, "leduc_poker", [256, 256], 129, "fused_wide")
    _fill(s, 0, 3, 160)
    slots = s._advantage_memories[0].sample_slots_many(129, 9, np.arange(1, 7))
    whole = _launch(ctx, [_job(s, 0, slots)])[0]
    first = _job(s, 0, slots[:3].contiguous())
    losses = _launch(ctx, [first])[0][3]
    halves = _launch(ctx, [_job(s, 0, slots[3:].contiguous(), first[1], step0=3)])[0]
    assert _same(whole[:3], halves[:3]) and np.array_equal(whole[3], np.concatenate([losses, halves[3]]))
    assert np.abs(whole[1]).max() > 0 and np.abs(whole[2]).max() > 0 and np.isfinite(whole[3]).all()


def test_bits_do_not_depend_on_the_run_or_on_the_other_jobs(osa, ctx, tabular):
    from open_spiel_amd.deep_cfr import fused_wide_plan
    plans = [fused_wide_plan(ctx, [30, 256, 256, 3], 256), fused_wide_plan(ctx, [30, 20, 3], 17)]
    assert (plans[0]["workgroups"], plans[1]["workgroups"]) == (8, 1)
    jobs = []
    for hidden, B in (([256, 256], 256), ([20], 17)):
        s = _solver(osa, ctx, tabular, "leduc_poker", hidden, B, "fused_wide")
        for kind in (0, 1):
            _fill(s, kind, 5 + kind, B + 16)
            jobs.append((s, kind, _parts(s, kind)[1].sample_slots_many(B, 7, [4, 5, 6])))
    alone = [_launch(ctx, [_job(*j)])[0] for j in jobs]
    again = [_launch(ctx, [_job(*j)])[0] for j in jobs]
    among = _launch(ctx, [_job(*j) for j in jobs[::-1]])[::-1]
    assert all(_same(a, b) and _same(a, c) and np.isfinite(a[3]).all() for a, b, c in zip(alone, again, among))
    assert plans == [fused_wide_plan(ctx, [30, 256, 256, 3], 256), fused_wide_plan(ctx, [30, 20, 3], 17)]


def test_solver_end_to_end_with_the_default_networks_and_refusals(osa, ctx, tabular):
    runs = {}
    for learner in ("torch", "fused_wide"):
        s = osa.deep_cfr.DeepCFRSolver(ctx, "kuhn_poker", learner=learner, batch_size_advantage=32, batch_size_strategy=32, num_iterations=2,
                                       num_traversals=64, advantage_network_train_steps=5, policy_network_train_steps=5)
        rows = []
        s.step_callback = lambda it, player, table: rows.append([t.cpu().numpy() for t in s.advantage_buffers[0].filled()]) if (it, player) == (1, 1) else None
        _, advantage_losses, policy_loss = s.solve()
        runs[learner] = rows[0]      # (player 0's rows of iteration 1 precede every update)
    assert _same(runs["torch"], runs["fused_wide"]) and len(runs["torch"][0]) >= 32
    assert s.iteration == 3 and np.isfinite(policy_loss) and all(np.isfinite(l) for p in (0, 1) for l in advantage_losses[p])
    assert np.abs(s.policy_table().sum(1) - 1).max() < 1e-12
    for kw in (dict(batch_size_advantage=None), dict(batch_size_strategy=2048), dict(policy_network_layers=(513,))):
        with pytest.raises(ValueError, match="learner='torch'"):
            _solver(osa, ctx, tabular, "kuhn_poker", [16], 32, "fused_wide", **kw)
    with pytest.raises(ValueError, match="'torch', 'fused' or 'fused_wide'"):
        _solver(osa, ctx, tabular, "kuhn_poker", [16], 32, "wide")
    slots = s._advantage_memories[0].sample_slots_many(32, 1, [1, 2, 3])
    slots[1, 3] = len(s._advantage_memories[0]) + 5        # out of range: the update's loss is NaN, its row counts as zeros
    out = _launch(ctx, [_job(s, 0, slots)])[0]
    assert np.isfinite(out[3][[0, 2]]).all() and np.isnan(out[3][1]) and np.isfinite(out[0]).all()
