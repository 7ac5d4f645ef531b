"""The fused Deep CFR learner on the device (osg_deep_cfr_learn; DeepCFRSolver(learner="fused")) against the NumPy float64
restatement (tests/deep_cfr_learn_cases.py).

A learner case fills the buffers of two DeepCFRSolver objects — learner="torch" and learner="fused" — with the same
synthetic rows on the game's real tensor matrix, makes the same U updates with both, and holds each against the float64
reference fed the slots that were drawn.  dev(p) = max |p - p64| / max |p64| over the parameters, those left out whose
reference has 0 < sqrt(v^) < 1e-5 at some update (at most 1 % of a case's).  The tolerance of a case is 8 x the largest
dev the torch float32 learner shows on the cases of its kind and U; the reference's smallest nonzero ReLU
pre-activation must exceed 100 x that tolerance.

Measured on an MI355X, in the order of lc.CASES, no case with a parameter left out (share 0): fused dev 4.5e-8 1.8e-7
4.7e-8 2.5e-7 4.7e-8 4.8e-8 | 1.3e-6 2.2e-7 5.4e-8 5.2e-8 6.2e-8 5.5e-8; torch dev 2.9e-8 1.8e-7 4.7e-8 2.5e-7 4.7e-8
4.8e-8 | 1.0e-6 1.6e-7 5.4e-8 5.2e-8 5.7e-8 5.5e-8 (after one update both are the rounding of p - lr).  Tolerances: kind 0
3.8e-7 (U = 1) and 2.0e-6 (U = 12), kind 1 4.5e-7 and 8.3e-6; smallest margin 6.4e-4 (U = 1), 1.0e-3 (U = 12)."""
import numpy as np
import pytest
import torch

import deep_cfr_learn_cases as lc

pytestmark = pytest.mark.gpu
LR = 1e-3


@pytest.fixture(scope="module")
def osa():
    import open_spiel_amd
    return open_spiel_amd


@pytest.fixture(scope="module")
def ctx(osa):
    return osa.Context(0)


@pytest.fixture(scope="module")
def tabular():
    return {}


def _solver(osa, ctx, tabular, game, hidden, B, learner, seed=1, **kw):
    if game not in tabular:
        tabular[game] = osa.TabularSolver(ctx, game)
    kw = dict(dict(policy_network_layers=hidden, advantage_network_layers=hidden, batch_size_advantage=B, batch_size_strategy=B), **kw)
    return osa.deep_cfr.DeepCFRSolver(ctx, game, learning_rate=LR, memory_capacity=4096, seed=seed, tabular=tabular[game], learner=learner, **kw)


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy()


def _parts(s, kind):
    if kind:
        return s._policy_network, s._strategy_memories, s._optimizer_policy, s._loss_policy
    return s._advantage_networks[0], s._advantage_memories[0], s._optimizer_advantages[0], s._loss_advantages


def _fill(s, kind, seed, size):
    infostates = s._rows_of[0].cpu().numpy() if kind == 0 else np.arange(s.tabular.num_infostates)
    info, iteration, values = lc.synthetic_rows(kind, seed, size, infostates, s._num_actions)
    for it in np.unique(iteration):
        rows = iteration == it
        _parts(s, kind)[1].append(torch.from_numpy(info[rows]).to(s.ctx.device), int(it), torch.from_numpy(values[rows]).to(s.ctx.device))


def _reference(s, kind, slots, before):
    net, memory = _parts(s, kind)[:2]
    rows = [t.cpu().numpy().reshape(*slots.shape, *t.shape[1:]) for t in memory.rows(slots.reshape(-1))]
    widths = [s._embedding_size] + [m.out_features for m in net.modules() if isinstance(m, torch.nn.Linear)]
    return lc.learn(kind, widths, before, s._tensors.cpu().numpy(), rows, LR)


def _run_case(osa, ctx, tabular, case):
    """(dev of torch, dev of fused, margin, share left out, loss of fused, of the reference) of one case."""
    kind, game, hidden, B, U, seed = case
    out = {}
    for learner in ("torch", "fused"):
        s = _solver(osa, ctx, tabular, game, list(hidden), B, learner, seed)
        _fill(s, kind, seed, B + 16)
        net, memory, opt, loss_fn = _parts(s, kind)
        before = _flat(net)
        loss = s._train(net, opt, loss_fn, memory, B, U)
        out[learner] = (_flat(net), loss, before)
    assert np.array_equal(out["torch"][2], before)
    ref = _reference(s, kind, s.last_slots, before)
    keep = ~ref[5]
    assert (~keep).mean() <= 0.01      # the seed's share of parameters left out
    return lc.dev(out["torch"][0], ref[0], keep), lc.dev(out["fused"][0], ref[0], keep), ref[4], (~keep).mean(), out["fused"][1], ref[3][-1]


@pytest.fixture(scope="module")
def measured(osa, ctx, tabular):
    return [_run_case(osa, ctx, tabular, case) for case in lc.CASES]


@pytest.mark.parametrize("k", range(len(lc.CASES)))
def test_learner_against_the_float64_reference(measured, k):
    kind, U = lc.CASES[k][0], lc.CASES[k][4]
    tol = 8 * max(m[0] for m, c in zip(measured, lc.CASES) if (c[0], c[4]) == (kind, U))
    d_torch, d_fused, margin, share, loss, loss64 = measured[k]
    print(f"case {lc.CASES[k]}: torch dev {d_torch:.3e}, fused dev {d_fused:.3e}, tolerance {tol:.3e}, margin {margin:.3e}, "
          f"left out {share:.4f}, loss {loss:.8g} against {loss64:.8g}")
    assert margin > 100 * tol
    assert d_fused <= tol
    assert abs(loss - loss64) <= 1e-4 * abs(loss64)      # a float32 mean of at most 768 terms


def _job(s, kind, slots, state=None, step0=0):
    """One job of the C entry on copies of the network's buffers (or on `state`): (job, [params, m, v, losses])."""
    net, memory = _parts(s, kind)[:2]
    flat = s._fused[net].params
    bufs = (state or [flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)])[:3] + [torch.empty(slots.shape[0], device=flat.device)]
    return s._fused_job(net, memory, slots, bufs[3], *bufs[:3], step0), bufs


def _launch(osa, ctx, pairs):
    from open_spiel_amd._abi import DeepCfrLearnJob, check, lib
    check(lib().osg_deep_cfr_learn(ctx._h, (DeepCfrLearnJob * len(pairs))(*[job for job, _ in pairs]), len(pairs)))
    ctx.synchronize()
    return [[b.cpu().numpy() for b in bufs] for _, bufs in pairs]


def test_moments_and_step_count_carry_across_calls(osa, ctx, tabular):
    s = _solver(osa, ctx, tabular, "leduc_poker", [64], 129, "fused")
    _fill(s, 0, 3, 160)
    slots = s._advantage_memories[0].sample_slots_many(129, 9, np.arange(1, 13))
    whole = _launch(osa, ctx, [_job(s, 0, slots)])[0]
    first = _job(s, 0, slots[:6].contiguous())
    losses = _launch(osa, ctx, [first])[0][3]
    halves = _launch(osa, ctx, [_job(s, 0, slots[6:].contiguous(), first[1], step0=6)])[0]
    assert all(np.array_equal(a, b) for a, b in zip(whole[:3], halves[:3])) and np.array_equal(whole[3], np.concatenate([losses, halves[3]]))
    assert np.abs(whole[1]).max() > 0 and np.abs(whole[2]).max() > 0 and np.isfinite(whole[3]).all()


def test_bits_do_not_depend_on_the_run_or_on_the_other_jobs(osa, ctx, tabular):
    from open_spiel_amd.deep_cfr import fused_plan
    wide = _solver(osa, ctx, tabular, "leduc_poker", [128, 128], 40, "fused")     # its moments stay in global memory
    assert not fused_plan(ctx, [30, 128, 128, 3], 40)["moments_resident"] and fused_plan(ctx, [30, 64, 3], 129)["moments_resident"]
    small = _solver(osa, ctx, tabular, "leduc_poker", [64], 129, "fused")
    jobs = []
    for s, B in ((wide, 40), (small, 129)):
        for kind in (0, 1):
            _fill(s, kind, 5 + kind, 160)
            jobs.append((s, kind, _parts(s, kind)[1].sample_slots_many(B, 7, [4, 5, 6])))
    alone = [_launch(osa, ctx, [_job(*j)])[0] for j in jobs]
    again = [_launch(osa, ctx, [_job(*j)])[0] for j in jobs]
    among = _launch(osa, ctx, [_job(*j) for j in jobs[::-1]])[::-1]
    for a, b, c in zip(alone, again, among):
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c)) and np.isfinite(a[3]).all()


def test_solver_end_to_end_and_refusals(osa, ctx, tabular):
    runs = {}
    for learner in ("torch", "fused"):
        s = _solver(osa, ctx, tabular, "kuhn_poker", None, 32, learner, 7, policy_network_layers=(32, 16), advantage_network_layers=(16, 8),
                    num_iterations=1, num_traversals=64, advantage_network_train_steps=20, policy_network_train_steps=20)
        s.solve()
        # (player 0's rows of iteration 1 precede every update; later rows see networks that differ in their last bits)
        runs[learner] = [t.cpu().numpy() for t in s.advantage_buffers[0].filled()]
        s._num_iterations = 2
        _, advantage_losses, policy_loss = s.solve()
    assert all(np.array_equal(a, b) for a, b in zip(runs["torch"], runs["fused"])) and len(runs["fused"][0]) >= 32
    assert s.iteration == 4 and np.isfinite(policy_loss) and all(np.isfinite(l) for p in (0, 1) for l in advantage_losses[p])
    assert np.abs(s.policy_table().sum(1) - 1).max() < 1e-12
    for kw in (dict(batch_size_advantage=None), dict(batch_size_strategy=2048), dict(policy_network_layers=(256, 256))):
        with pytest.raises(ValueError, match="learner='torch'"):
            _solver(osa, ctx, tabular, "kuhn_poker", [16], 32, "fused", **kw)
    slots = s._advantage_memories[0].sample_slots_many(32, 1, [1, 2, 3])
    slots[1, 3] = len(s._advantage_memories[0]) + 5        # out of range: the update's loss is NaN, its row counts as zeros
    out = _launch(osa, ctx, [_job(s, 0, slots)])[0]
    assert np.isfinite(out[3][[0, 2]]).all() and np.isnan(out[3][1]) and np.isfinite(out[0]).all()
