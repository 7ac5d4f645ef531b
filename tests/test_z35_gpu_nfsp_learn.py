"""The fused NFSP / DQN learner on the device (osg_*_sample_many, osg_nfsp_learn; NFSPSolver(learner="fused")) against the
NumPy float64 restatement (tests/nfsp_learn_cases.py).

The learner cases fill the buffers of two NFSPSolver objects — learner="torch" and learner="fused" — with the same
synthetic rows on the game's real tensor matrix and legal mask, make the same U updates with both, and hold each
against the float64 reference fed the slots that were drawn.  dev(x) = max |x - x64| / max(1, max |x64|) over parameters
and losses.  The tolerance of a case is 8 x the largest dev the torch float32 learner shows on the cases of its kind and
U; the reference's smallest branch margin must exceed 100 x that tolerance.

Measured on an MI355X (profiles/nfsp_learn_probe.txt): fused dev 0 to 7.1e-8, torch dev 0 to 7.1e-8 (on the [128] x 128 cases
2.0e-8 against 6.2e-8 and 7.1e-8), tolerances 6.0e-8 to 5.7e-7, smallest margin 4.2e-4."""
import numpy as np
import pytest
import torch

import nfsp_learn_cases as lc

pytestmark = pytest.mark.gpu

# (game, hidden, B, U, loss, discount, final rows)
DQN_CASES = [("kuhn_poker", [8], 1, 1, "mse", 1.0, "all"), ("kuhn_poker", [48], 40, 3, "huber", 0.9, "mixed"),
             ("leduc_poker", [128], 128, 3, "mse", 0.9, "none"), ("leduc_poker", [32, 16], 40, 1, "huber", 1.0, "mixed"),
             ("leduc_poker", [128], 128, 1, "mse", 1.0, "mixed"), ("kuhn_poker", [8], 40, 3, "mse", 1.0, "all")]
# (game, hidden, B, U, clip): 0.02 bites, 100 does not
SL_CASES = [("kuhn_poker", [8], 1, 1, None), ("kuhn_poker", [48], 40, 3, 0.02), ("leduc_poker", [128], 128, 3, 100.0),
            ("leduc_poker", [32, 16], 40, 1, 0.02), ("leduc_poker", [128], 128, 1, None), ("kuhn_poker", [8], 40, 3, 100.0)]
# lc.synthetic_rows seeds, chosen on the CPU with the reference alone: the first seed from 1 whose smallest branch margin
# exceeds 4e-4 (the tolerances come out near 7e-7)
SEEDS = {0: [1, 1, 1, 1, 1, 1], 1: [1, 3, 2, 1, 1, 1]}


@pytest.fixture(scope="module")
def osa():
    import open_spiel_amd
    return open_spiel_amd


@pytest.fixture(scope="module")
def ctx(osa):
    return osa.Context(0)


def _solver(osa, ctx, tabular, game, hidden, B, learner, **kw):
    from open_spiel_amd.nfsp import NFSPSolver
    if game not in tabular:
        tabular[game] = osa.TabularSolver(ctx, game, mccfr=True)
    return NFSPSolver(ctx, game, hidden, 4096, 0.1, batch_size=B, min_buffer_size_to_learn=1, rl_learning_rate=0.1, sl_learning_rate=0.1,
                      replay_buffer_capacity=4096, learner=learner, tabular=tabular[game], **kw)


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy()


def _fill(solver, kind, seed, size, finals, p=0):
    """lc.synthetic_rows into player p's ring (kind 0) or reservoir (kind 1); infostate 0 gets a single legal action."""
    dev = solver.ctx.device
    mask = lc.single_action_mask(solver._legal_mask.cpu().numpy())
    solver._legal_mask = torch.from_numpy(mask).to(dev)
    if solver._learner == "fused":
        solver._legal_mask_u8 = solver._legal_mask.to(torch.uint8).contiguous()
    rows = [torch.from_numpy(c).to(dev) for c in lc.synthetic_rows(kind, seed, size, mask, finals)]
    if kind == 0:
        solver.replay_buffers[p].append(*rows)
    else:
        solver.reservoir_buffers[p].append(rows[0], 0, rows[1])
    return mask


def _reference(solver, p, kind, before, target, mask, lr, **kw):
    """lc.learn on the rows player p's last fused call drew."""
    slots = solver.last_slots[p][1 - kind]
    got = [t.cpu().numpy() for t in (solver.replay_buffers[p] if kind == 0 else solver.reservoir_buffers[p]).rows(slots.reshape(-1))]
    rows = [r.reshape(*slots.shape, *r.shape[1:]) for r in (got if kind == 0 else [got[0], got[2]])]
    return lc.learn(kind, solver._widths, before, target, solver._tensors.cpu().numpy(), mask, rows, lr, **kw)


def _run_case(osa, ctx, tabular, kind, case, k):
    """(dev of torch, dev of fused, margin) of one case."""
    game, hidden, B, U = case[:4]
    kw = dict(loss_str=case[4], huber_loss_parameter=0.5, discount_factor=case[5]) if kind == 0 else dict(gradient_clipping=case[4])
    out = {}
    for learner in ("torch", "fused"):
        solver = _solver(osa, ctx, tabular, game, hidden, B, learner, **kw)
        mask = _fill(solver, kind, SEEDS[kind][k], B, case[6] if kind == 0 else None)
        net = (solver._q_networks if kind == 0 else solver._avg_networks)[0]
        before, target = _flat(net), _flat(solver._target_q_networks[0])
        if learner == "torch":
            losses = [(solver._learn_q if kind == 0 else solver._learn_average)(0) for _ in range(U)]
        else:
            solver._learn_fused([(U if kind else 0, 0 if kind else U, 0)] + [(0, 0, 0)] * (solver._num_players - 1))
            ref = _reference(solver, 0, kind, before, target, mask, 0.1,
                             **(dict(discount=case[5], loss=case[4], beta=0.5) if kind == 0 else dict(clip=case[4])))
            losses = [solver.last_rl_loss[0] if kind == 0 else solver.last_sl_loss[0]]   # the solver keeps a call's last loss
        out[learner] = (_flat(net), losses)
    return lc.dev(out["torch"], ref[:2]), lc.dev(out["fused"], (ref[0], ref[1][-1:])), ref[2]


@pytest.fixture(scope="module")
def measured(osa, ctx):
    """kind -> one entry per case, each run once."""
    tabular = {}
    return {kind: [_run_case(osa, ctx, tabular, kind, case, k) for k, case in enumerate(cases)]
            for kind, cases in ((0, DQN_CASES), (1, SL_CASES))}


@pytest.mark.parametrize("kind,k", [(kind, k) for kind, cases in ((0, DQN_CASES), (1, SL_CASES)) for k in range(len(cases))])
def test_learner_against_the_float64_reference(measured, kind, k):
    cases = DQN_CASES if kind == 0 else SL_CASES
    U = cases[k][3]
    tol = 8 * max(m[0] for m, c in zip(measured[kind], cases) if c[3] == U)
    d_torch, d_fused, margin = measured[kind][k]
    print(f"kind {kind} case {cases[k]}: torch dev {d_torch:.3e}, fused dev {d_fused:.3e}, tolerance {tol:.3e}, margin {margin:.3e}")
    assert margin > 100 * tol
    assert d_fused <= tol


@pytest.mark.parametrize("ring", [True, False])
@pytest.mark.parametrize("m", [1, 32, 128])
def test_batched_draws_equal_single_draws(osa, ctx, ring, m):
    from open_spiel_amd.nfsp import TransitionRing
    dev, streams = ctx.device, [3, 2 ** 40 + 1, 0, 77, 2 ** 63 + 5]
    for size in sorted({m, m + 1, 1000, 70001}):
        if ring:
            buf = TransitionRing(ctx, size)
            z = torch.zeros(size, dtype=torch.int32, device=dev)
            buf.append(z, z, z.float(), z, z.to(torch.uint8))
        else:
            buf = osa.deep_cfr.ReservoirBuffer(ctx, 2, size, 5, 1)
            buf.append(torch.zeros(size, dtype=torch.int32, device=dev), 0, torch.zeros((size, 2), device=dev))
        many = buf.sample_slots_many(m, 99, streams)
        for u, s in enumerate(streams):
            assert torch.equal(many[u], buf.sample_slots(m, 99, s)), (size, s)
            assert torch.equal(many[u], buf.sample_slots_many(m, 99, [s])[0]), (size, s)
    with pytest.raises(osa.OsgError):
        buf.sample_slots_many(1025, 0, [1])
    with pytest.raises(ValueError):
        buf.sample_slots_many(len(buf) + 1, 0, [1])


def test_bits_do_not_depend_on_the_run_or_on_the_other_jobs(osa, ctx):
    tabular = {}

    def run(owed):
        solver = _solver(osa, ctx, tabular, "leduc_poker", [48], 40, "fused", gradient_clipping=0.02)
        for p in (0, 1):
            for kind in (0, 1):
                _fill(solver, kind, 5 + kind, 64, "mixed", p)
        solver._learn_fused(owed)     # player 0's stream ids come first either way: the same batches
        return _flat(solver._q_networks[0]), _flat(solver._avg_networks[0])
    alone, again, among = run([(3, 3, 0), (0, 0, 0)]), run([(3, 3, 0), (0, 0, 0)]), run([(3, 3, 0), (2, 2, 0)])
    for a, b, c in zip(alone, again, among):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_solver_end_to_end_and_refusals(osa, ctx):
    from open_spiel_amd.nfsp import NFSPSolver
    solvers = {}
    for learner in ("torch", "fused"):
        s = NFSPSolver(ctx, "kuhn_poker", [16], 2000, 0.5, batch_size=8, min_buffer_size_to_learn=8, learn_every=16, episodes_per_step=64,
                       replay_buffer_capacity=2000, update_target_network_every=40, learner=learner)
        drawn = []
        if learner == "torch":
            for buffers in (s.replay_buffers, s.reservoir_buffers):
                for b in buffers:
                    b.sample_slots = (lambda f: lambda *a: drawn.append(f(*a)) or drawn[-1])(b.sample_slots)
        before = [[_flat(n) for n in nets] for nets in (s._q_networks, s._target_q_networks, s._avg_networks)]
        s.step()
        for b in (s.replay_buffers + s.reservoir_buffers if learner == "torch" else []):
            del b.sample_slots        # (the recorder holds its buffer: no reference cycle may outlive the context)
        solvers[learner] = (s, drawn)
    t, f = solvers["torch"][0], solvers["fused"][0]
    assert t.updates == f.updates and t.dqn_steps == f.dqn_steps and t.nfsp_steps == f.nfsp_steps
    assert sum(u[0] + u[1] for u in f.updates) >= 4 and all(u[0] and u[1] for u in f.updates)
    fused_slots = [row for p in range(2) for s in f.last_slots[p] if s is not None for row in s]
    assert len(fused_slots) == len(solvers["torch"][1]) and all(torch.equal(a, b) for a, b in zip(fused_slots, solvers["torch"][1]))
    for p in range(2):
        for kind in (1, 0):
            ref = _reference(f, p, kind, before[0 if kind == 0 else 2][p], before[1][p], f._legal_mask.cpu().numpy(), 0.01)
            d_t, d_f = (lc.dev((_flat((s._q_networks if kind == 0 else s._avg_networks)[p]), []), (ref[0], [])) for s in (t, f))
            print(f"player {p} kind {kind}: torch dev {d_t:.3e}, fused dev {d_f:.3e}")
            assert d_f <= 8 * d_t
    with pytest.raises(ValueError, match="learner='torch'"):
        NFSPSolver(ctx, "kuhn_poker", [16], 2000, 0.5, optimizer_str="adam", learner="fused")
    wide = NFSPSolver(ctx, "kuhn_poker", [200], 64, 0.5, batch_size=8, min_buffer_size_to_learn=8, learner="fused")
    _fill(wide, 0, 1, 16, "mixed")
    with pytest.raises(osa.OsgError, match="hidden widths"):
        wide._learn_fused([(0, 1, 0), (0, 0, 0)])
