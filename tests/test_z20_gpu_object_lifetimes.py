"""Every object that owns device memory, made, used until each of its lazily-made buffers exists, and dropped — three
times over in one process.  The same deterministic work on fresh objects gives the same numbers (round 3 equals round 1
exactly), and in the last round the context is closed BEFORE its objects go: they hold a reference on it, their buffers
are freed before that reference is dropped, and a new solver on the closed context is refused.

kuhn_poker and leduc_poker are the smallest trees that reach the one-workgroup, the split and the jobs paths.

The MCCFR rounds sample ONE trajectory per launch: the sampling kernels add into the delta tables with fp64 atomics, and
the order of the additions of several trajectories inside one launch is not fixed (tests/test_z3_gpu_comm.py compares
such tables within 1e-11 for that reason).  Measured with 512 trajectories per launch: leduc_poker regrets of two rounds
differed in 78 of 2808 cells by at most 2.8e-14 (relative 4.8e-14), kuhn_poker in none.  One trajectory is one thread
adding in program order, which is what "exactly" can be asked of."""
import ctypes as C
import gc

import numpy as np
import pytest

GAMES = ("kuhn_poker", "leduc_poker")


def _flat(prefix, value, out):
    """Every array of a (nested) result, by name."""
    import torch
    if isinstance(value, dict):
        for k, v in value.items():
            _flat(f"{prefix}.{k}", v, out)
    elif isinstance(value, torch.Tensor):
        out[prefix] = value.detach().cpu().numpy().copy()
    elif isinstance(value, (list, tuple)) and value and isinstance(value[0], str):
        out[prefix] = np.array(value)
    else:
        out[prefix] = np.array(value)


def _cfr(osa, ctx, game, general_kernel, monkeypatch, out):
    tag = f"{game}.cfr[{general_kernel}]"
    s = osa.TabularSolver(ctx, game, general_kernel=general_kernel)
    s.evaluate_and_update_policy(3)
    s.set_discounting(1.5, 0, 2)                      # the per-iteration factor table
    s.evaluate_and_update_policy(3)
    _flat(f"{tag}.eval", s.evaluate_policy(), out)
    if general_kernel == "grid":                      # the large trees' evaluation: its plan and its [H, P] array are made here
        monkeypatch.setenv("OSG_EVAL_GRID", "1")
        monkeypatch.setenv("OSG_EVAL_JOBS", "0")
        _flat(f"{tag}.eval_grid", s.evaluate_policy(), out)
        assert s.last_eval_kernel() == "k_geval"
        monkeypatch.delenv("OSG_EVAL_GRID")
        monkeypatch.delenv("OSG_EVAL_JOBS")
    _flat(f"{tag}.q", s.action_values(), out)
    _flat(f"{tag}.q_br", s.action_values(responder=0), out)
    s.set_discounting(enabled=False)                  # (CFR-BR is plain CFR)
    s.evaluate_and_update_policy_cfr_br(2)
    _flat(f"{tag}.tables", s.tables(), out)
    return s


def _round(osa, mcts, monkeypatch, close_context_first):
    import torch
    ctx = osa.Context(0)
    lib = osa.lib()
    out, alive = {}, []
    for game in GAMES:
        alive.append(_cfr(osa, ctx, game, False, monkeypatch, out))
        alive.append(_cfr(osa, ctx, game, "grid", monkeypatch, out))

        for kernel in (False, "grid"):                # the fused form (the weight table), the best response per level
            x = osa.XFPSolver(ctx, game, general_kernel=kernel)
            x.iterate(3)
            _flat(f"{game}.xfp[{kernel}].reaches", x.reaches(), out)
            _flat(f"{game}.xfp[{kernel}].tables", x.tables(), out)
            alive.append(x)

        m = osa.MMDSolver(ctx, game, alpha=0.1)
        m.set_params(0.05)
        m.iterate(3)
        out[f"{game}.mmd.gap"] = np.array(m.get_gap())
        m.reset()
        m.iterate(2)
        _flat(f"{game}.mmd.tables", m.tables(), out)
        alive.append(m)

        c = osa.TabularSolver(ctx, game, mccfr=True)
        first, second = c.mccfr_new_delta_buffer(), c.mccfr_new_delta_buffer()
        c.mccfr_sample_into(first, 0x5EED, 1)
        c.mccfr_apply_deltas_from(first)
        c.mccfr_sample_into(second, 0x5EED, 1, first_trajectory=1)
        c.mccfr_apply_deltas_from(second)
        _flat(f"{game}.mccfr.tables", c.tables(), out)
        alive.append(c)

    roots = osa.StateBatch(ctx, "tic_tac_toe", 64)    # a stepwise MCTS tree, made and dropped by the search
    res = mcts.search(roots, mcts.RolloutEvaluator(), max_simulations=16, uct_c=1.7, n_rollouts=1, seed=7)
    _flat("mcts", {k: res[k] for k in ("best_action", "child_visits", "child_reward")}, out)
    alive.append(roots)

    uid = C.create_string_buffer(128)                  # a single-rank communicator
    assert lib.osg_comm_unique_id(uid) == 0, lib.osg_last_error().decode()
    comm = C.c_void_p()
    assert lib.osg_comm_create(ctx._h, 0, 1, uid, C.byref(comm)) == 0, lib.osg_last_error().decode()
    v = torch.arange(64, dtype=torch.float64, device="cuda")
    assert lib.osg_allreduce_sum_f64(comm, C.c_void_p(v.data_ptr()), v.numel()) == 0, lib.osg_last_error().decode()
    _flat("comm.sum", v, out)

    ctx.synchronize()
    if close_context_first:
        handle = ctx._h
        ctx.close()
        ctx._h = handle                                # (the objects above keep the closed context alive)
        with pytest.raises(osa.OsgError):
            osa.TabularSolver(ctx, "kuhn_poker")
        ctx._h = None
    assert lib.osg_comm_destroy(comm) == 0, lib.osg_last_error().decode()
    del alive, roots, res, x, m, c, first, second
    gc.collect()
    torch.cuda.synchronize()
    if not close_context_first:
        ctx.close()
    return out


@pytest.mark.gpu
def test_three_rounds_of_every_owner_give_the_same_numbers(monkeypatch):
    import open_spiel_amd as osa
    from open_spiel_amd import mcts
    rounds = [_round(osa, mcts, monkeypatch, close_context_first=k == 2) for k in range(3)]
    assert rounds[0].keys() == rounds[2].keys() and len(rounds[0]) > 40
    for name, want in rounds[0].items():
        np.testing.assert_array_equal(rounds[2][name], want, err_msg=name)
