"""The context's grow-only buffers — staging scratch, MCTS node pool, log table, work queue — each grown, reused by a
smaller request, given back by Context.trim() and grown again on ONE context: every result equals the one a fresh
context gives (or, for the scratch, the path that does not stage at all)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("best_action", "child_visits", "child_reward", "child_outcome", "root_stats")


def _differ(a, b):
    """The outputs of two searches that are not the same bytes (root_stats holds NaN for an unproven root)."""
    return [k for k in FIELDS if a[k].cpu().numpy().tobytes() != b[k].cpu().numpy().tobytes()]


def _ttt(osa, ctx, n, seed=7):
    """n tic_tac_toe positions 0 .. 4 random moves into the game (none terminal)."""
    b = osa.StateBatch(ctx, "tic_tac_toe", n)
    b.synth(seed, 5)
    return b


def test_scratch_grown_reused_trimmed_and_grown_again():
    """osg_legal_mask with on_host=1 stages its [n, 1] u32 mask through the scratch: 256 bytes for 64 states (the
    buffer is made), 16 KiB for 4 096 (it grows), 64 states again (the larger buffer serves), then after trim() once
    more (it is made again).  Each host mask equals the mask the device path (no scratch) gives for the same batch."""
    import open_spiel_amd as osa
    from open_spiel_amd._abi import check, lib
    ctx = osa.Context(0)
    small, big = _ttt(osa, ctx, 64), _ttt(osa, ctx, 4096, seed=8)
    want = {b.n: b.legal_actions_mask_bits().cpu().numpy().view(np.uint32) for b in (small, big)}
    assert len(np.unique(want[64])) > 1   # the positions differ, so a stale or shifted row would show

    def host_mask(b):
        out = np.full((b.n, b.desc.mask_words), 0xFFFFFFFF, np.uint32)
        check(lib().osg_legal_mask(b._h, C.c_void_p(out.ctypes.data), 1))
        return out

    for step, b in enumerate((small, big, small)):
        assert np.array_equal(host_mask(b), want[b.n]), step
    ctx.trim()
    assert np.array_equal(host_mask(small), want[64])


def test_node_pool_and_log_table_grown_reused_trimmed_and_grown_again():
    """64 tic_tac_toe roots searched with 16, 64, 16 simulations, trim(), 16 again: the pool holds 1 + simulations x 9
    slots per root and the log table simulations + 2 entries, so the second search grows both, the third runs in the
    larger ones, and the fourth allocates the pool afresh beside the table that trim() leaves.  The three 16-simulation
    results are equal to each other and to a fresh context's; so is the 64-simulation one."""
    import open_spiel_amd as osa
    ctx = osa.Context(0)
    roots = _ttt(osa, ctx, 64)

    def search(r, sims):
        return r.mcts_search(uct_c=2.0, max_simulations=sims, n_rollouts=1, seed=11)

    s16, s64, again = search(roots, 16), search(roots, 64), search(roots, 16)
    ctx.trim()
    after_trim = search(roots, 16)
    fresh = {}
    for sims in (16, 64):
        other = osa.Context(0)
        fresh[sims] = search(_ttt(osa, other, 64), sims)
    assert int(s64["child_visits"].sum()) == 64 * 63 and int(s16["child_visits"].sum()) == 64 * 15
    assert not _differ(s16, fresh[16]) and not _differ(again, fresh[16]) and not _differ(after_trim, fresh[16])
    assert not _differ(s64, fresh[64])
    assert _differ(s16, s64)   # (and the comparison does tell two searches apart)


def test_work_queue_grown_reused_trimmed_and_grown_again(monkeypatch):
    """The wave-per-root search hands roots out through a queue in the context when there are more roots than resident
    wave slots: n > CUs x 4 SIMDs x 4 wavefronts (tic_tac_toe is compiled for 4 per SIMD, and its two 64-cell sets keep
    the queue form compiled in).  OSG_MCTS_SCHEDULE=queue, read at every launch, takes that path in index order.  Roots:
    one more than the slots (4 097 on the 256 CUs of an MI355X), 8 simulations each.  The queue is made by the first
    search, serves the second after a 64-root search that needs none, and is made again after trim(); the three results
    are equal to each other and to a fresh context's."""
    import torch
    import open_spiel_amd as osa
    monkeypatch.setenv("OSG_MCTS_SCHEDULE", "queue")
    n = torch.cuda.get_device_properties(0).multi_processor_count * 4 * 4 + 1

    def search(r):
        return r.mcts_search(uct_c=2.0, max_simulations=8, n_rollouts=1, seed=13, layout=2)

    ctx = osa.Context(0)
    roots, few = _ttt(osa, ctx, n), _ttt(osa, ctx, 64)
    first = search(roots)
    search(few)
    second = search(roots)
    ctx.trim()
    third = search(roots)
    fresh = search(_ttt(osa, osa.Context(0), n))
    assert int(first["child_visits"].sum()) == n * 7
    assert not _differ(first, fresh) and not _differ(second, fresh) and not _differ(third, fresh)
