"""Every action id at every position, one ply deep, against the oracle (tests/one_ply_fanout.py has the tables).

The other device tests replay trajectories: the refusal branch of the kernels is taken only by ids far outside the action
range, and only compared between two forms of the same kernel.  Here each of a game's positions (every ply of a few
playouts; for connect_four also a full-board draw and a win on the last cell, where columns fill up) is gathered 256
times and stepped with every byte there is — an occupied cell, a full column, a card that is gone, a fold with nothing to
call, a third raise, a move on a finished game, the ids of a folded hex record's meta bits, ids past the mask — and
with the 32-bit ids that would alias a legal action through a byte, a half word or the sign.  Illegal rows must come back
bit-unchanged with bit 6 set and the unchanged state's mask and status, and be counted exactly; legal rows must be the
oracle's child: status byte (poker's terminal code 7 included), successor mask, status(), observation and information
state tensors.  Every comparison is equality; tests/test_one_ply_fanout_cpu.py shows the tables equal to the reference
build's and the comparators sensitive."""
import ctypes as C
import re

import numpy as np
import pytest

import one_ply_fanout as F
from test_gpu_vector_env import OracleEnvironment

pytestmark = pytest.mark.gpu

CHUNK = 1 << 14     # legal rows whose tensors are compared at a time
_TABLES = {}


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


def table(oracle, game):
    """The oracle's table of a game, built once and shared by the tests (read-only)."""
    if game not in _TABLES:
        _TABLES[game] = F.build_fanout(oracle, game)
    return _TABLES[game]


def device_positions(ctx, tab):
    """The K positions as a device batch (histories replayed through apply_actions), checked against the table."""
    import torch
    import open_spiel_amd as osa
    base = osa.StateBatch(ctx, tab["game"], tab["K"])
    assert base.desc.mask_words == tab["W"]
    for t in range(tab["hist"].shape[1]):
        col = tab["hist"][:, t]
        if (col >= 0).any():
            base.apply_actions(torch.from_numpy(col.copy()))
    cur, term, rets = base.status()
    assert np.array_equal(cur.cpu().numpy(), tab["cur"]) and np.array_equal(term.cpu().numpy(), tab["term"])
    assert np.array_equal(rets.cpu().numpy(), tab["rets"])
    assert np.array_equal(base.legal_actions_mask_bits().cpu().numpy().view(np.uint32), tab["mask"])
    return base


def check_children(tab, batch, rows, child, what):
    """Rows `rows` of `batch` are the children `child` of the table: status(), legal mask and tensors."""
    import torch
    for lo in range(0, len(rows), CHUNK):
        r, c = rows[lo:lo + CHUNK], child[lo:lo + CHUNK]
        g = batch.gather(torch.from_numpy(r))
        cur, term, rets = g.status()
        got = dict(cur=cur.cpu().numpy(), term=term.cpu().numpy(), rets=rets.cpu().numpy(),
                   mask=g.legal_actions_mask_bits().cpu().numpy().view(np.uint32))
        assert F.compare_children(tab, c, got) == [], what
        want = torch.from_numpy(tab["child_obs"][c]).cuda().to(torch.float32)
        assert torch.equal(g.observation_tensor(0), want), f"{what}: observation_tensor(0) of the legal rows"
        if tab["info_size"]:
            want = torch.from_numpy(tab["child_info"][c]).cuda()
            assert torch.equal(g.information_state_tensor(0), want), f"{what}: information_state_tensor(0) of the legal rows"
        del g, want


def run_step(ctx, tab, src, src_words, a8, pos, act, in_place, what, mask=None, status=None, want_mask=True):
    """One osg_step launch of the fan-out batch and all its checks; returns (records, status bytes)."""
    import open_spiel_amd as osa
    n = len(pos)
    cmb = src.desc.compact_mask_bytes
    if in_place:
        dst = src.clone()
        m, s = dst.step(a8, mask=mask, status=status, want_mask=want_mask)
    else:
        dst = osa.StateBatch(ctx, tab["game"], n)
        m, s = src.step(a8, dst=dst, mask=mask, status=status, want_mask=want_mask)
        assert (src.raw_words() == src_words).all(), f"{what}: the source batch of an out-of-place step"
    words = dst.raw_words()
    got = dict(status=s.cpu().numpy(), mask=None if m is None else m.cpu().numpy().reshape(n, cmb),
               unchanged=(words == src_words).all(axis=0))
    assert (m is None) == (not want_mask)
    assert F.compare_step(tab, pos, act, got, cmb) == [], what
    e = F.expected_step(tab, pos, act)
    rows = np.nonzero(e["legal"])[0]
    check_children(tab, dst, rows, e["child"][rows], what)
    return words, got["status"]


@pytest.mark.parametrize("game", F.GAMES)
def test_step_every_action_byte(oracle, ctx, game):
    """osg_step, out of place and in place, at 256 K, 256 K + 1 and 256 K + 2 rows (the four- / two-, one- and two-state
    kernels), with the side arrays one byte into a larger allocation (the one-state kernels on an even batch; the guard
    bytes around them survive), and for hex boards of up to 128 cells without the mask row."""
    import torch
    tab = table(oracle, game)
    base = device_positions(ctx, tab)
    cmb = base.desc.compact_mask_bytes
    first = None
    for extra in (0, 1, 2):
        pos, act = F.step_rows(tab, extra)
        n = len(pos)
        src = base.gather(torch.from_numpy(pos))
        src_words = src.raw_words()
        assert (src_words == base.raw_words()[:, pos]).all()
        a8 = torch.from_numpy(act).cuda()
        for in_place in (False, True):
            out = run_step(ctx, tab, src, src_words, a8, pos, act, in_place, f"{game}: {n} rows, in_place={in_place}")
            if extra == 0 and not in_place:
                first = out
        if extra:
            continue
        # the same launch with the action, mask and status arrays at odd addresses
        abuf = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        mbuf = torch.full((n * cmb + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        sbuf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        abuf[1:n + 1] = a8
        m_view, s_view = mbuf[1:1 + n * cmb].view(n, cmb), sbuf[1:n + 1]
        assert abuf[1:n + 1].data_ptr() & 1 and m_view.data_ptr() & 1 and s_view.data_ptr() & 1
        words, st = run_step(ctx, tab, src, src_words, abuf[1:n + 1], pos, act, False, f"{game}: {n} rows, odd side arrays",
                             mask=m_view, status=s_view)
        assert (words == first[0]).all() and (st == first[1]).all()
        assert int(mbuf[0]) == 0xA5 and bool((mbuf[1 + n * cmb:] == 0xA5).all()), "mask guard bytes"
        assert int(sbuf[0]) == 0xA5 and bool((sbuf[1 + n:] == 0xA5).all()), "status guard bytes"
        assert bool((abuf[1:n + 1] == a8).all()) and int(abuf[0]) == 0xEE and bool((abuf[n + 1:] == 0xEE).all())
        if game.startswith("hex") and tab["A"] <= 129:
            for in_place in (False, True):
                words, st = run_step(ctx, tab, src, src_words, a8, pos, act, in_place,
                                     f"{game}: {n} rows, no mask row, in_place={in_place}", want_mask=False)
                assert (words == first[0]).all() and (st == first[1]).all()


@pytest.mark.parametrize("game", F.ALL_GAMES)
def test_apply_every_action_id(oracle, ctx, game):
    """osg_apply with 32-bit ids: 0 .. 32 * mask_words + 31 at every position, the ids that would alias each legal action
    (256 + a, 65536 + a, a - 256, a | 1 << 31), -2, INT_MAX, INT_MIN, and -1 (leave): the count comes back exact, refused
    and left rows are bit-unchanged, accepted rows are the oracle's children.  The two hex boards above 255 actions
    run here (and in the environment step below) only."""
    import torch
    from open_spiel_amd._abi import check, lib
    tab = table(oracle, game)
    base = device_positions(ctx, tab)
    pos, ids = F.apply_rows(tab)
    src = base.gather(torch.from_numpy(pos))
    before = src.raw_words()
    a = torch.from_numpy(ids).cuda()
    illegal = C.c_int64(-1)
    check(lib().osg_apply(src._h, a.data_ptr(), 0, C.byref(illegal)))
    got = dict(count=illegal.value, unchanged=(src.raw_words() == before).all(axis=0))
    assert F.compare_apply(tab, pos, ids, got) == [], game
    e = F.expected_apply(tab, pos, ids)
    assert e["count"] > 0 and int(e["legal"].sum()) >= len(tab["child_pos"])
    rows = np.nonzero(e["legal"])[0]
    check_children(tab, src, rows, e["child"][rows], f"{game}: osg_apply")
    ctx.synchronize()   # the count was handed out and cleared: nothing is left to report


def compact_is_refused(tab):
    """osg_env_step_compact serves one-byte action ids and doubled returns that fit a signed byte (include/osg_abi.h)."""
    return tab["A"] > 255 or (tab["game"].startswith("leduc") and tab["P"] >= 6)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("game", F.ALL_GAMES)
def test_env_step_every_action_id(oracle, ctx, game, compact):
    """osg_env_step (32-bit ids as for osg_apply) and osg_env_step_compact (bytes 0..254, 0xFF = leave) from running
    episodes, at an even and an odd batch size (two environments per thread / one): refused actions leave the record and
    yield the time step of the unchanged state, and the count reported at the next synchronisation is exact; accepted
    ones yield the oracle child's time step after chance was resolved on the row's counter stream; chance nodes and
    finished games, left alone, are resolved / reported LAST."""
    import torch
    import open_spiel_amd as osa
    from open_spiel_amd._abi import check, lib
    tab = table(oracle, game)
    og = oracle.Game(game)
    base = device_positions(ctx, tab)
    P, W = tab["P"], tab["W"]
    seed, offset, t = 0xFA17, 9000, 3
    if compact and compact_is_refused(tab):
        z = torch.zeros(64 * max(P, W * 4), dtype=torch.uint8, device="cuda")
        probe = base.gather(torch.zeros(8, dtype=torch.int64))
        assert lib().osg_env_step_compact(probe._h, z.data_ptr(), z.data_ptr(), seed, offset, t, z.data_ptr(), z.data_ptr()) != 0
        return

    def sample_events(state, row):
        env = OracleEnvironment(og, seed, offset + row, 1.0, True)
        env.state = state
        env._sample_external_events(t)

    for odd in (False, True):
        pos, ids = F.env_rows(tab, compact, odd)
        n = len(pos)
        assert (n & 1) == int(odd)
        want = F.expected_env(tab, og, pos, ids, sample_events)
        b = base.gather(torch.from_numpy(pos))
        before = b.raw_words()
        msk = torch.empty((n, W), dtype=torch.int32, device="cuda")
        ctx.synchronize()
        if compact:
            a8 = torch.from_numpy(np.where(ids < 0, 255, ids).astype(np.uint8)).cuda()
            flags = torch.from_numpy((F.MID | ((tab["cur"][pos].astype(np.int16) + 4) << 2)).astype(np.uint8)).cuda()
            rew2 = torch.empty((n, P), dtype=torch.int8, device="cuda")
            check(lib().osg_env_step_compact(b._h, a8.data_ptr(), flags.data_ptr(), seed, offset, t, rew2.data_ptr(), msk.data_ptr()))
            torch.cuda.synchronize()
            f = flags.cpu().numpy()
            got = dict(type=f & 3, cur=(f >> 2).astype(np.int8) - 4, reset=(f & 3) == F.LAST)
            r2 = rew2.cpu().numpy()
            assert np.array_equal(r2.astype(np.float64), 2.0 * want["rew"]), f"{game}: doubled rewards"
            got["rew"] = r2.astype(np.float64) * 0.5
        else:
            a = torch.from_numpy(ids).cuda()
            reset = torch.zeros(n, dtype=torch.uint8, device="cuda")
            cur = torch.empty(n, dtype=torch.int8, device="cuda")
            typ = torch.empty(n, dtype=torch.uint8, device="cuda")
            rew = torch.empty((n, P), dtype=torch.float64, device="cuda")
            check(lib().osg_env_step(b._h, a.data_ptr(), reset.data_ptr(), seed, offset, t, cur.data_ptr(), typ.data_ptr(),
                                     rew.data_ptr(), msk.data_ptr()))
            torch.cuda.synchronize()
            got = dict(type=typ.cpu().numpy(), cur=cur.cpu().numpy(), rew=rew.cpu().numpy(), reset=reset.cpu().numpy() != 0)
        got["mask"] = msk.cpu().numpy().view(np.uint32)
        got["unchanged"] = (b.raw_words() == before).all(axis=0)
        got["count"] = 0
        try:
            ctx.synchronize()
        except osa.OsgError as err:
            found = re.search(r"(\d+) illegal", str(err))
            assert found, str(err)
            got["count"] = int(found.group(1))
        assert F.compare_env(pos, ids, want, got) == [], f"{game}: compact={compact}, {n} rows"
        assert want["count"] > 0 and (want["type"] == F.LAST).any() and (want["type"] == F.MID).any()
