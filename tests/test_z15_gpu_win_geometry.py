"""The board rules on the device, on DIRECTED histories (tests/golden/win_geometry_vectors.npz, searched for by
tests/golden/make_win_geometry_vectors.py and recorded from the reference build): every connect_four line placement of
every direction for both colours on five geometries (the stored-result record, the run-time 64-bit geometry, and the
three 128-bit boards: the `K == 4` fast path, the generic loop, the widest board), draws, wins on the board's last cell
and column-wrap near misses; and hex chains whose relabelling flood is 135 to 153 steps deep on the three boards above
128 cells, with 16 x 16 and 11 x 11 as controls.  Random playouts — what every other device check of these rules
replays — leave a fifth to a half of the line placements of the larger boards unseen, practically never fill a board,
and never build a group deeper than a few dozen steps.

Expected values are the oracle's, computed here at run time, and the golden file's; all histories of a set go through
as one batch.  HexT::apply stopped its flood after 128 steps until this file was added: against that library the three
large hex boards failed test_ply_by_ply (the label planes of the observation tensor differ one ply before the last
stone, which is then not seen as a win) and 18 x 18 and 17 x 19 failed test_hex_playouts_from_the_chain_position (games
that run two to four plies past the oracle's); the controls and every connect_four case passed
(profiles/r10a_hex_flood_bound.txt).

C4_EDGE_SETS are the sets of tests/golden/win_geometry_edge_vectors.npz that the device serves: 7 x 8 (exactly 64
bits) with x_in_row = columns, where only whole rows are lines and the line test's largest shift is 63, the last
amount below the word's width, and x_in_row = 1.  The file's other sets (two columns of 31 and of 63 rows, x_in_row =
columns + 1, 7 x 16 with 16 in a row) are boards whose shifts reach the width: the parser refuses them
(tests/test_edge_games_cpu.py), and tests/test_win_geometry_goldens.py holds the oracle to them."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4_SETS = ["c4_6x7", "c4_5x6x3", "c4_8x8", "c4_9x10x5", "c4_7x15"]
C4_EDGE_SETS = ["c4e_7x8x8", "c4e_4x5x1"]
HEX_SETS = ["hex_19", "hex_18", "hex_17x19", "hex_16", "hex_11"]
LINE, DRAW, LAST_CELL, NEAR_MISS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


@pytest.fixture(scope="module")
def vectors():
    out = {}
    for name in ("win_geometry_vectors.npz", "win_geometry_edge_vectors.npz"):
        with np.load(os.path.join(ROOT, "tests", "golden", name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


_RECORDS = {}


def oracle_record(oracle, vectors, name):
    """The oracle's per-ply record of every history of a set, computed once and shared by the tests (never modified):
    game string, histories [n, L] int32 (-1 padded), legal mask [n, L + 1, W] uint32, player to move, terminal flag and
    returns at every ply (a history that has ended keeps its last position), hex: observation_tensor(0) of the plies
    from `obs_from` on (three plies before the shortest history ends: from the winner's first edge stone)."""
    if name in _RECORDS:
        return _RECORDS[name]
    game = bytes(vectors[f"{name}/game"]).decode()
    og = oracle.Game(game)
    hist = vectors[f"{name}/histories"].astype(np.int32)
    n, L = hist.shape
    W = og.mask_words
    mask = np.zeros((n, L + 1, W), np.uint32)
    cur = np.zeros((n, L + 1), np.int8)
    term = np.zeros((n, L + 1), np.uint8)
    rets = np.zeros((n, L + 1, 2), np.float64)
    is_hex = name.startswith("hex")
    obs_from = int((hist >= 0).sum(axis=1).min()) - 3 if is_hex else L + 1
    obs = np.zeros((n, L + 1, og.observation_tensor_size), np.float32) if is_hex else None
    for i in range(n):
        s = og.new_initial_state()
        for t in range(L + 1):
            if t == 0 or hist[i, t - 1] >= 0:
                for a in s.legal_actions():
                    mask[i, t, a >> 5] |= np.uint32(1 << (a & 31))
                cur[i, t], term[i, t], rets[i, t] = s.current_player(), s.is_terminal(), s.returns()
                if is_hex and t >= obs_from:
                    obs[i, t] = s.observation_tensor(0)
            else:
                mask[i, t], cur[i, t], term[i, t], rets[i, t] = mask[i, t - 1], cur[i, t - 1], term[i, t - 1], rets[i, t - 1]
                if is_hex and t >= obs_from:
                    obs[i, t] = obs[i, t - 1] if t > obs_from else s.observation_tensor(0)
            if t < L and hist[i, t] >= 0:
                s.apply_action(int(hist[i, t]))
    rec = dict(game=game, og=og, hist=hist, mask=mask, cur=cur, term=term, rets=rets, obs=obs, obs_from=obs_from)
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    # the golden file's results are the oracle's: end ply and final returns
    plies = (hist >= 0).sum(axis=1)
    end = vectors[f"{name}/end_ply"]
    first_terminal = np.where(term.any(axis=1), term.argmax(axis=1), -1)
    assert np.array_equal(first_terminal, end) and np.array_equal(rets[np.arange(n), plies], vectors[f"{name}/returns"])
    _RECORDS[name] = rec
    return rec


@pytest.mark.parametrize("name", C4_SETS + HEX_SETS + C4_EDGE_SETS)
def test_ply_by_ply(oracle, ctx, vectors, name):
    """apply_actions / status() / legal_actions_mask_bits() against the oracle at EVERY ply of every history; hex also
    observation_tensor(0) from the winner's first edge stone on (its label planes show a short flood one ply before
    the result does)."""
    import torch
    import open_spiel_amd as osa
    rec = oracle_record(oracle, vectors, name)
    n, L = rec["hist"].shape
    batch = osa.StateBatch(ctx, rec["game"], n)
    assert batch.desc.mask_words == rec["og"].mask_words
    for t in range(L + 1):
        bits = batch.legal_actions_mask_bits().cpu().numpy().view(np.uint32)
        cur, term, rets = batch.status()
        np.testing.assert_array_equal(term.cpu().numpy(), rec["term"][:, t], err_msg=f"{name}: terminal at ply {t}")
        np.testing.assert_array_equal(cur.cpu().numpy(), rec["cur"][:, t], err_msg=f"{name}: player at ply {t}")
        np.testing.assert_array_equal(rets.cpu().numpy(), rec["rets"][:, t], err_msg=f"{name}: returns at ply {t}")
        np.testing.assert_array_equal(bits, rec["mask"][:, t], err_msg=f"{name}: legal mask at ply {t}")
        if t >= rec["obs_from"]:
            np.testing.assert_array_equal(batch.observation_tensor(0).cpu().numpy(), rec["obs"][:, t],
                                          err_msg=f"{name}: observation tensor at ply {t}")
        if t < L:
            batch.apply_actions(torch.from_numpy(rec["hist"][:, t].copy()))
    ended = vectors[f"{name}/end_ply"] >= 0
    np.testing.assert_array_equal(batch.is_terminal().cpu().numpy(), ended)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("extra", [0, 1, 2])
@pytest.mark.parametrize("name", C4_SETS + ["hex_11"] + C4_EDGE_SETS)
def test_fused_step(oracle, ctx, vectors, name, extra, in_place):
    """The same histories through step(dst=...) and step() in place.  The set is padded (by repeating histories) to a
    multiple of four plus `extra`: the four-, one- and two-state kernels of the non-standard boards and hex, and
    k_step_c4std2 / k_step_c4std of the default board (even / odd batches), as tests/test_gpu_parity.py explains.
    Status byte, outcome bits, successor mask and the final returns(); the near misses end non-terminal with the
    oracle's mask.  (The boards above 255 actions have no fused step: hex from 16 x 16 up is refused.)"""
    import torch
    import open_spiel_amd as osa
    rec = oracle_record(oracle, vectors, name)
    n0, L = rec["hist"].shape
    n = (n0 + 3) // 4 * 4 + extra
    pick = np.arange(n) % n0
    hist, plies = rec["hist"][pick], (rec["hist"][pick] >= 0).sum(axis=1)
    a, b = osa.StateBatch(ctx, rec["game"], n), osa.StateBatch(ctx, rec["game"], n)
    cmb = a.desc.compact_mask_bytes
    for t in range(L):
        a8 = torch.from_numpy(np.where(hist[:, t] < 0, 255, hist[:, t]).astype(np.uint8)).cuda()
        if in_place:
            mask, status = a.step(a8)
        else:
            mask, status = a.step(a8, dst=b)
            a, b = b, a
        st = status.cpu().numpy()
        term = (st & 0x80) != 0
        np.testing.assert_array_equal(term, rec["term"][pick, t + 1] != 0, err_msg=f"{name}: terminal after ply {t}")
        assert not (st & 0x40).any(), "no action of a recorded history is illegal"
        live = ~term
        np.testing.assert_array_equal((st[live] & 15).astype(np.int64) - 1, rec["cur"][pick, t + 1][live])
        r0 = rec["rets"][pick, t + 1, 0]
        want = np.where(r0 > 0, 0, np.where(r0 < 0, 1, 2))
        np.testing.assert_array_equal(st[term] & 7, want[term], err_msg=f"{name}: outcome bits after ply {t}")
        m = mask.cpu().numpy()
        gold = rec["mask"][pick, t + 1]
        if cmb < 4:
            got = m.view(np.uint8 if cmb == 1 else np.uint16).reshape(n).astype(np.uint32)
            np.testing.assert_array_equal(got, gold[:, 0], err_msg=f"{name}: successor mask after ply {t}")
        else:
            np.testing.assert_array_equal(m.view(np.uint32).reshape(n, -1), gold, err_msg=f"{name}: successor mask after ply {t}")
    np.testing.assert_array_equal(a.returns().cpu().numpy(), rec["rets"][pick, plies])
    np.testing.assert_array_equal(a.returns().cpu().numpy()[:, 0], vectors[f"{name}/returns"][pick, 0])
    miss = vectors[f"{name}/kind"][pick] == NEAR_MISS
    assert not a.is_terminal().cpu().numpy()[miss].any() and a.is_terminal().cpu().numpy()[~miss].all()


def one_ply_alpha_beta(state, mover):
    """minimax.py's _alpha_beta one ply deep with `value_function=lambda s: 0.0` at a root where `mover` maximises, on
    the oracle's children: (value, best_action, nodes)."""
    value, best, alpha, beta, nodes = -float("inf"), -1, -float("inf"), float("inf"), 1
    for action in state.legal_actions():
        child = state.child(action)
        nodes += 1
        child_value = child.returns()[mover] if child.is_terminal() else 0.0
        if child_value > value:
            value, best = child_value, action
        alpha = max(alpha, value)
        if alpha >= beta:
            break
    return value, best, nodes


@pytest.mark.parametrize("name", C4_SETS + C4_EDGE_SETS)
def test_alpha_beta_one_ply_deep_finds_every_line(oracle, ctx, vectors, name):
    """From each line history minus its last move, alpha_beta_search(depth_limit=1, leaf_value=0.0): the value is 1.0
    for the mover, best_action the lowest legal action whose child the oracle calls a win, nodes 1 plus the children
    tried (all of them: nothing cuts off below an infinite beta) — AbRules<C4T...> on all five geometries."""
    import open_spiel_amd as osa
    rec = oracle_record(oracle, vectors, name)
    rows = np.nonzero(vectors[f"{name}/kind"] == LINE)[0]
    hist = rec["hist"][rows].copy()
    plies = (hist >= 0).sum(axis=1)
    last = hist[np.arange(len(rows)), plies - 1]
    hist[np.arange(len(rows)), plies - 1] = -1
    batch = osa.StateBatch(ctx, rec["game"], len(rows))
    for t in range(hist.shape[1]):
        if (hist[:, t] >= 0).any():
            batch.apply_actions(hist[:, t])
    value, best, nodes, status = (x.cpu().numpy() for x in batch.alpha_beta_search(depth_limit=1, leaf_value=0.0, max_nodes=1 << 10))
    want = []
    for i in range(len(rows)):
        s = rec["og"].new_initial_state()
        for a in hist[i, :plies[i] - 1]:
            s.apply_action(int(a))
        mover = (plies[i] - 1) & 1
        assert s.current_player() == mover
        want.append(one_ply_alpha_beta(s, mover))
        wins = [a for a in s.legal_actions() if s.child(a).is_terminal() and s.child(a).returns()[mover] == 1.0]
        assert want[-1][0] == 1.0 and want[-1][1] == wins[0] and int(last[i]) in wins and want[-1][2] == 1 + len(s.legal_actions())
    assert not status.any()
    assert np.array_equal(value, np.array([w[0] for w in want]))
    assert np.array_equal(best, np.array([w[1] for w in want], np.int32))
    assert np.array_equal(nodes, np.array([w[2] for w in want], np.int64))


@pytest.mark.parametrize("name", ["hex_19", "hex_18", "hex_17x19"])
def test_hex_playouts_from_the_chain_position(oracle, ctx, vectors, name):
    """rollout() from the chain positions before the winner's last two stones (some 40 empty cells; about a quarter of
    the playouts put the winner on both end cells, through the deep flood): summed returns AND ply counts equal
    oracle.replay_rollouts on the same counter streams, as in tests/test_gpu_parity.py, and the fill-kernel form
    (no ply counts) gives the same sums."""
    import open_spiel_amd as osa
    rec = oracle_record(oracle, vectors, name)
    hist = rec["hist"].copy()
    n = len(hist)
    plies = (hist >= 0).sum(axis=1)
    for i in range(n):
        hist[i, plies[i] - 3:] = -1
    roots = osa.StateBatch(ctx, rec["game"], n)
    for t in range(hist.shape[1]):
        if (hist[:, t] >= 0).any():
            roots.apply_actions(hist[:, t])
    assert not bool(roots.is_terminal().any())
    seed, offset, n_rollouts = 0xC0FFEE, 1000, 64
    total, steps = roots.rollout(seed, n_rollouts, index_offset=offset, want_steps=True)
    fill = roots.rollout(seed, n_rollouts, index_offset=offset)
    total, steps, fill = total.cpu().numpy(), steps.cpu().numpy(), fill.cpu().numpy()
    for i in range(n):
        want, want_steps = rec["og"].replay_rollouts(hist[i, :plies[i] - 3], seed, offset + i, n_rollouts)
        print(f"{name} root {i}: oracle {want} in {want_steps} plies, device {total[i]} in {steps[i]}, fill kernel {fill[i]}")
        np.testing.assert_allclose(total[i], want, rtol=0, atol=1e-12, err_msg=f"{name} root {i}")
        assert steps[i] == want_steps
    np.testing.assert_array_equal(fill, total)
