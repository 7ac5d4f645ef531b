"""The device against the oracle on every game string of the edge list that the parser serves (tests/edge_games.py:
the parameter space the parser accepts, walked along its limits — where the bitboard layouts change form or run out of
bits; the strings beyond the limits are refused, tests/test_edge_games_cpu.py).  The oracle is
pinned to the genuine reference build on the same strings by tests/test_edge_games_cpu.py.

Batches are 257 and 258 states: one partly filled 256-thread workgroup, an odd and an even count, so both the one-state
and the two-state kernels.  Every comparison is equality.  Per string: every ply of seeded playouts through osg_apply
(legal mask, player, terminal flag, returns; the tensors of every player at every 4th ply and the last), the fused step
(both sizes; the successor record after the last ply through returns() and the tensors), osg_env_step against
rl_environment's arithmetic on the oracle for 1.5 times the game's length, and for the boards small enough the solver
and the unlimited alpha-beta search against a minimax over the oracle."""
import math

import numpy as np
import pytest

import edge_games as eg
from test_gpu_vector_env import FIRST, LAST, MID, OracleEnvironment

pytestmark = pytest.mark.gpu

PLAYABLE = [g for g in eg.SERVED if g not in eg.RULES_ONLY]
SIZES = (257, 258)
SEED = 0xED6E5
TENSOR_STRIDE = 4


def num_actions(game):
    if game.startswith("connect_four"):
        return eg.c4_geometry(game)[1]
    if game.startswith("hex"):
        C, R, swap, _, _ = eg.hex_geometry(game)
        return C * R + swap
    return 3


FUSED = [g for g in PLAYABLE if num_actions(g) <= 255]     # action ids travel as one byte in osg_step


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


_RECORDS = {}


def winning_moves(R, C, K):
    """A connect_four history that ends with the first player's line: K stones in column 0 (the second player stacks
    K - 1 in column 1), or the first K cells of the bottom row (the second player plays on top of each, or, on a
    one-row board, comes in from the far end); None where the first player cannot be walked to a win like this."""
    if K == 1:
        return [0]
    if K <= R and C >= 2:
        return [0, 1] * (K - 1) + [0]
    if K <= C and R >= 2:
        return [c for i in range(K - 1) for c in (i, i)] + [K - 1]
    if K <= C and C >= 2 * K - 1:
        return [c for i in range(K - 1) for c in (i, C - 1 - i)] + [K - 1]
    return None


def directed_playout(og, rec, row, pick):
    """Overwrites playout `row` of a record with the game in which move t is pick(legal actions, t)."""
    s = og.new_initial_state()
    L = rec["actions"].shape[1]
    for t in range(L + 1):
        legal = s.legal_actions()
        rec["mask"][row, t] = 0
        for a in legal:
            rec["mask"][row, t, a >> 5] |= np.uint32(1 << (a & 31))
        rec["cur_player"][row, t], rec["terminal"][row, t], rec["returns"][row, t] = s.current_player(), s.is_terminal(), s.returns()
        if t < L:
            rec["actions"][row, t] = pick(legal, t) if legal else -1
            if legal:
                s.apply_action(pick(legal, t))


def record(oracle, game, n):
    """Seeded oracle playouts of a game, computed once per (game, n) and shared (never modified).  connect_four: random
    play rarely fills a column of a tall board before somebody wins, so the last two playouts are directed ones — always
    the lowest, always the highest legal column: column after column fills to the top, the colours alternating in it —,
    and neither does it ever line up 7, 8 or 15 stones: the third from last is winning_moves(), the first player's line."""
    if (game, n) not in _RECORDS:
        og = oracle.Game(game)
        rec = og.random_playouts(SEED, n)
        if game.startswith("connect_four"):
            directed_playout(og, rec, n - 1, lambda legal, t: min(legal))
            directed_playout(og, rec, n - 2, lambda legal, t: max(legal))
            R, C, K, _ = eg.c4_geometry(game)
            win = winning_moves(R, C, K)
            assert (win is not None) == eg.c4_win_possible(R, C, K), game
            if win:
                directed_playout(og, rec, n - 3, lambda legal, t: win[t])
                assert rec["returns"][n - 3, -1, 0] == 1.0 and (rec["actions"][n - 3] >= 0).sum() == len(win)
        for v in rec.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        rec["og"] = og
        _RECORDS[(game, n)] = rec
    return _RECORDS[(game, n)]


def assert_playouts_reach_the_edges(game, rec):
    """At least one terminal state; connect_four: a position with a full column (but where x_in_row = 1 ends the game
    with its first stone), and a win wherever a line exists and can be reached (record(): a directed playout makes
    one where random play does not)."""
    L = rec["actions"].shape[1]
    assert rec["terminal"][:, L].any() or game in eg.RULES_ONLY, game
    if game.startswith("connect_four"):
        R, C, K, _ = eg.c4_geometry(game)
        acts = rec["actions"]
        fullest = max(int((acts == c).sum(axis=1).max()) for c in range(C))
        assert fullest == (R if K > 1 else 1), f"{game}: no full column"
        if eg.c4_win_possible(R, C, K):
            assert (rec["returns"][:, L, 0] != 0).any(), f"{game}: no win"
        if not eg.c4_win_possible(R, C, K):
            assert not rec["returns"].any(), f"{game}: a line that cannot exist"


def compare_tensors(game, batch, states, og, what):
    for p in range(og.num_players):
        want = np.stack([s.observation_tensor(p) for s in states])
        np.testing.assert_array_equal(batch.observation_tensor(p).cpu().numpy(), want, err_msg=f"{game}: observation p{p} {what}")
        if og.information_state_tensor_size:
            want = np.stack([s.information_state_tensor(p) for s in states])
            np.testing.assert_array_equal(batch.information_state_tensor(p).cpu().numpy(), want, err_msg=f"{game}: information state p{p} {what}")


def final_states(rec):
    og = rec["og"]
    out = []
    for row in rec["actions"]:
        s = og.new_initial_state()
        for a in row:
            if a >= 0:
                s.apply_action(int(a))
        out.append(s)
    return out


@pytest.mark.parametrize("game", eg.SERVED)
def test_ply_by_ply(oracle, ctx, game):
    """The body of tests/test_gpu_parity.py::test_step_by_step_parity at 257 states, with the tensors of every player at
    every 4th ply and at the last (the single-row and single-column hex boards too: these are the rules)."""
    import torch
    import open_spiel_amd as osa
    n = SIZES[0]
    rec = record(oracle, game, n)
    og = rec["og"]
    L, W = og.max_plies, og.mask_words
    batch = osa.StateBatch(ctx, game, n)
    assert (batch.desc.mask_words, batch.desc.num_distinct_actions, batch.desc.max_game_length) == (W, og.num_distinct_actions, og.max_game_length)
    assert (batch.desc.obs_size, batch.desc.info_size) == (og.observation_tensor_size, og.information_state_tensor_size)
    states = [og.new_initial_state() for _ in range(n)]
    for t in range(L + 1):
        bits = batch.legal_actions_mask_bits().cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(bits, rec["mask"][:, t], err_msg=f"{game}: legal mask at ply {t}")
        cur, term, rets = batch.status()
        np.testing.assert_array_equal(cur.cpu().numpy(), rec["cur_player"][:, t], err_msg=f"{game}: player at ply {t}")
        np.testing.assert_array_equal(term.cpu().numpy(), rec["terminal"][:, t], err_msg=f"{game}: terminal at ply {t}")
        np.testing.assert_array_equal(rets.cpu().numpy(), rec["returns"][:, t], err_msg=f"{game}: returns at ply {t}")
        if t % TENSOR_STRIDE == 0 or t == L:
            compare_tensors(game, batch, states, og, f"at ply {t}")
        if t == L:
            break
        acts = rec["actions"][:, t]
        batch.apply_actions(torch.from_numpy(acts.astype(np.int32)))
        for s, a in zip(states, acts):
            if a >= 0:
                s.apply_action(int(a))
    assert_playouts_reach_the_edges(game, rec)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game", FUSED)
def test_fused_step(oracle, ctx, game, n):
    """The body of tests/test_gpu_parity.py::test_fused_step_parity (games of at most 255 actions), then the successor
    record after the last ply: returns() and the tensors of every player."""
    import torch
    import open_spiel_amd as osa
    rec = record(oracle, game, n)
    og = rec["og"]
    assert og.num_distinct_actions <= 255
    L = og.max_plies
    a, b = osa.StateBatch(ctx, game, n), osa.StateBatch(ctx, game, n)
    cmb = a.desc.compact_mask_bytes
    for t in range(L):
        acts = rec["actions"][:, t]
        a8 = torch.from_numpy(np.where(acts < 0, 255, acts).astype(np.uint8)).cuda()
        mask, status = a.step(a8, dst=b)
        st = status.cpu().numpy()
        term = (st & 0x80) != 0
        np.testing.assert_array_equal(term, rec["terminal"][:, t + 1] != 0, err_msg=f"{game}: terminal after ply {t}")
        assert not (st & 0x40).any(), "no action of an oracle playout is illegal"
        live = ~term
        np.testing.assert_array_equal((st[live] & 15).astype(np.int64) - 1, rec["cur_player"][:, t + 1][live])
        if a.desc.game_kind <= 2:  # board games: outcome in bits 0-2
            r0 = rec["returns"][:, t + 1, 0]
            want = np.where(r0 > 0, 0, np.where(r0 < 0, 1, 2))
            np.testing.assert_array_equal(st[term] & 7, want[term], err_msg=f"{game}: outcome bits after ply {t}")
        m = mask.cpu().numpy()
        gold = rec["mask"][:, t + 1]
        if cmb < 4:
            got = m.view(np.uint8 if cmb == 1 else np.uint16).reshape(n).astype(np.uint32)
            np.testing.assert_array_equal(got, gold[:, 0], err_msg=f"{game}: successor mask after ply {t}")
        else:
            np.testing.assert_array_equal(m.view(np.uint32).reshape(n, -1), gold, err_msg=f"{game}: successor mask after ply {t}")
        a, b = b, a
    np.testing.assert_array_equal(a.returns().cpu().numpy(), rec["returns"][:, L])
    compare_tensors(game, a, final_states(rec), og, "after the last fused step")
    assert_playouts_reach_the_edges(game, rec)


class StridedOracleEnvironment(OracleEnvironment):
    """OracleEnvironment whose time step carries the tensors only where `want_tensors` is set (they are compared at
    every 4th step; forming them for every player at every step is most of the oracle's time on the large boards).  On
    the steps in between only the player to move is asked for its legal actions: the others have none (spiel.h:366-372;
    the steps with tensors ask the oracle for every player)."""
    want_tensors = True

    def _time_step(self, first):
        if self.want_tensors:
            return super()._time_step(first)
        s, P = self.state, self.og.num_players
        step_type = FIRST if first else (LAST if s.is_terminal() else MID)
        self.should_reset = step_type == LAST
        rewards = None if first else s.returns() if s.is_terminal() else [0.0] * P
        discounts = None if first else [0.0 if step_type == LAST else self.discount] * P
        cp = s.current_player()
        return dict(info_state=None, legal_actions=[s.legal_actions(p) if p == cp else [] for p in range(P)], current_player=cp,
                    rewards=rewards, discounts=discounts, step_type=step_type)


@pytest.mark.parametrize("game", PLAYABLE)
def test_env_step(oracle, ctx, game):
    """osg_env_step (BatchedEnvironment) at 257 environments for 1.5 times the game's maximum length against
    rl_environment.Environment's arithmetic over the oracle (OracleEnvironment of tests/test_gpu_vector_env.py), fed
    with the same chance draws: step type, player, legal actions of every player, rewards and discounts at every step,
    the tensors of every player at every 4th step and the last."""
    import torch
    import open_spiel_amd as osa
    n, seed, offset, discount = SIZES[0], 0xE27, 7000, 0.99
    og = oracle.Game(game)
    P, A = og.num_players, og.num_distinct_actions
    steps = math.ceil(1.5 * og.max_plies)
    env = osa.BatchedEnvironment(ctx, game, n, discount=discount, seed=seed, index_offset=offset)
    use_obs = og.information_state_tensor_size == 0
    refs = [StridedOracleEnvironment(og, seed, offset + i, discount, use_obs) for i in range(n)]
    agent = np.random.default_rng(5)
    finished = 0
    # connect_four: environment 0 always plays its lowest legal column (columns fill), environment 1 the winning moves
    c4 = eg.c4_geometry(game)[:3] if game.startswith("connect_four") else None
    win = winning_moves(*c4) if c4 else None
    ply = [0] * n                      # stones on the board of each environment
    full_column = won = False
    for t in range(steps + 1):
        tensors = t % TENSOR_STRIDE == 0 or t == steps
        for r in refs:
            r.want_tensors = tensors
        if t == 0:
            ts, want = env.reset(), [r.reset(0) for r in refs]
        else:
            ts, want = env.step(torch.from_numpy(actions)), [r.step(actions[i], t) for i, r in enumerate(refs)]
        what = f"{game} step {t}"
        np.testing.assert_array_equal(ts.step_type.cpu().numpy(), [w["step_type"] for w in want], err_msg=what)
        np.testing.assert_array_equal(ts.observations["current_player"].cpu().numpy(), [w["current_player"] for w in want], err_msg=what)
        rewards = np.array([w["rewards"] or [0.0] * P for w in want])
        discounts = np.array([w["discounts"] or [0.0] * P for w in want])
        np.testing.assert_array_equal(ts.rewards.cpu().numpy(), rewards, err_msg=what)
        np.testing.assert_array_equal(ts.discounts.cpu().numpy(), discounts, err_msg=what)
        for p in range(P):
            legal = np.zeros((n, A), bool)
            for i, w in enumerate(want):
                legal[i, w["legal_actions"][p]] = True
            np.testing.assert_array_equal(ts.observations["legal_actions"][p].cpu().numpy(), legal, err_msg=f"{what} legal actions p{p}")
            if tensors:
                np.testing.assert_array_equal(ts.observations["info_state"][p].cpu().numpy(),
                                              np.stack([w["info_state"][p] for w in want]), err_msg=f"{what} tensor p{p}")
        actions, picks = np.zeros(n, np.int32), agent.random(n)
        for i, w in enumerate(want):
            legal = w["legal_actions"][w["current_player"]] if w["current_player"] >= 0 else []
            actions[i] = legal[int(picks[i] * len(legal))] if legal else 0  # ignored: the environment restarts
            finished += w["step_type"] == LAST
            if c4:
                ply[i] = 0 if w["step_type"] == FIRST else ply[i] + 1
                if i == 0 and legal:
                    actions[i] = min(legal)
                    full_column |= ply[i] >= c4[0] and (0 not in legal or c4[1] == 1)
                if i == 0 and w["step_type"] == LAST and c4[1] == 1 and c4[2] > 1:
                    full_column = True
                if i == 1 and legal and win and ply[i] < len(win):
                    actions[i] = win[ply[i]]
                won |= w["step_type"] == LAST and w["rewards"][0] != 0
    assert finished > 0, "the run must cover episode ends and restarts"
    if c4:
        assert won == eg.c4_win_possible(*c4), f"{game}: no win"
        assert full_column == (c4[2] > 1 or c4[0] == 1), f"{game}: no full column"


def minimax_value(s, memo):
    """The value of a position for player 0 by plain minimax over the oracle's states, one visit per position (keyed by
    the board string and the player to move)."""
    if s.is_terminal():
        return s.returns()[0]
    key = (str(s), s.current_player())
    if key not in memo:
        children = [minimax_value(s.child(a), memo) for a in s.legal_actions()]
        memo[key] = max(children) if s.current_player() == 0 else min(children)
    return memo[key]


@pytest.mark.parametrize("game", eg.SOLVABLE)
def test_solver_and_search_at_the_initial_position(oracle, ctx, game):
    """osg_solve_create's value of position 0 and osg_alpha_beta_search (unlimited depth) at the initial position equal
    the oracle's minimax value: the one- and two-row connect_four boards, x_in_row = 1, hex up to 3 x 3."""
    import open_spiel_amd as osa
    og = oracle.Game(game)
    memo = {}
    want = minimax_value(og.new_initial_state(), memo)
    positions = len(memo)
    assert positions <= 1 << 16
    solved = osa.SolvedGame(ctx, game)
    assert float(solved.values[0]) == want, game
    assert solved.n >= positions          # (terminal positions are listed too)
    value, best, nodes, status = osa.StateBatch(ctx, game, 1).alpha_beta_search()
    assert int(status[0]) == 0 and float(value[0]) == want, game
    child = og.new_initial_state().child(int(best[0]))
    assert minimax_value(child, memo) == want, f"{game}: best_action does not keep the value"


def test_solver_and_search_refuse_what_they_document(ctx):
    """include/osg_abi.h: osg_solve_create serves hex without swap, with the standard string, up to 64 cells;
    osg_alpha_beta_search hex up to 128 cells; playouts no single-row board.  Each refuses with OSG_ERR_UNSUPPORTED."""
    import open_spiel_amd as osa
    for game in (eg.hx(4, 8, swap=True), eg.hx(3, 11, explicit=True), eg.hx(5, 13)):
        assert game in eg.EDGE_GAMES
        with pytest.raises(osa.OsgError, match="osg error -2"):
            osa.SolvedGame(ctx, game)
    with pytest.raises(osa.OsgError, match="osg error -2"):
        osa.StateBatch(ctx, eg.hx(3, 43), 1).alpha_beta_search()
    for game in eg.RULES_ONLY:
        with pytest.raises(osa.OsgError, match="osg error -2"):
            osa.StateBatch(ctx, game, 4).rollout(1, 1)
