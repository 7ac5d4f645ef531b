"""One-ply fan-out tables: for a small set of positions per game, what EVERY action id does there.

The parity tests replay trajectories, so the only action a kernel ever sees at a position is the legal one the playout
drew.  `build_fanout` records, for each position, the oracle's legal set and the record of every legal child; the
functions below turn that into the expected output of a launch that steps the same position with every action id there
is (legal, occupied, out of range, aliasing, on a finished game, at a chance node), and compare a device's output with
it.  Everything is equality: there is no tolerance here.

This is a helper module (no tests in it): tests/test_one_ply_fanout_cpu.py checks the tables themselves (oracle against
the reference build, coverage of the edges, and that the comparators notice a perturbed answer),
tests/test_z16_gpu_one_ply_fanout.py runs the device against them.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GAMES = [
    "tic_tac_toe",
    "connect_four",
    "connect_four(rows=5,columns=6,x_in_row=3)",
    "connect_four(rows=8,columns=8)",
    "connect_four(rows=9,columns=10,x_in_row=5)",
    "connect_four(rows=7,columns=15,egocentric_obs_tensor=True)",
    "hex(board_size=9)",
    "hex(board_size=5)",
    "hex",
    "hex(num_cols=3,num_rows=4)",
    "hex(board_size=4,swap=True)",
    "hex(board_size=13)",
    "hex(board_size=14,swap=True)",
    "hex(board_size=15)",
    "kuhn_poker",
    "kuhn_poker(players=3)",
    "kuhn_poker(players=7)",
    "kuhn_poker(players=10)",
    "leduc_poker",
    "leduc_poker(players=3)",
    "leduc_poker(action_mapping=True)",
    "leduc_poker(suit_isomorphism=True)",
    "leduc_poker(players=5)",
    "leduc_poker(players=10)",
    "leduc_poker(players=7,action_mapping=True,starting_player=5)",
]
# above 255 actions: no one-byte action ids, so osg_apply and osg_env_step only; one playout each
GAMES_32BIT_ONLY = ["hex(board_size=19)", "hex(num_cols=17,num_rows=19,swap=True)"]
ALL_GAMES = GAMES + GAMES_32BIT_ONLY

# The playout seed of every game.  Fixed: tests/test_one_ply_fanout_cpu.py asserts the coverage conditions on the tables
# these seeds give; a seed that misses one is replaced here, the condition is never loosened.
DEFAULT_SEED = 0x1F0A
SEEDS = {g: DEFAULT_SEED for g in ALL_GAMES}

# connect_four geometries: the directed histories of tests/golden/win_geometry_vectors.npz (a full-board draw and a win
# on the board's last cell) are where columns fill up; random playouts end long before
GEOMETRY_SETS = {
    "connect_four": "c4_6x7",
    "connect_four(rows=5,columns=6,x_in_row=3)": "c4_5x6x3",
    "connect_four(rows=8,columns=8)": "c4_8x8",
    "connect_four(rows=9,columns=10,x_in_row=5)": "c4_9x10x5",
    "connect_four(rows=7,columns=15,egocentric_obs_tensor=True)": "c4_7x15",
}
KIND_DRAW, KIND_LAST_CELL = 1, 2
FOLDED_HEX = ["hex(board_size=9)", "hex", "hex(board_size=19)"]   # records whose planes carry the meta bits

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
FIRST, MID, LAST = 0, 1, 2


def num_playouts(og, game):
    return 1 if game in GAMES_32BIT_ONLY else min(max(256 // (og.max_plies + 1), 1), 16)


def _geometry_histories(game):
    name = GEOMETRY_SETS.get(game)
    if name is None:
        return []
    with np.load(os.path.join(ROOT, "tests", "golden", "win_geometry_vectors.npz")) as z:
        hist, kind = z[f"{name}/histories"], z[f"{name}/kind"]
    out = []
    for k in (KIND_DRAW, KIND_LAST_CELL):
        row = hist[np.nonzero(kind == k)[0][0]]
        out.append((k, [int(a) for a in row if a >= 0]))
    return out


def _bits(actions, W):
    """Action ids -> W little-endian u32 mask words."""
    b = np.zeros(32 * W, np.uint8)
    b[np.asarray(actions, np.int64)] = 1
    return np.packbits(b, bitorder="little").view(np.uint32)


def build_fanout(binding, game, seed=None):
    """The table of `game` from any binding with the oracle's call set (oracle_py, reference_py).

    Positions k = 0..K-1: every ply of the seeded playouts (the initial state, every chance node, the terminal state and
    the row after it, where the playout record is empty: the terminal position once more), then every ply of the two
    directed connect_four histories.  Per position: history, legal mask words, player, terminal flag, returns.  Per legal
    action of a position (chance outcomes at a chance node) one child record, ordered by (position, action): legal
    mask, player, terminal, returns, observation_tensor(0), information_state_tensor(0) where the game has one."""
    og = binding.Game(game)
    seed = SEEDS[game] if seed is None else seed
    W, P = og.mask_words, og.num_players
    rec = og.random_playouts(seed, num_playouts(og, game))
    histories = [(0, [int(a) for a in row if a >= 0]) for row in rec["actions"]] + _geometry_histories(game)
    board = not og.has_chance
    obs_dtype = np.uint8 if board else np.float32   # board tensors are 0 / 1 (asserted below): a quarter of the memory
    info_size = og.information_state_tensor_size

    pos = dict(hist=[], mask=[], cur=[], term=[], rets=[], source=[], moves=[])
    child = dict(pos=[], act=[], mask=[], cur=[], term=[], rets=[], obs=[], info=[])

    def record(s, hist, source, moves):
        k = len(pos["hist"])
        legal = s.legal_actions()
        pos["hist"].append(list(hist)); pos["mask"].append(_bits(legal, W)); pos["cur"].append(s.current_player())
        pos["term"].append(s.is_terminal()); pos["rets"].append(s.returns()); pos["source"].append(source)
        pos["moves"].append(moves)
        for a in legal:
            c = s.child(a)
            child["pos"].append(k); child["act"].append(a); child["mask"].append(_bits(c.legal_actions(), W))
            child["cur"].append(c.current_player()); child["term"].append(c.is_terminal()); child["rets"].append(c.returns())
            obs = c.observation_tensor(0)
            stored = obs.astype(obs_dtype)
            assert np.array_equal(stored.astype(np.float32), obs)
            child["obs"].append(stored)
            if info_size:
                child["info"].append(c.information_state_tensor(0))

    for source, hist in histories:
        s = og.new_initial_state()
        moves = 0
        for t in range(len(hist) + 1):
            record(s, hist[:t], source, moves)
            if t < len(hist):
                moves += s.current_player() >= 0
                s.apply_action(hist[t])
        if source == 0:
            record(s, hist, source, moves)      # the row after the playout's last action

    K, Nc = len(pos["hist"]), len(child["pos"])
    L = max(len(h) for h in pos["hist"])
    hist = np.full((K, max(L, 1)), -1, np.int32)
    for k, h in enumerate(pos["hist"]):
        hist[k, :len(h)] = h
    tab = dict(
        game=game, W=W, P=P, A=og.num_distinct_actions, C=og.max_chance_outcomes, poker=og.has_chance,
        obs_size=og.observation_tensor_size, info_size=info_size, K=K,
        hist=hist, hist_len=np.array([len(h) for h in pos["hist"]], np.int32),
        mask=np.array(pos["mask"], np.uint32).reshape(K, W), cur=np.array(pos["cur"], np.int8),
        term=np.array(pos["term"], np.uint8), rets=np.array(pos["rets"], np.float64).reshape(K, P),
        source=np.array(pos["source"], np.int8), moves=np.array(pos["moves"], np.int32),
        child_pos=np.array(child["pos"], np.int32), child_act=np.array(child["act"], np.int32),
        child_mask=np.array(child["mask"], np.uint32).reshape(Nc, W), child_cur=np.array(child["cur"], np.int8),
        child_term=np.array(child["term"], np.uint8), child_rets=np.array(child["rets"], np.float64).reshape(Nc, P),
        child_obs=np.array(child["obs"], obs_dtype).reshape(Nc, og.observation_tensor_size),
        child_info=np.array(child["info"], np.float32).reshape(Nc, info_size) if info_size else None,
    )
    # child_index[k, a] = row of the child of position k by action a, -1 where a is not legal there
    index = np.full((K, 32 * W), -1, np.int32)
    index[tab["child_pos"], tab["child_act"]] = np.arange(Nc, dtype=np.int32)
    tab["child_index"] = index
    assert not tab["mask"][tab["term"] != 0].any(), "a terminal state has no legal action"
    for v in tab.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return tab


def tables_equal(a, b):
    """Names of the entries in which two tables differ (empty: identical)."""
    bad = [k for k in a if k not in b] + [k for k in b if k not in a]
    for k, v in a.items():
        if k in b:
            w = b[k]
            same = (np.array_equal(v, w) and v.dtype == w.dtype) if isinstance(v, np.ndarray) else v == w if v is not None else w is None
            if not same:
                bad.append(k)
    return bad


def copy_table(tab):
    """A writable deep copy (for the perturbation checks; the shared tables stay read-only)."""
    return {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in tab.items()}


# ---- the status byte and the compact mask of osg_step (include/osg_abi.h) -------------------------------------------
def status_bytes(term, cur, rets0, poker):
    """bit7 terminal; terminal: bits 0-2 the outcome (board games 0 / 1 / 2 from player 0's return, poker 7);
    otherwise bits 0-3 the current player + 1 (0 = chance)."""
    term = np.asarray(term) != 0
    outcome = np.full(term.shape, 7, np.uint8) if poker else np.where(rets0 > 0, 0, np.where(rets0 < 0, 1, 2)).astype(np.uint8)
    live = ((np.asarray(cur).astype(np.int16) + 1) & 15).astype(np.uint8)
    return np.where(term, np.uint8(0x80) | outcome, live).astype(np.uint8)


def position_status(tab):
    return status_bytes(tab["term"], tab["cur"], tab["rets"][:, 0], tab["poker"])


def child_status(tab):
    return status_bytes(tab["child_term"], tab["child_cur"], tab["child_rets"][:, 0], tab["poker"])


def compact_mask(mask_words, cmb):
    """[n, W] u32 mask words as the [n, compact_mask_bytes] bytes osg_step writes (1, 2 or 4 * W bytes per state)."""
    m = np.ascontiguousarray(mask_words, np.uint32)
    n, W = m.shape
    if cmb == 4 * W:
        return m.view(np.uint8).reshape(n, cmb)
    assert cmb in (1, 2) and not (m[:, 0] >> np.uint32(8 * cmb)).any() and not m[:, 1:].any(), "the mask fits its compact form"
    return m[:, :1].copy().view(np.uint8).reshape(n, 4)[:, :cmb].copy()


def _legal(tab, pos, ids):
    """ids (int64) -> (legal [n] bool, child row [n], -1 where not legal)."""
    ids = np.asarray(ids, np.int64)
    in_range = (ids >= 0) & (ids < 32 * tab["W"])
    child = np.where(in_range, tab["child_index"][pos, np.where(in_range, ids, 0)], -1)
    return child >= 0, child


# ---- osg_step -----------------------------------------------------------------------------------------------------
def step_rows(tab, extra=0):
    """Row 256 k + j: position k, action byte j; then `extra` copies of position 0 with action 255."""
    K = tab["K"]
    pos = np.concatenate([np.repeat(np.arange(K, dtype=np.int64), 256), np.zeros(extra, np.int64)])
    act = np.concatenate([np.tile(np.arange(256, dtype=np.int64), K), np.full(extra, 255, np.int64)]).astype(np.uint8)
    return pos, act


def expected_step(tab, pos, act, fold=None):
    """What osg_step answers: legal [n], child [n], status [n] u8, mask words [n, W], unchanged [n] (the record equals
    the source row: every row but the legal ones).  `fold` maps the ids before the legality test: a model of a
    device that aliases ids, for the perturbation checks."""
    ids = act.astype(np.int64)
    skip = ids == 255
    if fold is not None:
        ids = fold(ids)
    legal, child = _legal(tab, pos, ids)
    legal &= ~skip
    child = np.where(legal, child, -1)
    stay = position_status(tab)[pos] | np.where(skip, 0, 0x40).astype(np.uint8)
    status = np.where(legal, child_status(tab)[child], stay).astype(np.uint8)
    mask = np.where(legal[:, None], tab["child_mask"][child], tab["mask"][pos])
    return dict(legal=legal, child=child, status=status, mask=mask, unchanged=~legal)


def ideal_step(tab, pos, act, cmb, fold=None):
    """The output of a device that implements `tab`: what compare_step takes as `got`."""
    e = expected_step(tab, pos, act, fold)
    return dict(status=e["status"], mask=compact_mask(e["mask"], cmb), unchanged=e["unchanged"])


def _report(out, what, bad, pos, act, want=None, got=None):
    rows = np.nonzero(bad)[0]
    if len(rows):
        r = rows[0]
        detail = "" if want is None else f": want {np.asarray(want)[r]!r}, got {np.asarray(got)[r]!r}"
        out.append(f"{what}: {len(rows)} row(s), first row {r} = position {pos[r]}, action {act[r]}{detail}")


def compare_step(tab, pos, act, got, cmb):
    """Mismatches (strings; empty = equal) between a device's osg_step output and the table.  got: status [n] u8,
    mask [n, cmb] u8 (None: not written), unchanged [n] bool (record bit-equal to the source row)."""
    e = expected_step(tab, pos, act)
    out = []
    _report(out, "status byte", got["status"] != e["status"], pos, act, e["status"], got["status"])
    if got["mask"] is not None:
        want = compact_mask(e["mask"], cmb)
        _report(out, "successor mask", (got["mask"] != want).any(axis=1), pos, act, want, got["mask"])
    _report(out, "record changed by a refused or skipped action", e["unchanged"] & ~got["unchanged"], pos, act)
    _report(out, "record not changed by a legal action", ~e["unchanged"] & got["unchanged"], pos, act)
    return out


# ---- osg_apply / osg_env_step: 32-bit ids -----------------------------------------------------------------------------
def id_rows(tab, positions, top):
    """(pos, ids) for the 32-bit entry points: per position the ids 0..top-1 and -1 (leave), -2, INT_MAX, INT_MIN, and per
    legal action a of the position the four ids that would alias it through a byte, a half word or the sign."""
    pos, ids = [], []
    for k in positions:
        legal = tab["child_act"][tab["child_pos"] == k].astype(np.int64)
        row = np.concatenate([np.arange(top, dtype=np.int64), [-1, -2, INT_MAX, INT_MIN],
                              256 + legal, 65536 + legal, legal - 256, legal + INT_MIN])
        pos.append(np.full(len(row), k, np.int64)); ids.append(row)
    if not pos:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    return np.concatenate(pos), np.concatenate(ids).astype(np.int32)


def apply_rows(tab):
    return id_rows(tab, range(tab["K"]), 32 * tab["W"] + 32)


def expected_apply(tab, pos, ids, fold=None):
    """legal [n], child [n], unchanged [n], count = the rows that are neither -1 nor legal."""
    ids = ids.astype(np.int64)
    skip = ids == -1
    legal, child = _legal(tab, pos, ids if fold is None else fold(ids))
    legal &= ~skip
    return dict(legal=legal, child=np.where(legal, child, -1), unchanged=~legal, count=int((~legal & ~skip).sum()))


def ideal_apply(tab, pos, ids, fold=None):
    e = expected_apply(tab, pos, ids, fold)
    return dict(unchanged=e["unchanged"], count=e["count"])


def compare_apply(tab, pos, ids, got):
    """got: unchanged [n] bool, count (what the call reported)."""
    e = expected_apply(tab, pos, ids)
    out = []
    if got["count"] != e["count"]:
        out.append(f"illegal count: want {e['count']}, got {got['count']}")
    _report(out, "record changed by a refused or skipped action", e["unchanged"] & ~got["unchanged"], pos, ids)
    _report(out, "record not changed by a legal action", ~e["unchanged"] & got["unchanged"], pos, ids)
    return out


def compare_children(tab, child, got):
    """The records of legal rows (gathered into a compact batch, row i = child[i]) against the table: got has cur [n],
    term [n], rets [n, P], mask [n, W] u32."""
    out = []
    for key, want in (("cur", tab["child_cur"][child]), ("term", tab["child_term"][child]),
                      ("rets", tab["child_rets"][child]), ("mask", tab["child_mask"][child])):
        g = np.asarray(got[key])
        bad = (g != want) if g.ndim == 1 else (g != want).any(axis=1)
        _report(out, f"child {key}", bad, tab["child_pos"][child], tab["child_act"][child], want, g)
    return out


# ---- osg_env_step / osg_env_step_compact ----------------------------------------------------------------------------
def env_rows(tab, compact, odd):
    """Player nodes get every id (0..254 for the byte form), chance nodes and terminal positions only -1; an odd batch
    ends with one more row of position 0 left as it is."""
    live = (tab["term"] == 0) & (tab["cur"] >= 0)
    if compact:
        ks = np.nonzero(live)[0]
        pos = np.repeat(ks.astype(np.int64), 256)
        ids = np.tile(np.concatenate([np.arange(255), [-1]]).astype(np.int32), len(ks))
    else:
        pos, ids = id_rows(tab, np.nonzero(live)[0], 32 * tab["W"] + 32)
    rest = np.nonzero(~live)[0].astype(np.int64)
    pos = np.concatenate([pos, rest])
    ids = np.concatenate([ids, np.full(len(rest), -1, np.int32)])
    if (len(pos) & 1) != int(odd):
        pos, ids = np.concatenate([pos, [0]]), np.concatenate([ids, np.array([-1], np.int32)])
    return pos, ids


def state_at(og, history):
    s = og.new_initial_state()
    for a in history:
        s.apply_action(int(a))
    return s


def expected_env(tab, og, pos, ids, sample_events):
    """The time step of every row after one environment step from `should_reset = 0`: the action (if legal) applied,
    then chance resolved by sample_events(state, row) in place — step type, player, rewards, mask words, the reset
    flag, whether the record must be bit-unchanged, and the number of refused actions."""
    n, P, W = len(pos), tab["P"], tab["W"]
    e = expected_apply(tab, pos, ids)
    out = dict(type=np.zeros(n, np.uint8), cur=np.zeros(n, np.int8), rew=np.zeros((n, P), np.float64),
               mask=np.zeros((n, W), np.uint32), count=e["count"],
               unchanged=e["unchanged"] & (tab["cur"][pos] != -1))
    if not tab["poker"]:    # no chance: the tables have every time step
        c, lg = e["child"], e["legal"]
        term = np.where(lg, tab["child_term"][c], tab["term"][pos]) != 0
        out["type"][:] = np.where(term, LAST, MID)
        out["cur"][:] = np.where(lg, tab["child_cur"][c], tab["cur"][pos])
        out["rew"][:] = np.where(term[:, None], np.where(lg[:, None], tab["child_rets"][c], tab["rets"][pos]), 0.0)
        out["mask"][:] = np.where(lg[:, None], tab["child_mask"][c], tab["mask"][pos])
        return out
    roots = {}
    for r in range(n):
        k = int(pos[r])
        if k not in roots:
            roots[k] = state_at(og, tab["hist"][k, :tab["hist_len"][k]])
        s = roots[k].clone()
        if e["legal"][r]:
            s.apply_action(int(ids[r]))
        sample_events(s, r)
        term = s.is_terminal()
        out["type"][r] = LAST if term else MID
        out["cur"][r] = s.current_player()
        out["rew"][r] = s.returns() if term else 0.0
        out["mask"][r] = _bits(s.legal_actions(), W)
    return out


def compare_env(pos, ids, want, got):
    """got: type, cur, rew, mask, reset [n], unchanged [n] bool, count."""
    out = []
    if got["count"] != want["count"]:
        out.append(f"illegal count: want {want['count']}, got {got['count']}")
    for key in ("type", "cur", "rew", "mask"):
        g = np.asarray(got[key])
        bad = (g != want[key]) if g.ndim == 1 else (g != want[key]).any(axis=1)
        _report(out, f"time step {key}", bad, pos, ids, want[key], g)
    _report(out, "should_reset", np.asarray(got["reset"]) != (want["type"] == LAST), pos, ids)
    _report(out, "record changed by a refused or skipped action", want["unchanged"] & ~got["unchanged"], pos, ids)
    return out
