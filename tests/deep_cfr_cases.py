"""NumPy restatement of the Deep CFR arithmetic (open_spiel_amd/csrc/osg_deep_cfr.h; the reference's
open_spiel/python/pytorch/deep_cfr.py) and the case builders of its tests: test_deep_cfr_goldens.py, test_deep_cfr_host.py
(CPU) and test_z31_gpu_deep_cfr.py.  tests/golden/make_deep_cfr_vectors.py scripts the reference's random draws with the
functions below, so what the goldens pin is the reference's own arithmetic over the device's streams.

The dtype rules are the reference's, taken literally: `max(0., x)` keeps a float32 scalar when x > 0 and gives a Python
float otherwise; np.sum over a list of float32 scalars adds in float32, over a mixed list in float64."""
import os
import subprocess

import numpy as np

from ismcts_cases import Rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deep_cfr_vectors.npz")
M64 = (1 << 64) - 1
BATCH_SIZES = (1, 63, 64, 65, 257)


# ---- section 1 of the rules -----------------------------------------------------------------------------------------------
def strategy(adv, legal, num_actions):
    """(_sample_action_from_advantage, deep_cfr.py:484-512) -> (p [num_actions] float64, branch 0 | 1 | 2)."""
    adv = np.asarray(adv, np.float32)
    p = np.zeros(num_actions, np.float64)
    pos = [bool(adv[a] > 0) for a in legal]
    if not any(pos):
        best = legal[0]
        for a in legal[1:]:
            if adv[a] > adv[best]:
                best = a
        p[best] = 1.0
        return p, 2
    if all(pos):
        s = np.float32(0)
        for a in legal:
            s = np.float32(s + adv[a])
        with np.errstate(all="ignore"):
            for a in legal:
                p[a] = np.float64(np.float32(adv[a] / s))
        return p, 0
    s = np.float64(0)
    for a in legal:
        s = s + (np.float64(adv[a]) if adv[a] > 0 else 0.0)
    for a in legal:
        p[a] = (np.float64(adv[a]) if adv[a] > 0 else 0.0) / s
    return p, 1


def choice(p, u):
    """RandomState.choice(len(p), p=p) for the uniform u: the index."""
    cdf = []
    acc = 0.0
    for x in p:
        acc = acc + float(x)
        cdf.append(acc)
    last = cdf[-1]
    pick = sum(1 for c in cdf if c / last <= u)
    return min(pick, len(cdf) - 1)


def opponent_draw(p, u):
    """(:466-468) probs = p / p.sum() over all action ids, then choice."""
    s = 0.0
    for x in p:
        s = s + float(x)
    return choice([float(x) / s for x in p], u)


def advantage_row(p, payoff, legal, num_actions):
    """(:442-458) -> (row float32 [num_actions], cfv)."""
    cfv = 0.0
    for k, a in enumerate(legal):
        cfv = cfv + float(p[a]) * float(payoff[k])
    row = np.zeros(num_actions, np.float32)
    for k, a in enumerate(legal):
        row[a] = np.float32(float(payoff[k]) - cfv)
    return row, cfv


def reservoir_index(seed, stream, n):
    """np.random.randint(0, n + 1) of the append with add index n, from the buffer's stream."""
    return (Rng(seed, n, stream).next() * (n + 1)) >> 64


def reservoir_slot(seed, stream, n, capacity):
    if n < capacity:
        return n
    idx = reservoir_index(seed, stream, n)
    return idx if idx < capacity else -1


def sample_key(seed, stream, slot):
    return Rng(seed, slot, stream).next()


class Reservoir:
    """ReservoirBuffer (deep_cfr.py:121-213) over (infostate index, iteration, values) rows."""

    def __init__(self, capacity, num_actions, seed, stream):
        self.capacity, self.seed, self.stream = int(capacity), int(seed), int(stream)
        self.info = np.full(self.capacity, -1, np.int32)
        self.iteration = np.zeros(self.capacity, np.int32)
        self.values = np.zeros((self.capacity, num_actions), np.float32)
        self.add_calls = 0
        self.writes = []          # the slot (-1: dropped) of every append

    def __len__(self):
        return min(self.add_calls, self.capacity)

    def append(self, info, iteration, values):
        slot = reservoir_slot(self.seed, self.stream, self.add_calls, self.capacity)
        if slot >= 0:
            self.info[slot], self.iteration[slot], self.values[slot] = info, iteration, values
        self.writes.append(slot)
        self.add_calls += 1

    def append_many(self, info, iteration, values):
        for i, v in zip(info, values):
            self.append(i, iteration, v)

    def sample(self, seed, stream, m):
        assert m <= len(self)
        keys = [(sample_key(seed, stream, k), k) for k in range(len(self))]
        return np.array([k for _, k in sorted(keys)[:m]], np.int64)

    def state(self):
        n = len(self)
        return self.add_calls, self.info[:n].copy(), self.iteration[:n].copy(), self.values[:n].copy()


# ---- the tree and a trajectory ----------------------------------------------------------------------------------------------
class Tree:
    """A game tree depth first (a parent before its children, children in action order): parent, kind (0 chance,
    1 decision, 2 terminal), action and prob of the edge from the parent, actor, info (infostate index), returns."""

    def __init__(self, parent, kind, action, prob, actor, info, returns, legal):
        self.parent, self.kind, self.action, self.prob = parent, kind, action, prob
        self.actor, self.info, self.returns = actor, info, returns
        self.legal = [[int(a) for a in row if a >= 0] for row in legal]     # per infostate, ascending ids
        self.num_actions = legal.shape[1]
        self.children = [[] for _ in parent]
        for h, q in enumerate(parent):
            if q >= 0:
                self.children[q].append(h)
        self.num_players = returns.shape[1]
        self.num_infostates = len(self.legal)


def strategy_table(tree, advantages):
    """[I, A] float64 and the branch of every infostate."""
    rows = [strategy(advantages[i], tree.legal[i], tree.num_actions) for i in range(tree.num_infostates)]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def traverse(tree, table, player, seed, g):
    """_traverse_game_tree(root, player) (:413-481) of trajectory g -> (advantage rows [(info, row)] in append order,
    strategy rows [(info, row)], draws)."""
    rng = Rng(seed, g, 0)
    adv_rows, strat_rows = [], []

    def walk(h):
        if tree.kind[h] == 2:
            return float(tree.returns[h, player])
        kids = tree.children[h]
        if tree.kind[h] == 0:
            return walk(kids[choice([tree.prob[c] for c in kids], rng.unit())])
        i = int(tree.info[h])
        legal = tree.legal[i]
        if tree.actor[h] == player:
            payoff = [walk(c) for c in kids]
            row, cfv = advantage_row(table[i], payoff, legal, tree.num_actions)
            adv_rows.append((i, row))
            return cfv
        strat_rows.append((i, table[i].astype(np.float32)))
        a = opponent_draw(table[i], rng.unit())
        return walk(kids[legal.index(a)])

    walk(0)
    return adv_rows, strat_rows, rng.draws


def row_bounds(tree, player):
    """(advantage rows, strategy rows) one trajectory can append at most."""
    H = len(tree.parent)
    adv, strat = [0] * H, [0] * H
    for h in range(H - 1, -1, -1):
        kids = tree.children[h]
        own = tree.kind[h] == 1 and tree.actor[h] == player
        opp = tree.kind[h] == 1 and not own
        a, s = [adv[c] for c in kids], [strat[c] for c in kids]
        adv[h] = 1 + sum(a) if own else max(a, default=0)
        strat[h] = sum(s) if own else (1 if opp else 0) + max(s, default=0)
    return adv[0], strat[0]


def run_step(tree, advantages, player, iteration, seed, first, count, adv_buf, strat_buf):
    """One osg_deep_cfr_traverse call -> per-trajectory (advantage rows, strategy rows, draws)."""
    table, _ = strategy_table(tree, advantages)
    out = []
    for j in range(count):
        a, s, d = traverse(tree, table, player, seed, first + j)
        out.append((a, s, d))
        # the reference interleaves the two buffers' appends; their streams are separate, so the order between them is free
        for i, row in a:
            if adv_buf is not None:
                adv_buf.append(i, iteration, row)
        for i, row in s:
            if strat_buf is not None:
                strat_buf.append(i, iteration, row)
    return out


def flatten(rows, num_actions):
    """[(info, row)] per trajectory -> offsets [T + 1], info [R], values [R, A]."""
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    info = np.array([i for r in rows for i, _ in r], np.int32)
    vals = np.array([v for r in rows for _, v in r], np.float32).reshape(-1, num_actions)
    return off, info, vals


# ---- goldens ------------------------------------------------------------------------------------------------------------------
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN, allow_pickle=False))
    return _golden


def golden_runs():
    g = golden()
    return [str(x) for x in g["runs"]]


def _strings(g, prefix):
    blob, lens = g[prefix + "_bytes"].tobytes(), g[prefix + "_len"]
    out, at = [], 0
    for n in lens:
        out.append(blob[at:at + n].decode())
        at += n
    return out


def golden_tree(game):
    g, t = golden(), "tree/" + game + "/"
    return Tree(g[t + "parent"], g[t + "kind"], g[t + "action"], g[t + "prob"], g[t + "actor"], g[t + "info"], g[t + "returns"],
                g[t + "legal"])


def golden_game(game):
    """keys (infostate strings, the goldens' infostate order), tensors [I, E], player [I]."""
    g, t = golden(), "tree/" + game + "/"
    return _strings(g, t + "keys"), g[t + "tensors"], g[t + "player"]


def golden_run(r):
    """The run's parameters and its steps: dicts with iteration, player, first, advantages [I, A] f32, adv / strat
    (offsets, info, values) per trajectory, draws [T], and every buffer's state after the step."""
    g, p = golden(), f"r{r}/"
    meta = {k: int(g[p + k]) for k in ("capacity", "traversals", "iterations", "seed", "res_seed", "players")}
    meta["game"] = golden_runs()[r].split("|")[0]
    steps = []
    for s in range(int(g[p + "steps"])):
        q = f"{p}s{s}/"
        step = dict(iteration=int(g[q + "iteration"]), player=int(g[q + "player"]), first=int(g[q + "first"]),
                    advantages=g[q + "advantages"], draws=g[q + "draws"],
                    adv=(g[q + "adv_off"], g[q + "adv_info"], g[q + "adv_vals"]),
                    strat=(g[q + "strat_off"], g[q + "strat_info"], g[q + "strat_vals"]), buffers={})
        for b in range(meta["players"] + 1):
            if q + f"b{b}/add_calls" in g:
                step["buffers"][b] = (int(g[q + f"b{b}/add_calls"]), g[q + f"b{b}/info"], g[q + f"b{b}/iteration"], g[q + f"b{b}/values"])
        steps.append(step)
    return meta, steps


def new_buffers(meta, num_actions):
    """Advantage buffer of player p on stream p, the strategy buffer on stream P."""
    return [Reservoir(meta["capacity"], num_actions, meta["res_seed"], b) for b in range(meta["players"] + 1)]


# ---- comparators (each is shown to reject a perturbed record in test_deep_cfr_goldens.py) ------------------------------------
def same_rows(got, want):
    """(offsets, info, values): the same rows in the same order, values bit for bit."""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].shape == want[2].shape
            and np.array_equal(np.ascontiguousarray(got[2], np.float32).view(np.uint32), np.ascontiguousarray(want[2], np.float32).view(np.uint32)))


def same_buffer(got, want):
    """(add_calls, info, iteration, values) of the filled slots."""
    return (got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3].shape == want[3].shape
            and np.array_equal(np.ascontiguousarray(got[3], np.float32).view(np.uint32), np.ascontiguousarray(want[3], np.float32).view(np.uint32)))


# ---- synthetic advantage tables -----------------------------------------------------------------------------------------------
def synthetic_advantages(tree, seed):
    """An [I, A] float32 table that forces every branch of the strategy rule: all legal outputs positive, one clipped,
    all <= 0 with a tie at the maximum, an exact 0, in rotation over the infostates, on top of seeded noise."""
    rng = np.random.default_rng(seed)
    I, A = tree.num_infostates, tree.num_actions
    adv = rng.standard_normal((I, A)).astype(np.float32)
    for i in range(I):
        legal, kind = tree.legal[i], i % 5
        if kind == 0:
            adv[i, legal] = np.abs(adv[i, legal]) + np.float32(0.01)
        elif kind == 1:
            adv[i, legal] = np.abs(adv[i, legal]) + np.float32(0.01)
            adv[i, legal[-1]] = -adv[i, legal[-1]]
        elif kind == 2:
            adv[i, legal] = np.float32(-0.25)            # a tie at the maximum: the first legal id
            adv[i, legal[0]] = np.float32(-0.5) if len(legal) > 2 else np.float32(-0.25)
        elif kind == 3:
            adv[i, legal[0]] = np.float32(0.0)            # an exact 0 among positive outputs: the fp64 branch
            adv[i, legal[1:]] = np.abs(adv[i, legal[1:]]) + np.float32(0.01)
    return adv


# ---- the stand-alone host program -------------------------------------------------------------------------------------------
def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "deep_cfr_host_test.cpp"), "-o", path])
    return path


def host_step(exe, workdir, tree, advantages, player, iteration, seed, first, count, buffers, name="step"):
    """The host program's run of one traverse call.  buffers: (adv, strat) Reservoir objects or None, whose state goes
    in and comes back.  -> (adv rows, strat rows, draws, bounds, branches, [buffer states])."""
    H, I, A = len(tree.parent), tree.num_infostates, tree.num_actions
    legal = np.full((I, A), -1, np.int32)
    for i, row in enumerate(tree.legal):
        legal[i, :len(row)] = row
    blob = [np.array([H, I, A, tree.num_players, player, iteration, count, len(buffers)], np.int32).tobytes(),
            np.array([seed, first], np.uint64).tobytes(),
            np.ascontiguousarray(tree.parent, np.int32).tobytes(), np.ascontiguousarray(tree.kind, np.int32).tobytes(),
            np.ascontiguousarray(tree.actor, np.int32).tobytes(), np.ascontiguousarray(tree.info, np.int32).tobytes(),
            np.ascontiguousarray(tree.prob, np.float64).tobytes(), np.ascontiguousarray(tree.returns, np.float64).tobytes(),
            legal.tobytes(), np.ascontiguousarray(advantages, np.float32).tobytes()]
    for b in buffers:
        blob += [np.array([b.capacity, b.add_calls], np.int64).tobytes(), np.array([b.seed, b.stream], np.uint64).tobytes(),
                 b.info.tobytes(), b.iteration.tobytes(), b.values.tobytes()]
    src, dst = os.path.join(workdir, name + ".in"), os.path.join(workdir, name + ".out")
    with open(src, "wb") as f:
        f.write(b"".join(blob))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(dst, "rb").read()
    at = [0]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, at[0]).copy()
        at[0] += a.nbytes
        return a

    bounds = take(np.int64, 2)
    branches = take(np.int32, I)
    draws = take(np.int32, count)
    rows = []
    for _ in range(2):
        off = take(np.int64, count + 1)
        rows.append((off, take(np.int32, int(off[-1])), take(np.float32, int(off[-1]) * A).reshape(-1, A)))
    states = []
    for b in buffers:
        add_calls = int(take(np.int64, 1)[0])
        n = min(add_calls, b.capacity)
        info, it, vals = take(np.int32, b.capacity), take(np.int32, b.capacity), take(np.float32, b.capacity * A).reshape(-1, A)
        b.add_calls, b.info, b.iteration, b.values = add_calls, info, it, vals
        states.append((add_calls, info[:n].copy(), it[:n].copy(), vals[:n].copy()))
    assert at[0] == len(raw)
    return rows[0], rows[1], draws, bounds, branches, states
