"""Shared by tests/test_efr_goldens.py, tests/test_efr_native.py and tests/test_z27_gpu_efr.py: the goldens of
extensive-form regret minimization (tests/golden/efr_vectors.npz, made by tests/golden/make_efr_vectors.py from the
reference's own efr.py), a restatement in Python floats of open_spiel_amd/csrc/osg_efr.h — the same items, every sum in
the header's order — and the input file of tests/native/efr_host_test.cpp.

TOLERANCE: the largest absolute deviation of the host program (the header's functions, whole iterations) from the
reference's run, over every checkpoint of every golden run (R, current, cumulative and average policy) and every
regret-matching unit case, was measured at 6.39e-14 (the cumulative policy of kuhn_poker(players=3) `tips` / `bhv` after
10 iterations; the unit cases alone: 5.77e-15); the bound is 100 x that figure, rounded up: 6.4e-12.  The sources of the
deviation: the reference sums through BLAS / LAPACK (np.inner, matmul, gelsd) and the header in its own fixed orders with
a one-sided Jacobi SVD, and an iteration feeds the difference of a few ulps into the next."""
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "efr_vectors.npz")
MEASURED = 6.4e-14
TOLERANCE = 100 * MEASURED
TYPES = ["blind action", "informed action", "blind cf", "informed cf", "bps", "cfps", "csps", "tips", "bhv"]
EXTERNAL_ONLY = (0, 2, 4)
MAX_KEYS = 16
ZERO_COL = 0xF
EPS = 2.220446049250313e-16

_cache = {}


def load():
    if "v" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["v"] = {k: z[k] for k in z.files}
    return _cache["v"]


def runs(v=None):
    """[(run number, game string, deviation set name)]"""
    v = load() if v is None else v
    return [(r, *str(name).split("|")) for r, name in enumerate(v["runs"])]


def run_ids():
    return [f"{g}-{d}".replace(" ", "_") for _, g, d in runs()]


def keys_of(v, r):
    raw, lens = bytes(v[f"r{r}/keys_bytes"]), v[f"r{r}/keys_len"]
    at = np.concatenate([[0], np.cumsum(lens)])
    return [raw[at[i]:at[i + 1]].decode() for i in range(len(lens))]


def by_legal(v, r, table):
    """A golden [I, 3] table by action id as [I, A] by legal-action index (the solver's layout)."""
    legal, nact = v[f"r{r}/legal"], v[f"r{r}/nact"]
    A = int(nact.max())
    out = np.zeros((len(nact), A))
    for i in range(len(nact)):
        for a in range(nact[i]):
            out[i, a] = table[i, legal[i, a]]
    return out


class Layout:
    """The game tree of a golden run numbered level by level (a parent's children contiguous), as the solver flattens it;
    the information states keep the golden's numbering."""

    def __init__(self, v, r, game):
        t = {k: v[f"tree/{game}/{k}"] for k in ("parent", "kind", "action", "prob", "info", "returns")}
        H = len(t["parent"])
        kids = [[] for _ in range(H)]
        for h in range(1, H):
            kids[t["parent"][h]].append(h)
        order, level_off, frontier = [], [0], [0]
        while frontier:
            order += frontier
            level_off.append(len(order))
            frontier = [c for h in frontier for c in kids[h]]
        new = np.zeros(H, np.int64)
        new[order] = np.arange(H)
        self.H, self.P, self.D = H, t["returns"].shape[1], len(level_off) - 1
        self.level_off = np.array(level_off, np.int32)
        self.nact = v[f"r{r}/nact"].astype(np.int32)
        self.I, self.A = len(self.nact), int(self.nact.max())
        self.legal = v[f"r{r}/legal"][:, :self.A].astype(np.int32)
        self.info_player = v[f"r{r}/player"].astype(np.int32)
        self.parent = np.full(H, -1, np.int32)
        self.first_child = np.zeros(H, np.int32)
        self.kind, self.nchild, self.aidx = np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros(H, np.int32)
        self.actor, self.info = np.full(H, -1, np.int32), np.full(H, -1, np.int32)
        self.edge_prob, self.term_ret = np.zeros(H), np.zeros((H, self.P))
        for old in range(H):
            h = new[old]
            self.kind[h], self.nchild[h] = t["kind"][old], len(kids[old])
            self.first_child[h] = new[kids[old][0]] if kids[old] else 0
            self.edge_prob[h], self.term_ret[h] = t["prob"][old], t["returns"][old]
            if t["kind"][old] == 1:
                self.info[h] = t["info"][old]
                self.actor[h] = self.info_player[t["info"][old]]
            for k, c in enumerate(kids[old]):
                self.parent[new[c]], self.aidx[new[c]] = h, k
        members = [[] for _ in range(self.I)]
        for old in range(H):   # depth first: the reference's visiting order
            if t["kind"][old] == 1:
                members[t["info"][old]].append(int(new[old]))
        self.mem_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
        self.mem = np.array([h for m in members for h in m], np.int32)
        self.M = len(self.mem)
        self.mem_index = np.full(H, -1, np.int32)
        self.mem_index[self.mem] = np.arange(self.M)
        self.path_off, self.path = [0], []
        for h in self.mem:
            rev, x = [], int(h)
            while self.parent[x] >= 0:
                par = int(self.parent[x])
                chance = self.kind[par] == 0
                slot = self.P if chance else int(self.actor[par])
                idx = x if chance else int(self.info[par]) * self.A + int(self.aidx[x])
                rev.append((slot << 24) | ((1 if chance else 0) << 23) | idx)
                x = par
            self.path += rev[::-1]
            self.path_off.append(len(self.path))


def layout(v, r, game):
    key = ("layout", game)
    if key not in _cache:
        _cache[key] = Layout(v, r, game)
    return _cache[key]


# ---- osg_efr.h restated ------------------------------------------------------------------------------------------------
def build_tables(lay, type_):
    """efr_build_tables: dict of per-deviation lists and per-infostate structures."""
    I, A = lay.I, lay.A
    own_info, own_aidx, mown = [None] * I, [None] * I, [None] * lay.M
    for i in range(I):
        for m in range(lay.mem_off[i], lay.mem_off[i + 1]):
            infos, aidxs, members, x = [], [], [], int(lay.mem[m])
            while lay.parent[x] >= 0:
                par = int(lay.parent[x])
                if lay.kind[par] == 1 and lay.actor[par] == lay.info_player[i]:
                    infos.insert(0, int(lay.info[par]))
                    aidxs.insert(0, int(lay.aidx[x]))
                    members.insert(0, int(lay.mem_index[par]))
                x = par
            if m == lay.mem_off[i]:
                own_info[i], own_aidx[i] = infos, aidxs
            assert infos == own_info[i] and aidxs == own_aidx[i]
            mown[m] = members
    L = max(1, max(len(o) for o in own_info))
    T = dict(type=type_, L=L, own_info=own_info, mown=mown, dev_off=[0], info=[], target=[], source=[], none=[], weights=[],
             memory=[], slot=[], mask=[], cols=[], keys=[])
    depth = max(len(o) for o in own_info) + 1
    T["depths"] = [[i for i in range(I) if len(own_info[i]) == k] for k in range(depth)]
    for i in range(I):
        n, ln = int(lay.nact[i]), len(own_info[i])
        prior = [[int(a) for a in lay.legal[e, :lay.nact[e]]] for e in own_info[i]]
        history = [prior[j][own_aidx[i][j]] for j in range(ln)]
        devs = []
        ones, zeros = [1] * ln, [0] * ln
        prefix = lambda k: [1] * k + [0] * (ln - k)

        def external(none, w, mem):
            for t in range(n):
                devs.append((t, -1, none, list(w), list(mem)))

        def internal(none, w, mem):
            for t in range(n):
                for s in range(n):
                    if s != t:
                        devs.append((t, s, none, list(w), list(mem)))

        def sequences(add):
            add(True, zeros, history)
            if ln > 0:
                add(False, ones, history)
            for k in range(ln):
                add(False, prefix(k), history)

        def modified(add):
            for k in range(ln):
                for alt in prior[k]:
                    mem = list(history)
                    mem[k] = alt
                    add(False, prefix(k), mem)

        if type_ == 0:
            external(False, ones, history)
        elif type_ == 1:
            internal(False, ones, history)
        elif type_ == 2:
            external(True, zeros, zeros)
        elif type_ == 3:
            internal(True, zeros, zeros)
        elif type_ == 4:
            sequences(external)
        elif type_ == 5:
            sequences(internal)
        elif type_ == 6:
            modified(external)
            external(False, ones, history)
            internal(True, zeros, zeros)
            external(True, zeros, zeros)
        elif type_ == 7:
            modified(internal)
            internal(True, zeros, zeros)
        else:
            if ln == 0:
                internal(True, zeros, history)
            for k in range(ln):
                pick = [0] * (k + 1)
                while True:
                    mem = [prior[j][pick[j]] for j in range(k + 1)] + [0] * (ln - k - 1)
                    internal(False, prefix(k), mem)
                    j = k
                    while j >= 0:
                        pick[j] += 1
                        if pick[j] < len(prior[j]):
                            break
                        pick[j] = 0
                        j -= 1
                    if j < 0:
                        break
        keys = []
        for t, s, none, w, mem in devs:
            key = t | ((s + 1) << 4)
            if key not in keys:
                keys.append(key)
            mask, cols = 0, 0
            for j in range(ln):
                if none or not w[j]:
                    continue
                pos = prior[j].index(mem[j])
                col = prior[j].index(pos) if pos in prior[j] else ZERO_COL
                mask |= 1 << j
                cols |= col << (4 * j)
            T["info"].append(i); T["target"].append(t); T["source"].append(s); T["none"].append(int(none))
            T["weights"].append([-1] * L if none else w + [-1] * (L - ln)); T["memory"].append(mem + [-1] * (L - ln))
            T["slot"].append(keys.index(key)); T["mask"].append(mask); T["cols"].append(cols)
        T["keys"].append(keys)
        T["dev_off"].append(len(T["info"]))
    return T


def min_norm_solve(g, n):
    """efr_min_norm_solve: g[c][r] column-major (n + 1 rows); returns (x, rank)."""
    v = [[1.0 if r == c else 0.0 for r in range(n)] for c in range(n)]
    for _ in range(40):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                alpha = beta = gamma = 0.0
                for r in range(n + 1):
                    alpha = alpha + g[p][r] * g[p][r]
                    beta = beta + g[q][r] * g[q][r]
                    gamma = gamma + g[p][r] * g[q][r]
                if gamma == 0.0 or abs(gamma) <= EPS * math.sqrt(alpha * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (2.0 * gamma)
                tn = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / math.sqrt(1.0 + tn * tn)
                sn = cs * tn
                for mat, rows in ((g, n + 1), (v, n)):
                    for r in range(rows):
                        a, b = mat[p][r], mat[q][r]
                        mat[p][r] = cs * a - sn * b
                        mat[q][r] = sn * a + cs * b
        if not rotated:
            break
    norm2 = []
    for c in range(n):
        sq = 0.0
        for r in range(n + 1):
            sq = sq + g[c][r] * g[c][r]
        norm2.append(sq)
    cut = EPS * math.sqrt(max(norm2))
    x, rank = [0.0] * n, 0
    for c in range(n):
        if not math.sqrt(norm2[c]) > cut:
            continue
        rank += 1
        w = g[c][n] / norm2[c]
        for r in range(n):
            x[r] = x[r] + v[c][r] * w
    return x, rank


def regret_match(n, keys, y, external_only):
    """efr_regret_match: (row, rank or -1)."""
    z = 0.0
    for k in range(len(keys)):
        z = z + y[k]
    if not z > 0.0:
        return [1.0 / n] * n, -1
    if external_only:
        out = [0.0] * n
        for k, key in enumerate(keys):
            out[key & 0xF] = out[key & 0xF] + y[k] / z
        return out, -1
    g = [[(-1.0 if r == c else 0.0) for r in range(n)] + [1.0] for c in range(n)]
    for k, key in enumerate(keys):
        w = y[k] / z
        target, source = key & 0xF, ((key >> 4) & 0xF) - 1
        if source < 0:
            for c in range(n):
                g[c][target] = g[c][target] + w
        else:
            for c in range(n):
                if c != source:
                    g[c][c] = g[c][c] + w
            g[source][target] = g[source][target] + w
    x, rank = min_norm_solve(g, n)
    total = 0.0
    for a in range(n):
        x[a] = 0.0 if x[a] < 0.0 else (1.0 if x[a] > 1.0 else x[a])
        total = total + x[a]
    with np.errstate(all="ignore"):
        return [float(np.float64(x[a]) / np.float64(total)) for a in range(n)], rank


def memreach(mask, cols, rows, pol):
    r = 1.0
    for j in range(8):
        if (mask >> j) & 1:
            c = (cols >> (4 * j)) & 0xF
            r = r * (0.0 if c == ZERO_COL else pol[rows[j]][c])
    return r


class State:
    def __init__(self, lay, T):
        self.pol = [[1.0 / lay.nact[i]] * int(lay.nact[i]) + [0.0] * (lay.A - int(lay.nact[i])) for i in range(lay.I)]
        self.cum = [[0.0] * lay.A for _ in range(lay.I)]
        self.R = [0.0] * len(T["info"])
        self.y = [[0.0] * MAX_KEYS for _ in range(lay.I)]
        self.mpol = [[0.0] * lay.A for _ in range(lay.M)]

    def average(self, lay):
        out = np.zeros((lay.I, lay.A))
        for i in range(lay.I):
            n, total = int(lay.nact[i]), 0.0
            for a in range(n):
                total = total + self.cum[i][a]
            for a in range(n):
                out[i, a] = 1.0 / n if total == 0 else self.cum[i][a] / total
        return out


def iterate(lay, T, s):
    """One iteration: the items of osg_efr.h in the phases' order."""
    P, A = lay.P, lay.A
    ext_only = T["type"] in EXTERNAL_ONLY
    value = [None] * lay.H
    for h in range(lay.H - 1, -1, -1):   # (levels deepest first; within a level the items are independent)
        k, fc = lay.kind[h], int(lay.first_child[h])
        if k == 2:
            value[h] = [float(x) for x in lay.term_ret[h]]
            continue
        probs = [float(lay.edge_prob[fc + a]) for a in range(lay.nchild[h])] if k == 0 else s.pol[lay.info[h]]
        row = []
        for p in range(P):
            x = 0.0
            for a in range(lay.nchild[h]):
                x = x + probs[a] * value[fc + a][p]
            row.append(x)
        value[h] = row
    mcf, mown_reach, live = [0.0] * lay.M, [0.0] * lay.M, [False] * lay.M
    for m in range(lay.M):
        reach = [1.0] * (P + 1)
        for e in range(lay.path_off[m], lay.path_off[m + 1]):
            code = lay.path[e]
            slot, idx = (code >> 24) & 0xF, code & 0x7FFFFF
            reach[slot] = reach[slot] * (float(lay.edge_prob[idx]) if (code >> 23) & 1 else s.pol[idx // A][idx % A])
        me = int(lay.actor[lay.mem[m]])
        live[m] = any(reach[p] != 0.0 for p in range(P))
        before = after = 1.0
        for p in range(me):
            before = before * reach[p]
        for p in range(me + 1, P + 1):
            after = after * reach[p]
        mcf[m], mown_reach[m] = before * after, reach[me]
    visited = [False] * lay.I
    for i in range(lay.I):
        for m in range(lay.mem_off[i], lay.mem_off[i + 1]):
            if live[m]:
                visited[i] = True
                for a in range(lay.nact[i]):
                    s.cum[i][a] = s.cum[i][a] + s.pol[i][a] * mown_reach[m]
    for k in range(len(T["info"])):
        i = T["info"][k]
        n, pl, target, source = int(lay.nact[i]), int(lay.info_player[i]), T["target"][k], T["source"][k]
        mr = memreach(T["mask"][k], T["cols"][k], T["own_info"][i], s.pol)
        dev = []
        for r in range(n):
            x = 0.0
            for c in range(n):
                if (r == target) if source < 0 else ((r == c and c != source) or (r == target and c == source)):
                    x = x + s.pol[i][c]
            dev.append(x)
        acc = s.R[k]
        for m in range(lay.mem_off[i], lay.mem_off[i + 1]):
            if not live[m]:
                continue
            h = int(lay.mem[m])
            fc = int(lay.first_child[h])
            dv = 0.0
            for a in range(n):
                dv = dv + dev[a] * value[fc + a][pl]
            acc = acc + mr * ((dv * mcf[m]) - (mcf[m] * value[h][pl]))
        s.R[k] = acc
    for infos in T["depths"]:
        for i in infos:
            n, keys = int(lay.nact[i]), T["keys"][i]
            y = [0.0 if visited[i] else s.y[i][k] for k in range(len(keys))]
            row = s.pol[i][:n]
            for m in range(lay.mem_off[i], lay.mem_off[i + 1]):
                for k in range(T["dev_off"][i], T["dev_off"][i + 1]):
                    r = s.R[k] if s.R[k] > 0.0 else 0.0
                    y[T["slot"][k]] = y[T["slot"][k]] + r * memreach(T["mask"][k], T["cols"][k], T["mown"][m], s.mpol)
                row, _ = regret_match(n, keys, y, ext_only)
                s.mpol[m][:n] = row
            s.y[i][:len(keys)] = y
            s.pol[i][:n] = row


# ---- the host program ------------------------------------------------------------------------------------------------
def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "efr_host_test.cpp"), "-o", path])
    return path


def _i32(a):
    return np.ascontiguousarray(a, np.int32).tobytes()


def _f64(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def write_layout(lay, f, more_sizes=()):
    """The layout as the host programs read it: the sizes (and the caller's own, in the same header), the sixteen int
    arrays, edge_prob and term_ret."""
    f.write(_i32([lay.H, lay.I, lay.A, lay.P, lay.D, lay.M, len(lay.path), *more_sizes]))
    for a in (lay.level_off, lay.parent, lay.first_child, lay.kind, lay.nchild, lay.aidx, lay.actor, lay.info, lay.mem_off,
              lay.mem, lay.mem_index, lay.nact, lay.legal, lay.info_player, lay.path_off, lay.path):
        f.write(_i32(a))
    f.write(_f64(lay.edge_prob) + _f64(lay.term_ret))


def write_case(v, r, path):
    """The input of `efr_host_test run`: the layout, the golden's deviation tables and its checkpoints."""
    _, game, name = runs(v)[r]
    lay = layout(v, r, game)
    i32, f64 = _i32, _f64
    Lg = v[f"r{r}/dev_weights"].shape[1]
    C = len(v[f"r{r}/checkpoints"])
    with open(path, "wb") as f:
        write_layout(lay, f, (TYPES.index(name), C, len(v[f"r{r}/dev_target"]), Lg))
        for k in ("dev_count", "dev_target", "dev_source", "dev_weights_none", "dev_weights", "dev_memory", "checkpoints"):
            f.write(i32(v[f"r{r}/{k}"]))
        for c in range(C):
            f.write(f64(v[f"r{r}/R"][c]))
            for k in ("cur", "cum", "avg"):
                f.write(f64(by_legal(v, r, v[f"r{r}/{k}"][c])))
    return lay


def read_host_state(v, r, lay, path):
    """[(state [D + I * 16], cur [I, A], cum [I, A])] per checkpoint, as the host program left them."""
    raw = np.fromfile(path, np.float64)
    D = len(v[f"r{r}/dev_target"])
    n = D + lay.I * MAX_KEYS + 2 * lay.I * lay.A
    out = []
    for c in range(len(v[f"r{r}/checkpoints"])):
        part = raw[c * n:(c + 1) * n]
        out.append((part[:D + lay.I * MAX_KEYS], part[D + lay.I * MAX_KEYS:][:lay.I * lay.A].reshape(lay.I, lay.A),
                    part[D + lay.I * MAX_KEYS + lay.I * lay.A:].reshape(lay.I, lay.A)))
    return out


def write_unit_cases(v, path):
    n = len(v["rm/A"])
    with open(path, "wb") as f:
        f.write(np.array([n], np.int32).tobytes())
        for j in range(n):
            nk = int(v["rm/nkeys"][j])
            f.write(np.array([v["rm/A"][j], v["rm/external_only"][j], nk], np.int32).tobytes())
            f.write(np.array([int(v["rm/key_target"][j, k]) | ((int(v["rm/key_source"][j, k]) + 1) << 4) for k in range(nk)], np.int32).tobytes())
            f.write(np.ascontiguousarray(v["rm/y"][j, :nk], np.float64).tobytes())
    return n
