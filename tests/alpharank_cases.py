"""Shared by tests/golden/make_alpharank_vectors.py, tests/test_alpharank_goldens.py, tests/test_alpharank_native.py,
tests/test_z29_gpu_alpharank.py and tools/probe_alpharank.py: the alpha-rank cases, the payoff tensors made from a kind
and a seed, what the reference's own egt/alpharank.py left in tests/golden/alpharank_vectors.npz, a plain NumPy
restatement of open_spiel_amd/csrc/osg_alpharank.h in the header's order of sums (the multiply-add is NOT fused, as
there), and the input file of tests/native/alpharank_host_test.cpp."""
import collections
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINITE, INFINITE, SWEEP = 0, 1, 2
OK, REDUCIBLE, NO_STOP = 0, 1, 2
LANES = 64
LDS_BYTES = 160 * 1024   # a workgroup's LDS on gfx950
LDS_RESERVE = 1024       # what osg_alpharank keeps free of it
U = 2.0 ** -53

# eps_rho: the relative error of the header's rho against its 50-digit value.  The two roundings of u = alpha * (pc - pr)
# dominate it: rho ~ exp((m - 1) u) for u < 0 magnifies them (m - 1) |u| times, and a rho that does not underflow has
# (m - 1) |u| <= ln 1e300 = 690.8, so 690.8 * 2^-52 = 1.53e-13, and a few ulp for exp, expm1 and the quotient.
# tests/golden/make_alpharank_vectors.py measured 9.32e-14 over the finite-alpha cases (at alpha = 100, |u| up to 190).
EPS_RHO = 1.6e-13

Case = collections.namedtuple("Case", "name kind seed shape single mode m alpha eps min_iters max_iters scale exact_only")


def _case(name, kind, seed, shape, mode=SWEEP, single=False, m=50, alpha=100.0, eps=0.0, min_iters=10, max_iters=100, scale=1.0,
          exact_only=False):
    return Case(name, kind, seed, tuple(shape), single, mode, m, float(alpha), float(eps), min_iters, max_iters, float(scale), exact_only)


_FINITE_SCALE = {0.1: 10.0, 1.0: 1.0, 10.0: 0.05}   # alpha * |pc - pr| stays below 2: m |u| <= 100, no rho underflows

CASES = (
    # trivial and singleton
    _case("1x1", "general", 11, (1, 1)),
    _case("1x3", "general", 13, (1, 3)),
    _case("3x1x2", "general", 312, (3, 1, 2)),
    # integer payoffs with ties
    _case("2x2/int", "int", 22, (2, 2)),
    _case("4x4/zs_int", "zero_sum_int", 44, (4, 4)),
    _case("3x3x3/int", "int", 333, (3, 3, 3)),
    # general
    _case("3x5", "general", 36, (3, 5)),
    _case("3x5/ref2.6e-8", "general", 35, (3, 5), exact_only=True),   # the reference's eigen-solve is 2.6e-8 from the exact pi here
    _case("6x6", "general", 66, (6, 6)),
    _case("8x8", "general", 89, (8, 8)),
    _case("4x4x4", "general", 446, (4, 4, 4)),
    _case("2^4", "general", 2223, (2, 2, 2, 2)),
    _case("2^5", "general", 22224, (2, 2, 2, 2, 2)),
    # wavefront edges: n = 63, 64, 65
    _case("7x9", "general", 79, (7, 9)),
    _case("8x8/b", "general", 808, (8, 8)),
    _case("5x13", "general", 513, (5, 13)),
    # around n = 128, and around the LDS limit of the matrix form (n = 142 fits 160 KiB beside the vector, 143 does not)
    _case("8x16", "general", 816, (8, 16)),
    _case("3x43", "general", 345, (3, 43)),
    _case("11x12", "general", 1113, (11, 12)),
    _case("2x71", "general", 272, (2, 71)),
    _case("11x13", "general", 1114, (11, 13)),
    # global form
    _case("16x16", "general", 1616, (16, 16)),
    _case("8x8x8", "general", 888, (8, 8, 8)),
    _case("32x32/eps1e-3", "general", 3232, (32, 32), mode=INFINITE, eps=1e-3),
    # single population
    _case("rps", "rps", 0, (3, 3), single=True),
    _case("single5", "general", 5, (5, 5), single=True),
    _case("single5/eps", "general", 5, (5, 5), single=True, mode=INFINITE, eps=0.01),
    _case("4x4/eps", "general", 404, (4, 4), mode=INFINITE, eps=0.01),
) + tuple(
    _case(f"{name}/alpha{alpha:g}", "general", seed, shape, mode=FINITE, alpha=alpha, scale=_FINITE_SCALE[alpha])
    for name, seed, shape in (("2x2", 1022, (2, 2)), ("4x4", 1045, (4, 4)), ("6x6", 1066, (6, 6)), ("3x3x3", 1334, (3, 3, 3)))
    for alpha in (0.1, 1.0, 10.0)
) + (
    # where the reference's eigen-solve raises "Expected 1 stationary distribution".  (Seeds at which a fixation probability
    # falls between 4.9e-324 and 2.2e-308 are avoided: a subnormal rho keeps few bits, and pi lies up to 6e-8 (relative)
    # from the exact one there, e.g. at seed 3514 with alpha = 10.)
    _case("3x5/alpha10", "general", 3523, (3, 5), mode=FINITE, alpha=10.0, exact_only=True),
    _case("3x5/alpha100", "general", 3532, (3, 5), mode=FINITE, alpha=100.0, exact_only=True),
)
BY_NAME = {c.name: c for c in CASES}
SWEEP_CASES = tuple(c for c in CASES if c.mode == SWEEP)


def n_states(case):
    return case.shape[0] if case.single else int(np.prod(case.shape))


def n_moves(case):
    return case.shape[0] - 1 if case.single else int(sum(k - 1 for k in case.shape))


def fits_lds(n):
    """Whether osg_alpharank keeps the n x n matrix in LDS beside the vector x and the bytes it reserves."""
    return 8 * (n * n + n) + LDS_RESERVE <= LDS_BYTES


def bound(case):
    """The entrywise relative bound against the exact pi: 8 n 2^-53 for the subtraction-free elimination, and for finite
    alpha 2 n eps_rho more (O'Cinneide's entrywise perturbation bound)."""
    n = n_states(case)
    return 8.0 * n * U + (2.0 * n * EPS_RHO if case.mode == FINITE else 0.0)


def tensors(case):
    """[P, K_0 .. K_{P-1}] float64 (single population: [1, K, K])."""
    shape, P = case.shape, len(case.shape)
    rng = np.random.RandomState(case.seed)
    if case.kind == "rps":
        return np.array([[[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]]])
    if case.single:
        return rng.uniform(-1.0, 1.0, size=(1,) + shape) * case.scale
    if case.kind == "general":
        return rng.uniform(-1.0, 1.0, size=(P,) + shape) * case.scale
    if case.kind == "int":
        return rng.randint(-2, 3, size=(P,) + shape).astype(np.float64)
    if case.kind == "zero_sum_int":
        a = rng.randint(-3, 4, size=shape).astype(np.float64)
        return np.stack([a, -a])
    raise ValueError(case.kind)


# ---- the restatement of osg_alpharank.h ----
def neighbours(shape, single):
    """(cols [n, moves], at_col, at_row): per state and move the column state and where the deviating player's two
    payoffs lie in the flat tensors (ar_neighbour)."""
    if single:
        K = shape[0]
        s = np.arange(K)[:, None]
        mv = np.arange(K - 1)[None, :]
        r = mv + (mv >= s)
        return r, r * K + s, s * K + r
    n = int(np.prod(shape))
    ids = np.arange(n)
    strides = [int(np.prod(shape[p + 1:])) for p in range(len(shape))]
    cols, at_col, at_row = [], [], []
    for p, K in enumerate(shape):
        own = (ids // strides[p]) % K
        for j in range(K - 1):
            alt = j + (j >= own)
            col = ids + (alt - own) * strides[p]
            cols.append(col)
            at_col.append(p * n + col)
            at_row.append(p * n + ids)
    if not cols:
        z = np.zeros((n, 0), np.int64)
        return z, z, z
    return np.stack(cols, 1), np.stack(at_col, 1), np.stack(at_row, 1)


def eta_of(shape, single):
    moves = shape[0] - 1 if single else sum(k - 1 for k in shape)
    with np.errstate(divide="ignore"):
        return float(np.float64(1.0) / np.float64(moves))


def rho(pc, pr, alpha, m):
    md = float(m)
    with np.errstate(all="ignore"):
        u = alpha * (pc - pr)
        positive = np.expm1(-u) / np.expm1(-(md * u))
        negative = (np.exp((md - 1.0) * u) * np.expm1(u)) / np.expm1(md * u)
        out = np.where(np.abs(u) <= 1e-14, 1.0 / md, np.where(u > 0.0, positive, negative))
    return np.where(np.isfinite(pc) & np.isfinite(pr), out, np.nan)


def entries(T, single, mode, eps=None, alpha=None, m=None):
    """(cols [n, moves], values [n, moves]): the off-diagonal entries, move by move."""
    T = np.asarray(T, np.float64)
    shape = T.shape[1:]
    cols, at_col, at_row = neighbours(shape, single)
    flat = T.reshape(-1)
    pc, pr = flat[at_col], flat[at_row]
    eta = eta_of(shape, single)
    if mode == FINITE:
        return cols, eta * rho(pc, pr, alpha, m)
    with np.errstate(invalid="ignore"):
        tie = np.abs(pc - pr) <= 1e-14 + 1e-5 * np.abs(pr)
        values = np.where(tie, eta * 0.5, np.where(pc > pr, eta * (1.0 - eps), eta * eps))
    return cols, np.where(np.isfinite(pc) & np.isfinite(pr), values, np.nan)


def dense(cols, values):
    n = cols.shape[0]
    a = np.zeros((n, n))
    if cols.shape[1]:
        a[np.arange(n)[:, None], cols] = values
    return a


def lane_sum(v):
    """ar_lane_sum: 64 partial sums over j = l, l + 64, .. ascending from 0.0, then the pairwise tree."""
    c = len(v)
    rows = max(-(-c // LANES), 1)
    buf = np.zeros(rows * LANES)
    buf[:c] = v
    part = np.zeros(LANES)
    for row in buf.reshape(rows, LANES):
        part = part + row
    while len(part) > 1:
        part = part[0::2] + part[1::2]
    return float(part[0])


def stationary(a):
    """(pi, status): ar_stationary on a copy of the matrix."""
    a = np.array(a, np.float64)
    n = a.shape[0]
    with np.errstate(all="ignore"):
        for k in range(n - 1, 0, -1):
            s = lane_sum(a[k, :k])
            if not (s > 0.0 and np.isfinite(s)):
                return np.full(n, np.nan), REDUCIBLE
            q = a[:k, k] / s
            a[:k, k] = q
            a[:k, :k] = a[:k, :k] + q[:, None] * a[k, :k][None, :]
        x = np.zeros(n)
        x[0] = 1.0
        for i in range(n - 1):
            x[i + 1:] = x[i + 1:] + x[i] * a[i, i + 1:]
        total = lane_sum(x)
        if not np.isfinite(total):
            return np.full(n, np.nan), REDUCIBLE
        return x / total, OK


def marginals(shape, single, pi):
    """Flat [sum K_p]: per player and strategy the sum of pi over the profiles that play it, ids ascending from 0.0."""
    pi = np.asarray(pi, np.float64)
    if single:
        return pi.copy()
    out = []
    for p, K in enumerate(shape):
        rows = np.moveaxis(pi.reshape(shape), p, 0).reshape(K, -1)
        acc = np.zeros(K)
        for col in range(rows.shape[1]):
            acc = acc + rows[:, col]
        out.append(acc)
    return np.concatenate(out)


Result = collections.namedtuple("Result", "pi status eps iterations marginals")


def solve(T, single=False, mode=SWEEP, m=50, alpha=100.0, eps=0.0, min_iters=10, max_iters=100, history=None):
    """osg_alpharank's answer for one problem.  `history`: a list that receives (eps_t, pi_t) of every sweep step."""
    T = np.asarray(T, np.float64)
    shape = T.shape[1:]

    def done(pi, status, e, t):
        if status != OK:
            pi = np.full(len(pi), np.nan)
        return Result(pi, status, e, t, marginals(shape, single, pi))

    if mode != SWEEP:
        pi, status = stationary(dense(*entries(T, single, mode, eps, alpha, m)))
        return done(pi, status, eps if mode == INFINITE else 0.0, 0)
    e = 0.5 if eps == 0.0 else eps
    prev, t = None, 0
    while True:
        pi, status = stationary(dense(*entries(T, single, INFINITE, e)))
        if history is not None:
            history.append((e, pi))
        if status != OK:
            return done(pi, status, e, t)
        if t > min_iters and bool(np.all(np.abs(pi - prev) <= 1e-8 + 1e-5 * np.abs(prev))):
            return done(pi, OK, e, t)
        if t + 1 >= max_iters:
            return done(pi, NO_STOP, e, t)
        prev, e, t = pi, e * 0.5, t + 1


def solve_case(case, **changes):
    kw = dict(single=case.single, mode=case.mode, m=case.m, alpha=case.alpha, eps=case.eps, min_iters=case.min_iters,
              max_iters=case.max_iters)
    kw.update(changes)
    return solve(tensors(case), **kw)


_RESTATED = {}


def restated():
    """name -> Result of every case by the restatement, computed once per process.  Read only."""
    if not _RESTATED:
        for c in CASES:
            r = solve_case(c)
            for x in (r.pi, r.marginals):
                x.setflags(write=False)
            _RESTATED[c.name] = r
    return _RESTATED


def meta_solver(**kwargs):
    """The restatement as a PSROSolver `meta_solver` callable: the sweep, then the marginals."""
    def run(meta_games):
        T = np.stack([np.asarray(t, np.float64) for t in meta_games])
        r = solve(T, **kwargs)
        if r.status != OK:
            raise RuntimeError(f"alpha-rank: status {r.status}")
        return [np.array(x) for x in np.split(r.marginals, np.cumsum(T.shape[1:])[:-1])]
    return run


# ---- the goldens ----
def params_row(case):
    return np.array([case.mode, case.m, case.alpha, case.eps, case.min_iters, case.max_iters, int(case.single), case.seed, case.scale,
                     int(case.exact_only)], np.float64)


Golden = collections.namedtuple("Golden", "pi_ref eps_ref iterations_ref entries_ref pi_exact ref_err marginals_ref exact_only")


def load():
    """name -> Golden; the file's recorded parameters must be CASES'."""
    with np.load(os.path.join(ROOT, "tests", "golden", "alpharank_vectors.npz")) as z:
        names = bytes(z["names"]).decode().split("\n")
        kinds = bytes(z["kinds"]).decode().split("\n")
        assert names == [c.name for c in CASES], "tests/golden/alpharank_vectors.npz was recorded for another list of cases"
        out = {}
        for i, c in enumerate(CASES):
            assert kinds[i] == c.kind and tuple(z[f"{c.name}/shape"]) == c.shape and np.array_equal(z[f"{c.name}/params"], params_row(c)), c.name
            exact_only = bool(z[f"{c.name}/exact_only"])
            out[c.name] = Golden(None if exact_only else z[f"{c.name}/pi_ref"], float(z[f"{c.name}/eps_ref"]),
                                 int(z[f"{c.name}/iterations_ref"]), None if exact_only else z[f"{c.name}/entries_ref"],
                                 z[f"{c.name}/pi_exact"], float(z[f"{c.name}/ref_err"]),
                                 None if exact_only else z[f"{c.name}/marginals_ref"], exact_only)
        return out


# ---- tests/native/alpharank_host_test.cpp ----
def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "alpharank_host_test.cpp"), "-o", path])
    return path


def write_cases(cases, restated, golden, path):
    """Per case: P, the shape padded to 5, mode, m, min_iters, max_iters, exact_only, status, iterations (int32 x 12);
    alpha, eps, the bound, eps_used (float64 x 4); the tensors; the restatement's entries at eps_used [n, moves], pi [n]
    and marginals [SK]; the exact pi [n]."""
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes())
        for c in cases:
            r = restated[c.name]
            T = tensors(c)
            dims = list(c.shape) + [0] * (5 - len(c.shape))
            f.write(np.array([1 if c.single else len(c.shape)] + dims + [c.mode, c.m, c.min_iters, c.max_iters, int(c.exact_only),
                                                                          r.status, r.iterations], np.int32).tobytes())
            f.write(np.array([c.alpha, c.eps, bound(c), r.eps], np.float64).tobytes())
            f.write(np.ascontiguousarray(T, np.float64).tobytes())
            _, values = entries(T, c.single, c.mode, r.eps, c.alpha, c.m)
            for x in (values, r.pi, r.marginals, golden[c.name].pi_exact):
                f.write(np.ascontiguousarray(x, np.float64).tobytes())
