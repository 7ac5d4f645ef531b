"""Shared by tests/golden/make_meta_solver_vectors.py, tests/test_meta_solver_goldens.py, tests/test_meta_solver_native.py
and tests/test_z25_gpu_meta_solvers.py: the cases of PSRO's meta-strategy solvers (projected replicator dynamics and
regret matching on a normal-form meta-game), the payoff tensors made from a kind and a seed, the goldens the reference's
own files left in tests/golden/meta_solver_vectors.npz, a plain NumPy restatement of the one order of every sum that
open_spiel_amd/csrc/osg_meta_solver.h fixes, and the input file of tests/native/meta_solver_host_test.cpp."""
import collections
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE = 1e-12            # absolute against the reference: population_cases.TOLERANCE; strategies are at most 1
RM_RECORDING_BOUND = 1e-13   # regret matching is recorded only at horizons where the restatement is this close
PRD, RM = 0, 1
INITIAL_SEED = 7000          # + the case's seed: the seeded non-uniform initial strategies

Case = collections.namedtuple("Case", "name kind seed shape method iterations dt gamma window use_approx initial")


def _case(name, kind, seed, shape, method, iterations, dt=1e-3, gamma=1e-6, window=None, use_approx=False, initial=False):
    return Case(name, kind, seed, tuple(shape), method, iterations, dt, gamma, window, use_approx, initial)


# The smallest shapes that can still go wrong, each at a few horizons; both projections; window None / 1 / 10; seeded
# initial strategies; a gamma at which the clamp of the projection is active (5x5/prd_clamp, 12x12/approx_clamp) and one
# with n * gamma >= 1, where the bisection answers rho = 0 and u_tmp[-1] is read (rps/prd_rho0).  Regret matching stays
# at a few hundred iterations: beyond that a rounding difference flips which regrets are positive.
CASES = (
    _case("1x1/prd", "general", 1, (1, 1), PRD, 10),
    _case("1x1/rm", "general", 1, (1, 1), RM, 10),
    _case("1x3/prd", "general", 2, (1, 3), PRD, 500),
    _case("1x3/approx", "general", 2, (1, 3), PRD, 500, use_approx=True, window=10),
    _case("1x3/rm", "general", 2, (1, 3), RM, 100, window=1),
    _case("2x2/prd", "zero_sum", 3, (2, 2), PRD, 1000, initial=True),
    _case("2x2/prd0", "zero_sum", 3, (2, 2), PRD, 0, initial=True),
    _case("2x2/rm", "zero_sum", 3, (2, 2), RM, 200),
    _case("rps/prd", "rps", 0, (3, 3), PRD, 20000, initial=True),
    _case("rps/prd_w1", "rps", 0, (3, 3), PRD, 1000, dt=1e-2, window=1, initial=True),
    _case("rps/prd_rho0", "rps", 0, (3, 3), PRD, 50, gamma=0.4, initial=True),
    _case("rps/rm", "rps", 0, (3, 3), RM, 300, initial=True),
    _case("brps/prd", "brps", 0, (3, 3), PRD, 5000, gamma=1e-8),
    _case("brps/rm", "brps", 0, (3, 3), RM, 300, gamma=1e-8),
    _case("ref2/prd", "ref_test", 0, (2, 3), PRD, 5000, gamma=1e-8, window=10),
    _case("ref2/rm", "ref_test", 0, (2, 3), RM, 200, window=10),
    _case("ref3/prd", "ref_test", 0, (2, 2, 3), PRD, 2000, window=10),
    _case("ref3/rm", "ref_test", 0, (2, 2, 3), RM, 200, window=10),
    _case("5x5/prd100", "zero_sum", 5, (5, 5), PRD, 100),
    _case("5x5/prd", "zero_sum", 5, (5, 5), PRD, 20000, dt=1e-2),
    _case("5x5/prd_w10", "zero_sum", 5, (5, 5), PRD, 3000, dt=1e-2, window=10),
    _case("5x5/prd_w1", "zero_sum", 5, (5, 5), PRD, 3000, dt=1e-2, window=1),
    _case("5x5/prd_clamp", "zero_sum", 5, (5, 5), PRD, 3000, dt=5e-2, gamma=0.05),
    _case("5x5/approx", "zero_sum", 5, (5, 5), PRD, 3000, dt=1e-2, use_approx=True),
    _case("5x5/rm100", "zero_sum", 5, (5, 5), RM, 100),
    _case("5x5/rm", "zero_sum", 5, (5, 5), RM, 300, window=10),
    _case("12x12/prd", "zero_sum", 12, (12, 12), PRD, 2000, dt=1e-2),
    _case("12x12/approx_clamp", "zero_sum", 12, (12, 12), PRD, 2000, dt=5e-2, gamma=0.02, use_approx=True, window=10),
    _case("12x12/rm", "zero_sum", 12, (12, 12), RM, 200),
    _case("9x7/prd", "general", 97, (9, 7), PRD, 1000, dt=1e-2, initial=True),
    _case("9x7/rm", "general", 97, (9, 7), RM, 200, initial=True),
    _case("2x3x2/prd", "general", 232, (2, 3, 2), PRD, 1000, dt=1e-2),
    _case("2x3x2/rm", "general", 232, (2, 3, 2), RM, 200, window=1),
    _case("4x3x5/prd", "general", 435, (4, 3, 5), PRD, 1000, dt=1e-2, initial=True),
    _case("4x3x5/approx", "general", 435, (4, 3, 5), PRD, 1000, dt=1e-2, use_approx=True, window=10),
    _case("4x3x5/rm", "general", 435, (4, 3, 5), RM, 200, window=10),
    _case("1x4x1/prd", "general", 141, (1, 4, 1), PRD, 300, dt=1e-2),
    _case("2^5/prd", "general", 25, (2, 2, 2, 2, 2), PRD, 500, dt=1e-2),
    _case("2^5/rm", "general", 25, (2, 2, 2, 2, 2), RM, 100),
    _case("64x64/prd", "zero_sum", 64, (64, 64), PRD, 60, dt=5e-2),
    _case("64x64/approx", "zero_sum", 64, (64, 64), PRD, 60, dt=5e-2, use_approx=True),
    _case("64x64/rm", "zero_sum", 64, (64, 64), RM, 60),
    # 3 * 8000 doubles = 192 000 bytes: more than the 163 840 bytes of LDS a workgroup can have on gfx950
    _case("20x20x20/prd", "general", 2020, (20, 20, 20), PRD, 20, dt=5e-2, initial=True),
    _case("20x20x20/rm", "general", 2020, (20, 20, 20), RM, 20),
)
BY_NAME = {c.name: c for c in CASES}
LDS_BYTES = 160 * 1024   # a workgroup's LDS on gfx950


def fits_lds(case):
    """Whether the kernel can keep the case's tensors in LDS beside the two strategy buffers (and 1 KiB it reserves)."""
    P, cells, SK = len(case.shape), int(np.prod(case.shape)), sum(case.shape)
    return 8 * (2 * SK + P * cells) + 1024 <= LDS_BYTES


def tensors(kind, seed, shape):
    """[P, K_0 .. K_{P-1}] float64: the payoff tensors of a case."""
    shape = tuple(shape)
    P = len(shape)
    if kind == "general":
        return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(P,) + shape)
    if kind == "zero_sum":
        a = np.random.RandomState(seed).uniform(-1.0, 1.0, size=shape)
        return np.stack([a, -a])
    if kind == "rps":
        a = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
        return np.stack([a, -a])
    if kind == "brps":   # biased rock-paper-scissors (matrix_brps)
        a = np.array([[0.0, -25.0, 50.0], [25.0, 0.0, -5.0], [-50.0, 5.0, 0.0]])
        return np.stack([a, -a])
    if kind == "ref_test":   # projected_replicator_dynamics_test.py / regret_matching_test.py: every player the same tensor
        t = {(2, 3): [[2, 1, 0], [0, -1, -2]],
             (2, 2, 3): [[[2, 1, 0], [1, 0, -1]], [[1, 0, -1], [0, -1, -2]]]}[shape]
        return np.stack([np.array(t, np.float64)] * P)
    raise ValueError(kind)


def initial_strategies(case):
    """Flat [sum K] seeded non-uniform strategies, or None (uniform)."""
    if not case.initial:
        return None
    rng = np.random.RandomState(INITIAL_SEED + case.seed)
    parts = [rng.uniform(0.1, 1.0, size=k) for k in case.shape]
    return np.concatenate([p / p.sum() for p in parts])


def split(flat, shape):
    return [np.array(x) for x in np.split(np.asarray(flat), np.cumsum(shape)[:-1])]


# ---- the restatement of osg_meta_solver.h: explicit ascending loops over every summed index ----
def _values(tensor, strategies, p):
    """v[a]: the other players contracted from the last to the first, each contraction a full intermediate whose every
    element is summed from 0.0 over the contracted index ascending (elementwise over the indices that remain)."""
    x = np.moveaxis(tensor, p, 0)
    for q in [q for q in range(len(strategies) - 1, -1, -1) if q != p]:
        acc = np.zeros(x.shape[:-1])
        for j in range(x.shape[-1]):
            acc = acc + x[..., j] * strategies[q][j]
        x = acc
    return x


def _ascending_sum(x):
    total = 0.0
    for value in x:
        total = total + float(value)
    return total


def _bisect_left(b):
    lo, hi = 0, len(b)
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if not b[mid]:
            lo = mid + 1
        else:
            hi = mid
    return lo


def _simplex_projection(u, gamma, stats):
    n = len(u)
    idx = np.arange(n)
    before = (u[None, :] > u[:, None]) | ((u[None, :] == u[:, None]) & (idx[None, :] < idx[:, None]))
    rank = before.sum(axis=1)
    srt = np.empty(n)
    srt[rank] = u
    u_tmp, b, cumsum = np.empty(n), [], 0.0
    for i in range(n):
        cumsum = float(srt[0]) if i == 0 else cumsum + float(srt[i])
        u_tmp[i] = (1.0 - cumsum - float(n - (i + 1)) * gamma) / float(i + 1)
        b.append(float(srt[i]) + u_tmp[i] <= gamma)
    rho = _bisect_left(b)
    shift = u_tmp[rho - 1 if rho > 0 else n - 1]
    x = u + shift
    if stats is not None:
        stats["rho0"] += rho == 0
        stats["clamped"] += int((x < gamma).sum())
    return np.where((x >= gamma) | (x != x), x, gamma)


def _approx_projection(u, gamma, stats):
    c = np.where(u < gamma, gamma, u)
    if stats is not None:
        stats["clamped"] += int((u < gamma).sum())
    return c / _ascending_sum(c)


def solve(T, method, iterations, dt=1e-3, gamma=1e-6, window=None, use_approx=False, initial=None, stats=None):
    """(average, last), each flat [sum K]: osg_meta_solver.h's arithmetic in its order.  T [P, K_0 .. K_{P-1}]."""
    T = np.asarray(T, np.float64)
    P, shape = T.shape[0], T.shape[1:]
    s = [np.full(k, 1.0 / k) for k in shape] if initial is None else split(np.asarray(initial, np.float64), shape)
    regrets = [np.full(k, 1.0 / 1e6) for k in shape]
    count = iterations + 1 if not window or window > iterations + 1 else window
    first = iterations + 1 - count
    total = [np.zeros(k) + (s[p] if first == 0 else 0.0) for p, k in enumerate(shape)]
    for t in range(1, iterations + 1):
        new = []
        for p in range(P):
            v = _values(T[p], s, p)
            avg = _ascending_sum(v * s[p])
            if method == PRD:
                u = s[p] + dt * (s[p] * (v - avg))
                new.append(_approx_projection(u, gamma, stats) if use_approx else _simplex_projection(u, gamma, stats))
            else:
                regrets[p] = regrets[p] + (v - avg)
                positive = np.where(regrets[p] < 0.0, 0.0, regrets[p])
                total_regret = _ascending_sum(positive)
                uniform = 1.0 / float(len(v))
                new.append(gamma * uniform + (1.0 - gamma) * (positive / total_regret) if total_regret > 0.0
                           else np.full(len(v), uniform))
        s = new
        if t >= first:
            total = [total[p] + s[p] for p in range(P)]
    return np.concatenate(total) / float(count), np.concatenate(s)


def solve_case(case, stats=None):
    return solve(tensors(case.kind, case.seed, case.shape), case.method, case.iterations, case.dt, case.gamma, case.window,
                 case.use_approx, initial_strategies(case), stats)


_RESTATED = {}


def restated():
    """name -> (average, last, stats) of every case by the restatement, computed once per process.  Read only."""
    if not _RESTATED:
        for c in CASES:
            stats = collections.Counter()
            average, last = solve_case(c, stats)
            for x in (average, last):
                x.setflags(write=False)
            _RESTATED[c.name] = (average, last, stats)
    return _RESTATED


def meta_solver(method, **kwargs):
    """The restatement as a PSROSolver `meta_solver` callable, with the reference's keyword names."""
    names = {"prd_iterations": "iterations", "prd_dt": "dt", "prd_gamma": "gamma", "average_over_last_n_strategies": "window"}
    kw = {names.get(k, k): v for k, v in kwargs.items()}

    def run(meta_games):
        T = np.stack([np.asarray(t, np.float64) for t in meta_games])
        return split(solve(T, method, **kw)[0], T.shape[1:])
    return run


# ---- the goldens ----
def params_row(case):
    return np.array([case.method, case.iterations, case.dt, case.gamma, case.window or 0, int(case.use_approx), int(case.initial),
                     case.seed], np.float64)


def load():
    """name -> the reference's average strategies (flat); the file's recorded parameters must be CASES'."""
    with np.load(os.path.join(ROOT, "tests", "golden", "meta_solver_vectors.npz")) as z:
        names = bytes(z["names"]).decode().split("\n")
        kinds = bytes(z["kinds"]).decode().split("\n")
        assert names == [c.name for c in CASES], "tests/golden/meta_solver_vectors.npz was recorded for another list of cases"
        out = {}
        for i, c in enumerate(CASES):
            assert kinds[i] == c.kind and tuple(z[f"{c.name}/shape"]) == c.shape and np.array_equal(z[f"{c.name}/params"], params_row(c)), c.name
            out[c.name] = z[f"{c.name}/average"]
        return out


PSRO_GAMES = ("kuhn_poker", "kuhn_poker(players=3)")
PSRO_ITERATIONS, PSRO_PRD_ITERATIONS = 4, 2000


def load_psro():
    """game -> per PSRO iteration (the payoff tensors [P, K_0 .. K_{P-1}] that PSROSolver(meta_solver="prd",
    prd_iterations=2000) handed its meta-solver on the device, the reference's PRD answer on them, flat)."""
    with np.load(os.path.join(ROOT, "tests", "golden", "meta_solver_vectors.npz")) as z:
        return {g: [(z[f"psro/{g}/it{k}/tensors"], z[f"psro/{g}/it{k}/average"]) for k in range(PSRO_ITERATIONS)] for g in PSRO_GAMES}


# ---- tests/native/meta_solver_host_test.cpp ----
def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "meta_solver_host_test.cpp"), "-o", path])
    return path


def write_cases(cases, restated, golden, path):
    """Per case: P, K[5], method, iterations, window, use_approx, has_initial (int32 x 11); dt, gamma; the tensors; the
    initial strategies (where given); the restatement's average and last iterate; the reference's average."""
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes())
        for c in cases:
            init = initial_strategies(c)
            K = list(c.shape) + [0] * (5 - len(c.shape))
            f.write(np.array([len(c.shape)] + K + [c.method, c.iterations, c.window or 0, int(c.use_approx), int(init is not None)], np.int32).tobytes())
            f.write(np.array([c.dt, c.gamma], np.float64).tobytes())
            f.write(np.ascontiguousarray(tensors(c.kind, c.seed, c.shape), np.float64).tobytes())
            if init is not None:
                f.write(init.tobytes())
            for x in (restated[c.name][0], restated[c.name][1], golden[c.name]):
                f.write(np.ascontiguousarray(x, np.float64).tobytes())
