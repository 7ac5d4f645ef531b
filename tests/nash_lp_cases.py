"""The exact Nash meta-solver's cases, shared by its CPU and GPU tests: the matrices, a NumPy restatement of
open_spiel_amd/csrc/osg_nash_lp.h (the same operations in the same order: bit for bit), the HiGHS reference and the
certificate every answer must pass."""
import math
import os
import subprocess

import numpy as np
from scipy.optimize import linprog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, MAX_PIVOTS = 1e-12, 20000   # kNlEps, kNlMaxPivots


def _matrices():
    rng = lambda seed: np.random.default_rng(9100 + seed)
    base = rng(3).integers(-3, 4, (6, 5)).astype(np.float64)
    skew = rng(8).standard_normal((64, 64))
    return {
        "1x1": np.array([[-2.5]]), "1x6": rng(1).standard_normal((1, 6)), "6x1": rng(2).standard_normal((6, 1)),
        "pennies": np.array([[1.0, -1.0], [-1.0, 1.0]]), "rps": np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]]),
        "constant_5x7": np.full((5, 7), 0.75), "duplicates_18x10": np.tile(base, (3, 2)),
        "integers_33x17": rng(4).integers(-2, 3, (33, 17)).astype(np.float64),
        "normal_64x3": rng(5).standard_normal((64, 3)), "normal_3x64": rng(6).standard_normal((3, 64)),
        "normal_64x64": rng(7).standard_normal((64, 64)), "skew_64x64": skew - skew.T,
        "signs_64x64": rng(9).integers(-1, 2, (64, 64)).astype(np.float64), "scaled_40x40": rng(10).standard_normal((40, 40)) * 1e6,
    }


CASES = _matrices()


def _compensated_sum(values):   # nl_sum: ascending, every rounding error collected beside the sum
    s = e = 0.0
    for v in values:
        t = s + v
        e = e + (((s - t) + v) if abs(s) >= abs(v) else ((v - t) + s))
        s = t
    return s + e


def solve(A):
    """osg_nash_lp.h's nl_solve: (x, y, v, pivots, status)."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    nan = (np.full(m, np.nan), np.full(n, np.nan), np.nan)
    if not np.isfinite(A).all():
        return (*nan, 0, 1)
    lo, hi = A.min(), A.max()
    span = hi - lo
    T = np.empty((m + 1, n + 1))
    T[:m, :n] = (A - lo) / span + 1.0 if span > 0.0 else 1.0
    T[:m, n], T[m, :n], T[m, n] = 1.0, -1.0, 0.0
    cols, rows = np.arange(n), n + np.arange(m)
    pivots = 0
    while True:
        enter = np.flatnonzero(T[m, :n] < -EPS)
        if not len(enter):
            break
        c = enter[np.argmin(cols[enter])]
        cand = np.flatnonzero(T[:m, c] > EPS)
        if pivots == MAX_PIVOTS or not len(cand):
            return (*nan, pivots, 2)
        ratio = T[cand, n] / T[cand, c]
        ties = cand[ratio == ratio.min()]
        r = ties[np.argmin(rows[ties])]
        p = T[r, c]
        row, col = T[r] / p, T[:, c].copy()
        T -= np.outer(col, row)   # the product is rounded, then subtracted
        T[:, c] = -(col / p)
        T[r] = row
        T[r, c] = 1.0 / p
        cols[c], rows[r] = rows[r], cols[c]
        pivots += 1
    yp, xp = np.zeros(n), np.zeros(m)
    yp[rows[rows < n]] = np.maximum(T[:m, n][rows < n], 0.0)
    xp[cols[cols >= n] - n] = np.maximum(T[m, :n][cols >= n], 0.0)
    sy, sx = _compensated_sum(yp), _compensated_sum(xp)
    return xp / sx, yp / sy, (1.0 / sy - 1.0) * span + lo, pivots, 0


_RESTATED = {}


def restated(name):
    if name not in _RESTATED:
        _RESTATED[name] = solve(CASES[name])
    return _RESTATED[name]


def meta_solver(meta_games):
    """The restatement as a PSROSolver `meta_solver` callable."""
    x, y, _, _, status = solve(meta_games[0])
    assert status == 0
    return [x, y]


# ---- the reference: HiGHS on the reference's LPs (lp_solver.solve_zero_sum_matrix_game) ----
def highs(A):
    """(x, y, v) with v from the row player's LP: max v s.t. x^T A >= v, x a distribution; y from the column player's."""
    m, n = A.shape
    row = linprog(np.r_[np.zeros(m), -1.0], A_ub=np.c_[-A.T, np.ones(n)], b_ub=np.zeros(n), A_eq=[np.r_[np.ones(m), 0.0]], b_eq=[1.0],
                  bounds=[(0, None)] * m + [(None, None)], method="highs")
    col = linprog(np.r_[np.zeros(n), 1.0], A_ub=np.c_[A, -np.ones(m)], b_ub=np.zeros(m), A_eq=[np.r_[np.ones(n), 0.0]], b_eq=[1.0],
                  bounds=[(0, None)] * n + [(None, None)], method="highs")
    assert row.status == 0 and col.status == 0
    return row.x[:m], col.x[:n], -row.fun


def gap(A, x, y):
    return float((A @ y).max() - (x @ A).min())


def scale(A):
    return max(1.0, float(np.abs(A).max()))


_BOUND = []


def bound():
    """max(1e-12, 100 x HiGHS's largest relative gap on CASES): 1e-12 is the project's bound for the meta-solvers, and the
    factor 100 is there because a tableau method without refinement stops on eps, not on a residual."""
    if not _BOUND:
        worst = max(abs(gap(A, *highs(A)[:2])) / scale(A) for A in CASES.values())
        print(f"HiGHS's largest relative gap: {worst:.3g}")
        _BOUND.append(max(1e-12, 100.0 * worst))
    return _BOUND[0]


def certify(A, x, y, v, status, what=""):
    """The certificate of a Nash pair in plain fp64; returns (gap, |v - v_highs|), both relative to scale(A)."""
    A = np.asarray(A, np.float64)
    assert status == 0, what
    for s in (x, y):
        assert (s >= 0.0).all() and abs(math.fsum(s) - 1.0) <= 4 * 2.0**-52, what
    g, dv, b = gap(A, x, y), abs(v - highs(A)[2]), bound()
    print(f"{what}: gap {g / scale(A):.3g}, |v - v_highs| {dv / scale(A):.3g} (relative; bound {b:.3g})")
    assert -b <= g <= b * scale(A) and dv <= b * scale(A), what
    return g / scale(A), dv / scale(A)


# ---- tests/native/nash_lp_host_test.cpp ----
def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "nash_lp_host_test.cpp"), "-o", path])
    return path


def write_cases(path):
    """Per case: rows, cols, pivots, status (int32 x 4); the matrix; the restatement's x, y and v."""
    with open(path, "wb") as f:
        f.write(np.array([len(CASES)], np.int32).tobytes())
        for name, A in CASES.items():
            x, y, v, pivots, status = restated(name)
            f.write(np.array([*A.shape, pivots, status], np.int32).tobytes())
            for a in (A, x, y, [v]):
                f.write(np.ascontiguousarray(a, np.float64).tobytes())
