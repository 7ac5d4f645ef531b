"""The exact Nash meta-solver's cases, shared by its CPU and GPU tests: the matrices, a NumPy restatement of
open_spiel_amd/csrc/osg_nash_lp.h (the same operations in the same order: bit for bit), the HiGHS reference and the
certificate every answer must pass.

HiGHS's largest relative duality gap, measured: 2.02e-14 over CASES; g = 1.14e-10 over the sweep (on offset 4x5; by family:
normal 2.56e-13, signs 6.26e-13, binary 2.20e-13, saddle 0, offset 1.14e-10, constant 0, diagonal 4.18e-16, skew 4.63e-15,
duplicates 1.48e-16; no optimum reported on 4 offset matrices: 4x2, 31x63, 64x63, 64x64).  The restatement's largest gap
over the sweep is 8.02e-12 (binary 64x31; the bound of `binary` is 2.2e-11), its most pivots 638."""
import math
import os
import subprocess

import numpy as np
from scipy.optimize import linprog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, PIVOT_EPS, MAX_PIVOTS = 1e-12, 1e-9, 20000   # kNlEps, kNlPivotEps, kNlMaxPivots


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

# ---- the sweep: every ordered pair of SIDES, one matrix per family from a fixed seed ----
SIDES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64)
FAMILIES = ("normal", "signs", "binary", "saddle", "offset", "constant", "diagonal", "skew", "duplicates")
_SWEEP = {}


def _shape_matrices(m, n):
    """One generator per shape, drawn in a fixed order (normal, signs, binary first: small-integer tables in that draw
    order are where a pivot on rounding noise was found, at 63x64)."""
    r = np.random.default_rng(m * 100 + n)
    out = {"normal": r.standard_normal((m, n))}
    out["signs"] = r.integers(-1, 2, (m, n)).astype(np.float64)
    out["binary"] = r.integers(0, 2, (m, n)).astype(np.float64)
    out["saddle"] = np.add.outer(r.integers(-3, 4, m), r.integers(-3, 4, n)).astype(np.float64)
    out["offset"] = 1e6 + 1e-3 * r.standard_normal((m, n))
    out["constant"] = np.full((m, n), r.standard_normal())
    k = min(m, n)
    d = r.uniform(0.5, 2.0, k)
    out["diagonal"] = np.zeros((m, n))   # surplus rows: 0, surplus columns: max d + 1; both strictly dominated
    out["diagonal"][:, k:] = d.max() + 1.0
    out["diagonal"][np.arange(k), np.arange(k)] = d
    block = r.integers(-3, 4, (3, 2)).astype(np.float64)
    out["duplicates"] = np.tile(block, (-(-m // 3), -(-n // 2)))[:m, :n].copy()
    if m == n:
        s = r.standard_normal((m, n))
        out["skew"] = s - s.T
    return out


def families(m, n):
    return [f for f in FAMILIES if f != "skew" or m == n]


def sweep_matrix(m, n, family):
    """The sweep's fp64 matrix of a shape and a family; the same array on every call (do not write to it)."""
    if (m, n) not in _SWEEP:
        _SWEEP[m, n] = _shape_matrices(m, n)
    return _SWEEP[m, n][family]


def sweep():
    """(m, n, family) of every matrix of the sweep."""
    return [(m, n, f) for m in SIDES for n in SIDES for f in families(m, n)]


def diagonal_answer(A):
    """The unique equilibrium of a `diagonal` matrix: (weights 1/d_i normalised, over the leading diagonal; the value)."""
    d = [float(A[i, i]) for i in range(min(A.shape))]
    total = math.fsum(1.0 / v for v in d)
    return np.array([1.0 / v / total for v in d]), 1.0 / total


def saddle_value(A):
    return float(A.min(axis=1).max())


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
    with np.errstate(over="ignore"):
        pre = 1.0 if np.isfinite(hi - lo) else 0.5   # nl_range
    base = lo * pre
    span = hi * pre - base
    T = np.empty((m + 1, n + 1))
    T[:m, :n] = (A * pre - base) / span + 1.0 if span > 0.0 else 1.0
    T[:m, n], T[m, :n], T[m, n] = 1.0, -1.0, 0.0
    cols, rows = np.arange(n), n + np.arange(m)
    pivots = 0
    while True:
        enter = np.flatnonzero(T[m, :n] < -EPS)
        if not len(enter):
            break
        c = enter[np.argmin(cols[enter])]
        cand = np.flatnonzero(T[:m, c] > PIVOT_EPS)
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
    return xp / sx, yp / sy, ((1.0 / sy - 1.0) * span + base) / pre, pivots, 0


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
def highs(A, must=True):
    """(x, y, v) with v from the row player's LP: max v s.t. x^T A >= v, x a distribution; y from the column player's.
    must=False: None where HiGHS reports no optimum."""
    m, n = A.shape
    row = linprog(np.r_[np.zeros(m), -1.0], A_ub=np.c_[-A.T, np.ones(n)], b_ub=np.zeros(n), A_eq=[np.r_[np.ones(m), 0.0]], b_eq=[1.0],
                  bounds=[(0, None)] * m + [(None, None)], method="highs")
    col = linprog(np.r_[np.zeros(n), 1.0], A_ub=np.c_[A, -np.ones(m)], b_ub=np.zeros(m), A_eq=[np.r_[np.ones(n), 0.0]], b_eq=[1.0],
                  bounds=[(0, None)] * n + [(None, None)], method="highs")
    if not must and (row.status != 0 or col.status != 0):
        return None
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


_SWEEP_BOUND = {}


def sweep_bound(family=None):
    """bound() measured on the sweep's own matrices instead of CASES, for the same reasons: max(1e-12, 100 x g), g HiGHS's
    largest relative gap.  With a family: g over that family's matrices alone, which is never the wider bound (HiGHS's
    gap on `offset` is a thousand times its gap elsewhere).  HiGHS ends without an optimum on a few `offset` matrices
    (1e6 + 1e-3 * normal is badly scaled for its tolerances); those have no gap to measure."""
    if not _SWEEP_BOUND:
        none = 0
        for m, n, f in sweep():
            A = sweep_matrix(m, n, f)
            a = highs(A, must=False)
            none += a is None
            _SWEEP_BOUND[f] = max(_SWEEP_BOUND.get(f, 0.0), abs(gap(A, *a[:2])) / scale(A) if a else 0.0)
        _SWEEP_BOUND[None] = max(_SWEEP_BOUND.values())
        print(f"HiGHS's largest relative gap over the sweep (g): {_SWEEP_BOUND[None]:.3g}; it reports no optimum on {none} matrices;"
              f" by family: " + ", ".join(f"{f} {_SWEEP_BOUND[f]:.3g}" for f in FAMILIES))
    return max(1e-12, 100.0 * _SWEEP_BOUND[family])


def certificate(A, x, y, v, status, b, what=""):
    """The certificate of a Nash pair in plain fp64, with no solver: two distributions, a duality gap within the bound b
    and a value between the two players' guarantees (v None: not checked).  Returns the gap relative to scale(A)."""
    A = np.asarray(A, np.float64)
    assert status == 0, what
    for s in (x, y):
        assert (s >= 0.0).all() and abs(math.fsum(s) - 1.0) <= 4 * 2.0**-52, what
    g = gap(A, x, y)
    assert -b <= g <= b * scale(A), (what, g / scale(A))
    if v is not None:
        assert (x @ A).min() - b * scale(A) <= v <= (A @ y).max() + b * scale(A), (what, v)
    return g / scale(A)


def value_against_highs(A, v, b, what=""):
    """|v - HiGHS's value| relative to scale(A), within b."""
    A = np.asarray(A, np.float64)
    dv = abs(v - highs(A)[2])
    assert dv <= b * scale(A), (what, dv / scale(A))
    return dv / scale(A)


def certify(A, x, y, v, status, what=""):
    """Both halves with bound(); returns (gap, |v - v_highs|), both relative to scale(A)."""
    b = bound()
    g, dv = certificate(A, x, y, v, status, b, what), value_against_highs(A, v, b, what)
    print(f"{what}: gap {g:.3g}, |v - v_highs| {dv:.3g} (relative; bound {b:.3g})")
    return g, dv


def family_property(family, A, x, y, v, b, what=""):
    """What a sweep family is checked by beyond the certificate."""
    m, n = A.shape
    if family == "saddle":
        assert abs(v - saddle_value(A)) <= b * scale(A), what
    elif family == "constant":
        assert v == A[0, 0], what
    elif family == "diagonal":
        w, value = diagonal_answer(A)
        k = len(w)
        assert abs(v - value) <= b * scale(A), what
        assert np.abs(x[:k] - w).max() <= b * scale(A) and np.abs(y[:k] - w).max() <= b * scale(A), what
        assert not x[k:].any() and not y[k:].any(), what   # the dominated rows and columns
    elif family == "skew":
        assert abs(v) <= b * scale(A), what


# ---- the fp64 range: (name, matrix, k) with the certificate evaluated on matrix * 2**k, which is exact ----
def range_cases():
    big = np.array([[1.0, -1.0], [-1.0, 1.0]])
    tiny = np.random.default_rng(9200).integers(0, 8, (3, 5)) * 5e-324
    return [("1e308", big * 1e308, -1000), ("9e307", big * 9e307, -1000), ("largest", big * np.finfo(np.float64).max, -1000),
            ("normal_64x64_quarter_1e308", np.random.default_rng(9201).standard_normal((64, 64)) * (1e308 / 4), -1000),
            ("subnormal_2x2", np.array([[5e-324, 0.0], [0.0, 5e-324]]), 1074), ("subnormal_3x5", tiny, 1074)]


def certify_range(A, k, x, y, v, status, b, what=""):
    """A huge matrix (k < 0): the certificate on A * 2**k and v * 2**k, so that the check does not overflow.  A subnormal
    one (k > 0): the gap on A * 2**k; v is rounded to the subnormal grid, so only its place in [min A, max A] is checked."""
    assert np.isfinite(v) and A.min() <= v <= A.max(), (what, v)
    return certificate(np.ldexp(A, k), x, y, float(np.ldexp(v, k)) if k < 0 else None, status, b, what)


SCALINGS = (-900, -40, 40, 900)


def scaling_matrices():
    """The matrices whose multiples by 2**k, k in SCALINGS, must give the same x, y and pivots and the value times 2**k."""
    return {"integers_33x17": CASES["integers_33x17"], "normal_64x64": CASES["normal_64x64"], "rps": CASES["rps"],
            "sweep_normal_5x31": sweep_matrix(5, 31, "normal"), "sweep_signs_63x64": sweep_matrix(63, 64, "signs"),
            "sweep_offset_32x33": sweep_matrix(32, 33, "offset")}


# ---- tests/native/nash_lp_host_test.cpp ----
def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "nash_lp_host_test.cpp"), "-o", path])
    return path


def write_matrices(path, solved):
    """Per (matrix, the restatement's answer): rows, cols, pivots, status (int32 x 4); the matrix; x, y and v."""
    with open(path, "wb") as f:
        f.write(np.array([len(solved)], np.int32).tobytes())
        for A, (x, y, v, pivots, status) in solved:
            f.write(np.array([*A.shape, pivots, status], np.int32).tobytes())
            for a in (A, x, y, [v]):
                f.write(np.ascontiguousarray(a, np.float64).tobytes())


def write_cases(path):
    write_matrices(path, [(A, restated(name)) for name, A in CASES.items()])
