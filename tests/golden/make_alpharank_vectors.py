#!/usr/bin/env python3
"""Golden alpha-rank distributions, produced by RUNNING the reference's own open_spiel/python/egt/alpharank.py and
egt/utils.py, imported unmodified from where they lie.  They need NumPy and SciPy; stand-ins go into sys.modules for
`absl`, `pyspiel` (egt/utils.py imports it for helpers that are not on this path) and
open_spiel.python.egt.alpharank_visualizer (matplotlib is not needed).  The marginals come from
psro_v2/utils.get_alpharank_marginals where that module imports with the stand-ins; otherwise they are axis sums of the
reference's pi, and the file says which under `marginals_source`.  Run in the build container (needs the reference tree):

    python tests/golden/make_alpharank_vectors.py [--out FILE]

Output: tests/golden/alpharank_vectors.npz (np.savez_compressed).  The payoff tensors are not stored:
alpharank_cases.tensors() makes them from the kind, the seed and the scale.

  names, kinds, marginals_source
  <case>/shape, <case>/params      alpharank_cases.params_row
  <case>/pi_ref [n]                the reference's pi (compute(), or sweep_pi_vs_epsilon())
  <case>/eps_ref, iterations_ref   the epsilon the reference's sweep returned and its num_iters (0 / the given eps otherwise)
  <case>/entries_ref [n, moves]    the reference's transition matrix at eps_ref, its off-diagonal entries move by move
                                   (alpharank_cases.neighbours names the columns)
  <case>/marginals_ref [sum K]
  <case>/pi_exact [n]              GTH on the reference's own matrix in fractions.Fraction (n <= 64) or numpy.longdouble;
                                   for finite alpha on eta * rho with rho evaluated by mpmath in 50 digits
  <case>/ref_err                   max |pi_ref - pi_exact|
  <case>/exact_only                1: the reference raised or did worse than 1e-12; only pi_exact is kept

The recorder asserts, per case: the reference's sweep printed no "Error:" line; at every sweep step that tests the stop
rule max(|pi - prev| - (1e-8 + 1e-5 |prev|)) is at least 1e-12 away from zero, for the reference's pis and for exact ones
(GTH in longdouble; Fraction at the last step where n <= 64); no payoff pair lies within 1e-9 (relative) of the tie rule's
boundary; for finite alpha every nonzero |u| >= 1e-3; ref_err <= 1e-12 unless the case is declared exact-only, and a case
declared exact-only does fail in the reference.  It also measures eps_rho, the relative error of the restated rho
against the 50-digit one, and prints how far the restatement lies from the exact pi (relative) and from the reference.
"""
import argparse
import contextlib
import fractions
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alpharank_cases as ac  # noqa: E402

F = fractions.Fraction


def reference_modules():
    if not os.path.isdir(os.path.join(REFERENCE, "open_spiel", "python", "egt")):
        raise RuntimeError("needs the reference sources")
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    if "absl" not in sys.modules:
        import logging
        absl = types.ModuleType("absl")
        absl.logging = logging
        sys.modules["absl"], sys.modules["absl.logging"] = absl, logging
    sys.modules["pyspiel"] = types.ModuleType("pyspiel")
    sys.modules["open_spiel.python.egt.alpharank_visualizer"] = types.ModuleType("open_spiel.python.egt.alpharank_visualizer")
    from open_spiel.python.egt import alpharank
    try:
        from open_spiel.python.algorithms.psro_v2 import utils as psro_utils
        get_marginals, source = psro_utils.get_alpharank_marginals, "psro_v2/utils.get_alpharank_marginals"
    except Exception as e:  # pylint: disable=broad-except
        print("psro_v2/utils does not import with the stand-ins:", repr(e))
        get_marginals, source = None, "axis sums of the reference's pi"
    return alpharank, get_marginals, source


def tables_of(case):
    T = ac.tensors(case)
    return [T[0]] if case.single else list(T)


def reference_matrix(alpharank, case, eps):
    tables = tables_of(case)
    if case.single:
        c, _ = alpharank._get_singlepop_transition_matrix(tables[0], False, case.m, case.alpha, False, True, None,
                                                          use_inf_alpha=case.mode != ac.FINITE, inf_alpha_eps=eps)
    else:
        c, _ = alpharank._get_multipop_transition_matrix(tables, False, case.m, case.alpha,
                                                         use_inf_alpha=case.mode != ac.FINITE, inf_alpha_eps=eps)
    return c


def gth_exact(c):
    """GTH in rational arithmetic on the off-diagonals of c (floats are taken exactly, Fractions as they are)."""
    n = len(c)
    a = [[F(c[i][j]) for j in range(n)] for i in range(n)]
    for k in range(n - 1, 0, -1):
        s = sum(a[k][:k])
        rk = a[k]
        for i in range(k):
            q = a[i][k] / s
            a[i][k] = q
            if q:
                ri = a[i]
                for j in range(k):
                    if rk[j]:
                        ri[j] += q * rk[j]
    x = [F(1)] + [F(0)] * (n - 1)
    for k in range(1, n):
        x[k] = sum(x[i] * a[i][k] for i in range(k))
    total = sum(x)
    return [v / total for v in x]


def gth_longdouble(c):
    a = np.array(c, np.longdouble)
    n = len(a)
    for k in range(n - 1, 0, -1):
        s = a[k, :k].sum()
        a[:k, k] /= s
        a[:k, :k] += a[:k, k][:, None] * a[k, :k][None, :]
    x = np.zeros(n, np.longdouble)
    x[0] = 1
    for k in range(1, n):
        x[k] = (x[:k] * a[:k, k]).sum()
    return x / x.sum()


def exact_pi(c):
    """(pi as float64, pi as Fractions or longdoubles)."""
    if len(c) <= 64:
        pi = gth_exact(c)
        return np.array([float(v) for v in pi]), pi
    pi = gth_longdouble(c)
    return pi.astype(np.float64), pi


def exact_finite_matrix(case):
    """eta * rho with rho in 50 digits, as Fractions; and the largest relative error of the restated rho."""
    import mpmath
    mpmath.mp.dps = 50
    T = ac.tensors(case)
    cols, at_col, at_row = ac.neighbours(case.shape, case.single)
    flat = T.reshape(-1)
    n, moves = cols.shape
    restated = ac.rho(flat[at_col], flat[at_row], case.alpha, case.m)
    c = [[F(0)] * n for _ in range(n)]
    worst = 0.0
    for i in range(n):
        for mv in range(moves):
            u = F(case.alpha) * (F(float(flat[at_col[i, mv]])) - F(float(flat[at_row[i, mv]])))
            u_float = case.alpha * (flat[at_col[i, mv]] - flat[at_row[i, mv]])
            if abs(u_float) <= 1e-14:
                r = F(1, case.m)
            else:
                assert abs(u_float) >= 1e-3, f"{case.name}: |u| = {abs(u_float):.3g} < 1e-3: replace the seed"
                um = mpmath.mpf(u.numerator) / mpmath.mpf(u.denominator)
                value = (1 - mpmath.exp(-um)) / (1 - mpmath.exp(-case.m * um))
                sign, man, exp, _ = value._mpf_
                r = F(-int(man) if sign else int(man)) * F(2) ** int(exp)
            if r > F(1, 10 ** 300):   # (a rho that underflows is 0 by the header's rule)
                worst = max(worst, abs(float((F(float(restated[i, mv])) - r) / r)))
            c[i][int(cols[i, mv])] = r / moves
    return c, worst


def margin(pi, prev):
    return float(np.max(np.abs(pi - prev) - (1e-8 + 1e-5 * np.abs(prev))))


def check_ties(case):
    T = ac.tensors(case)
    _, at_col, at_row = ac.neighbours(case.shape, case.single)
    flat = T.reshape(-1)
    pc, pr = flat[at_col], flat[at_row]
    gap, limit = np.abs(pc - pr), 1e-14 + 1e-5 * np.abs(pr)
    near = np.abs(gap - limit) <= 1e-9 * np.maximum(limit, 1e-300)
    assert not near.any(), f"{case.name}: a payoff pair lies on the tie rule's boundary"


def record(case, modules, out, stats):
    alpharank, get_marginals, _ = modules
    check_ties(case)
    tables = tables_of(case)
    name = case.name
    history = []
    mine = ac.solve_case(case, history=history)
    assert mine.status == ac.OK, f"{name}: the restatement's status is {mine.status}"
    failed, pi_ref, eps_ref, iterations_ref = None, None, case.eps if case.mode == ac.INFINITE else 0.0, 0
    printed = io.StringIO()
    try:
        with contextlib.redirect_stdout(printed):
            if case.mode == ac.SWEEP:
                steps = []
                genuine = alpharank.compute

                def recording(*args, **kwargs):
                    result = genuine(*args, **kwargs)
                    steps.append((kwargs["inf_alpha_eps"], np.array(result[2], np.float64)))
                    return result
                alpharank.compute = recording
                try:
                    pi_ref, eps_ref = alpharank.sweep_pi_vs_epsilon(tables, warm_start_epsilon=case.eps or None, return_epsilon=True,
                                                                    min_iters=case.min_iters, max_iters=case.max_iters)
                finally:
                    alpharank.compute = genuine
                iterations_ref = len(steps) - 1
            else:
                pi_ref = alpharank.compute(tables, m=case.m, alpha=case.alpha, use_inf_alpha=case.mode == ac.INFINITE,
                                           inf_alpha_eps=case.eps)[2]
    except (ValueError, RuntimeError) as e:
        failed = repr(e)
    assert "Error:" not in printed.getvalue(), f"{name}: the reference's sweep took its error path"
    if case.mode == ac.SWEEP:
        assert failed is None, f"{name}: {failed}"
        assert eps_ref == mine.eps and iterations_ref == mine.iterations, \
            f"{name}: the reference stopped at {eps_ref} ({iterations_ref}), the restatement at {mine.eps} ({mine.iterations})"
        assert [e for e, _ in steps] == [e for e, _ in history]
        exact_steps = {}
        for t in range(case.min_iters + 1, len(steps)):
            for label, seq in (("reference", [p for _, p in steps]), ("restatement", [p for _, p in history])):
                g = margin(seq[t], seq[t - 1])
                assert abs(g) >= 1e-12, f"{name}: the {label}'s stop margin at step {t} is {g:.3g}"
                assert (g <= 0) == (t == len(steps) - 1), f"{name}: {label} step {t} margin {g:.3g}"
            for k in (t - 1, t):
                if k not in exact_steps:
                    exact_steps[k] = gth_longdouble(reference_matrix(alpharank, case, steps[k][0])).astype(np.float64)
            g = margin(exact_steps[t], exact_steps[t - 1])
            assert abs(g) >= 1e-12 and (g <= 0) == (t == len(steps) - 1), f"{name}: the exact stop margin at step {t} is {g:.3g}"
    # the exact pi
    if case.mode == ac.FINITE:
        c_exact, eps_rho = exact_finite_matrix(case)
        stats["eps_rho"] = max(stats["eps_rho"], eps_rho)
        pi_exact, _ = exact_pi(c_exact)
        c_ref = reference_matrix(alpharank, case, 0.0)
    else:
        c_ref = reference_matrix(alpharank, case, eps_ref)
        pi_exact, _ = exact_pi(c_ref)
    cols, values = ac.entries(ac.tensors(case), case.single, case.mode, eps_ref, case.alpha, case.m)
    n = cols.shape[0]
    entries_ref = c_ref[np.arange(n)[:, None], cols] if cols.shape[1] else np.zeros((n, 0))
    if case.mode != ac.FINITE:
        assert np.array_equal(entries_ref, values), f"{name}: the restated entries are not the reference's bits"
        off = c_ref.copy()
        np.fill_diagonal(off, 0.0)
        assert np.array_equal(off, ac.dense(cols, values)), f"{name}: the reference has entries elsewhere"
    ref_err = float("nan") if failed else float(np.max(np.abs(pi_ref - pi_exact)))
    does_worse = failed is not None or not ref_err <= 1e-12
    assert does_worse == case.exact_only, f"{name}: exact_only = {case.exact_only}, but the reference: {failed or ref_err}"
    rel = float(np.max(np.abs(mine.pi - pi_exact) / pi_exact))
    stats["rel"] = max(stats["rel"], rel)
    stats["rel/bound"] = max(stats["rel/bound"], rel / ac.bound(case) if n > 1 else 0.0)
    assert rel <= ac.bound(case), f"{name}: the restatement lies {rel:.3g} (relative) from the exact pi, the bound is {ac.bound(case):.3g}"
    if not does_worse:
        stats["vs_ref"] = max(stats["vs_ref"], float(np.max(np.abs(mine.pi - pi_ref))))
        stats["ref_err"] = max(stats["ref_err"], ref_err)
    print(f"{name}: n = {n}, eps {eps_ref:.3g} after {iterations_ref} iterations, ref_err {ref_err:.3g}, restatement vs exact "
          f"{rel:.3g} relative (bound {ac.bound(case):.3g})" + (f", the reference: {failed}" if failed else ""), flush=True)
    out[f"{name}/shape"] = np.array(case.shape, np.int32)
    out[f"{name}/params"] = ac.params_row(case)
    out[f"{name}/eps_ref"] = np.float64(eps_ref)
    out[f"{name}/iterations_ref"] = np.int32(iterations_ref)
    out[f"{name}/pi_exact"] = pi_exact
    out[f"{name}/ref_err"] = np.float64(ref_err)
    out[f"{name}/exact_only"] = np.int32(does_worse)
    if not does_worse:
        pi_ref = np.asarray(pi_ref, np.float64)
        out[f"{name}/pi_ref"] = pi_ref
        out[f"{name}/entries_ref"] = entries_ref
        if get_marginals is not None:
            marg = get_marginals(tables, pi_ref)
            marg = np.asarray(marg, np.float64) if case.single else np.concatenate([np.asarray(x, np.float64) for x in marg])
        else:
            marg = pi_ref.copy() if case.single else np.concatenate(
                [pi_ref.reshape(case.shape).sum(axis=tuple(q for q in range(len(case.shape)) if q != p)) for p in range(len(case.shape))])
        out[f"{name}/marginals_ref"] = marg


def main(path=None, only=None):
    modules = reference_modules()
    path = path or os.path.join(ROOT, "tests", "golden", "alpharank_vectors.npz")
    out = {"names": np.frombuffer("\n".join(c.name for c in ac.CASES).encode(), np.uint8),
           "kinds": np.frombuffer("\n".join(c.kind for c in ac.CASES).encode(), np.uint8),
           "marginals_source": np.frombuffer(modules[2].encode(), np.uint8)}
    stats = dict.fromkeys(("eps_rho", "rel", "rel/bound", "vs_ref", "ref_err"), 0.0)
    failures = []
    for c in ac.CASES:
        if only and c.name not in only:
            continue
        try:
            record(c, modules, out, stats)
        except AssertionError as e:
            failures.append(str(e))
            print("REFUSED", e, flush=True)
    print("marginals:", modules[2])
    print("measured: eps_rho {eps_rho:.3g}; restatement vs exact {rel:.3g} relative ({rel/bound:.3g} of the bound); restatement vs "
          "reference {vs_ref:.3g}; largest ref_err {ref_err:.3g}".format(**stats))
    if failures:
        raise SystemExit(f"{len(failures)} cases refused: replace their seeds")
    if not only:
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    main(a.out, a.only)
