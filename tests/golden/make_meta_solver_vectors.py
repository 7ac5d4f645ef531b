#!/usr/bin/env python3
"""Golden meta-strategies of PSRO's meta-solvers, produced by RUNNING the reference's own
open_spiel/python/algorithms/projected_replicator_dynamics.py and regret_matching.py (with nfg_utils.py), imported
unmodified from where they lie; they need only NumPy.  Run in the build container (needs the reference tree):

    python tests/golden/make_meta_solver_vectors.py [--psro-games FILE]

Output: tests/golden/meta_solver_vectors.npz (np.savez_compressed).  The payoff tensors are not stored:
meta_solver_cases.tensors() makes them from the kind and the seed, meta_solver_cases.initial_strategies() the seeded
initial strategies.

  names, kinds                 newline-joined case names and tensor kinds, in the order of meta_solver_cases.CASES
  <case>/shape [P] int32
  <case>/params [8]            method (0 prd, 1 rm), iterations, dt, gamma, window (0: None), use_approx, seeded initial
                               strategies (0 / 1), seed
  <case>/average [sum K]       the reference's averaged strategies, player after player
  psro/<game>/it<k>/tensors    the payoff tensors [P, K_0 .. K_{P-1}] that PSROSolver(ctx, game, meta_solver="prd",
                               meta_solver_kwargs=dict(prd_iterations=2000)) handed its meta-solver in iteration k = 0 .. 3
                               (kuhn_poker with 2 and 3 players).  They come from a device run, which this recorder cannot
                               make: --psro-games names an .npz of them (keys <game>/it<k>, np.stack(solver.meta_games())
                               before every iteration()); without the option the entries of the present golden file are kept.
  psro/<game>/it<k>/average    the reference's projected_replicator_dynamics(tensors, prd_iterations=2000), flat

The recorder also runs meta_solver_cases.solve(), the restatement of the device's order of summation, and prints how far
it lies from the reference.  Regret matching amplifies a rounding difference once it flips the sign of a regret, so a
regret-matching case is refused here unless the two agree within meta_solver_cases.RM_RECORDING_BOUND (1e-13): shorten
its horizon instead.

Consumers: tests/test_meta_solver_goldens.py, tests/test_meta_solver_native.py (CPU), tests/test_z25_gpu_meta_solvers.py
(the HIP engine).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meta_solver_cases as mc  # noqa: E402


def reference_modules():
    if not os.path.isdir(os.path.join(REFERENCE, "open_spiel", "python", "algorithms")):
        raise RuntimeError("needs the reference sources")
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from open_spiel.python.algorithms import projected_replicator_dynamics, regret_matching
    return projected_replicator_dynamics, regret_matching


def reference_solve(modules, case):
    """The reference's answer for a case, flat."""
    prd, rm = modules
    T = mc.tensors(case.kind, case.seed, case.shape)
    init = mc.initial_strategies(case)
    init = None if init is None else mc.split(init, case.shape)
    if case.method == mc.PRD:
        out = prd.projected_replicator_dynamics(list(T), prd_initial_strategies=init, prd_iterations=case.iterations, prd_dt=case.dt,
                                                prd_gamma=case.gamma, average_over_last_n_strategies=case.window,
                                                use_approx=case.use_approx)
    else:
        out = rm.regret_matching(list(T), initial_strategies=init, iterations=case.iterations, gamma=case.gamma,
                                 average_over_last_n_strategies=case.window)
    return np.concatenate([np.asarray(x, np.float64) for x in out])


def psro_entries(modules, path, games_file):
    """The psro/ arrays: recorded anew from `games_file`, or carried over from the golden file at `path`."""
    out = {}
    if games_file is None:
        with np.load(path) as z:
            return {k: z[k] for k in z.files if k.startswith("psro/")}
    with np.load(games_file) as z:
        for g in mc.PSRO_GAMES:
            for k in range(mc.PSRO_ITERATIONS):
                T = np.asarray(z[f"{g}/it{k}"], np.float64)
                want = np.concatenate(modules[0].projected_replicator_dynamics(list(T), prd_iterations=mc.PSRO_PRD_ITERATIONS))
                dev = float(np.abs(mc.solve(T, mc.PRD, mc.PSRO_PRD_ITERATIONS)[0] - want).max())
                print(f"psro/{g}/it{k} {T.shape[1:]}: restatement within {dev:.3g} of the reference", flush=True)
                out[f"psro/{g}/it{k}/tensors"], out[f"psro/{g}/it{k}/average"] = T, want
    return out


def main(path=None, psro_games=None):
    modules = reference_modules()
    path = path or os.path.join(ROOT, "tests", "golden", "meta_solver_vectors.npz")
    psro = psro_entries(modules, path, psro_games)
    out = {"names": np.frombuffer("\n".join(c.name for c in mc.CASES).encode(), np.uint8),
           "kinds": np.frombuffer("\n".join(c.kind for c in mc.CASES).encode(), np.uint8)}
    worst = {mc.PRD: 0.0, mc.RM: 0.0}
    for c in mc.CASES:
        want = reference_solve(modules, c)
        dev = float(np.abs(mc.solve_case(c)[0] - want).max())
        worst[c.method] = max(worst[c.method], dev)
        print(f"{c.name}: restatement within {dev:.3g} of the reference", flush=True)
        if c.method == mc.RM and not dev <= mc.RM_RECORDING_BOUND:
            raise SystemExit(f"{c.name}: regret matching is not stable at {c.iterations} iterations; record a shorter horizon")
        out[f"{c.name}/shape"] = np.array(c.shape, np.int32)
        out[f"{c.name}/params"] = mc.params_row(c)
        out[f"{c.name}/average"] = want
    out.update(psro)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays; worst deviation of the restatement: prd",
          f"{worst[mc.PRD]:.3g}, rm {worst[mc.RM]:.3g}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--psro-games")
    a = ap.parse_args()
    main(a.out, a.psro_games)
