"""Magnetic mirror descent (MMDSolver) on the device: checks every run of tests/golden/mmd_vectors.npz first (x, avg_x,
pi, the gap: within 1e-12 of the reference's own mmd_dilated.py), then times iterations/s on kuhn_poker (resident form,
iterate(1000)), solver-iterations/s over 16 384 kuhn_poker replicas with distinct (alpha, stepsize), and iterations/s on
leduc_poker in both forms beside plain CFR on the same game in the same session.  --reference also times the reference's
Python MMDDilatedEnt on the host (needs the reference tree); --reference-only does nothing else.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time
import numpy as np

def reference_rows():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_mmd_vectors
    pyspiel, mmd_dilated, _ = make_mmd_vectors.reference_modules()
    for game, alpha, iters in [("kuhn_poker", 0.1, 200), ("leduc_poker", 0.05, 5)]:
        solver = mmd_dilated.MMDDilatedEnt(pyspiel.load_game(game), alpha)
        solver.update_sequences()
        t = time.time()
        for _ in range(iters): solver.update_sequences()
        dt = (time.time() - t) / iters
        print(f"{game} reference MMDDilatedEnt (Python, host, one core) s/iteration {dt:.4f} iterations/s {1 / dt:.2f}", flush=True)

if "--reference" in sys.argv or "--reference-only" in sys.argv:
    reference_rows()
if "--reference-only" in sys.argv:
    sys.exit(0)

import torch, open_spiel_amd as osa
import mmd_cases
ctx = osa.Context(0)

# ---- the goldens ----
v = mmd_cases.load()
for run in mmd_cases.run_names(v):
    game = bytes(v[f"{run}/game"]).decode()
    for kw in ({}, dict(general_kernel=True)):
        s = osa.MMDSolver(ctx, game, float(v[f"{run}/alpha"][0]), float(v[f"{run}/stepsize"][0]), **kw)
        where = {k: i for i, k in enumerate(mmd_cases.keys_of(v, game))}
        back = np.argsort(np.array([where[k] for k in s.tables()["keys"]]))
        worst = 0.0
        for c in range(len(v[f"{run}/t"])):
            alpha = float(v[f"{run}/alpha"][c])
            s.set_params(alpha, float(v[f"{run}/stepsize"][c]))
            s.iterate(int(v[f"{run}/iters"][c]))
            got = dict(x=s.current_sequences(), avg_x=s.get_avg_sequences(), pi=s.tables()["cur_policy"])
            worst = max([worst] + [float(np.abs(t[back] - v[f"{run}/{n}"][c]).max()) for n, t in got.items()])
            if alpha > 0:
                worst = max(worst, abs(s.get_gap() - v[f"{run}/gap"][c]))
        print(f"{run} {s.last_kernel()} t={s.iteration} worst |device - reference| {worst:.3g} NashConv {s.nash_conv():.10f} "
              f"reference {v[f'{run}/nash_conv'][-1]:.10f}", flush=True)
        assert worst <= mmd_cases.TOLERANCE

# ---- rates ----
def rate(game, label, make, step, warm, iters, reps, scale=1):
    """`reps` timed calls of `iters` iterations each, after a warm-up call of the same form."""
    solver = make()
    step(solver, warm); torch.cuda.synchronize()
    t = time.time()
    for _ in range(reps): step(solver, iters)
    torch.cuda.synchronize(); dt = time.time() - t
    n = iters * reps * scale
    print(f"{game} {label} iterations/s {n / dt:.4g} us/iteration {dt / n * 1e6:.4g} ({reps} x {iters}{' x %d replicas' % scale if scale > 1 else ''}) "
          f"kernel {solver.last_kernel()}", flush=True)

mmd_step = lambda solver, n: solver.iterate(n)
cfr_step = lambda solver, n: solver.evaluate_and_update_policy(n)
B = 16384
rate("kuhn_poker", "MMD iterate(n)", lambda: osa.MMDSolver(ctx, "kuhn_poker", 0.1), mmd_step, 100, 1000, 20)
rate("kuhn_poker", "MMD iterate(n), general form", lambda: osa.MMDSolver(ctx, "kuhn_poker", 0.1, general_kernel=True), mmd_step, 100, 1000, 2)
rate("kuhn_poker", "MMD sweep, solver-iterations/s", lambda: osa.MMDSolver(ctx, "kuhn_poker", np.linspace(0.0, 2.0, B), np.linspace(0.1, 1.0, B), replicas=B),
     mmd_step, 100, 1000, 5, scale=B)
rate("kuhn_poker", "CFR iterate(n)", lambda: osa.TabularSolver(ctx, "kuhn_poker"), cfr_step, 100, 1000, 20)
rate("leduc_poker", "MMD iterate(n)", lambda: osa.MMDSolver(ctx, "leduc_poker", 0.05), mmd_step, 100, 1000, 5)
rate("leduc_poker", "MMD iterate(n), general form", lambda: osa.MMDSolver(ctx, "leduc_poker", 0.05, general_kernel=True), mmd_step, 100, 1000, 2)
rate("leduc_poker", "CFR iterate(n)", lambda: osa.TabularSolver(ctx, "leduc_poker"), cfr_step, 100, 1000, 5)
