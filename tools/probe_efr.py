"""Extensive-form regret minimization (EFRSolver) on the device: checks every run of tests/golden/efr_vectors.npz first
(R, current, cumulative and average policy within efr_cases.TOLERANCE of the reference's own efr.py, both kernel forms),
then times iterations/s on kuhn_poker, leduc_poker and leduc_poker(players=3) per deviation set in both forms: per row a
warm-up call, then the median of 3 calls that each end in a device synchronise.  --reference also times the reference's
Python EFRSolver on the host (needs the reference tree); --reference-only does nothing else.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time
import numpy as np

SETS = ["blind cf", "informed cf", "bps", "cfps", "csps", "tips", "bhv"]

def reference_rows():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_efr_vectors
    pyspiel, efr, _ = make_efr_vectors.reference_modules()
    for game, sets, iters in [("kuhn_poker", SETS, 20), ("leduc_poker", ["blind cf", "tips", "bhv"], 2)]:
        for name in sets:
            solver = efr.EFRSolver(pyspiel.load_game(game), name)
            solver.evaluate_and_update_policy()
            t = time.time()
            for _ in range(iters): solver.evaluate_and_update_policy()
            dt = (time.time() - t) / iters
            print(f"{game} | {name} reference EFRSolver (Python, host, one core) s/iteration {dt:.4g} iterations/s {1 / dt:.4g}", flush=True)

if "--reference" in sys.argv or "--reference-only" in sys.argv:
    reference_rows()
if "--reference-only" in sys.argv:
    sys.exit(0)

import torch, open_spiel_amd as osa
import efr_cases as ec
ctx = osa.Context(0)

# ---- the goldens ----
v = ec.load()
solvers = {}
for r, game, name in ec.runs(v):
    for form in ("resident", "levels"):
        s = solvers.setdefault(game, osa.EFRSolver(ctx, game, name, form))
        s.set_deviations(name, form)
        dev = s.tables()
        where = {k: i for i, k in enumerate(dev["keys"])}
        rows = np.array([where[k] for k in ec.keys_of(v, r)])
        off = s.deviations()["offsets"]
        worst, done = 0.0, 0
        for c, upto in enumerate(v[f"r{r}/checkpoints"]):
            s.evaluate_and_update_policy(int(upto) - done)
            done = int(upto)
            t = s.tables()
            R = np.concatenate([s.regret_state()[off[i]:off[i + 1]] for i in rows])
            worst = max(worst, float(np.abs(R - v[f"r{r}/R"][c]).max()),
                        *[float(np.abs(t[n][rows] - ec.by_legal(v, r, v[f"r{r}/{k}"][c])).max())
                          for n, k in (("cur_policy", "cur"), ("cum_policy", "cum"), ("avg_policy", "avg"))])
        print(f"{game} | {name} {s.last_kernel()} t={s.iteration} {s.num_deviations} deviations worst |device - reference| {worst:.3g}", flush=True)
        assert worst <= ec.TOLERANCE

# ---- rates ----
def rate(game, solver, name, form):
    try:
        solver.set_deviations(name, form)
    except osa.OsgError as e:
        print(f"{game} | {name} [{form}] refused: {e}", flush=True)
        return
    solver.evaluate_and_update_policy(1); torch.cuda.synchronize()
    t = time.time(); solver.evaluate_and_update_policy(1); torch.cuda.synchronize()
    iters = int(max(1, min(2000, 0.3 / max(time.time() - t, 1e-6))))
    solver.evaluate_and_update_policy(iters); torch.cuda.synchronize()   # the warm-up call of the timed shape
    times = []
    for _ in range(3):
        t = time.time(); solver.evaluate_and_update_policy(iters); torch.cuda.synchronize()
        times.append(time.time() - t)
    dt = float(np.median(times)) / iters
    print(f"{game} | {name} [{form}] {solver.num_deviations} deviations (at most {solver.max_deviations} per infostate, L {solver.memory}) "
          f"iterations/s {1 / dt:.4g} ms/iteration {dt * 1e3:.4g} (median of 3 x {iters}, spread {min(times) / iters * 1e3:.4g} .. "
          f"{max(times) / iters * 1e3:.4g} ms) kernel {solver.last_kernel()}", flush=True)

for game in ("kuhn_poker", "leduc_poker", "leduc_poker(players=3)"):
    t = time.time()
    solver = solvers.get(game) or osa.EFRSolver(ctx, game, "blind cf")
    print(f"{game}: {solver.num_histories} histories, {solver.num_infostates} infostates (solver made in {time.time() - t:.1f} s)", flush=True)
    # (3-player leduc: the sets whose tables stay in the millions of deviations; the others are not timed here)
    for name in (SETS if solver.num_histories <= 65536 else ["blind cf", "informed cf", "tips"]):
        for form in ("resident", "levels"):
            if form == "resident" and solver.num_histories > 65536:
                continue   # (one workgroup over 1.8 million histories: the levels form is the one that serves it)
            rate(game, solver, name, form)
