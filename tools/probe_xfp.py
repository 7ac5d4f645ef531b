"""Extensive-form fictitious play (XFPSolver) on the device: checks the leduc_poker checkpoints of
tests/golden/xfp_vectors.npz first, then times iterations/s on kuhn_poker (fused form, iterate(1000)), leduc_poker and
3-player leduc_poker, each beside CFR-BR — the sibling with the same best-response work — on the same game in the same
session.  --reference also times one iteration of the reference's Python XFPSolver on the host (needs the reference tree).
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import time
import numpy as np

def reference_rows():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_xfp_vectors
    pyspiel, fictitious_play, _, _ = make_xfp_vectors.reference_modules()
    for game, iters in [("kuhn_poker", 20), ("leduc_poker", 3)]:
        solver = fictitious_play.XFPSolver(pyspiel.load_game(game))
        solver.iteration()
        t = time.time()
        for _ in range(iters): solver.iteration()
        dt = (time.time() - t) / iters
        print(f"{game} reference XFPSolver (Python, host, one core) s/iteration {dt:.4f} iterations/s {1 / dt:.2f}", flush=True)

if "--reference" in sys.argv:
    reference_rows()
if "--reference-only" in sys.argv:
    reference_rows()
    sys.exit(0)

import torch, open_spiel_amd as osa
ctx = osa.Context(0)

# ---- the leduc_poker checkpoints ----
with np.load(os.path.join(ROOT, "tests", "golden", "xfp_vectors.npz")) as z:
    keys = bytes(z["leduc_poker/keys"]).decode().split("\n")
    golden, nash = z["leduc_poker/policy"], {t: float(z[f"nash_conv/leduc_poker/{t}"]) for t in (10, 20, 25)}
s = osa.XFPSolver(ctx, "leduc_poker")
where = {k: i for i, k in enumerate(keys)}
order = np.array([where[k] for k in s.tables()["keys"]])
worst = 0.0
for t in range(1, 26):
    s.iteration()
    worst = max(worst, float(np.abs(s.tables()["cur_policy"] - golden[t - 1][order]).max()))
    if t in nash:
        nc = s.nash_conv()
        print(f"leduc_poker XFP T={t} NashConv {nc:.10f} reference {nash[t]:.10f}", flush=True)
        assert abs(nc - nash[t]) <= 1e-9
print(f"leduc_poker XFP 1..25 worst |device - reference| {worst:.3g} kernel {s.last_kernel()}", flush=True)
assert worst <= 1e-12

# ---- rates ----
def rate(game, label, make, step, warm, iters, reps, per_call=False):
    """`reps` timed calls of `iters` iterations each (per_call: one iteration per call), after a warm-up of the same form."""
    solver = make()
    step(solver, warm); torch.cuda.synchronize()
    t = time.time()
    for _ in range(reps):
        if per_call:
            for _ in range(iters): step(solver, 1)
        else:
            step(solver, iters)
    torch.cuda.synchronize(); dt = time.time() - t
    n = iters * reps
    print(f"{game} {label} iterations/s {n / dt:.1f} us/iteration {dt / n * 1e6:.2f} ({reps} x {iters}) kernel {solver.last_kernel()} "
          f"eval {solver.last_eval_kernel()}", flush=True)

xfp = lambda game, **kw: (lambda: osa.XFPSolver(ctx, game, **kw))
cfr = lambda game: (lambda: osa.TabularSolver(ctx, game))
xfp_step = lambda solver, n: solver.iterate(n)
br_step = lambda solver, n: solver.evaluate_and_update_policy_cfr_br(n)
for game, iters, reps in [("kuhn_poker", 1000, 50), ("kuhn_poker(players=3)", 1000, 20), ("leduc_poker", 1000, 5),
                          ("leduc_poker(players=3)", 50, 2)]:
    warm = min(iters, 100)
    rate(game, "XFP iterate(n)", xfp(game), xfp_step, warm, iters, reps)
    if game.startswith("kuhn"):
        rate(game, "XFP iterate(n), general form", xfp(game, general_kernel=True), xfp_step, warm, iters, max(1, reps // 5))
        rate(game, "XFP one iteration per call", xfp(game), xfp_step, warm, iters, max(1, reps // 5), per_call=True)
    rate(game, "CFR-BR iterate(n)", cfr(game), br_step, warm, iters, reps if not game.startswith("kuhn") else max(1, reps // 5))
