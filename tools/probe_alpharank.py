"""Alpha-rank on the device (open_spiel_amd.meta_solvers, PSROSolver(meta_solver="alpharank")): checks every case of
tests/golden/alpharank_vectors.npz first (the restatement's bits with infinite alpha and for the sweep, the entrywise
relative bound against the exact pi everywhere), then times, as the median of 3 synchronised calls after a warm-up: one
sweep on 8x8, 32x32, 8x8x8 and 64x64 in both forms of the kernel where they apply, a batch of 1 024 problems of 8x8 in
one call, and PSROSolver(meta_solver="alpharank") iterations on leduc_poker (20) and on 3-player kuhn_poker
(--kuhn3-iterations N, default 10: its K^3 profiles pass the served 4 096 after 16).  --reference also times the
reference's sweep_pi_vs_epsilon on the host for the same shapes (needs the reference tree; --reference-max-profiles N,
default 1 024, skips larger shapes); --reference-only does nothing else.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time
import numpy as np
import alpharank_cases as ac

TIMED = [(88, (8, 8)), (3232, (32, 32)), (888, (8, 8, 8)), (6464, (64, 64))]

def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

def timed_tensors(seed, shape):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(len(shape),) + shape)

def reference_rows():
    import contextlib, io
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_alpharank_vectors as gen
    alpharank = gen.reference_modules()[0]
    limit = option("--reference-max-profiles", 1024)
    for seed, shape in TIMED:
        if int(np.prod(shape)) > limit:
            print(f"{'x'.join(map(str, shape))} reference sweep_pi_vs_epsilon: skipped (more than {limit} profiles)", flush=True)
            continue
        T = list(timed_tensors(seed, shape))
        printed = io.StringIO()
        t = time.time()
        try:
            with contextlib.redirect_stdout(printed):
                _, eps = alpharank.sweep_pi_vs_epsilon(T, return_epsilon=True)
            outcome = f"stopped at eps {eps:.3g}"
        except Exception as e:  # pylint: disable=broad-except
            outcome = f"raised {e!r}"
        dt = time.time() - t
        print(f"{'x'.join(map(str, shape))} reference sweep_pi_vs_epsilon (NumPy / SciPy eig, host, one core): {dt:.4g} s, {outcome}, "
              f"{printed.getvalue().count('Error:')} error-path steps", flush=True)

if "--reference" in sys.argv or "--reference-only" in sys.argv:
    reference_rows()
if "--reference-only" in sys.argv:
    sys.exit(0)

import torch, open_spiel_amd as osa
ms = osa.meta_solvers
ctx = osa.Context(0)
print(f"# tools/probe_alpharank.py on {torch.cuda.get_device_name(0)}", flush=True)

# ---- the goldens ----
golden, restated = ac.load(), ac.restated()
worst = {True: 0.0, False: 0.0}
for c in ac.CASES:
    mode = {ac.FINITE: "finite", ac.INFINITE: "infinite", ac.SWEEP: "sweep"}[c.mode]
    out = ms.solve_alpharank(ctx, ac.tensors(c)[None], mode=mode, m=c.m, alpha=c.alpha, eps=c.eps, min_iters=c.min_iters, max_iters=c.max_iters,
                             single_population=c.single)
    want = restated[c.name]
    assert (out["status"][0], out["iterations"][0], out["eps"][0]) == (want.status, want.iterations, want.eps), c.name
    if c.mode != ac.FINITE:
        assert np.array_equal(out["pi"][0], want.pi) and np.array_equal(out["marginals"][0], want.marginals), c.name
    rel = float(np.max(np.abs(out["pi"][0] - golden[c.name].pi_exact) / golden[c.name].pi_exact))
    assert rel <= ac.bound(c), (c.name, rel)
    worst[c.mode == ac.FINITE] = max(worst[c.mode == ac.FINITE], rel)
print(f"{len(ac.CASES)} recorded cases: the restatement's bits with infinite alpha and for the sweep; worst relative deviation from the exact "
      f"pi: infinite alpha {worst[False]:.3g}, finite alpha {worst[True]:.3g}", flush=True)

# ---- times ----
def median_of_3(label, call, per=None):
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t = time.time(); call(); torch.cuda.synchronize(); times.append(time.time() - t)
    mid = sorted(times)[1]
    extra = f", {mid / per[0] * 1e6:.4g} us/{per[1]}" if per else ""
    print(f"{label}: median of 3 calls {mid * 1e3:.4g} ms{extra} (all: {' '.join(f'{x * 1e3:.4g}' for x in times)})", flush=True)

for seed, shape in TIMED:
    n = int(np.prod(shape))
    T = torch.as_tensor(timed_tensors(seed, shape)[None], device=ctx.device)
    for form in ("lds", "global"):
        if form == "lds" and not ac.fits_lds(n):
            continue
        out = ms.solve_alpharank(ctx, T, form=form, device=True)
        steps = int(out["iterations"][0]) + 1
        if int(out["status"][0]) != 0:
            print(f"{'x'.join(map(str, shape))} sweep, form {form}: status {int(out['status'][0])} after {steps} epsilons", flush=True)
        median_of_3(f"{'x'.join(map(str, shape))} sweep ({steps} epsilons, stops at {float(out['eps'][0]):.3g}), form {form} (device pointers)",
                    lambda: ms.solve_alpharank(ctx, T, form=form, device=True), per=(steps, "epsilon"))
B = 1024
batch = torch.as_tensor(np.stack([timed_tensors(1000 + k, (8, 8)) for k in range(B)]), device=ctx.device)
out = ms.solve_alpharank(ctx, batch, device=True)
print(f"8x8, {B} problems: statuses {np.bincount(out['status'].cpu().numpy()).tolist()}, sweeps of {int(out['iterations'].min()) + 1} to "
      f"{int(out['iterations'].max()) + 1} epsilons", flush=True)
median_of_3(f"8x8 sweep, {B} problems in one call (device pointers)", lambda: ms.solve_alpharank(ctx, batch, device=True), per=(B, "problem"))

for game, iters in (("leduc_poker", 20), ("kuhn_poker(players=3)", option("--kuhn3-iterations", 10))):
    psro = osa.PSROSolver(ctx, game, meta_solver="alpharank")
    psro.iteration(); torch.cuda.synchronize()   # warm-up
    psro = osa.PSROSolver(ctx, game, meta_solver="alpharank")
    t = time.time()
    for _ in range(iters):
        psro.iteration()
    torch.cuda.synchronize()
    dt = time.time() - t
    print(f"{game} PSROSolver(meta_solver='alpharank'): {iters} iterations in {dt * 1e3:.4g} ms, {dt / iters * 1e3:.4g} ms/iteration, "
          f"population {psro.meta_games()[0].shape}, NashConv of the alpha-rank marginals {psro.nash_conv():.6f}", flush=True)
