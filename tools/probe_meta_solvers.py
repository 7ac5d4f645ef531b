"""PSRO's meta-solvers on the device (open_spiel_amd.meta_solvers, PSROSolver(meta_solver="prd")): checks every case of
tests/golden/meta_solver_vectors.npz first (the restatement's bits, within 1e-12 of the reference's own
projected_replicator_dynamics.py / regret_matching.py), then times, as the median of 3 synchronised calls after a
warm-up: one PRD solve at the reference's defaults (10^5 iterations) on 8x8, 32x32 and 8x8x8 in both forms of the kernel,
a batch of 1 024 problems of 8x8, and 20 PSROSolver(meta_solver="prd") iterations on leduc_poker.  --reference also times
the reference's NumPy PRD on the host for the same shapes (needs the reference tree; --reference-iterations N, default
2 000, scaled to 10^5); --reference-only does nothing else.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time
import numpy as np
import meta_solver_cases as mc

DEFAULT_ITERATIONS = int(1e5)
TIMED = [("general", 88, (8, 8)), ("general", 3232, (32, 32)), ("general", 888, (8, 8, 8))]

def reference_rows():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_meta_solver_vectors as gen
    prd, _ = gen.reference_modules()
    n = int(sys.argv[sys.argv.index("--reference-iterations") + 1]) if "--reference-iterations" in sys.argv else 2000
    for kind, seed, shape in TIMED:
        T = list(mc.tensors(kind, seed, shape))
        prd.projected_replicator_dynamics(T, prd_iterations=10)
        t = time.time()
        prd.projected_replicator_dynamics(T, prd_iterations=n)
        per = (time.time() - t) / n
        print(f"{'x'.join(map(str, shape))} reference projected_replicator_dynamics (NumPy, host, one core): {per * 1e6:.4g} us/iteration, "
              f"{per * DEFAULT_ITERATIONS:.4g} s at its default of {DEFAULT_ITERATIONS} iterations", flush=True)

if "--reference" in sys.argv or "--reference-only" in sys.argv:
    reference_rows()
if "--reference-only" in sys.argv:
    sys.exit(0)

import torch, open_spiel_amd as osa
ms = osa.meta_solvers
ctx = osa.Context(0)
print(f"# tools/probe_meta_solvers.py on {torch.cuda.get_device_name(0)}", flush=True)

# ---- the goldens ----
golden, restated = mc.load(), mc.restated()
worst = {mc.PRD: 0.0, mc.RM: 0.0}
for c in mc.CASES:
    init = mc.initial_strategies(c)
    average, last = ms.solve_meta_games(ctx, mc.tensors(c.kind, c.seed, c.shape)[None], "prd" if c.method == mc.PRD else "rm",
                                        iterations=c.iterations, dt=c.dt, gamma=c.gamma, window=c.window, use_approx=c.use_approx,
                                        initial=None if init is None else init[None], return_last=True)
    assert np.array_equal(average[0], restated[c.name][0]) and np.array_equal(last[0], restated[c.name][1]), c.name
    worst[c.method] = max(worst[c.method], float(np.abs(average[0] - golden[c.name]).max()))
print(f"{len(mc.CASES)} recorded cases: the restatement's bits; worst |device - reference| prd {worst[mc.PRD]:.3g}, rm {worst[mc.RM]:.3g}", flush=True)
assert max(worst.values()) <= mc.TOLERANCE

# ---- times ----
def median_of_3(label, call, per=None):
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t = time.time(); call(); torch.cuda.synchronize(); times.append(time.time() - t)
    mid = sorted(times)[1]
    extra = f", {mid / per[0] * 1e6:.4g} us/{per[1]}" if per else ""
    print(f"{label}: median of 3 calls {mid * 1e3:.4g} ms{extra} (all: {' '.join(f'{x * 1e3:.4g}' for x in times)})", flush=True)

for kind, seed, shape in TIMED:
    T = torch.as_tensor(mc.tensors(kind, seed, shape)[None], device=ctx.device)
    for form in ("lds", "global"):
        median_of_3(f"{'x'.join(map(str, shape))} PRD, {DEFAULT_ITERATIONS} iterations, form {form} (device pointers)",
                    lambda: ms.solve_meta_games(ctx, T, "prd", iterations=DEFAULT_ITERATIONS, form=form, device=True),
                    per=(DEFAULT_ITERATIONS, "iteration"))
B = 1024
batch = torch.as_tensor(np.stack([mc.tensors("general", 1000 + k, (8, 8)) for k in range(B)]), device=ctx.device)
median_of_3(f"8x8 PRD, {B} problems in one call, {DEFAULT_ITERATIONS} iterations each (device pointers)",
            lambda: ms.solve_meta_games(ctx, batch, "prd", iterations=DEFAULT_ITERATIONS, device=True), per=(B, "problem"))

game, iters = "leduc_poker", 20
for label, kwargs in (("prd_iterations=1000", dict(prd_iterations=1000)), ("the reference's defaults, 10^5 iterations", {})):
    psro = osa.PSROSolver(ctx, game, meta_solver="prd", meta_solver_kwargs=kwargs)
    psro.iteration(); torch.cuda.synchronize()   # warm-up
    psro = osa.PSROSolver(ctx, game, meta_solver="prd", meta_solver_kwargs=kwargs)
    t = time.time()
    for _ in range(iters):
        psro.iteration()
    torch.cuda.synchronize()
    dt = time.time() - t
    print(f"{game} PSROSolver(meta_solver='prd', {label}): {iters} iterations in {dt * 1e3:.4g} ms, {dt / iters * 1e3:.4g} ms/iteration, "
          f"population {psro.meta_games()[0].shape}, NashConv of the PRD mixture {psro.nash_conv():.6f}", flush=True)
