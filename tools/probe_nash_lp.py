"""The exact Nash meta-solver on the device (open_spiel_amd.meta_solvers.solve_zero_sum_matrix_games,
PSROSolver(meta_solver="nash_lp")): checks every case of tests/nash_lp_cases.py first (the restatement's bits and the
certificate against HiGHS), then times, as the median of 3 synchronised calls after a warm-up: 1 024 problems of 64x64
and of 8x8 per call (standard normal entries, device pointers) and one problem of each, and 20 PSROSolver iterations on
leduc_poker with "nash_lp" beside "prd" at 1 000 iterations.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time
import numpy as np
import nash_lp_cases as nc
import torch, open_spiel_amd as osa
ms = osa.meta_solvers
ctx = osa.Context(0)
print(f"# tools/probe_nash_lp.py on {torch.cuda.get_device_name(0)}", flush=True)

# ---- the cases ----
worst_gap = worst_value = 0.0
for name, A in nc.CASES.items():
    out = ms.solve_zero_sum_matrix_games(ctx, A[None])
    x, y, v, pivots, status = nc.restated(name)
    assert np.array_equal(out["row"][0], x) and np.array_equal(out["col"][0], y) and out["value"][0] == v and out["pivots"][0] == pivots, name
    g, dv = nc.certify(A, out["row"][0], out["col"][0], out["value"][0], out["status"][0], name)
    worst_gap, worst_value = max(worst_gap, g), max(worst_value, dv)
print(f"{len(nc.CASES)} cases: the restatement's bits; largest relative gap {worst_gap:.3g}, largest relative |v - v_highs| {worst_value:.3g}, "
      f"bound {nc.bound():.3g}", flush=True)

# ---- times ----
def median_of_3(label, call, per=None):
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t = time.time(); call(); torch.cuda.synchronize(); times.append(time.time() - t)
    mid = sorted(times)[1]
    extra = f", {mid / per[0] * 1e6:.4g} us/{per[1]}" if per else ""
    print(f"{label}: median of 3 calls {mid * 1e3:.4g} ms{extra} (all: {' '.join(f'{x * 1e3:.4g}' for x in times)})", flush=True)

B = 1024
for side in (64, 8):
    batch = torch.as_tensor(np.random.default_rng(side).standard_normal((B, side, side)), device=ctx.device)
    for count in (B, 1):
        out = ms.solve_zero_sum_matrix_games(ctx, batch[:count], device=True)
        pivots = out["pivots"].cpu().numpy()
        assert (out["status"].cpu().numpy() == 0).all()
        median_of_3(f"{side}x{side}, {count} problems in one call (device pointers; pivots: mean {pivots.mean():.4g}, most {pivots.max()})",
                    lambda: ms.solve_zero_sum_matrix_games(ctx, batch[:count], device=True), per=(float(pivots.sum()), "pivot"))

game, iters = "leduc_poker", 20
for solver, kwargs in (("nash_lp", None), ("prd", dict(prd_iterations=1000))):
    psro = osa.PSROSolver(ctx, game, meta_solver=solver, meta_solver_kwargs=kwargs)
    psro.iteration(); torch.cuda.synchronize()   # warm-up
    psro = osa.PSROSolver(ctx, game, meta_solver=solver, meta_solver_kwargs=kwargs)
    t = time.time()
    for _ in range(iters):
        psro.iteration()
    torch.cuda.synchronize()
    dt = time.time() - t
    print(f"{game} PSROSolver(meta_solver={solver!r}, {kwargs}): {iters} iterations in {dt * 1e3:.4g} ms, {dt / iters * 1e3:.4g} ms/iteration, "
          f"population {psro.meta_games()[0].shape}, NashConv of the mixture {psro.nash_conv():.6f}", flush=True)
