"""Payoff tensors, policy aggregation and PSRO on the device (TabularSolver.payoff_tensors / aggregate_policies,
PSROSolver): checks every case of tests/golden/population_vectors.npz first (every return and every aggregated cell
within 1e-12 of the reference's own expected_game_score.py / policy_aggregator.py), then times, as the median of 3
synchronised calls after a warm-up: payoff_tensors for K = 16 on leduc_poker and K = 8 on leduc_poker(players=3), one
aggregate_policies on each, and 20 PSROSolver iterations on leduc_poker, with NashConv per iteration beside XFPSolver's
(uniform-weight PSRO is fictitious play with kept oracles: the curves lie together until an argmax tie parts them;
printed, not asserted).  --reference also times the reference's policy_value and PolicyAggregator on the host (needs the
reference tree); --reference-only does nothing else.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time
import numpy as np
import population_cases as pc

TIMED = [("leduc_poker", 16), (pc.LARGE_GAME, 8)]

def reference_rows():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_population_vectors as gen
    gen.MODULES = gen.reference_modules()
    av = gen.avc.load()
    for game_string, K in TIMED:
        gen.prepare(game_string, int(av["seed"]), av)
        g = gen.GAMES[game_string]
        P, kinds = g["P"], len(g["kinds"])
        t = time.time()
        gen.run(("returns", game_string, len(g["profiles"]) - 1))
        walk = time.time() - t
        t = time.time()
        gen.run(("aggregate", game_string, next(iter(g["weights"])), 0))
        agg = time.time() - t
        print(f"{game_string} reference policy_value (Python, host, one core) s/profile {walk:.4g}: K = {K} would take {walk * K ** P:.4g} s; "
              f"PolicyAggregator of {kinds} tables s/player {agg:.4g}: all {P} players {agg * P:.4g} s", flush=True)

if "--reference" in sys.argv or "--reference-only" in sys.argv:
    reference_rows()
if "--reference-only" in sys.argv:
    sys.exit(0)

import torch, open_spiel_amd as osa
import action_value_cases as avc
ctx = osa.Context(0)
print(f"# tools/probe_psro.py on {torch.cuda.get_device_name(0)}", flush=True)

# ---- the goldens ----
v = pc.load()
solvers, orders = {}, {}
for game in pc.GAMES:
    s = solvers[game] = osa.TabularSolver(ctx, game)
    keys = s.tables()["keys"]
    where = {k: i for i, k in enumerate(sorted(keys))}
    order = orders[game] = np.array([where[k] for k in keys])
    back = np.argsort(order)
    stack = np.ascontiguousarray(pc.recorded_stack(v, game)[:, order])
    worst = float(np.abs(s.profile_returns(stack, v[f"{game}/profiles"]) - v[f"{game}/returns"]).max())
    print(f"{game} returns of {len(v[f'{game}/profiles'])} profiles {s.last_eval_kernel()} worst |device - reference| {worst:.3g}", flush=True)
    assert worst <= pc.TOLERANCE
    for name in pc.weights_of(v, game):
        agg = s.aggregate_policies(stack, v[f"{game}/weights/{name}"], epsilon=float(v["epsilon"]))[back]
        if game == pc.LARGE_GAME:
            worst = float(np.abs(agg[::pc.ROW_STRIDE] - v[f"{game}/aggregate/{name}_rows"]).max())
            total = float(np.abs(agg.sum(axis=0) - v[f"{game}/aggregate/{name}_colsum"]).max())
            print(f"{game} aggregate/{name} {s.last_eval_kernel()} worst |device - reference| rows {worst:.3g} column sums {total:.3g}", flush=True)
            assert total <= pc.colsum_tolerance(len(agg))
        else:
            worst = float(np.abs(agg - v[f"{game}/aggregate/{name}"]).max())
            print(f"{game} aggregate/{name} {s.last_eval_kernel()} worst |device - reference| {worst:.3g}", flush=True)
        assert worst <= pc.TOLERANCE

# ---- times ----
def median_of_3(label, call):
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t = time.time(); call(); torch.cuda.synchronize(); times.append(time.time() - t)
    print(f"{label}: median of 3 calls {sorted(times)[1] * 1e3:.4g} ms (all: {' '.join(f'{x * 1e3:.4g}' for x in times)})", flush=True)

for game, K in TIMED:
    s, nact = solvers[game], v[f"{game}/nact"][orders[game]]
    P = int(v[f"{game}/num_players"])
    stack = torch.as_tensor(np.stack([avc.policy_table("random", nact, s.amax, 100 + k) for k in range(K)]), device=ctx.device)
    weights = torch.as_tensor(pc.weight_matrix("seeded", P, K), device=ctx.device)
    median_of_3(f"{game} payoff_tensors K = {K} ({K ** P} profiles, device pointers, {s.num_histories} histories)",
                lambda: s.payoff_tensors(stack, device=True))
    median_of_3(f"{game} aggregate_policies K = {K} (device pointers)", lambda: s.aggregate_policies(stack, weights, device=True))

game, iters = "leduc_poker", 20
psro, xfp = osa.PSROSolver(ctx, game), osa.XFPSolver(ctx, game)
psro.iteration(); torch.cuda.synchronize()   # warm-up
psro = osa.PSROSolver(ctx, game)
t = time.time()
for _ in range(iters):
    psro.iteration()
torch.cuda.synchronize()
dt = time.time() - t
print(f"{game} PSROSolver (uniform meta-solver): {iters} iterations in {dt * 1e3:.4g} ms, {dt / iters * 1e3:.4g} ms/iteration, "
      f"population {psro.meta_games()[0].shape}", flush=True)
psro = osa.PSROSolver(ctx, game)
print("iteration  NashConv(PSRO aggregate)  NashConv(XFP average)")
for it in range(iters + 1):
    print(f"{it:9d}  {psro.nash_conv():.12f}  {xfp.nash_conv():.12f}", flush=True)
    psro.iteration(); xfp.iteration()
