"""Per-infostate action values and reaches (TabularSolver.action_values) on the device: checks every case of
tests/golden/action_value_vectors.npz first (every output within 1e-12 of the reference's own action_value.py), then
times calls/s on kuhn_poker, leduc_poker and leduc_poker(players=3) with host pointers and with device pointers, beside
osg_cfr_evaluate_policy on the same solver in the same session.  --reference also times the reference's Python walk on
the host (needs the reference tree; leduc_poker(players=3) takes minutes); --reference-only does nothing else.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time
import numpy as np

GAMES = ["kuhn_poker", "leduc_poker", "leduc_poker(players=3)"]

def reference_rows():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_action_value_vectors as gen
    pyspiel, policy, action_value, _, _ = gen.reference_modules()
    for game_string in GAMES:
        game = pyspiel.load_game(game_string)
        t = time.time()
        pol = policy.TabularPolicy(game)
        built = time.time() - t
        walker = action_value.TreeWalkCalculator(game)
        t = time.time()
        walker.compute_all_states_action_values([pol] * game.num_players())
        dt = time.time() - t
        print(f"{game_string} reference TreeWalkCalculator (Python, host, one core) s/call {dt:.4g} calls/s {1 / dt:.4g} "
              f"(TabularPolicy built in {built:.3g} s) root {walker.root_values}", flush=True)

if "--reference" in sys.argv or "--reference-only" in sys.argv:
    reference_rows()
if "--reference-only" in sys.argv:
    sys.exit(0)

import torch, open_spiel_amd as osa
import action_value_cases as avc
ctx = osa.Context(0)

# ---- the goldens ----
v = avc.load()
solvers = {}
for game in avc.SMALL_GAMES + (avc.LARGE_GAME,):
    s = solvers[game] = osa.TabularSolver(ctx, game)
    where = {k: i for i, k in enumerate(sorted(s.tables()["keys"]))}
    order = np.array([where[k] for k in s.tables()["keys"]])
    back = np.argsort(order)
    for case in avc.case_names(v, game):
        b = int(v[f"{case}/responder"])
        got = s.action_values("table", avc.case_policy(v, case)[order], responder=None if b < 0 else b)
        worst = float(np.abs(got["root_values"] - v[f"{case}/root_values"]).max())
        for name in avc.VECTORS + avc.TABLES:
            dev = got[name][back]
            if f"{case}/{name}" in v:
                worst = max(worst, float(np.abs(dev - v[f"{case}/{name}"]).max()))
            else:
                stride, total = (avc.ROW_STRIDE, "colsum") if name in avc.TABLES else (avc.VECTOR_STRIDE, "sum")
                worst = max(worst, float(np.abs(dev[::stride] - v[f"{case}/{name}_rows"]).max()),
                            float(np.abs(dev.sum(axis=0) - v[f"{case}/{name}_{total}"]).max()))
        if b >= 0:
            worst = max(worst, abs(got["best_response_value"] - float(v[f"{case}/best_response_value"])))
            assert np.array_equal(got["best_index"][back], v[f"{case}/best_index"])
        print(f"{case} {s.last_eval_kernel()} worst |device - reference| {worst:.3g}", flush=True)
        assert worst <= avc.TOLERANCE

# ---- rates ----
def rate(game, label, call, warm, reps, kernel):
    for _ in range(warm): call()
    torch.cuda.synchronize()
    t = time.time()
    for _ in range(reps): call()
    torch.cuda.synchronize(); dt = time.time() - t
    print(f"{game} {label} calls/s {reps / dt:.4g} us/call {dt / reps * 1e6:.4g} ({reps} calls) kernel {kernel()}", flush=True)

for game in GAMES:
    s = solvers[game]
    s.evaluate_and_update_policy(10)
    table = s.tables()["avg_policy"]
    d_table = torch.from_numpy(table).to(ctx.device)
    reps = 200 if game == avc.LARGE_GAME else 2000
    rate(game, "action_values, host pointers", lambda: s.action_values("table", table), 20, reps, s.last_eval_kernel)
    rate(game, "action_values, device pointers", lambda: s.action_values("table", d_table, device=True), 20, reps, s.last_eval_kernel)
    rate(game, "action_values of the average policy, device pointers", lambda: s.action_values("average", device=True), 20, reps, s.last_eval_kernel)
    if game != avc.LARGE_GAME:
        rate(game, "action_values vs a best responder, host pointers", lambda: s.action_values("table", table, responder=1), 20, reps, s.last_eval_kernel)
    rate(game, "evaluate_policy (NashConv)", lambda: s.evaluate_policy("table", table), 20, reps, s.last_eval_kernel)
