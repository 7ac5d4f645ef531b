"""Exhaustive enumeration and retrograde solve (Game.solve / osg_solve_create) on the device: checks every full-solve
case of tests/golden/solve_vectors.npz first (counts per level, the sorted state strings or their SHA-256, every value
position by position), then reports states/s for tic_tac_toe, connect_four(rows=4,columns=5), connect_four(rows=5,
columns=5) and hex(board_size=4): the whole call (enumeration + backward pass + the result's copies into torch tensors),
and the same positions as roots of one alpha_beta_search batch for comparison.  Wall clock around synchronised calls,
median of --reps runs after one warm-up; one process, one device.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import statistics
import time
import numpy as np
import torch, open_spiel_amd as osa
import solve_cases as sc

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
ctx = osa.Context(0)
GEOMETRY = {"hex3x4": ("hex", 3, 4), "c4_4x4": ("connect_four", 4, 4), "c4_4x4k3": ("connect_four", 4, 4),
            "c4_3x5k3": ("connect_four", 3, 5)}

# ---- the goldens ----
for case in sc.solve_cases():
    s = osa.Game(sc.field(case, "game")).solve(ctx)
    assert s.n == sc.field(case, "count"), case
    assert np.diff(s.level_offsets.cpu().numpy()).tolist() == sc.field(case, "level_counts").tolist(), case
    keys = sc.keys(case)
    if keys is not None:
        strings = s.state_strings()
        order = sorted(range(s.n), key=strings.__getitem__)
        assert [strings[i] for i in order] == keys, case
        assert (s.values.cpu().numpy()[order] == sc.field(case, "values")).all(), case
    else:
        kind, rows, cols = GEOMETRY[case]
        strings = sc.render_strings(kind, s.states.raw_words(), rows, cols)
        order = sorted(range(s.n), key=strings.__getitem__)
        assert sc.sha256_of([strings[i] for i in order]) == sc.field(case, "keys_sha256"), case
        assert (s.values.cpu().numpy()[order] == sc.field(case, "values")).all(), case
    assert float(s.values[0]) == sc.field(case, "root_value"), case
    print(f"{case}: {s.n} states, {s.num_levels} levels, {s.num_edges} edges, root value {float(s.values[0]):+.0f}: equals the goldens", flush=True)
    s.close()

# ---- rates ----
def timed(call):
    call()
    ts = []
    for _ in range(reps):
        ctx.synchronize(); torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        ctx.synchronize(); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return out, statistics.median(ts), min(ts), max(ts)

for game in ["tic_tac_toe", "connect_four(rows=4,columns=5)", "connect_four(rows=5,columns=5)", "hex(board_size=4)"]:
    lib, C = osa.lib(), __import__("ctypes")
    def create():
        h = C.c_void_p()
        osa._abi.check(lib.osg_solve_create(ctx._h, game.encode(), -1, 1, 1 << 27, C.byref(h)))
        lib.osg_solve_destroy(h)
    _, med_c, lo_c, hi_c = timed(create)
    s, med, lo, hi = timed(lambda: osa.Game(game).solve(ctx, max_states=1 << 27))
    print(f"{game}: {s.n} states {s.num_edges} edges {s.num_levels} levels root {float(s.values[0]):+.0f} distance {int(s.distance[0])} | "
          f"osg_solve_create (enumerate + solve) median {med_c * 1e3:.2f} ms [{lo_c * 1e3:.2f}, {hi_c * 1e3:.2f}] = {s.n / med_c:.4g} states/s | "
          f"Game.solve incl. result tensors median {med * 1e3:.2f} ms [{lo * 1e3:.2f}, {hi * 1e3:.2f}] = {s.n / med:.4g} states/s", flush=True)
    if s.n <= 2_000_000:
        (value, best, nodes, status), med_ab, lo_ab, hi_ab = timed(lambda: s.states.alpha_beta_search(maximizing_player=0, max_nodes=1 << 26))
        ok = bool((status == 0).all()) and bool((value == s.values).all())
        print(f"{game}: alpha_beta_search on the same {s.n} positions as roots: median {med_ab * 1e3:.2f} ms [{lo_ab * 1e3:.2f}, {hi_ab * 1e3:.2f}] = "
              f"{s.n / med_ab:.4g} roots/s, {int(nodes.sum())} nodes, values {'equal' if ok else 'DIFFER FROM'} the table", flush=True)
    s.close()
