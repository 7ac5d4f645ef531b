#!/usr/bin/env python3
"""Rates of the batched information-set MCTS (osg_ismcts_search, k_ismcts) on the device, in simulations/s:

  leduc    leduc_poker, 2^14 roots x 1 024 simulations
  kuhn     kuhn_poker, 2^16 roots x 256 simulations

Roots are the golden roots of tests/golden/ismcts_vectors.npz tiled over the batch (UCT, uct_c 2, one rollout, unlimited
world samples, MAX_VISIT_COUNT).  Before anything is timed, every golden case is searched at its row of a 257-root batch
and compared with the reference's tree (status, policy and return sums bit for bit, sampled action, node count).  Beside
each workload the same roots go through osg_mcts_search(layout=1) — the perfect-information lane-per-root search over the
one true deal — with the same simulations as a yardstick for the machinery the two share.  Each is launched once to warm
up and then timed `--repeats` times with a host clock around launch + synchronise; the median is reported with the spread.

  timeout 900 python tools/probe_ismcts.py [--only leduc,kuhn] [--repeats 3] [--out profiles/ismcts_probe.txt]
  python tools/probe_ismcts.py --reference      # the reference's Python ISMCTSBot on one host core (needs its sources)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ismcts_cases as ic  # noqa: E402

WORKLOADS = {"leduc": ("leduc_poker", 1 << 14, 1024), "kuhn": ("kuhn_poker", 1 << 16, 256)}


def batch_from_histories(osa, ctx, game, histories):
    batch = osa.StateBatch(ctx, game, len(histories))
    for t in range(max(len(h) for h in histories)):
        batch.apply_actions(np.array([h[t] if t < len(h) else -1 for h in histories], np.int32))
    return batch


def roots_of(cases, game):
    seen = []
    for c in cases:
        if c["game"] == game and c["history"] not in seen:
            seen.append(c["history"])
    return seen


def check_goldens(osa, ctx, cases, emit):
    groups = {}
    for c in cases:
        groups.setdefault((c["game"], c["seed"]) + tuple(c[k] for k in ic.KNOBS), []).append(c)
    for group in groups.values():
        g = group[0]
        fill = roots_of(cases, g["game"])
        rows = {c["index"]: c for c in group}
        batch = batch_from_histories(osa, ctx, g["game"], [rows[r]["history"] if r in rows else fill[r % len(fill)] for r in range(257)])
        out = batch.ismcts_search(uct_c=g["uct_c"], max_simulations=g["max_simulations"], n_rollouts=g["n_rollouts"],
                                  max_world_samples=g["max_world_samples"], final_policy_type=g["final_policy_type"],
                                  puct=g["child_selection_policy"] == 2, seed=g["seed"])
        out = {k: v.cpu().numpy() for k, v in out.items()}
        for r, c in rows.items():
            A = out["policy"].shape[1]
            same = (out["status"][r] == c["status"] and out["sampled_action"][r] == c["sampled_action"] and
                    out["nodes"][r] == len(c["nodes"]) and
                    np.array_equal(out["policy"][r].view(np.uint64)[~np.isnan(c["policy"][:A])],
                                   c["policy"][:A].view(np.uint64)[~np.isnan(c["policy"][:A])]) and
                    out["child_return_sum"][r].tobytes() == c["nodes"][0][4][:A].tobytes() and
                    (out["child_visits"][r] == c["nodes"][0][3][:A]).all())
            assert same, f"{c['game']} index {c['index']}: the device differs from the golden case"
    emit(f"goldens: {len(cases)} cases in {len(groups)} launches of 257 roots equal the reference's trees")


def timed(ctx, repeats, call):
    call()
    ctx.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    return np.array(times), out


def line(what, sims, times):
    med = float(np.median(times))
    return (f"    {what}: {med * 1e3:.2f} ms median of {len(times)} (min {times.min() * 1e3:.2f}, max {times.max() * 1e3:.2f}): "
            f"{sims / med:.4g} simulations/s")


def reference_rate(emit):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_ismcts_vectors as mk
    mods = mk.reference_modules()
    pyspiel, ismcts, mcts = mods
    for game_string, sims in (("kuhn_poker", 256), ("leduc_poker", 1024)):
        game = pyspiel.load_game(game_string)
        history = mk.roots_of(pyspiel, game_string)[0]
        times = []
        for rep in range(3):
            t0 = time.perf_counter()
            mk.run_case(mods, game, history, (sims, 1, 0, 2, 1, 2.0), 7, rep)
            times.append(time.perf_counter() - t0)
        emit(f"reference ISMCTSBot (Python, one host core), {game_string}, {sims} simulations: "
             f"{sims / float(np.median(times)):.4g} simulations/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="leduc,kuhn")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if a.reference:
        reference_rate(emit)
    else:
        import torch
        import open_spiel_amd as osa
        from open_spiel_amd import _abi
        ctx = osa.Context(0)
        emit(f"# tools/probe_ismcts.py on {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH, ROOT)}")
        cases = ic.load_cases()
        check_goldens(osa, ctx, cases, emit)
        for name in a.only.split(","):
            game, n, sims = WORKLOADS[name]
            fill = roots_of(cases, game)
            batch = batch_from_histories(osa, ctx, game, [fill[r % len(fill)] for r in range(n)])
            emit(f"{game}: {n} roots x {sims} simulations, {len(fill)} distinct roots tiled")
            times, out = timed(ctx, a.repeats, lambda: batch.ismcts_search(max_simulations=sims, seed=11))
            status, nodes = out["status"].cpu().numpy(), out["nodes"].cpu().numpy()
            assert not status.any()
            emit(line("osg_ismcts_search", n * sims, times) + f"; {nodes.mean():.1f} nodes per root (largest {nodes.max()})")
            times, _ = timed(ctx, a.repeats, lambda: batch.mcts_search(max_simulations=sims, seed=11, layout=1))
            emit(line("osg_mcts_search(layout=1), same roots", n * sims, times))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
