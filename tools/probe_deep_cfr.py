"""Deep CFR probe: the goldens first, then traversal and row rates on leduc_poker and one full solver iteration.

    python tools/probe_deep_cfr.py [--traversals 16384] [--repeats 5]
    python tools/probe_deep_cfr.py --reference [--reference-traversals 200]

Without --reference (needs an MI355X): every recorded step of tests/golden/deep_cfr_vectors.npz is replayed on the device
and compared bit for bit; then, on leduc_poker with a fixed synthetic advantage table, `--traversals` traversals per
step for each player into buffers of 2^20 rows (median of `--repeats` steps: traversals/s, rows/s), and one full
DeepCFRSolver iteration (both players' steps with training, then the strategy network) with the reference's default
networks, batches of 2 048 rows.  profiles/deep_cfr_probe.txt is one run of this script.

--reference (needs the reference sources, no GPU): the reference's own DeepCFRSolver._traverse_game_tree on leduc_poker on
one host core, traversals/s over `--reference-traversals` traversals per player."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_reference(traversals):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_deep_cfr_vectors as maker
    pyspiel, deep_cfr = maker.reference_modules()
    import torch
    torch.set_num_threads(1)
    game = pyspiel.load_game("leduc_poker")
    solver = deep_cfr.DeepCFRSolver(game, memory_capacity=1 << 20)
    for player in range(2):
        t0 = time.perf_counter()
        for _ in range(traversals):
            solver._traverse_game_tree(solver._root_node, player)
        dt = time.perf_counter() - t0
        rows = int(solver.advantage_buffers[player].add_calls)
        print(f"reference, leduc_poker, player {player}: {traversals / dt:.4g} traversals/s on one host core "
              f"({traversals} traversals, {rows} advantage rows, {dt:.2f} s)")


def check_goldens(osa, ctx):
    import numpy as np
    import torch
    import deep_cfr_cases as dc
    steps_checked = 0
    for r in range(len(dc.golden_runs())):
        meta, steps = dc.golden_run(r)
        solver = osa.TabularSolver(ctx, meta["game"], mccfr=True)
        keys, _, _ = dc.golden_game(meta["game"])
        index = {k: i for i, k in enumerate(keys)}
        gold_of_dev = np.array([index[k] for k in solver.tables()["keys"]], np.int64)
        P, A = meta["players"], solver.amax
        buffers = [osa.ReservoirBuffer(ctx, A, meta["capacity"], meta["res_seed"], b) for b in range(P + 1)]
        for step in steps:
            table = torch.from_numpy(np.ascontiguousarray(step["advantages"][gold_of_dev], np.float32)).to(ctx.device)
            solver.deep_cfr_traverse(table, step["player"], step["iteration"], meta["seed"], len(step["draws"]), step["first"],
                                     buffers[step["player"]], buffers[P])
            s = solver.deep_cfr_staged()
            for k in ("adv", "strat"):
                got = (s[k + "_offsets"].cpu().numpy(), gold_of_dev[s[k + "_info"].cpu().numpy()].astype(np.int32),
                       s[k + "_values"].cpu().numpy())
                if not dc.same_rows(got, step[k]):
                    raise SystemExit(f"golden run {r}: the {k} rows of a step differ")
            for b, want in step["buffers"].items():
                info, it, vals = buffers[b].filled()
                got = (buffers[b].add_calls, gold_of_dev[info.cpu().numpy()].astype(np.int32), it.cpu().numpy(), vals.cpu().numpy())
                if not dc.same_buffer(got, want):
                    raise SystemExit(f"golden run {r}: buffer {b} differs")
            steps_checked += 1
    print(f"goldens: {steps_checked} recorded steps reproduced bit for bit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traversals", type=int, default=1 << 14)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--reference-traversals", type=int, default=200)
    args = ap.parse_args()
    if args.reference:
        time_reference(args.reference_traversals)
        return
    import numpy as np
    import torch
    import open_spiel_amd as osa

    ctx = osa.Context(0)
    check_goldens(osa, ctx)
    game, T = "leduc_poker", args.traversals
    solver = osa.TabularSolver(ctx, game, mccfr=True)
    I, A = solver.num_infostates, solver.amax
    table = torch.from_numpy(np.random.default_rng(1).standard_normal((I, A)).astype(np.float32)).to(ctx.device)
    bufs = [osa.ReservoirBuffer(ctx, A, 1 << 20, 3, b) for b in range(3)]
    print(f"{game}: {T} traversals per step, buffers of 2^20 rows, median of {args.repeats} steps after one warm-up step")
    for player in range(2):
        times, rows = [], (0, 0)
        for k in range(args.repeats + 1):
            ctx.synchronize()
            t0 = time.perf_counter()
            rows = solver.deep_cfr_traverse(table, player, 1, 7, T, (2 * k + player) * T, bufs[player], bufs[2])
            ctx.synchronize()
            times.append(time.perf_counter() - t0)
        dt = statistics.median(times[1:])
        print(f"  player {player}: {dt * 1e3:.3f} ms per step; {T / dt:.4g} traversals/s, {(rows[0] + rows[1]) / dt:.4g} rows/s "
              f"({rows[0]} advantage + {rows[1]} strategy rows in the last step)")
    deep = osa.DeepCFRSolver(ctx, game, num_iterations=1, num_traversals=T, batch_size_advantage=2048, batch_size_strategy=2048,
                             memory_capacity=1 << 20, tabular=solver)
    for label in ("first (includes torch's warm-up)", "second"):
        ctx.synchronize()
        t0 = time.perf_counter()
        _, losses, policy_loss = deep.solve()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        print(f"  DeepCFRSolver, one iteration of 2 x {T} traversals with training, {label}: {dt * 1e3:.1f} ms "
              f"(advantage losses {[round(v[-1], 4) for v in losses.values()]}, policy loss {policy_loss:.4f}); "
              f"NashConv of the policy network {deep.nash_conv():.4f}")


if __name__ == "__main__":
    main()
