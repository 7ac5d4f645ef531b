"""Self-play throughput probe: connect_four and hex(9) at 2^14 environments with RolloutEvaluator.

Per game: a warm-up that plays the environments out of step with each other, then three synchronised runs of PLIES
plies; the median run gives rows/s and games/s, and a second set of three runs with a synchronisation between the
search and select + commit gives the per-ply split.  Output: profiles/selfplay_probe.txt is one run of this script.

    python tools/probe_selfplay.py [--envs 16384] [--simulations 32] [--plies 24]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 14)
    ap.add_argument("--simulations", type=int, default=32)
    ap.add_argument("--plies", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=48)
    args = ap.parse_args()
    import open_spiel_amd as osa
    from open_spiel_amd import mcts

    ctx = osa.Context(0)
    print(f"self-play probe: {args.envs} environments, RolloutEvaluator, {args.simulations} simulations per move, UCT c = 1.4, "
          f"temperature 1, temperature_drop 10, ring of 2^20 rows; median of 3 runs of {args.plies} plies after {args.warmup} "
          f"warm-up plies")
    for game in ("connect_four", "hex(board_size=9)"):
        envs = osa.StateBatch(ctx, game, args.envs)
        buf = osa.ReplayBuffer(ctx, game, 1 << 20)
        sp = osa.SelfPlay(envs, buf, mcts.RolloutEvaluator(), max_simulations=args.simulations, uct_c=1.4, puct=False,
                          temperature=1.0, temperature_drop=10, seed=1)
        for _ in range(args.warmup):
            sp.step()
        ctx.synchronize()
        whole = []
        for _ in range(3):
            seen0, games = buf.total_seen, 0
            t0 = time.perf_counter()
            for _ in range(args.plies):
                games = games + sp.step()["finished"].sum()
            ctx.synchronize()
            dt = time.perf_counter() - t0
            whole.append((dt, buf.total_seen - seen0, int(games)))
        split = []
        for _ in range(3):
            t_search = t_rest = 0.0
            for _ in range(args.plies):
                ctx.synchronize()
                t0 = time.perf_counter()
                res = sp.search(sp.steps)
                ctx.synchronize()
                t1 = time.perf_counter()
                sp.select(res["child_visits"], res["best_action"], res["root_value"])
                sp.commit()
                sp.steps += 1
                ctx.synchronize()
                t2 = time.perf_counter()
                t_search += t1 - t0
                t_rest += t2 - t1
            split.append((t_search / args.plies, t_rest / args.plies))
        dt, rows, games = sorted(whole)[1]
        search_ms = statistics.median(s for s, _ in split) * 1e3
        rest_ms = statistics.median(r for _, r in split) * 1e3
        print(f"{game}: {dt / args.plies * 1e3:.3f} ms per ply; {rows / dt:.4g} rows/s, {games / dt:.4g} games/s "
              f"({rows} rows, {games} games in the median run); per ply: search {search_ms:.3f} ms, "
              f"select + commit {rest_ms:.3f} ms ({100 * rest_ms / (search_ms + rest_ms):.1f} %)")
        sp.close()
        buf.close()


if __name__ == "__main__":
    main()
