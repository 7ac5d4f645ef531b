"""NFSP probe: the goldens first, then episode and row rates on leduc_poker, one full NFSPSolver.step, and the NashConv
of the average policy along a short kuhn_poker and leduc_poker run.  Writes profiles/nfsp_probe.txt (--out).

    python tools/probe_nfsp.py [--episodes 65536] [--out profiles/nfsp_probe.txt]
    python tools/probe_nfsp.py --reference [--reference-episodes 20000] [--out ...]      (appends)

Without --reference (needs an MI355X): every recorded chunk of tests/golden/nfsp_vectors.npz is replayed on the device
and compared bit for bit; then, on leduc_poker with fixed synthetic tables, `--episodes` episodes per call into rings
and reservoirs of 2^20 rows, with the two [I, A] tables read through the caches and staged in LDS (median of 3
synchronised calls after a warm-up call: episodes/s, rows/s); one full NFSPSolver.step (the forward passes, the
episodes, the updates they owe); and the runs: RUN_STEPS steps of RUN_EPISODES episodes with the hyperparameters below,
NashConv of the average policy at a few points.

--reference (needs the reference sources, no GPU): the reference's own agents in the loop of examples/kuhn_nfsp.py on
one host core with the same hyperparameters and as many episodes: episodes/s, and the NashConv of their average
policies (a best response computed here on the enumerated tree)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HYPER = dict(hidden_layers_sizes=[64], reservoir_buffer_capacity=200000, anticipatory_param=0.1, batch_size=128, rl_learning_rate=0.01,
             sl_learning_rate=0.01, min_buffer_size_to_learn=1000, learn_every=64, replay_buffer_capacity=20000,
             epsilon_start=0.06, epsilon_end=0.001, epsilon_decay_duration=200000)
RUN_EPISODES, RUN_STEPS, RUN_MARKS = 128, 320, (40, 80, 160, 320)
RUN_GAMES = ("kuhn_poker", "leduc_poker")


def nash_conv_on_tree(tree, policy):
    """tree: deep_cfr_cases.Tree; policy [I][legal index].  sum_p (best-response value of p - value of p)."""
    import numpy as np
    P = tree.num_players
    H = len(tree.parent)
    total = 0.0
    for p in range(P):
        cf = np.zeros(H)
        cf[0] = 1.0
        members = {}
        for h in range(H):
            kids = tree.children[h]
            if tree.kind[h] == 0:
                for c in kids:
                    cf[c] = cf[h] * tree.prob[c]
            elif tree.kind[h] == 1:
                i = int(tree.info[h])
                if tree.actor[h] == p:
                    members.setdefault(i, []).append(h)
                for k, c in enumerate(kids):
                    cf[c] = cf[h] * (1.0 if tree.actor[h] == p else policy[i][k])
        best, memo = {}, {}

        def value(h, respond):
            key = (h, respond)
            if key in memo:
                return memo[key]
            kids = tree.children[h]
            if tree.kind[h] == 2:
                v = float(tree.returns[h, p])
            elif tree.kind[h] == 0:
                v = sum(tree.prob[c] * value(c, respond) for c in kids)
            else:
                i = int(tree.info[h])
                if respond and tree.actor[h] == p:
                    if i not in best:
                        scores = [sum(cf[m] * value(tree.children[m][k], True) for m in members[i]) for k in range(len(kids))]
                        best[i] = int(np.argmax(scores))
                    v = value(kids[best[i]], True)
                else:
                    v = sum(policy[i][k] * value(c, respond) for k, c in enumerate(kids))
            memo[key] = v
            return v

        sys.setrecursionlimit(10000)
        total += value(0, True) - value(0, False)
    return total


def run_reference(episodes, say):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import numpy as np
    import make_nfsp_vectors as maker
    import deep_cfr_cases as dc
    pyspiel, rl_environment, dqn, nfsp = maker.reference_modules()
    import torch
    torch.set_num_threads(1)
    for game_string in RUN_GAMES:
        game, tree, _ = maker.mk.game_tree(pyspiel, game_string)
        ctree = dc.Tree(tree["parent"], tree["kind"], tree["action"], tree["prob"], tree["actor"], tree["info"], tree["returns"], tree["legal"])
        env = rl_environment.Environment(game)
        size, A = env.observation_spec()["info_state"][0], env.action_spec()["num_actions"]
        kwargs = {k: v for k, v in HYPER.items() if k not in ("hidden_layers_sizes", "reservoir_buffer_capacity", "anticipatory_param")}
        agents = [nfsp.NFSP(p, size, A, HYPER["hidden_layers_sizes"], HYPER["reservoir_buffer_capacity"], HYPER["anticipatory_param"], **kwargs)
                  for p in range(game.num_players())]

        def conv():
            policy = []
            with torch.inference_mode():
                for i in range(ctree.num_infostates):
                    legal = ctree.legal[i]
                    mask = np.zeros(A, bool)
                    mask[legal] = True
                    with agents[int(tree["player"][i])].temp_mode_as(nfsp.MODE.AVERAGE_POLICY):
                        logits = agents[int(tree["player"][i])]._avg_network(torch.FloatTensor(tree["tensors"][i]).unsqueeze(0)).squeeze(0)
                    logits = torch.where(torch.BoolTensor(mask), logits, torch.full_like(logits, float(torch.finfo(torch.float).min)))
                    probs = torch.softmax(logits, -1).double().numpy()
                    policy.append([probs[a] / probs[legal].sum() for a in legal])
            return nash_conv_on_tree(ctree, policy)

        say(f"reference, {game_string}: NashConv of the initial average policy {conv():.4f}")
        t0 = time.perf_counter()
        done, spent = 0, 0.0
        for mark in RUN_MARKS:
            target = min(mark * RUN_EPISODES, episodes)
            while done < target:
                time_step = env.reset()
                while not time_step.last():
                    player_id = time_step.observations["current_player"]
                    agent_output = agents[player_id].step(time_step)
                    time_step = env.step([agent_output.action])
                for agent in agents:
                    agent.step(time_step)
                done += 1
            spent = time.perf_counter() - t0
            say(f"reference, {game_string}: after {done} episodes NashConv {conv():.4f} ({done / spent:.4g} episodes/s on one host core, learning included)")
            t0 = time.perf_counter() - spent
            if done >= episodes:
                break


def check_goldens(osa, ctx, say):
    import numpy as np
    import torch
    import nfsp_cases as nc
    from open_spiel_amd.nfsp import TransitionRing
    checked = 0
    for r in range(len(nc.golden_runs())):
        meta, chunks = nc.golden_run(r)
        solver = osa.TabularSolver(ctx, meta["game"], mccfr=True)
        keys, _, _ = nc.golden_game(meta["game"])
        index = {k: i for i, k in enumerate(keys)}
        gold_of_dev = np.array([index[k] for k in solver.tables()["keys"]], np.int64)
        gold = lambda info: np.where(info >= 0, gold_of_dev[np.clip(info, 0, None)], -1).astype(np.int32)   # noqa: E731
        P, A = meta["players"], solver.amax
        rings = [TransitionRing(ctx, meta["ring_capacity"]) for _ in range(P)]
        reservoirs = [osa.ReservoirBuffer(ctx, A, meta["res_capacity"], meta["res_seed"], p) for p in range(P)]
        q, avg = (torch.from_numpy(np.ascontiguousarray(meta[k][gold_of_dev], np.float32)).to(ctx.device) for k in ("q", "avg"))
        for chunk in chunks:
            solver.nfsp_collect(q, avg, meta["eps"], meta["anticipatory"], meta["seed"], len(chunk["draws"]), chunk["first"], rings, reservoirs)
            s = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in solver.nfsp_staged().items()}
            got = dict(draws=s["draws"], modes=s["modes"],
                       ring=(s["ring_offsets"], gold(s["ring_info"]), s["ring_action"], s["ring_reward"], gold(s["ring_next"]), s["ring_final"]),
                       sl=(s["sl_offsets"], gold(s["sl_info"]), s["sl_probs"]))
            if not nc.same_chunk(got, chunk):
                raise SystemExit(f"golden run {r}: the rows of a chunk differ")
            for p in range(P):
                info, action, reward, nxt, final = (t.cpu().numpy() for t in rings[p].filled())
                if not nc.same_ring((rings[p].entry_index, gold(info), action, reward, gold(nxt), final), chunk["rings"][p]):
                    raise SystemExit(f"golden run {r}: ring {p} differs")
                info, _, vals = reservoirs[p].filled()
                if not nc.same_reservoir((reservoirs[p].add_calls, gold(info.cpu().numpy()), vals.cpu().numpy()), chunk["reservoirs"][p]):
                    raise SystemExit(f"golden run {r}: reservoir {p} differs")
            checked += 1
    say(f"goldens: {checked} recorded chunks reproduced bit for bit")


def median_of_3(ctx, call):
    times, last = [], None
    for _ in range(4):
        ctx.synchronize()
        t0 = time.perf_counter()
        last = call()
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times[1:]), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=1 << 16)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--reference-episodes", type=int, default=RUN_EPISODES * RUN_STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nfsp_probe.txt"))
    args = ap.parse_args()
    log = open(args.out, "a" if args.reference else "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    hyper = ", ".join(f"{k}={v}" for k, v in HYPER.items())
    if args.reference:
        say("\npython tools/probe_nfsp.py --reference   (one host core, no GPU)")
        say(f"hyperparameters: {hyper}")
        run_reference(args.reference_episodes, say)
        return
    import numpy as np
    import torch
    import nfsp_cases as nc
    import open_spiel_amd as osa
    from open_spiel_amd.nfsp import TransitionRing

    say("python tools/probe_nfsp.py            (one MI355X, one run)")
    ctx = osa.Context(0)
    check_goldens(osa, ctx, say)
    game, E = "leduc_poker", args.episodes
    solver = osa.TabularSolver(ctx, game, mccfr=True)
    A = solver.amax
    keys, _, _ = nc.golden_game(game)
    index = {k: i for i, k in enumerate(keys)}
    gold_of_dev = np.array([index[k] for k in solver.tables()["keys"]], np.int64)
    q, avg = (torch.from_numpy(np.ascontiguousarray(t[gold_of_dev], np.float32)).to(ctx.device)
              for t in nc.synthetic_tables(nc.golden_tree(game), 1))
    rings = [TransitionRing(ctx, 1 << 20) for _ in range(2)]
    reservoirs = [osa.ReservoirBuffer(ctx, A, 1 << 20, 3, p) for p in range(2)]
    say(f"{game}: {E} episodes per call, anticipatory 0.1, epsilon 0.06, rings and reservoirs of 2^20 rows, median of 3 synchronised calls after a warm-up call")
    first = [0]

    def collect():
        first[0] += E
        return solver.nfsp_collect(q, avg, 0.06, 0.1, 7, E, first[0], rings, reservoirs)

    for home in ("caches", "lds"):
        os.environ["OSG_NFSP_TABLES"] = home
        dt, totals = median_of_3(ctx, collect)
        rows = int(totals[:, :2].sum())
        say(f"  tables in {home:6s}: {dt * 1e3:.3f} ms per call; {E / dt:.4g} episodes/s, {rows / dt:.4g} rows/s "
            f"({int(totals[:, 0].sum())} transitions + {int(totals[:, 1].sum())} supervised rows in the last call)")
    os.environ.pop("OSG_NFSP_TABLES")
    full = osa.NFSPSolver(ctx, game, **dict(HYPER, hidden_layers_sizes=[128]), episodes_per_step=E, tabular=solver)
    dt, _ = median_of_3(ctx, full.step)
    say(f"  NFSPSolver.step, {E} episodes, hidden [128], the {sum(u[0] + u[1] for u in full.updates) // 4} updates a step owes included: "
        f"{dt * 1e3:.1f} ms (median of 3 after a warm-up step)")
    say(f"runs: {RUN_STEPS} steps of {RUN_EPISODES} episodes; {hyper}")
    for g in RUN_GAMES:
        run = osa.NFSPSolver(ctx, g, **HYPER, episodes_per_step=RUN_EPISODES)
        say(f"  {g}: NashConv of the initial average policy {run.nash_conv():.4f}")
        ctx.synchronize()
        t0 = time.perf_counter()
        for k in range(1, RUN_STEPS + 1):
            run.step()
            if k in RUN_MARKS:
                ctx.synchronize()
                spent = time.perf_counter() - t0
                say(f"  {g}: after {run.episodes} episodes NashConv {run.nash_conv():.4f} ({run.episodes / spent:.4g} episodes/s, learning included; "
                    f"updates per player (Q, average, target copies) {run.updates})")
                t0 = time.perf_counter() - spent


if __name__ == "__main__":
    main()
