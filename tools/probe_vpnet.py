"""The fused policy-value forward (osg_vpnet_forward, mcts.VPNetEvaluator(model, forward="fused")) against the torch
forward of the same alpha_zero.VPNetMLP: microseconds per evaluate() — observation pack, legal mask, forward, the answers
as the search reads them — and per round of mcts._search_joint, the two paths alternating in one run (the median of the
pairs).  Shapes: the connect_four net 126-256-256 at 2^10, 2^13 and 2^16 states and hex(9) at 729-256-256.  Writes
profiles/vpnet_probe.txt (or the file named as the first argument).

`probe_vpnet.py learn [file]` times the two learners of alpha_zero.VPNetLearner the same way: one learn(buffer, batch, 64,
seed) call — the draw, the observation and mask pack, 64 updates — of VPNetMLP(126, 7, 256, 1) at batch 256 and 1024, per
update; writes profiles/vpnet_learn_probe.txt."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import open_spiel_amd as osa
from open_spiel_amd import alpha_zero, mcts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = 7


def timed(ctx, fn, reps):
    fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main(path):
    ctx = osa.Context(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tools/probe_vpnet.py on {torch.cuda.get_device_name(0)}: alternating pairs, median of {PAIRS}")
    for game, n, sims in (("connect_four", 1 << 10, 64), ("connect_four", 1 << 13, 64), ("connect_four", 1 << 16, 32), ("hex(board_size=9)", 1 << 13, 32)):
        batch = osa.StateBatch(ctx, game, n)
        batch.random_steps(3, 6)
        torch.manual_seed(0)
        model = alpha_zero.VPNetMLP(batch.desc.obs_size, batch.num_distinct_actions, 256, 1).to(ctx.device)
        evaluators = {"torch": mcts.VPNetEvaluator(model), "fused": mcts.VPNetEvaluator(model, forward="fused")}
        everything = torch.ones(n, dtype=torch.bool, device=ctx.device)
        reps = max(20, min(2000, (1 << 21) // n))
        got = {k: [] for k in evaluators}
        rounds = {k: [] for k in evaluators}
        for _ in range(PAIRS):
            for name, ev in evaluators.items():
                got[name].append(timed(ctx, lambda: ev.evaluate(batch, everything, everything), reps))
        for _ in range(3):
            for name, ev in evaluators.items():
                dt = timed(ctx, lambda: mcts._search_joint(batch, ev, sims, 1.4, 1, False, 0, 0, 0, True, False, None, use_graph=False), 1)
                rounds[name].append(dt / sims)
        flop = 2.0 * n * sum(o * i for o, i in model.layer_shapes)
        med = {k: sorted(v)[len(v) // 2] for k, v in got.items()}
        rnd = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
        say(f"{game} n = {n}, net {batch.desc.obs_size}-256-256, A = {batch.num_distinct_actions} ({flop / 1e9:.2f} GFLOP a forward, "
            f"R = {evaluators['fused'].rows_per_workgroup}):")
        for k in evaluators:
            say(f"  {k:5s} evaluate {med[k] * 1e6:8.1f} us (min {min(got[k]) * 1e6:.1f}, max {max(got[k]) * 1e6:.1f}; {flop / med[k] / 1e12:.1f} TFLOP/s "
                f"end to end), _search_joint {rnd[k] * 1e6:8.1f} us per round of {sims}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main_learn(path):
    ctx = osa.Context(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    updates = 64
    say(f"tools/probe_vpnet.py learn on {torch.cuda.get_device_name(0)}: alternating pairs, median of {PAIRS}; {updates} updates per call")
    buf = alpha_zero.ReplayBuffer(ctx, "connect_four", 1 << 16)
    alpha_zero.SelfPlay(osa.StateBatch(ctx, "connect_four", 1024), buf, mcts.RolloutEvaluator(), max_simulations=8, uct_c=1.4, seed=1).run(1 << 14)
    for batch in (256, 1024):
        learners = {}
        for name in ("torch", "fused"):
            torch.manual_seed(0)
            learners[name] = alpha_zero.VPNetLearner(ctx, alpha_zero.VPNetMLP(126, 7, 256, 1).to(ctx.device), 1e-3, learner=name)
        got = {k: [] for k in learners}
        for pair in range(PAIRS):
            for name, learner in learners.items():
                got[name].append(timed(ctx, lambda: learner.learn(buf, batch, updates, seed=pair), 3) / updates)
        med = {k: sorted(v)[len(v) // 2] for k, v in got.items()}
        plan = learners["fused"].plan(batch)
        flop = 6.0 * batch * sum(o * i for o, i in learners["fused"].model.layer_shapes)
        say(f"connect_four net 126-256-(1)-7, batch {batch} (R = {plan['rows']}, G = {plan['workgroups']}, {flop / 1e9:.2f} GFLOP an update):")
        for k in learners:
            say(f"  {k:5s} {med[k] * 1e6:8.1f} us per update (min {min(got[k]) * 1e6:.1f}, max {max(got[k]) * 1e6:.1f}; {flop / med[k] / 1e12:.2f} TFLOP/s end to end)")
        say(f"  torch / fused = {med['torch'] / med['fused']:.2f}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "learn":
        main_learn(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "vpnet_learn_probe.txt"))
        sys.exit(0)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vpnet_probe.txt"))
