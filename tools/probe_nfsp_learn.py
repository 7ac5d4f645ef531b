"""The fused NFSP learner against the torch learner on one GPU: the workload of profiles/nfsp_probe.txt (leduc_poker,
2^16 episodes per step, hidden [128]).  A warm-up step of each, then alternating pairs of synchronised steps; the two
new calls alone (batched draws, osg_nfsp_learn) on the buffers the steps filled; and one kuhn_poker NashConv trace of
40 960 episodes with learner="fused" beside the torch one.  Writes profiles/nfsp_learn_probe.txt (or the file named as the only argument)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_nfsp import HYPER, RUN_EPISODES, RUN_MARKS, RUN_STEPS  # noqa: E402

PAIRS = 3


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return time.perf_counter() - t0


def main():
    import numpy as np
    import open_spiel_amd as osa
    from open_spiel_amd.deep_cfr import SAMPLE_SALT
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    ctx = osa.Context(0)
    game, E = "leduc_poker", 1 << 16
    tabular = osa.TabularSolver(ctx, game, mccfr=True)
    solvers = {learner: osa.NFSPSolver(ctx, game, **dict(HYPER, hidden_layers_sizes=[128]), episodes_per_step=E, tabular=tabular, learner=learner)
               for learner in ("torch", "fused")}
    say(f"{game}, {E} episodes per step, hidden [128], batch 128; warm-up step, then {PAIRS} alternating pairs")
    for s in solvers.values():
        s.step()
    times = {learner: [] for learner in solvers}
    for _ in range(PAIRS):
        for learner, s in solvers.items():
            before = sum(u[0] + u[1] for u in s.updates)
            times[learner].append((timed(ctx, s.step), sum(u[0] + u[1] for u in s.updates) - before))
    for learner, runs in times.items():
        say(f"  learner={learner}: " + ", ".join(f"{dt * 1e3:.1f} ms ({n} updates)" for dt, n in runs))
    t, f = (float(np.median([dt for dt, _ in times[k]])) for k in ("torch", "fused"))
    say(f"  medians: torch {t * 1e3:.1f} ms, fused {f * 1e3:.1f} ms per step: {t / f:.1f} x; {E / t:.4g} and {E / f:.4g} episodes/s")
    s = solvers["fused"]
    U = 2048
    streams = np.arange(1, U + 1, dtype=np.uint64)
    for name, buffer in (("ring", s.replay_buffers[0]), ("reservoir", s.reservoir_buffers[0])):
        dt = min(timed(ctx, lambda: buffer.sample_slots_many(128, 7 ^ SAMPLE_SALT, streams)) for _ in range(3))
        say(f"  sample_slots_many, {name} of {len(buffer)} rows, {U} streams x 128: {dt * 1e3:.2f} ms ({dt / U * 1e6:.2f} us per draw)")
    for U in (256, 2048):
        owed = [(U, U, 0)] * 2
        dts = [timed(ctx, lambda: s._learn_fused(owed)) for _ in range(3)]
        say(f"  draws + osg_nfsp_learn, 4 jobs x {U} updates: {min(dts) * 1e3:.2f} ms")
    a, b = (min(timed(ctx, lambda: s._learn_fused([(U, U, 0)] * 2)) for _ in range(3)) for U in (512, 2560))
    say(f"  per update of one network (the slope between 512 and 2 560 updates per job, draws included): {(b - a) / 2048 * 1e6:.2f} us")
    say(f"kuhn_poker run: {RUN_STEPS} steps of {RUN_EPISODES} episodes, the hyperparameters of profiles/nfsp_probe.txt")
    for learner in ("torch", "fused"):
        run = osa.NFSPSolver(ctx, "kuhn_poker", **HYPER, episodes_per_step=RUN_EPISODES, learner=learner)
        trace = [f"{run.nash_conv():.4f}"]
        ctx.synchronize()
        t0 = time.perf_counter()
        for k in range(1, RUN_STEPS + 1):
            run.step()
            if k in RUN_MARKS:
                trace.append(f"{run.nash_conv():.4f}")
        ctx.synchronize()
        say(f"  learner={learner}: NashConv at 0, " + ", ".join(str(m * RUN_EPISODES) for m in RUN_MARKS) + " episodes: " + " ".join(trace) +
            f" ({run.episodes / (time.perf_counter() - t0):.4g} episodes/s, evaluations included)")
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nfsp_learn_probe.txt"), "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
