"""The fused Deep CFR learner against the torch learner on one GPU: one DeepCFRSolver iteration on leduc_poker at the
settings of the reference's examples/deep_cfr_pytorch.py (networks (64,), batches 256, 375 advantage updates per player;
40 traversals), learner="torch" against learner="fused" in the same process.  A warm-up iteration of each, then
alternating pairs of synchronised iterations and their medians; then the new call alone on the buffers the iterations
filled: microseconds per update for one job and for four jobs side by side.  Writes profiles/deep_cfr_learn_probe.txt (or
the file named as the only argument).

`wide` as the first argument runs the wide form instead: the same iteration with the solver's default (256, 256) networks,
learner="torch" against learner="fused_wide", and osg_deep_cfr_learn_wide alone per update at batches 256 and 1024; it
writes profiles/deep_cfr_learn_wide_probe.txt (or the file named as the second argument)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS, UPDATES = 3, 375


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return time.perf_counter() - t0


def iteration(s):
    for p in range(s._num_players):
        s.traverse(p)
        s._reinitialize_advantage_network(p)
        s._learn_advantage_network(p)
    s._iteration += 1


def main_wide(path):
    import numpy as np
    import torch
    import open_spiel_amd as osa
    from open_spiel_amd._abi import check, lib
    from open_spiel_amd.deep_cfr import DeepCFRSolver, fused_wide_plan
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    ctx = osa.Context(0)
    game = "leduc_poker"
    tabular = osa.TabularSolver(ctx, game)
    solvers = {learner: DeepCFRSolver(ctx, game, policy_network_layers=(256, 256), advantage_network_layers=(256, 256), num_traversals=40,
                                      learning_rate=1e-3, batch_size_advantage=256, batch_size_strategy=256, memory_capacity=int(1e6),
                                      advantage_network_train_steps=UPDATES, tabular=tabular, learner=learner)
               for learner in ("torch", "fused_wide")}
    say(f"{game}, networks (256, 256), batches 256, {UPDATES} advantage updates per player and iteration, 40 traversals; plan {fused_wide_plan(ctx, [30, 256, 256, 3], 256)}")
    say(f"two warm-up iterations of each learner, then {PAIRS} alternating pairs of synchronised iterations")
    for s in solvers.values():
        iteration(s)
        iteration(s)
    times = {learner: [] for learner in solvers}
    for _ in range(PAIRS):
        for learner, s in solvers.items():
            times[learner].append(timed(ctx, lambda: iteration(s)))
    for learner, runs in times.items():
        say(f"  learner={learner}: " + ", ".join(f"{dt * 1e3:.1f} ms" for dt in runs) + f" ({len(solvers[learner].advantage_buffers[0])} rows held by player 0)")
    t, f = (float(np.median(times[k])) for k in ("torch", "fused_wide"))
    say(f"  medians: torch {t * 1e3:.1f} ms, fused_wide {f * 1e3:.1f} ms per iteration ({2 * UPDATES} updates): {t / f:.1f} x")
    s = solvers["fused_wide"]
    for _ in range(2):      # (rows for the batch of 1024)
        iteration(s)
    net, memory = s._advantage_networks[0], s.advantage_buffers[0]
    flat = s._fused[net].params
    for B in (256, 1024):
        if B > len(memory):
            say(f"  ({len(memory)} rows held: no batch of {B})")
            continue
        slots = memory.sample_slots_many(B, 11, np.arange(1, UPDATES + 1))
        bufs = [flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat), torch.empty(UPDATES, device=flat.device)]
        job = s._fused_job(net, memory, slots, bufs[3], bufs[0], bufs[1], bufs[2], 0)
        dts = sorted(timed(ctx, lambda: check(lib().osg_deep_cfr_learn_wide(ctx._h, C.byref(job), 1))) for _ in range(3))
        say(f"  osg_deep_cfr_learn_wide alone, 1 job x {UPDATES} updates of {B} rows ({fused_wide_plan(ctx, [30, 256, 256, 3], B)['workgroups']} workgroups): "
            f"median {dts[1] * 1e3:.2f} ms, {dts[1] / UPDATES * 1e6:.1f} us per update")
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")


def main():
    import numpy as np
    import torch
    import open_spiel_amd as osa
    from open_spiel_amd._abi import DeepCfrLearnJob, check, lib
    from open_spiel_amd.deep_cfr import DeepCFRSolver, fused_plan
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    ctx = osa.Context(0)
    game = "leduc_poker"
    tabular = osa.TabularSolver(ctx, game)
    solvers = {learner: DeepCFRSolver(ctx, game, policy_network_layers=(64,), advantage_network_layers=(64,), num_iterations=400, num_traversals=40,
                                      learning_rate=1e-3, batch_size_advantage=256, batch_size_strategy=256, memory_capacity=int(1e6),
                                      policy_network_train_steps=2500, advantage_network_train_steps=UPDATES, tabular=tabular, learner=learner)
               for learner in ("torch", "fused")}
    say(f"{game}, networks (64,), batches 256, {UPDATES} advantage updates per player and iteration, 40 traversals; plan {fused_plan(ctx, [30, 64, 3], 256)}")
    say(f"two warm-up iterations of each learner, then {PAIRS} alternating pairs of synchronised iterations")
    for s in solvers.values():
        iteration(s)
        iteration(s)
    times = {learner: [] for learner in solvers}
    for _ in range(PAIRS):
        for learner, s in solvers.items():
            times[learner].append(timed(ctx, lambda: iteration(s)))
    for learner, runs in times.items():
        say(f"  learner={learner}: " + ", ".join(f"{dt * 1e3:.1f} ms" for dt in runs) + f" ({len(solvers[learner].advantage_buffers[0])} rows held by player 0)")
    t, f = (float(np.median(times[k])) for k in ("torch", "fused"))
    say(f"  medians: torch {t * 1e3:.1f} ms, fused {f * 1e3:.1f} ms per iteration ({2 * UPDATES} updates): {t / f:.1f} x")
    s = solvers["fused"]
    net, memory = s._advantage_networks[0], s.advantage_buffers[0]
    flat = s._fused[net].params
    for n_jobs in (1, 4):
        for U in (UPDATES, 4 * UPDATES):
            slots = memory.sample_slots_many(256, 11, np.arange(1, U + 1))
            bufs = [[flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat), torch.empty(U, device=flat.device)] for _ in range(n_jobs)]
            jobs = [s._fused_job(net, memory, slots, b[3], b[0], b[1], b[2], 0) for b in bufs]
            arr = (DeepCfrLearnJob * n_jobs)(*jobs)
            dts = sorted(timed(ctx, lambda: check(lib().osg_deep_cfr_learn(ctx._h, arr, n_jobs))) for _ in range(3))
            say(f"  osg_deep_cfr_learn alone, {n_jobs} job(s) x {U} updates of 256 rows: median {dts[1] * 1e3:.2f} ms, {dts[1] / U * 1e6:.1f} us per update of a job")
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "deep_cfr_learn_probe.txt"), "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["wide"]:
        main_wide(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "deep_cfr_learn_wide_probe.txt"))
    else:
        main()
