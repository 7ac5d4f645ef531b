#!/usr/bin/env python3
"""Rates of the batched alpha-beta search (osg_alpha_beta_search, k_alpha_beta) on the device: nodes/s and roots/s for

  ttt      the tic_tac_toe golden set (tests/golden/minimax_vectors.npz, full depth) tiled to 2^20 roots
  c4       connect_four, depth 8, leaf constant 0, 2^16 random positions (StateBatch.synth: seeded, up to 20 plies)
  hex9     hex(board_size=9), depth 3, leaf constant 0, 2^14 random positions (up to 40 plies)
  one      ONE tic_tac_toe root (the initial position, 18 297 nodes): a single dependent chain on one lane

Every search carries a node budget; a root that exhausts it is reported (and not counted).  Each workload is launched
once to warm up and then timed `--repeats` times with a host clock around launch + synchronise; the median is reported
with the spread.  Where the golden results exist (ttt, one) the outputs are compared with them first.

  timeout 600 python tools/probe_minimax.py [--only ttt,c4] [--repeats 5] [--out profiles/<name>.log]
  OSG_VARIANT_LIB=<another build of the library> python tools/probe_minimax.py     # an A/B of two builds
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import open_spiel_amd as osa  # noqa: E402
from open_spiel_amd import _abi  # noqa: E402


def golden_ttt():
    with np.load(os.path.join(ROOT, "tests", "golden", "minimax_vectors.npz")) as z:
        return {k: z[f"ttt_full/{k}"] for k in ("histories", "value", "best_action", "nodes", "status")}


def batch_from_histories(ctx, game, histories):
    batch = osa.StateBatch(ctx, game, len(histories))
    for t in range(histories.shape[1]):
        column = histories[:, t].astype(np.int32)
        if (column >= 0).any():
            batch.apply_actions(column)
    return batch


def timed(ctx, batch, repeats, **kw):
    out = batch.alpha_beta_search(**kw)   # warm-up: code object, workspace
    ctx.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = batch.alpha_beta_search(**kw)
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    value, best, nodes, status = (t.cpu().numpy() for t in out)
    return np.array(times), value, best, nodes, status


def report(emit, what, n, times, nodes, status, budget):
    done = status == 0
    total = int(nodes[done].sum())
    med = float(np.median(times))
    emit(f"{what}: {n} roots, {total} nodes (largest tree {int(nodes[done].max())}, budget {budget}; "
         f"{int((status == 2).sum())} roots over budget, {int((status == 1).sum())} at the depth limit)")
    emit(f"    {med * 1e3:.3f} ms median of {len(times)} (min {times.min() * 1e3:.3f}, max {times.max() * 1e3:.3f}): "
         f"{total / med:.4g} nodes/s, {n / med:.4g} roots/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ttt,c4,hex9,one")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    ctx = osa.Context(0)
    emit(f"# tools/probe_minimax.py on {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH, ROOT)}")
    only = a.only.split(",")
    if "ttt" in only:
        g = golden_ttt()
        tile = np.arange(1 << 20) % len(g["status"])
        batch = batch_from_histories(ctx, "tic_tac_toe", g["histories"][tile])
        budget = 1 << 16
        times, value, best, nodes, status = timed(ctx, batch, a.repeats, max_nodes=budget)
        assert not status.any() and np.array_equal(value, g["value"][tile]) and np.array_equal(best, g["best_action"][tile]) \
            and np.array_equal(nodes, g["nodes"][tile]), "tic_tac_toe: the outputs differ from the golden results"
        report(emit, "tic_tac_toe, full depth, golden set tiled", len(tile), times, nodes, status, budget)
    if "c4" in only:
        batch = osa.StateBatch(ctx, "connect_four", 1 << 16)
        batch.synth(0xC4, 20)
        budget = 1 << 22
        times, value, best, nodes, status = timed(ctx, batch, a.repeats, depth_limit=8, leaf_value=0.0, max_nodes=budget)
        report(emit, "connect_four, depth 8, leaf constant 0, random positions of up to 19 plies", 1 << 16, times, nodes, status, budget)
    if "hex9" in only:
        batch = osa.StateBatch(ctx, "hex(board_size=9)", 1 << 14)
        batch.synth(0x9E, 40)
        budget = 1 << 22
        times, value, best, nodes, status = timed(ctx, batch, a.repeats, depth_limit=3, leaf_value=0.0, max_nodes=budget)
        report(emit, "hex(board_size=9), depth 3, leaf constant 0, random positions of up to 39 plies", 1 << 14, times, nodes, status, budget)
    if "one" in only:
        batch = osa.StateBatch(ctx, "tic_tac_toe", 1)
        budget = 1 << 16
        times, value, best, nodes, status = timed(ctx, batch, max(a.repeats, 20), max_nodes=budget)
        assert (float(value[0]), int(best[0]), int(nodes[0]), int(status[0])) == (0.0, 0, 18297, 0)
        report(emit, "tic_tac_toe, ONE root (the initial position)", 1, times, nodes, status, budget)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
