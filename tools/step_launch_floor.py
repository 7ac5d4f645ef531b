#!/usr/bin/env python3
"""Host cost of issuing one StateBatch.step, beside the kernel it launches: one JSON record on stdout.

Every figure is a host clock (time.perf_counter) around `--calls` back-to-back calls that end in a device synchronise,
divided by the calls, after `--warmup` untimed calls; each is the median of `--repeats` such windows.
  a_*  StateBatch.step on a 2-state connect_four batch: the kernel is negligible, so this is the host floor of the path
  b_*  the same call on bench.py's headline batch (2^20 synthetic connect_four states, seed 0x5EED, out of place)
  c    osg_copy_bytes of the same bytes (35 B x states, half read, half written), issued as bench.py issues it
  d_*  osg_step called directly through ctypes with its arguments prepared in advance (no checks): the native part
Each a / b figure is given for the path StateBatch.step takes (`step_path`: the native call, or the Python body under
OSG_STEP_PY=1) and for the Python body itself (`*_step_py_us`), so one run compares the two.
Usage: step_launch_floor.py [--states 1048576] [--calls 2000] [--warmup 200] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED
C4_DEPTH_MOD = 36           # bench.py's synthetic depths
BYTES_PER_STATE = 35        # 16 R + 16 W state, 1 action, 1 mask, 1 status


def per_call_us(torch, fn, calls, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / calls * 1e6)
    return statistics.median(windows), min(windows), max(windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import ctypes as C
    import torch
    import open_spiel_amd as osa
    from open_spiel_amd import engine
    from open_spiel_amd._abi import check, lib

    ctx = osa.Context(0)
    rec = {"tool": "step_launch_floor", "states": args.states, "calls": args.calls, "repeats": args.repeats,
           "step_path": "python" if engine._native_step is None else "native",
           "OSG_STEP_PY": os.environ.get("OSG_STEP_PY", "")}
    spread = {}

    def measure(key, fn):
        med, lo, hi = per_call_us(torch, fn, args.calls, args.warmup, args.repeats)
        rec[key] = round(med, 3)
        spread[key] = [round(lo, 3), round(hi, 3)]

    def step_figures(prefix, src, actions):
        dst = osa.StateBatch(ctx, "connect_four", src.n)
        mask, status = src.step_buffers()
        measure(f"{prefix}_step_us", lambda: src.step(actions, dst=dst, mask=mask, status=status))
        measure(f"{prefix}_step_py_us", lambda: src._step_py(actions, dst=dst, mask=mask, status=status))
        f, sh, dh = lib().osg_step, src._h, dst._h
        pa, pm, ps = actions.data_ptr(), mask.data_ptr(), status.data_ptr()
        measure(f"d_{prefix}_ctypes_osg_step_us", lambda: f(sh, dh, pa, pm, ps))
        assert int((status & 0x40).sum().item()) == 0, "synthetic actions must all be legal"

    # (a) two states: the launch costs the host path alone
    tiny = osa.StateBatch(ctx, "connect_four", 2)
    tiny_actions, _ = tiny.synth(SEED, C4_DEPTH_MOD)
    step_figures("a", tiny, tiny_actions)
    # (b) the headline batch, (d) the bare ctypes call at both sizes
    src = osa.StateBatch(ctx, "connect_four", args.states)
    actions, _ = src.synth(SEED, C4_DEPTH_MOD)
    step_figures("b", src, actions)
    # (c) the copy of the same bytes, issued as bench.py's copy_ceiling issues it
    half = (BYTES_PER_STATE * args.states // 2) // 16 * 16
    a = torch.zeros(half, dtype=torch.uint8, device="cuda")
    b = torch.empty(half, dtype=torch.uint8, device="cuda")
    measure("c_copy_bytes_us", lambda: check(lib().osg_copy_bytes(ctx._h, b.data_ptr(), a.data_ptr(), half)))
    rec["copy_bytes"] = 2 * half
    rec["spread_min_max_us"] = spread
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
