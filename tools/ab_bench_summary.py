#!/usr/bin/env python3
"""The table of an A/B of the headline from the output directories of tools/ab_bench.sh, one per lease:
every pair's value, ms_per_step, a_step_us and b_step_us for both trees; medians, ranges and spreads per lease and
pooled; whether the change's median lies beyond the parent's BEST run of the lease; the traced k_step_c4std2 figures;
the `bench.py --full` pair of each lease.
  python tools/ab_bench_summary.py <lease 1 directory> <lease 2 directory> ...   > profiles/<tag>_step_ab.txt"""
import csv
import json
import os
import statistics
import sys

FULL_KEYS = ["value", "ms_per_step", "roofline.hbm_avg_launch_us", "roofline.avg_launch_us", "persistent.value",
             "secondary.mcts.value", "secondary.cfr.value", "secondary.mccfr.value", "secondary.env_step.value",
             "secondary.hex_step.value"]


def last_json(path):
    with open(path) as f:
        for line in reversed(f.read().strip().splitlines()):
            if line.strip().startswith("{"):
                return json.loads(line)
    raise SystemExit(f"no JSON line in {path}")


def get(rec, dotted):
    for k in dotted.split("."):
        rec = rec.get(k) if isinstance(rec, dict) else None
    return rec


def main():
    leases = sys.argv[1:]
    rows = []
    for li, d in enumerate(leases, 1):
        for p in range(1, 6):
            r = {"lease": li, "pair": p}
            for tree in ("parent", "change"):
                b, f = last_json(f"{d}/{tree}_bench_{p}.log"), last_json(f"{d}/{tree}_floor_{p}.log")
                r[tree] = (b["value"], b["ms_per_step"], f["a_step_us"], f["b_step_us"])
            rows.append(r)
    print("lease pair   parent value  ms_per_step a_step_us b_step_us   change value  ms_per_step a_step_us b_step_us")
    for r in rows:
        print(f"{r['lease']:5d} {r['pair']:4d}   " +
              "   ".join(f"{v[0]:12.4e} {v[1]:10.6f} {v[2]:9.3f} {v[3]:9.3f}" for v in (r["parent"], r["change"])))

    def line(label, sel, k, name, higher):
        pa = [r["parent"][k] for r in rows if sel(r)]
        ch = [r["change"][k] for r in rows if sel(r)]
        mp, mc = statistics.median(pa), statistics.median(ch)
        best = max(pa) if higher else min(pa)
        beyond = mc > best if higher else mc < best
        print(f"{label}: {name} ({'higher' if higher else 'lower'} is better): parent median {mp:.6g} (range {min(pa):.6g}-{max(pa):.6g}, "
              f"spread (max-min)/median {(max(pa) - min(pa)) / mp * 100:.2f} %), change median {mc:.6g} (range {min(ch):.6g}-{max(ch):.6g}, "
              f"spread {(max(ch) - min(ch)) / mc * 100:.2f} %): {(mc / mp - 1) * 100:+.2f} %; parent's best {best:.6g}: "
              f"change median {'beyond it' if beyond else 'NOT beyond it'}")

    groups = [(f"all {len(rows)} pairs", lambda r: True)] + [(f"lease {i}", lambda r, i=i: r["lease"] == i) for i in range(1, len(leases) + 1)]
    for label, sel in groups:
        for k, (name, higher) in enumerate((("value", True), ("ms_per_step", False), ("a_step_us", False), ("b_step_us", False))):
            line(label, sel, k, name, higher)

    print("\ntraced k_step_c4std2 (rocprofv3 --kernel-trace --stats of `python bench.py`, one run per tree and lease, nothing else traced):")
    for li, d in enumerate(leases, 1):
        for tree in ("parent", "change"):
            path = f"{d}/kernel_stats_{tree}.csv"
            if not os.path.exists(path):
                continue
            with open(path) as f:
                for r in csv.DictReader(f):
                    if "k_step_c4std2" in r["Name"]:
                        print(f"  lease {li} {tree:6s}: {r['Calls']} launches, avg {float(r['AverageNs']) / 1e3:.3f} us, "
                              f"min {float(r['MinNs']) / 1e3:.3f} us, max {float(r['MaxNs']) / 1e3:.3f} us")

    print("\nbench.py --full, one alternating pair per lease (parent, change, change / parent):")
    for li, d in enumerate(leases, 1):
        if not os.path.exists(f"{d}/change_full.log"):
            continue
        pa, ch = last_json(f"{d}/parent_full.log"), last_json(f"{d}/change_full.log")
        for k in FULL_KEYS:
            a, b = get(pa, k), get(ch, k)
            if isinstance(a, (int, float)) and isinstance(b, (int, float)) and a:
                print(f"  {li} {k:38s} {a:14.6g} {b:14.6g} {b / a:8.4f}")
        print(f"  {li} parity_checked_states {get(pa, 'parity.parity_checked_states') or get(pa, 'parity_checked_states')} / "
              f"{get(ch, 'parity.parity_checked_states') or get(ch, 'parity_checked_states')}")


if __name__ == "__main__":
    main()
