"""Shared by tests/test_mmd_native.py and tests/test_z17_gpu_mmd.py: the goldens of magnetic mirror descent
(tests/golden/mmd_vectors.npz) and the input file of tests/native/mmd_host_test.cpp."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE = 1e-12   # absolute, for x, avg_x, pi and the gap against the reference (the issue's bound)
GAMES = ("kuhn_poker", "leduc_poker")


def load():
    with np.load(os.path.join(ROOT, "tests", "golden", "mmd_vectors.npz")) as z:
        return {k: z[k] for k in z.files}


def run_names(v, game=None):
    names = bytes(v["runs"]).decode().split("\n")
    return [r for r in names if game is None or bytes(v[f"{r}/game"]).decode() == game]


def keys_of(v, game):
    return bytes(v[f"{game}/keys"]).decode().split("\n")


def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "mmd_host_test.cpp"), "-o", path])
    return path


def write_cases(v, game, path):
    """The game's layout renumbered breadth-first (new row = bfs_rank[row]) and every run of the game, the kuhn_poker
    QRE fixed point as a last run; returns [(run name, checkpoints)] in file order."""
    rank = v[f"{game}/bfs_rank"]
    I, A = v[f"{game}/legal"].shape
    order = np.argsort(rank)   # order[new] = old

    def cells(c):   # a cell index in the new numbering (-1 stays)
        c = np.asarray(c)
        return np.where(c < 0, -1, rank[np.maximum(c, 0) // A] * A + np.maximum(c, 0) % A).astype(np.int32)

    def table(t):
        return np.ascontiguousarray(np.asarray(t, np.float64)[order]).tobytes()

    pred = v[f"{game}/pred_info"][order]
    runs = run_names(v, game)
    defaults = sorted(k for k in v if k.startswith(f"{game}/default_stepsize/"))
    listed = []
    with open(path, "wb") as f:
        f.write(np.array([I, A, len(v[f"{game}/term_seq"]), len(runs) + (game == "kuhn_poker"), len(defaults)], np.int32).tobytes())
        f.write(v[f"{game}/nact"][order].astype(np.int32).tobytes())
        f.write(v[f"{game}/player"][order].astype(np.int32).tobytes())
        f.write(np.where(pred < 0, -1, rank[np.maximum(pred, 0)]).astype(np.int32).tobytes())
        f.write(v[f"{game}/pred_action"][order].astype(np.int32).tobytes())
        f.write(np.ascontiguousarray(cells(v[f"{game}/term_seq"])).tobytes())
        f.write(np.ascontiguousarray(v[f"{game}/term_cu"], np.float64).tobytes())
        for k in defaults:
            f.write(np.array([float(k.rsplit("/", 1)[1]), float(v[k])], np.float64).tobytes())
        for r in runs:
            C = len(v[f"{r}/t"])
            f.write(np.array([C, 0], np.int32).tobytes() + np.array([TOLERANCE], np.float64).tobytes())
            for c in range(C):
                f.write(np.array([v[f"{r}/iters"][c]], np.int32).tobytes())
                f.write(np.array([v[f"{r}/alpha"][c], v[f"{r}/stepsize"][c], v[f"{r}/gap"][c]], np.float64).tobytes())
                f.write(table(v[f"{r}/x"][c]) + table(v[f"{r}/avg_x"][c]) + table(v[f"{r}/pi"][c]))
            listed.append((r, C))
        if game == "kuhn_poker":   # the QRE: its own gap at it (no update), then one update from it
            # (the 8-digit vectors are not a consistent sequence form beyond 1e-8, so its bounds are the reference's own,
            # rtol 1e-6 against the QRE and a gap <= 1e-6, which the callers check on the tables the program leaves)
            f.write(np.array([2, 1], np.int32).tobytes() + np.array([np.inf], np.float64).tobytes())
            f.write(table(v["qre/pi"]) + table(v["qre/x"]))
            f.write(np.array([0], np.int32).tobytes())
            f.write(np.array([v["qre/alpha"], v["qre/stepsize"], v["qre/gap"]], np.float64).tobytes())
            f.write(table(v["qre/x"]) + table(v["qre/x"]) + table(v["qre/pi"]))
            f.write(np.array([1], np.int32).tobytes())
            f.write(np.array([v["qre/alpha"], v["qre/stepsize"], np.nan], np.float64).tobytes())
            f.write(table(v["qre/x_after"]) + table(v["qre/avg_x_after"]) + table(v["qre/pi_after"]))
            listed.append(("qre", 2))
    return listed


def read_host_tables(v, game, listed, path):
    """{(run, checkpoint): (x, avg_x, pi, gap)} the host program left (argv[3]), back in the goldens' row order."""
    rank = v[f"{game}/bfs_rank"]
    I, A = v[f"{game}/legal"].shape
    raw = np.fromfile(path, np.float64)
    out, at = {}, 0
    for r, C in listed:
        for c in range(C):
            x, avg, pi = (raw[at + k * I * A: at + (k + 1) * I * A].reshape(I, A)[rank] for k in range(3))
            out[(r, c)] = (x, avg, pi, raw[at + 3 * I * A])
            at += 3 * I * A + 1
    return out
