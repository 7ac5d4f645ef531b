"""Shared by tests/golden/make_action_value_vectors.py, tests/test_action_values_goldens.py,
tests/test_action_values_native.py and tests/test_z18_gpu_action_values.py: the goldens of the per-infostate action
values (tests/golden/action_value_vectors.npz), the policy tables of its cases and the input file of
tests/native/action_values_host_test.cpp."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE = 1e-12   # absolute, every output against the reference (the project's bound for fp64 tables: mmd_cases.TOLERANCE)
SMALL_GAMES = ("kuhn_poker", "kuhn_poker(players=3)", "kuhn_poker(players=5)", "leduc_poker")
LARGE_GAME = "leduc_poker(players=3)"
TWO_PLAYER = ("kuhn_poker", "leduc_poker")
POLICIES = ("uniform", "random", "first")
VECTORS = ("reach", "cf_reach", "chance_reach", "player_reach")          # [I]
TABLES = ("action_values", "cf_reach_by_value", "weighted_values")      # [I, Amax] and [I, Amax, P]
ROW_STRIDE = 16   # the large game records every 16th row of its tables, and their column sums,
VECTOR_STRIDE = 4  # and of the random table's [I] vectors every 4th row and their sums


def policy_table(kind, nact, amax, seed):
    """The case's policy in the legal-index layout, rows in sorted-key order; padding cells 0."""
    nact = np.asarray(nact)
    used = np.arange(amax)[None, :] < nact[:, None]
    if kind == "uniform":
        return np.where(used, 1.0 / nact[:, None], 0.0)
    if kind == "random":   # full support: weights U[0.05, 1) normalised
        w = np.where(used, np.random.RandomState(seed).uniform(0.05, 1.0, size=(len(nact), amax)), 0.0)
        return w / w.sum(axis=1, keepdims=True)
    if kind == "first":    # exact zeros: every row plays its first legal action
        out = np.zeros((len(nact), amax))
        out[:, 0] = 1.0
        return out
    raise ValueError(kind)


def load():
    with np.load(os.path.join(ROOT, "tests", "golden", "action_value_vectors.npz")) as z:
        return {k: z[k] for k in z.files}


def keys_of(v, game):
    return bytes(v[f"{game}/keys"]).decode().split("\n")


def case_names(v, game=None):
    names = bytes(v["cases"]).decode().split("\n")
    return [c for c in names if game is None or bytes(v[f"{c}/game"]).decode() == game]


def case_policy(v, case):
    game = bytes(v[f"{case}/game"]).decode()
    return policy_table(bytes(v[f"{case}/policy"]).decode(), v[f"{game}/nact"], v[f"{game}/legal"].shape[1], int(v["seed"]))


def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "action_values_host_test.cpp"), "-o", path])
    return path


def tree_links(nchild):
    """(parent, first_child) of every history from the children counts of the level-ordered tree."""
    nchild = np.asarray(nchild, np.int64)
    first_child = 1 + np.concatenate([[0], np.cumsum(nchild)[:-1]])
    parent = np.full(len(nchild), -1, np.int64)
    parent[1:] = np.repeat(np.arange(len(nchild)), nchild)
    return parent.astype(np.int32), np.where(nchild > 0, first_child, 0).astype(np.int32)


def write_cases(v, game, path):
    """The game's flattened tree and every case of the game for the host program; returns the case names in file order.
    Header: H, I, A, P, M, cases; then the tree arrays, then per case: responder, best_response_value, the policy and
    every expected output."""
    cases = case_names(v, game)
    g = lambda name: v[f"{game}/{name}"]
    I, A = g("legal").shape
    H, P, M = len(g("nchild")), int(g("num_players")), len(g("mem"))
    parent, _ = tree_links(g("nchild"))
    term_ret = np.zeros((H, P))
    term_ret[g("kind") == 2] = g("term_ret")
    with open(path, "wb") as f:
        f.write(np.array([H, I, A, P, M, len(cases)], np.int32).tobytes())
        f.write(parent.tobytes())
        for name in ("kind", "actor", "info", "nact", "player", "mem_off", "mem"):
            f.write(np.ascontiguousarray(g(name), np.int32).tobytes())
        f.write(np.ascontiguousarray(g("edge_prob"), np.float64).tobytes())
        f.write(np.ascontiguousarray(term_ret, np.float64).tobytes())
        for c in cases:
            responder = int(v[f"{c}/responder"])
            f.write(np.array([responder, 0], np.int32).tobytes())
            f.write(np.array([v[f"{c}/best_response_value"] if responder >= 0 else 0.0], np.float64).tobytes())
            f.write(np.ascontiguousarray(case_policy(v, c), np.float64).tobytes())
            f.write(np.ascontiguousarray(v[f"{c}/best_index"] if responder >= 0 else np.full(I, -1), np.int32).tobytes())
            f.write(np.ascontiguousarray(v[f"{c}/root_values"], np.float64).tobytes())
            for name in VECTORS + TABLES:
                f.write(np.ascontiguousarray(v[f"{c}/{name}"], np.float64).tobytes())
    return cases
