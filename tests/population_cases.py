"""Shared by tests/golden/make_population_vectors.py, tests/test_population_goldens.py, tests/test_population_native.py
and tests/test_z24_gpu_population.py: the goldens of the payoff tensors and the aggregated policies of a population
(tests/golden/population_vectors.npz), the policy tables of its cases, their profile lists and weight matrices, and the
input file of tests/native/population_host_test.cpp.  The layout (rows, legal actions) and the flattened trees of the
small games are those of tests/golden/action_value_vectors.npz."""
import itertools
import os
import subprocess

import numpy as np

import action_value_cases as avc

ROOT = avc.ROOT
TOLERANCE = avc.TOLERANCE   # 1e-12 absolute against the reference: returns are at most 13 in magnitude, probabilities at most 1
SMALL_GAMES = avc.SMALL_GAMES
LARGE_GAME = avc.LARGE_GAME
GAMES = SMALL_GAMES + (LARGE_GAME,)
KINDS = ("uniform", "random", "first", "random2")
SEED2_OFFSET = 1000        # "random2" is policy_table("random") with the action values' seed + this
WEIGHT_SEED = 20240        # + player: the seeded weight matrix
EPSILON = 1e-40            # PolicyAggregator's default
ROW_STRIDE = avc.ROW_STRIDE
# the tables whose goldens are recorded, per game
RECORDED_KINDS = {"kuhn_poker": KINDS, "leduc_poker": KINDS, "kuhn_poker(players=3)": KINDS,
                  "kuhn_poker(players=5)": KINDS[:2], LARGE_GAME: KINDS[:3]}
RECORDED_WEIGHTS = {"kuhn_poker": ("uniform", "seeded", "onehot"), "leduc_poker": ("uniform", "seeded", "onehot"),
                    "kuhn_poker(players=3)": ("uniform", "seeded", "onehot"), "kuhn_poker(players=5)": ("seeded", "onehot"),
                    LARGE_GAME: ("seeded",)}
LARGE_PROFILES = ((0, 0, 0), (0, 1, 2), (2, 1, 0), (1, 1, 1))


def colsum_tolerance(rows):
    """The bound for a column sum over `rows` rows of probabilities (np.sum(axis=0), row after row): every cell within
    TOLERANCE, and two running sums of at most `rows` that each round `rows` times by at most half a spacing."""
    return rows * TOLERANCE + rows * float(np.spacing(float(rows)))


def table(kind, nact, amax, seed):
    """One policy table of a population in the legal-index layout (action_value_cases.policy_table)."""
    if kind == "random2":
        return avc.policy_table("random", nact, amax, seed + SEED2_OFFSET)
    return avc.policy_table(kind, nact, amax, seed)


def table_stack(kinds, nact, amax, seed):
    return np.stack([table(k, nact, amax, seed) for k in kinds])


def all_profiles(P, K):
    return np.array(list(itertools.product(range(K), repeat=P)), np.int32).reshape(-1, P)


def recorded_profiles(game, P):
    if game == LARGE_GAME:
        return np.array(LARGE_PROFILES, np.int32)
    return all_profiles(P, len(RECORDED_KINDS[game]))


def weight_matrix(kind, P, K):
    """[P, K] rows on the simplex.  "uniform": 1 / K.  "seeded": a seeded draw of U[0.1, 1) normalised, and where there
    are more than two tables an exact zero for player p at table p mod K (a different table for each of up to K players).
    "onehot": player p plays table (p + 1) mod K alone."""
    if kind == "uniform":
        return np.full((P, K), 1.0 / K)
    if kind == "seeded":
        w = np.stack([np.random.RandomState(WEIGHT_SEED + p).uniform(0.1, 1.0, size=K) for p in range(P)])
        if K > 2:
            w[np.arange(P), np.arange(P) % K] = 0.0
        return w / w.sum(axis=1, keepdims=True)
    if kind == "onehot":
        w = np.zeros((P, K))
        w[np.arange(P), (np.arange(P) + 1) % K] = 1.0
        return w
    raise ValueError(kind)


def splice(tables, profile, player):
    """The table whose rows at player p's infostates come from tables[profile[p]]."""
    tables, player = np.asarray(tables), np.asarray(player)
    return tables[np.asarray(profile)[player], np.arange(tables.shape[1])]


def load():
    with np.load(os.path.join(ROOT, "tests", "golden", "population_vectors.npz")) as z:
        return {k: z[k] for k in z.files}


def kinds_of(v, game):
    return bytes(v[f"{game}/tables"]).decode().split("\n")


def weights_of(v, game):
    return bytes(v[f"{game}/weight_kinds"]).decode().split("\n")


def recorded_stack(v, game):
    return table_stack(kinds_of(v, game), v[f"{game}/nact"], int(v[f"{game}/amax"]), int(v["seed"]))


def build_host_test(path, extra=()):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off", *extra,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "population_host_test.cpp"), "-o", path])
    return path


def write_cases(v, av, game, path):
    """The game's flattened tree (from the action values' goldens `av`) and every recorded case of the game for the host
    program.  Header: H, I, A, P, M, K, profiles, weight matrices; the tree arrays; epsilon; the table stack; the profiles
    and their returns; per weight matrix the weights and the aggregated table."""
    g = lambda name: av[f"{game}/{name}"]
    I, A = g("legal").shape
    H, P, M = len(g("nchild")), int(g("num_players")), len(g("mem"))
    parent, _ = avc.tree_links(g("nchild"))
    term_ret = np.zeros((H, P))
    term_ret[g("kind") == 2] = g("term_ret")
    stack = recorded_stack(v, game)
    profiles, names = v[f"{game}/profiles"], weights_of(v, game)
    with open(path, "wb") as f:
        f.write(np.array([H, I, A, P, M, len(stack), len(profiles), len(names)], np.int32).tobytes())
        f.write(parent.tobytes())
        for name in ("kind", "actor", "info", "nact", "player", "mem_off", "mem"):
            f.write(np.ascontiguousarray(g(name), np.int32).tobytes())
        f.write(np.ascontiguousarray(g("edge_prob"), np.float64).tobytes())
        f.write(np.ascontiguousarray(term_ret, np.float64).tobytes())
        f.write(np.array([float(v["epsilon"])], np.float64).tobytes())
        f.write(np.ascontiguousarray(stack, np.float64).tobytes())
        f.write(np.ascontiguousarray(profiles, np.int32).tobytes())
        f.write(np.ascontiguousarray(v[f"{game}/returns"], np.float64).tobytes())
        for name in names:
            f.write(np.ascontiguousarray(v[f"{game}/weights/{name}"], np.float64).tobytes())
            f.write(np.ascontiguousarray(v[f"{game}/aggregate/{name}"], np.float64).tobytes())
    return len(profiles), len(names)
