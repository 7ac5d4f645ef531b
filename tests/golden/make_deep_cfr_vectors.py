#!/usr/bin/env python3
"""Golden runs of Deep CFR, produced by RUNNING the reference's own open_spiel/python/pytorch/deep_cfr.py (imported
unmodified from where it lies) over the genuine games (oracle/_ref/libspiel_ref.so through oracle/pyspiel_over_capi.py).
Run in the build container (needs the reference sources; CPU only, under a minute):

    python tests/golden/make_deep_cfr_vectors.py

What is scripted, and only that: the module-level `np` of deep_cfr.py is a proxy whose `random` takes its draws from the
device's counter streams (tests/deep_cfr_cases.py) —
  choice(a, p=)        NumPy's rule (cdf = cumsum(p); cdf /= cdf[-1]; searchsorted(u, side="right")) on the next uniform
                       of the running trajectory's stream Rng(seed, g, 0);
  randint(0, n + 1)    the reservoir rule of the buffer being appended to: mulhi64(Rng(res_seed, n, stream).next(), n + 1),
                       stream = the player for an advantage buffer, P for the strategy buffer;
  choice(n, size=, replace=False)   the restated sample (the m smallest keys) — only the training of the reference's
                       networks consumes it, and the goldens record the networks' outputs, not the rule.
The `tree` module (dm-tree, not installed here) is a stand-in with map_structure over NamedTuples.  The restated choice
rule is checked below against genuine np.random.RandomState(k).choice(p=...) fed the uniform RandomState(k).random_sample()
yields, over many k.

The maker drives the reference's loop itself (solve(), deep_cfr.py:369-390, one call at a time) so that it can record,
per (iteration, player) step, what every player's advantage network answers for every infostate (batch-of-one forward
passes, as _sample_action_from_advantage makes them).

Output: tests/golden/deep_cfr_vectors.npz (np.savez_compressed).  `runs` lists "<game>|<capacity>".
  "tree/<game>/": parent, kind (0 chance, 1 decision, 2 terminal), action, prob, actor, info [H], returns [H, P] — the game
      tree depth first (a parent before its children, children in action order), info an index into the infostates in
      order of first visit; keys_bytes / keys_len their strings, tensors [I, E] f32, player [I], legal [I, A] (-1 padded).
  "r<r>/": capacity, traversals, iterations, seed (trajectory streams), res_seed, players, steps; per step "s<s>/":
      iteration, player, first (global index of the step's first trajectory), advantages [I, A] f32 (row i from the
      network of infostate i's player), draws [T], adv_off / strat_off [T + 1], adv_info / strat_info [R], adv_vals /
      strat_vals [R, A] f32 in append order, and per buffer b (player b's advantage buffer; b = P the strategy buffer)
      "b<b>/": add_calls, info, iteration, values of the filled slots after the step.

Asserted here: the three branches of the strategy rule all occur at visited nodes; in the small-capacity runs add_calls
crosses the capacity inside one player's step and at least one slot is overwritten twice within a step."""
import importlib.machinery
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deep_cfr_cases as dc   # noqa: E402

SEED, RES_SEED = 0xDEE9CF5, 0x5EED0B0F
# game, capacity, traversals per step, iterations, advantage layers, batch size of the advantage training
RUNS = [("kuhn_poker", 12, 8, 3, (8,), 6), ("kuhn_poker", 1 << 12, 8, 2, (8,), 6),
        ("kuhn_poker(players=3)", 24, 6, 2, (8,), 6), ("leduc_poker", 48, 5, 2, (12, 8), 16),
        ("leduc_poker", 1 << 14, 4, 2, (12, 8), 16)]


def tree_stand_in():
    mod = types.ModuleType("tree")
    mod.__spec__ = importlib.machinery.ModuleSpec("tree", None)

    def map_structure(fn, *structs):
        first = structs[0]
        if isinstance(first, tuple):
            return type(first)(*[map_structure(fn, *leaves) for leaves in zip(*structs)])
        return fn(*structs)

    mod.map_structure = map_structure
    sys.modules["tree"] = mod


def reference_modules():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference_py)
    tree_stand_in()
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from open_spiel.python.pytorch import deep_cfr
    return pyspiel, deep_cfr


class Script:
    """np.random of deep_cfr.py."""

    def __init__(self):
        self.rng = None          # the running trajectory's stream
        self.buffer = None       # stream of the buffer being appended to
        self.indices = []

    def seed(self, _):
        pass

    def choice(self, a, size=None, replace=True, p=None):
        if p is None:            # ReservoirBuffer.sample
            assert not replace and isinstance(a, int)
            m = int(size[0])
            keys = sorted((dc.sample_key(RES_SEED ^ 0x5A, 99, k), k) for k in range(a))
            return np.array([k for _, k in keys[:m]], np.int64)
        idx = dc.choice([float(x) for x in p], self.rng.unit())
        return list(a)[idx]

    def randint(self, low, high):
        n = int(high) - 1
        assert low == 0 and self.buffer is not None
        idx = dc.reservoir_index(RES_SEED, self.buffer, n)
        self.indices.append(idx)
        return idx

    def shuffle(self, _):
        raise AssertionError("the golden runs train from sampled batches")


class NumpyProxy:
    def __init__(self, script):
        self.random = script

    def __getattr__(self, name):
        return getattr(np, name)


def check_choice_rule():
    """dc.choice against genuine RandomState.choice(p=) on the same uniform."""
    gen = np.random.default_rng(5)
    for k in range(4000):
        n = int(gen.integers(1, 9))
        p = gen.random(n)
        if k % 3 == 0:
            p[gen.integers(0, n)] = 0.0
        if p.sum() == 0:
            p[0] = 1.0
        p = p / p.sum()
        u = np.random.RandomState(k).random_sample()
        want = int(np.random.RandomState(k).choice(n, p=p))
        assert dc.choice(list(p), u) == want, (k, p, u)
    for u, want in ((0.0, 0), (0.5, 1), (np.nextafter(0.5, 0), 0), (np.nextafter(1.0, 0), 1)):   # cdf_k <= u goes past k
        assert dc.choice([0.5, 0.5], u) == want


def game_tree(pyspiel, game_string):
    game = pyspiel.load_game(game_string)
    P, A = game.num_players(), game.num_distinct_actions()
    rec = dict(parent=[], kind=[], action=[], prob=[], actor=[], info=[], returns=[])
    keys, tensors, player, legal = [], [], [], []
    index = {}

    def walk(state, parent, action, prob):
        h = len(rec["parent"])
        rec["parent"].append(parent); rec["action"].append(action); rec["prob"].append(prob)
        if state.is_terminal():
            rec["kind"].append(2); rec["actor"].append(-1); rec["info"].append(-1); rec["returns"].append(list(state.returns()))
            return
        rec["returns"].append([0.0] * P)
        if state.is_chance_node():
            rec["kind"].append(0); rec["actor"].append(-1); rec["info"].append(-1)
            for a, pr in state.chance_outcomes():
                walk(state.child(a), h, a, pr)
            return
        cur = state.current_player()
        key = state.information_state_string(cur)
        if key not in index:
            index[key] = len(keys)
            keys.append(key)
            tensors.append(np.array(state.information_state_tensor(cur), np.float32))
            player.append(cur)
            la = list(state.legal_actions())
            assert la == sorted(la) and len(la) <= A
            legal.append(la + [-1] * (A - len(la)))
        rec["kind"].append(1); rec["actor"].append(cur); rec["info"].append(index[key])
        for a in state.legal_actions():
            walk(state.child(a), h, a, 0.0)

    walk(game.new_initial_state(), -1, -1, 0.0)
    blob = "".join(keys).encode()
    out = dict(parent=np.array(rec["parent"], np.int32), kind=np.array(rec["kind"], np.int8), action=np.array(rec["action"], np.int32),
               prob=np.array(rec["prob"], np.float64), actor=np.array(rec["actor"], np.int8), info=np.array(rec["info"], np.int32),
               returns=np.array(rec["returns"], np.float64), keys_bytes=np.frombuffer(blob, np.uint8),
               keys_len=np.array([len(k.encode()) for k in keys], np.int32), tensors=np.array(tensors, np.float32),
               player=np.array(player, np.int8), legal=np.array(legal, np.int32))
    assert len({t.tobytes() for t in tensors}) == len(tensors), "two infostates share a tensor"
    return game, out, {t.tobytes(): i for i, t in enumerate(tensors)}


def make_run(pyspiel, deep_cfr, torch, script, spec, trees, out, r, seen_branches):
    game_string, capacity, traversals, iterations, layers, batch = spec
    game, tree, by_tensor = trees[game_string]
    P, A = game.num_players(), game.num_distinct_actions()
    I = len(tree["player"])
    solver = deep_cfr.DeepCFRSolver(game, policy_network_layers=(8,), advantage_network_layers=layers, num_iterations=iterations,
                                    num_traversals=traversals, learning_rate=1e-2, batch_size_advantage=batch,
                                    batch_size_strategy=batch, memory_capacity=capacity, advantage_network_train_steps=3, seed=11 + r)
    rows = {"adv": [], "strat": []}

    def hooked(kind, stream, inner):
        def call(*args):
            data = args[-1]
            script.buffer = stream
            inner(*args)
            script.buffer = None
            rows[kind].append((by_tensor[np.asarray(data[0], np.float32).tobytes()], np.asarray(data[2], np.float32).copy()))
        return call

    inner_adv = solver._append_to_advantage_buffer
    solver._append_to_advantage_buffer = lambda player, data: hooked("adv", player, inner_adv)(player, data)
    solver._append_to_stategy_buffer = hooked("strat", P, solver._append_to_stategy_buffer)

    p = f"r{r}/"
    out.update({p + "capacity": capacity, p + "traversals": traversals, p + "iterations": iterations, p + "seed": SEED + r,
                p + "res_seed": RES_SEED, p + "players": P})
    ctree = dc.Tree(tree["parent"], tree["kind"], tree["action"], tree["prob"], tree["actor"], tree["info"], tree["returns"], tree["legal"])
    visited_branches = set()
    crossed = twice = False
    step = 0
    for it in range(1, iterations + 1):
        assert solver._iteration == it
        for player in range(P):
            q = f"{p}s{step}/"
            with torch.inference_mode():
                adv = np.stack([solver._advantage_networks[int(tree["player"][i])](
                    torch.FloatTensor(np.expand_dims(tree["tensors"][i], axis=0)))[0].cpu().numpy() for i in range(I)]).astype(np.float32)
            _, branch = dc.strategy_table(ctree, adv)
            first = ((it - 1) * P + player) * traversals
            draws, adv_rows, strat_rows = [], [], []
            before = [None if b is None else int(b.add_calls) for b in solver._advantage_memories + [solver._strategy_memories]]
            for j in range(traversals):
                script.rng = dc.Rng(SEED + r, first + j, 0)
                rows["adv"], rows["strat"] = [], []
                solver._traverse_game_tree(solver._root_node, player)
                draws.append(script.rng.draws)
                adv_rows.append(rows["adv"]); strat_rows.append(rows["strat"])
                for i, _ in rows["adv"] + rows["strat"]:
                    visited_branches.add(int(branch[i]))
            script.rng = None
            ao, ai, av = dc.flatten(adv_rows, A)
            so, si, sv = dc.flatten(strat_rows, A)
            out.update({q + "iteration": it, q + "player": player, q + "first": first, q + "advantages": adv,
                        q + "draws": np.array(draws, np.int32), q + "adv_off": ao, q + "adv_info": ai, q + "adv_vals": av,
                        q + "strat_off": so, q + "strat_info": si, q + "strat_vals": sv})
            for b, mem in enumerate(solver._advantage_memories + [solver._strategy_memories]):
                if mem is None:
                    continue
                n = len(mem)
                info = np.array([by_tensor[mem.experience[0][k].tobytes()] for k in range(n)], np.int32)
                out.update({q + f"b{b}/add_calls": int(mem.add_calls), q + f"b{b}/info": info,
                            q + f"b{b}/iteration": mem.experience[1][:n, 0].astype(np.int32),
                            q + f"b{b}/values": mem.experience[2][:n].astype(np.float32)})
                was = before[b] or 0
                if was < capacity < int(mem.add_calls):
                    crossed = True
                writes = [dc.reservoir_slot(RES_SEED, b, n, capacity) for n in range(was, int(mem.add_calls))]
                writes = [w for w in writes if w >= 0]
                if len(writes) != len(set(writes)):
                    twice = True
            if solver._reinitialize_advantage_networks:
                solver._reinitialize_advantage_network(player)
            solver._learn_advantage_network(player)
            step += 1
        solver._iteration += 1
    out[p + "steps"] = step
    seen_branches |= visited_branches
    print(f"{game_string} capacity {capacity}: {step} steps, branches at visited nodes {sorted(visited_branches)}, "
          f"crossed {crossed}, a slot overwritten twice within a step {twice}")
    return crossed, twice


def main():
    check_choice_rule()
    pyspiel, deep_cfr = reference_modules()
    import torch
    torch.set_num_threads(1)
    script = Script()
    deep_cfr.np = NumpyProxy(script)
    out = {"runs": np.array([f"{g}|{c}" for g, c, *_ in RUNS])}
    trees = {}
    for g in sorted({s[0] for s in RUNS}):
        trees[g] = game_tree(pyspiel, g)
        out.update({f"tree/{g}/{k}": v for k, v in trees[g][1].items()})
    branches = set()
    for r, spec in enumerate(RUNS):
        crossed, twice = make_run(pyspiel, deep_cfr, torch, script, spec, trees, out, r, branches)
        if spec[1] < 1000:
            assert crossed and twice, "the small-capacity run must cross its capacity inside a step and overwrite a slot twice"
        else:
            assert not crossed
    assert branches == {0, 1, 2}, branches
    np.savez_compressed(dc.GOLDEN, **out)
    print(dc.GOLDEN, os.path.getsize(dc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
