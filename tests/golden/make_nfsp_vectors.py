#!/usr/bin/env python3
"""Golden runs of NFSP, produced by RUNNING the reference's own open_spiel/python/pytorch/nfsp.py and dqn.py (imported
unmodified from where they lie) under the loop of open_spiel/python/examples/kuhn_nfsp.py, over the genuine games
(oracle/_ref/libspiel_ref.so through oracle/pyspiel_over_capi.py) inside the reference's rl_environment.Environment.
Run in the build container (needs the reference sources; CPU only, under a minute):

    python tests/golden/make_nfsp_vectors.py

What is scripted, and only that: the module-level `np` of nfsp.py and dqn.py is a proxy whose `random` takes its draws
from the device's counter streams (tests/nfsp_cases.py) —
  uniform()            the mode draw (_sample_episode_policy): the k-th call is draw k % P of episode k // P's stream
                       Rng(seed, g, 0) (agent p draws the mode of its next episode when the running one ends);
  rand()               the explore test of _act_epsilon_greedy: the next uniform of the running episode's stream;
  choice(list)         the explore action: list[below(len(list))] on the next draw;
  choice(arange, p=)   the average policy's action: NumPy's rule (cdf = cumsum(p); cdf /= cdf[-1];
                       searchsorted(u, side="right")) on the next uniform;
  randint(0, n + 1)    the reservoir rule of the buffer being appended to: mulhi64(Rng(res_seed, n, p).next(), n + 1);
and the environment's chance_event_sampler (a constructor argument) takes choice(p=) over state.chance_outcomes() on the
next uniform of the episode's stream.  The `tree` module (dm-tree, not installed here) is the stand-in of
make_deep_cfr_vectors.py, and enum.StrEnum (Python 3.11) a two-line stand-in where Python is older.  The restated
choice rule is checked against genuine np.random.RandomState as that maker does.

The networks are frozen by parameters only: min_buffer_size_to_learn is huge, so learn() returns before it samples, and
epsilon_start == epsilon_end makes the exponential schedule exactly constant.  A run records what the Q network and the
average-policy network of every infostate's player answer (batch-of-one forward passes, as _act_epsilon_greedy and _act
make them), then per chunk of episodes every row in append order and after the chunk every buffer slot and counter.

Output: tests/golden/nfsp_vectors.npz (np.savez_compressed).  `runs` lists "<game>|<tag>".
  "tree/<game>/": as in deep_cfr_vectors.npz.
  "r<r>/": ring_capacity, res_capacity, episodes (per chunk), chunks, seed, res_seed, players, eps [P], anticipatory [P],
      q [I, A] f32, avg [I, A] f32; per chunk "c<c>/": first, draws [E], modes [E] (bit p: BEST_RESPONSE), the rows in the
      layout of nfsp_cases.flatten_chunk (ring_off, ring_info, ring_action, ring_reward, ring_next, ring_final; sl_off,
      sl_info, sl_probs), dqn_steps / nfsp_steps [P] (the agents' counters), and per player b "ring<b>/" entry_index and
      the filled slots' columns, "res<b>/" add_calls, info, probs.

Asserted here: both modes occur for every player and both branches of the epsilon-greedy rule (in the runs that mix
them); in the small-capacity runs a ring wraps more than once and a reservoir slot is overwritten twice inside one
chunk."""
import enum
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import deep_cfr_cases as dc   # noqa: E402
import nfsp_cases as nc       # noqa: E402
import make_deep_cfr_vectors as mk   # noqa: E402

SEED, RES_SEED = 0x2F5B0C1, 0x5EED0F5B
HUGE = 1 << 40
# game, tag, anticipatory, epsilon, ring capacity, reservoir capacity, episodes per chunk, chunks, hidden layers
RUNS = [("kuhn_poker", "mixed", 0.5, 0.3, 7, 5, 40, 3, (8,)),
        ("kuhn_poker", "roomy", 0.5, 0.3, 1 << 12, 1 << 12, 40, 2, (8,)),
        ("kuhn_poker(players=3)", "mixed", 0.5, 0.3, 9, 6, 40, 3, (8,)),
        ("leduc_poker", "mixed", 0.5, 0.3, 16, 10, 40, 3, (12, 8)),
        ("kuhn_poker", "dqn", 1.0, 0.3, 7, 5, 30, 2, (8,)),
        ("leduc_poker", "average", 0.0, 0.3, 16, 10, 30, 2, (12, 8))]


def reference_modules():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference_py)
    mk.tree_stand_in()
    if not hasattr(enum, "StrEnum"):
        class StrEnum(str, enum.Enum):
            __str__ = str.__str__
        enum.StrEnum = StrEnum
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from open_spiel.python import rl_environment
    from open_spiel.python.pytorch import dqn, nfsp
    return pyspiel, rl_environment, dqn, nfsp


class Script:
    """np.random of nfsp.py and dqn.py, and the environment's chance sampler."""

    def __init__(self):
        self.seed_value, self.players = 0, 1
        self.uniform_calls = 0
        self.rng = None          # the running episode's stream
        self.buffer = None       # stream of the reservoir being appended to
        self.branches = [0, 0]   # explore, greedy
        self.eps = None

    def start_run(self, seed, players, eps):
        self.seed_value, self.players, self.uniform_calls, self.eps = seed, players, 0, eps

    def start_episode(self, g):
        self.rng = dc.Rng(self.seed_value, g, 0)
        for _ in range(self.players):
            self.rng.unit()

    def seed(self, _=None):
        pass

    def uniform(self):
        k = self.uniform_calls
        self.uniform_calls += 1
        rng = dc.Rng(self.seed_value, k // self.players, 0)
        for _ in range(k % self.players):
            rng.unit()
        return rng.unit()

    def rand(self):
        u = self.rng.unit()
        self.branches[0 if u < self.eps else 1] += 1
        return u

    def choice(self, a, size=None, replace=True, p=None):
        assert size is None, "the golden runs never learn"
        if p is None:
            a = list(a)
            return a[self.rng.below(len(a))]
        return list(a)[dc.choice([float(x) for x in p], self.rng.unit())]

    def randint(self, low, high):
        n = int(high) - 1
        assert low == 0 and self.buffer is not None
        return nc.dc.reservoir_index(RES_SEED, self.buffer, n)

    # rl_environment.Environment(chance_event_sampler=...)
    def __call__(self, state):
        actions, probs = zip(*state.chance_outcomes())
        return actions[dc.choice([float(x) for x in probs], self.rng.unit())]


def make_run(rl_environment, nfsp, torch, script, spec, trees, out, r):
    game_string, tag, anticipatory, eps, ring_cap, res_cap, episodes, chunks, hidden = spec
    game, tree, by_tensor = trees[game_string]
    P, A = game.num_players(), game.num_distinct_actions()
    I = len(tree["player"])
    script.start_run(SEED + r, P, eps)
    env = rl_environment.Environment(game, chance_event_sampler=script)
    size = env.observation_spec()["info_state"][0]
    agents = [nfsp.NFSP(p, size, A, list(hidden), res_cap, anticipatory, replay_buffer_capacity=ring_cap, epsilon_start=eps,
                        epsilon_end=eps, min_buffer_size_to_learn=HUGE, seed=100 + 10 * r + p) for p in range(P)]
    sl_rows = [[] for _ in range(P)]

    for p, agent in enumerate(agents):
        def hooked(time_step, agent_output, inner=agent.add_transition, p=p):
            script.buffer = p
            inner(time_step, agent_output)
            script.buffer = None
            info = by_tensor[np.asarray(time_step.observations["info_state"][p], np.float32).tobytes()]
            sl_rows[p].append((info, np.asarray(agent_output.probs, dtype=np.float32).copy()))
        agent.add_transition = hooked

    def ring_rows_since(p, before):
        """What the reference's own ring received since entry index `before` (capacity permitting: read at once)."""
        buf = agents[p]._rl_agent._replay_buffer
        if buf is None:
            return []
        rows = []
        for n in range(before, int(buf.entry_index)):
            k = n % ring_cap
            final = bool(buf.experience.is_final_step[k])
            nxt = -1 if final else by_tensor[buf.experience.next_info_state[k].astype(np.float32).tobytes()]
            assert bool(buf.experience.legal_actions_mask[k].any()) != final
            rows.append((by_tensor[buf.experience.info_state[k].astype(np.float32).tobytes()], int(buf.experience.action[k]),
                         np.float32(buf.experience.reward[k]), nxt, int(final)))
        return rows

    with torch.inference_mode():
        q = np.stack([agents[int(tree["player"][i])]._rl_agent._q_network(
            torch.tensor(np.asarray(tree["tensors"][i]).reshape(1, -1), dtype=torch.float32)).squeeze(0).numpy() for i in range(I)]).astype(np.float32)
        avg = []
        for i in range(I):
            mask = np.zeros(A, bool)
            mask[[a for a in tree["legal"][i] if a >= 0]] = True
            logits = agents[int(tree["player"][i])]._avg_network(torch.FloatTensor(tree["tensors"][i]).unsqueeze(0)).squeeze(0)
            logits = torch.where(torch.BoolTensor(mask), logits, torch.full_like(logits, float(torch.finfo(torch.float).min)))
            avg.append(torch.nn.functional.softmax(logits, dim=-1).numpy())
        avg = np.stack(avg).astype(np.float32)

    pre = f"r{r}/"
    out.update({pre + "ring_capacity": ring_cap, pre + "res_capacity": res_cap, pre + "episodes": episodes, pre + "chunks": chunks,
                pre + "seed": SEED + r, pre + "res_seed": RES_SEED, pre + "players": P, pre + "eps": np.full(P, eps, np.float64),
                pre + "anticipatory": np.full(P, anticipatory, np.float64), pre + "q": q, pre + "avg": avg})
    modes_seen = [set() for _ in range(P)]
    wrapped = twice = False
    script.branches = [0, 0]
    for c in range(chunks):
        eps_rows = []
        entry0 = [0 if a._rl_agent._replay_buffer is None else int(a._rl_agent._replay_buffer.entry_index) for a in agents]
        add0 = [0 if a._reservoir_buffer is None else int(a._reservoir_buffer.add_calls) for a in agents]
        for j in range(episodes):
            g = c * episodes + j
            modes = 0
            for p, agent in enumerate(agents):
                best = agent._mode == nfsp.MODE.BEST_RESPONSE
                modes |= int(best) << p
                modes_seen[p].add(best)
            before = [0 if a._rl_agent._replay_buffer is None else int(a._rl_agent._replay_buffer.entry_index) for a in agents]
            for rows in sl_rows:
                rows.clear()
            script.start_episode(g)
            ring = [[] for _ in range(P)]

            def drain():
                for p in range(P):
                    ring[p] += ring_rows_since(p, before[p])
                    buf = agents[p]._rl_agent._replay_buffer
                    before[p] = 0 if buf is None else int(buf.entry_index)

            time_step = env.reset()
            while not time_step.last():
                player_id = time_step.observations["current_player"]
                agent_output = agents[player_id].step(time_step)
                time_step = env.step([agent_output.action])
                drain()                      # a small ring is read before its slots are written again
            for agent in agents:
                agent.step(time_step)
            drain()
            eps_rows.append(dict(modes=modes, draws=script.rng.draws, ring=ring, sl=[list(rows) for rows in sl_rows]))
        chunk = nc.flatten_chunk(eps_rows, P, A)
        k = f"{pre}c{c}/"
        out.update({k + "first": c * episodes, k + "draws": chunk["draws"], k + "modes": chunk["modes"], k + "ring_off": chunk["ring"][0],
                    k + "sl_off": chunk["sl"][0], k + "sl_info": chunk["sl"][1], k + "sl_probs": chunk["sl"][2],
                    k + "dqn_steps": np.array([a._rl_agent._iteration for a in agents], np.int64),
                    k + "nfsp_steps": np.array([a._iteration for a in agents], np.int64)})
        out.update({k + "ring_" + f: chunk["ring"][1 + n] for n, f in enumerate(nc.RING_FIELDS)})
        for p, agent in enumerate(agents):
            buf = agent._rl_agent._replay_buffer
            n = 0 if buf is None else int(len(buf))
            cols, entry = [], 0
            if buf is not None:      # the filled slots, in slot order
                entry = int(buf.entry_index)
                for slot in range(n):
                    final = bool(buf.experience.is_final_step[slot])
                    cols.append((by_tensor[buf.experience.info_state[slot].astype(np.float32).tobytes()], int(buf.experience.action[slot]),
                                 np.float32(buf.experience.reward[slot]),
                                 -1 if final else by_tensor[buf.experience.next_info_state[slot].astype(np.float32).tobytes()], int(final)))
            out[k + f"ring{p}/entry_index"] = entry
            for m, (f, d) in enumerate(zip(nc.RING_FIELDS, nc.RING_DTYPES)):
                out[k + f"ring{p}/{f}"] = np.array([row[m] for row in cols], d)
            res = agent._reservoir_buffer
            n = 0 if res is None else len(res)
            out[k + f"res{p}/add_calls"] = 0 if res is None else int(res.add_calls)
            out[k + f"res{p}/info"] = np.array([by_tensor[res.experience.info_state[s].astype(np.float32).tobytes()] for s in range(n)], np.int32)
            out[k + f"res{p}/probs"] = (np.zeros((0, A), np.float32) if res is None else res.experience.action_probs[:n].astype(np.float32))
            if entry - entry0[p] > 2 * ring_cap:
                wrapped = True
            writes = [dc.reservoir_slot(RES_SEED, p, m, res_cap) for m in range(add0[p], 0 if res is None else int(res.add_calls))]
            writes = [w for w in writes if w >= 0]
            if max([writes.count(w) for w in set(writes)], default=0) >= 2:
                twice = True
    print(f"{game_string} {tag}: modes {[sorted(m) for m in modes_seen]}, explore / greedy decisions {script.branches}, "
          f"a ring wrapped more than once inside a chunk {wrapped}, a reservoir slot written twice inside a chunk {twice}")
    return modes_seen, list(script.branches), wrapped, twice


def main():
    mk.check_choice_rule()
    pyspiel, rl_environment, dqn, nfsp = reference_modules()
    import torch
    torch.set_num_threads(1)
    script = Script()
    proxy = mk.NumpyProxy(script)
    nfsp.np = proxy
    dqn.np = proxy
    out = {"runs": np.array([f"{s[0]}|{s[1]}" for s in RUNS])}
    trees = {}
    for g in sorted({s[0] for s in RUNS}):
        trees[g] = mk.game_tree(pyspiel, g)
        out.update({f"tree/{g}/{k}": v for k, v in trees[g][1].items()})
    for r, spec in enumerate(RUNS):
        modes, branches, wrapped, twice = make_run(rl_environment, nfsp, torch, script, spec, trees, out, r)
        if spec[1] == "mixed":
            assert all(m == {True, False} for m in modes), "both modes must occur for every player"
            assert branches[0] > 0 and branches[1] > 0, "both branches of the epsilon-greedy rule must occur"
            assert wrapped and twice, "a small-capacity run must wrap its ring more than once and overwrite a reservoir slot twice"
        if spec[1] == "roomy":
            assert not wrapped
        if spec[1] == "dqn":
            assert all(m == {True} for m in modes)
        if spec[1] == "average":
            assert all(m == {False} for m in modes) and branches == [0, 0]
    np.savez_compressed(nc.GOLDEN, **out)
    print(nc.GOLDEN, os.path.getsize(nc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
