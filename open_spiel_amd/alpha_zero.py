"""AlphaZero self-play for a batch of environments: the actor half of alpha_zero_torch/alpha_zero.cc (PlayGame) and
python/algorithms/alpha_zero/alpha_zero.py (_play_game) on the device.

Every ply, `mcts.search` searches all environments at once, `osg_selfplay_select` turns the visit counts into policy
targets p[a] = visits[a] ^ (1 / temperature) / sum and chooses the moves (drawn from p for the first temperature_drop
moves of a game, the search's best action afterwards), and `osg_selfplay_commit` plays them, finds the games that ended
and appends their trajectories — (state, policy, value = player 0's outcome) per ply — to a ring of training rows
(`ReplayBuffer`: replay_buffer.py's append / sample).  Rows hold state records; observation tensors and legal masks are
packed for the rows a learner samples.  The learner (model, loss, optimiser) is the user's.

    buffer = ReplayBuffer(ctx, "connect_four", 1 << 20)
    actor = SelfPlay(StateBatch(ctx, "connect_four", 1 << 14), buffer, VPNetEvaluator(model), max_simulations=64,
                     uct_c=1.4, dirichlet_alpha=1.0, dirichlet_epsilon=0.25, seed=1)
    actor.run(1 << 16)
    batch = buffer.sample(1024, seed=step)       # TrainInput(observation, legals_mask, policy, value)
"""
import collections
import ctypes as C
import weakref

import torch

from . import _abi, mcts
from ._abi import OsgError, check, lib
from .engine import StateBatch

TrainInput = collections.namedtuple("TrainInput", "observation legals_mask policy value")
_MASK64 = (1 << 64) - 1


# What separates the root noise's streams from the move draws': both are Rng(seed, index_offset + env, ply) of osg_common.h,
# which has no domain of its own per use, so the noise takes its seed from another one.
NOISE_SALT = 0x6E6F6973655F7A31


def noise_seed(seed):
    """The seed of SelfPlay(seed=seed)'s root noise: never the move draws' stream for the same (environment, ply)."""
    return (int(seed) ^ NOISE_SALT) & _MASK64


class ReplayBuffer:
    """The newest `capacity` training rows on the device, sampled uniformly (replay_buffer.py; the C++
    SerializableCircularBuffer).  A row: state record, policy [A] f32, value f32 (player 0's outcome of its game),
    root_value f32, player i8, action i32."""

    def __init__(self, ctx, game_string, capacity):
        self.ctx = ctx
        self.game_string = game_string
        h = C.c_void_p()
        check(lib().osg_replay_create(ctx._h, game_string.encode(), int(capacity), C.byref(h)))
        self._h = h
        self.capacity = int(capacity)
        self.states = StateBatch.borrowed(ctx, game_string, lib().osg_replay_states(h), self)
        self.num_distinct_actions = self.states.num_distinct_actions
        self._users = weakref.WeakSet()   # the SelfPlay objects that hold the raw handle

    def close(self):
        """Free the ring now.  Refused while a SelfPlay that appends to it is open: close that first."""
        if self._h:
            if any(sp._h for sp in self._users):
                raise OsgError("ReplayBuffer.close: a SelfPlay still appends to this buffer; close it first")
            self.states.close()
            lib().osg_replay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sizes(self):
        size, seen, cap = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().osg_replay_sizes(self._h, C.byref(size), C.byref(seen), C.byref(cap)))
        return size.value, seen.value

    def __len__(self):
        return self._sizes()[0]

    @property
    def total_seen(self):
        return self._sizes()[1]

    def sample_rows(self, m, seed, index_offset=0):
        """index[j] = Rng(seed, index_offset + j, 0).below(len(self)); (index [m] i64, states: StateBatch of m states,
        policy [m, A] f32, value [m] f32)."""
        m = int(m)
        if m < 1:
            raise OsgError("ReplayBuffer.sample: m must be >= 1")
        if not self._h:
            raise OsgError("ReplayBuffer.sample: the buffer is closed")
        dev = self.ctx.device   # (an empty buffer is refused by the call below, which reads the size once)
        states = StateBatch(self.ctx, self.game_string, m)
        policy = torch.empty((m, self.num_distinct_actions), dtype=torch.float32, device=dev)
        value = torch.empty(m, dtype=torch.float32, device=dev)
        index = torch.empty(m, dtype=torch.int64, device=dev)
        check(lib().osg_replay_sample(self._h, int(seed) & _MASK64, int(index_offset), m, states._h, policy.data_ptr(),
                                      value.data_ptr(), index.data_ptr()))
        return index, states, policy, value

    def sample(self, m, seed, index_offset=0):
        """m rows drawn uniformly with replacement as a TrainInput on the device: observation [m, obs] f32 (the current
        player's, as state.observation_tensor() in both references), legals_mask [m, A] bool, policy [m, A] f32,
        value [m] f32."""
        _, states, policy, value = self.sample_rows(m, seed, index_offset)
        return TrainInput(states.observation_tensor(-1), states.legal_actions_bool(), policy, value)

    def rows(self, index):
        """The stored rows `index` names (slots in [0, capacity)): dict(states: StateBatch, policy, value, root_value,
        player, action)."""
        dev = self.ctx.device
        idx = torch.as_tensor(index, dtype=torch.int64, device=dev).contiguous()
        m = idx.numel()
        out = {
            "policy": torch.empty((m, self.num_distinct_actions), dtype=torch.float32, device=dev),
            "value": torch.empty(m, dtype=torch.float32, device=dev),
            "root_value": torch.empty(m, dtype=torch.float32, device=dev),
            "player": torch.empty(m, dtype=torch.int8, device=dev),
            "action": torch.empty(m, dtype=torch.int32, device=dev),
        }
        check(lib().osg_replay_rows(self._h, idx.data_ptr(), m, *[out[k].data_ptr() for k in
                                                                  ("policy", "value", "root_value", "player", "action")]))
        out["states"] = self.states.gather(idx)
        return out


class SelfPlay:
    """PlayGame (alpha_zero.cc:109-167) in every environment of `envs` at once, games restarting as they end.

    evaluator, max_simulations, uct_c, puct, solve, dirichlet_alpha, dirichlet_epsilon: the search's (mcts.search);
    temperature, temperature_drop, cutoff_value: PlayGame's (cutoff_value None = never).  Streams: environment i draws
    the move of its k-th ply since construction on Rng(seed, index_offset + i, k); the search of step s runs with seed
    search_seed(s) and draws its root noise on Rng(noise_seed(seed), index_offset + i, s) — a salted seed, so that the
    noise of a root and the draw of its move, which share stream and sub-stream numbers, never share a stream."""

    def __init__(self, envs, buffer, evaluator, max_simulations, uct_c, temperature=1.0, temperature_drop=10,
                 cutoff_value=None, dirichlet_alpha=0.0, dirichlet_epsilon=0.0, puct=True, solve=False, seed=0,
                 index_offset=0, n_rollouts=1):
        if int(max_simulations) < 2:
            raise OsgError("SelfPlay: max_simulations must be >= 2 (one simulation never expands the root)")
        self.envs, self.buffer, self.evaluator = envs, buffer, evaluator
        self.ctx = envs.ctx
        self.max_simulations, self.uct_c, self.puct, self.solve = int(max_simulations), float(uct_c), bool(puct), bool(solve)
        self.dirichlet_alpha, self.dirichlet_epsilon = float(dirichlet_alpha), float(dirichlet_epsilon)
        self.n_rollouts = int(n_rollouts)
        self.seed, self.index_offset = int(seed) & _MASK64, int(index_offset)
        if cutoff_value is None:
            cutoff_value = envs.desc.max_utility + 1.0
        cfg = _abi.SelfPlayCfg(float(temperature), float(cutoff_value), int(temperature_drop), 0, self.seed, self.index_offset)
        self._h = None
        if not buffer._h:
            raise OsgError("SelfPlay: the replay buffer is closed")
        h = C.c_void_p()
        check(lib().osg_selfplay_create(envs._h, buffer._h, C.byref(cfg), C.byref(h)))
        self._h = h
        buffer._users.add(self)
        self.steps = 0   # plies played by every environment = the next step's index

    def close(self):
        if self._h:
            lib().osg_selfplay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_seed(self, step):
        """The seed of step `step`'s search: one splitmix increment per step away from `seed`."""
        return (self.seed + 0x9E3779B97F4A7C15 * (int(step) + 1)) & _MASK64

    def select(self, child_visits, best_action, root_value):
        """osg_selfplay_select on a search's results: (policy [n, A] f32, action [n] i32); the ply is staged."""
        n, A, dev = self.envs.n, self.envs.num_distinct_actions, self.ctx.device
        visits = torch.as_tensor(child_visits, dtype=torch.int32, device=dev).contiguous()
        best = torch.as_tensor(best_action, dtype=torch.int32, device=dev).contiguous()
        rootv = torch.as_tensor(root_value, dtype=torch.float64, device=dev).contiguous()
        if visits.shape != (n, A) or best.numel() != n or rootv.numel() != n:
            raise OsgError("SelfPlay.select: child_visits [n, A], best_action [n], root_value [n]")
        policy = torch.empty((n, A), dtype=torch.float32, device=dev)
        action = torch.empty(n, dtype=torch.int32, device=dev)
        check(lib().osg_selfplay_select(self._h, visits.data_ptr(), best.data_ptr(), rootv.data_ptr(), policy.data_ptr(),
                                        action.data_ptr()))
        return policy, action

    def commit(self, want_counts=False):
        """osg_selfplay_commit: (finished [n] bool, returns [n] f64: player 0's return where a game ended)
        (+ (games, rows) of this call with want_counts, which waits for the device)."""
        n, dev = self.envs.n, self.ctx.device
        finished = torch.empty(n, dtype=torch.uint8, device=dev)
        returns = torch.empty(n, dtype=torch.float64, device=dev)
        counts = (C.c_int64 * 2)() if want_counts else None
        check(lib().osg_selfplay_commit(self._h, finished.data_ptr(), returns.data_ptr(), counts))
        if want_counts:
            return finished.bool(), returns, (counts[0], counts[1])
        return finished.bool(), returns

    def staged(self, t):
        """Ply t of the running trajectories: dict(states, policy, action, root_value, player, length, ply_counter)."""
        n, A, dev = self.envs.n, self.envs.num_distinct_actions, self.ctx.device
        out = {
            "policy": torch.empty((n, A), dtype=torch.float32, device=dev),
            "action": torch.empty(n, dtype=torch.int32, device=dev),
            "root_value": torch.empty(n, dtype=torch.float32, device=dev),
            "player": torch.empty(n, dtype=torch.int8, device=dev),
            "length": torch.empty(n, dtype=torch.int32, device=dev),
            "ply_counter": torch.empty(n, dtype=torch.int64, device=dev),
        }
        states = StateBatch(self.ctx, self.envs.game_string, n)
        check(lib().osg_selfplay_staged(self._h, int(t), states._h, *[out[k].data_ptr() for k in
                                                                      ("policy", "action", "root_value", "player", "length",
                                                                       "ply_counter")]))
        out["states"] = states
        return out

    def search(self, step):
        """The search of step `step` over the environments as they stand (mcts.search's dictionary with root_value)."""
        noisy = self.dirichlet_alpha > 0
        return mcts.search(self.envs, self.evaluator, max_simulations=self.max_simulations, uct_c=self.uct_c,
                           n_rollouts=self.n_rollouts, solve=self.solve, seed=self.search_seed(step),
                           index_offset=self.index_offset, puct=self.puct, dirichlet_alpha=self.dirichlet_alpha,
                           dirichlet_epsilon=self.dirichlet_epsilon, noise_seed=noise_seed(self.seed) if noisy else None, noise_sub=step,
                           want_root_value=True)

    def step(self):
        """One ply in every environment: search, select, commit.  Device tensors: action [n] i32, policy [n, A] f32,
        root_value [n] f64, finished [n] bool, returns [n] f64 (player 0's return of the games that ended)."""
        res = self.search(self.steps)
        policy, action = self.select(res["child_visits"], res["best_action"], res["root_value"])
        finished, returns = self.commit()
        self.steps += 1
        return {"action": action, "policy": policy, "root_value": res["root_value"], "finished": finished,
                "returns": returns}

    def run(self, min_new_rows):
        """step() until the buffer has seen min_new_rows more rows; returns the number of steps taken."""
        target = self.buffer.total_seen + int(min_new_rows)
        taken = 0
        while self.buffer.total_seen < target:
            self.step()
            taken += 1
        return taken
