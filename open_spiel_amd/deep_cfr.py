"""Deep CFR (open_spiel/python/pytorch/deep_cfr.py; Brown et al., https://arxiv.org/abs/1811.00164) with the traversals,
the sampled advantages and the reservoir buffers on the device.

The networks do not change while one player's traversals of one iteration run, so one forward pass over all infostate
tensors — an [I, A] table of advantage-network outputs — stands for every per-node forward pass of the reference, and one
TabularSolver.deep_cfr_traverse call does all num_traversals traversals and all reservoir appends of that step.  The
networks, their losses and Adam are torch's; a buffer row is (infostate index, iteration, values) and the tensor the
reference stores with each row is looked up in TabularSolver.infostate_tensors() when a batch is formed.

What is pinned against the reference (tests/golden/make_deep_cfr_vectors.py) is the device's part: given the networks'
outputs, the rows, their order and the buffers' contents are the reference's, bit for bit, for the device's random
streams.  One deliberate difference: with batch_size=None the reference trains on its whole np.empty array,
uninitialised rows included, until the buffer is full; here only the filled rows are used."""
import collections
import ctypes as C

import numpy as np
import torch
from torch import nn

from ._abi import OsgError, check, describe, lib
from .engine import TabularSolver

RESERVOIR_SALT = 0x7265736572766F69   # the buffers' streams are keyed apart from the trajectories'
SAMPLE_SALT = 0x73616D706C655F6B


class ReservoirBuffer:
    """ReservoirBuffer (deep_cfr.py:121-213) on the device: `capacity` rows of (infostate index int32, iteration int32,
    values float32 [num_actions]).  The row with add index n goes to slot n while n < capacity, else to
    mulhi64(Rng(seed, n, stream).next(), n + 1) if that is below capacity, else nowhere."""

    def __init__(self, ctx, num_actions, capacity, seed=0, stream=0):
        self.ctx, self.num_actions, self.capacity = ctx, int(num_actions), int(capacity)
        self.seed, self.stream = int(seed) & (2 ** 64 - 1), int(stream)
        h = C.c_void_p()
        check(lib().osg_reservoir_create(ctx._h, self.num_actions, self.capacity, self.seed, self.stream, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                lib().osg_reservoir_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _sizes(self):
        size, calls, cap = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().osg_reservoir_sizes(self._h, C.byref(size), C.byref(calls), C.byref(cap)))
        return size.value, calls.value

    def __len__(self):
        return self._sizes()[0]

    @property
    def add_calls(self):
        return self._sizes()[1]

    def clear(self):
        check(lib().osg_reservoir_clear(self._h))

    def _tensor(self, t, dtype, shape, what):
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
                or t.device != self.ctx.device):
            raise OsgError(f"ReservoirBuffer.{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on {self.ctx.device}")
        return t.data_ptr()

    def append(self, info, iteration, values):
        """len(info) sequential appends in row order: info [m] int32, values [m, num_actions] float32 (device)."""
        m = int(info.shape[0])
        check(lib().osg_reservoir_append(self._h, m, self._tensor(info, torch.int32, (m,), "append"), int(iteration),
                                         self._tensor(values, torch.float32, (m, self.num_actions), "append")))

    def sample_slots(self, num_samples, seed, stream=0):
        """num_samples distinct filled slots [int64, device]: the smallest keys Rng(seed, slot, stream).next()."""
        if num_samples > len(self):
            raise ValueError(f"{num_samples} elements could not be sampled from size {len(self)}")
        slots = torch.empty(int(num_samples), dtype=torch.int64, device=self.ctx.device)
        check(lib().osg_reservoir_sample(self._h, int(seed) & (2 ** 64 - 1), int(stream), int(num_samples), slots.data_ptr()))
        return slots

    def rows(self, slots):
        """(infostate index int32 [m], iteration int32 [m], values float32 [m, num_actions]) of the given slots."""
        m = int(slots.shape[0])
        dev = self.ctx.device
        info = torch.empty(m, dtype=torch.int32, device=dev)
        iteration = torch.empty(m, dtype=torch.int32, device=dev)
        values = torch.empty((m, self.num_actions), dtype=torch.float32, device=dev)
        check(lib().osg_reservoir_rows(self._h, self._tensor(slots, torch.int64, (m,), "rows"), m, info.data_ptr(),
                                       iteration.data_ptr(), values.data_ptr()))
        return info, iteration, values

    def sample(self, num_samples, seed, stream=0):
        return self.rows(self.sample_slots(num_samples, seed, stream))

    def filled(self):
        """Every filled row in slot order."""
        return self.rows(torch.arange(len(self), dtype=torch.int64, device=self.ctx.device))


class MLP(nn.Module):
    """Linear + ReLU per hidden size, then LayerNorm and a Linear layer (and an optional final activation)."""

    def __init__(self, input_size, hidden_sizes, output_size, final_activation=None, seed=42):
        super().__init__()
        torch.manual_seed(seed)
        layers, width = [], input_size
        for size in hidden_sizes:
            layers.append(nn.Sequential(nn.Linear(width, size), nn.ReLU()))
            width = size
        layers += [nn.LayerNorm(width), nn.Linear(width, output_size)]
        if final_activation is not None:
            layers.append(final_activation)
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)

    @torch.no_grad()
    def reset(self):
        for m in self.modules():
            if callable(getattr(m, "reset_parameters", None)):
                m.reset_parameters()


class DeepCFRSolver:
    """DeepCFRSolver of the reference (its keyword names and defaults) over a game string; `tabular` may hand in an
    existing TabularSolver of the game (any kind: its tables are not touched).

    Per (iteration, player) step: one forward pass of every player's advantage network over its infostates gives the
    [I, A] table, one deep_cfr_traverse call with first_trajectory = ((iteration - 1) * P + player) * num_traversals
    does the traversals and the appends, then the player's advantage network trains from the buffer's rows; nothing
    crosses to the host but the row counts.  With batch_size_* = None the filled rows are the batch (the reference
    takes its whole array, uninitialised rows included)."""

    def __init__(self, ctx, game, policy_network_layers=(256, 256), advantage_network_layers=(128, 128), num_iterations=100,
                 num_traversals=20, learning_rate=1e-4, batch_size_advantage=None, batch_size_strategy=None,
                 memory_capacity=int(1e6), policy_network_train_steps=1, advantage_network_train_steps=1,
                 reinitialize_advantage_networks=True, device=None, seed=42, print_nash_convs=False, tabular=None):
        self.ctx, self.game_string = ctx, game
        if device is not None and torch.device(device) != ctx.device:
            raise OsgError(f"DeepCFRSolver: the networks live on the context's device {ctx.device}")
        desc = describe(game)
        self.tabular = tabular if tabular is not None else TabularSolver(ctx, game)
        self._num_players, self._num_actions = desc.num_players, self.tabular.amax
        if desc.num_distinct_actions != self._num_actions:
            raise OsgError("DeepCFRSolver: the table's width is not the game's number of distinct actions")
        self._embedding_size = desc.info_size
        self._batch_size_advantage, self._batch_size_strategy = batch_size_advantage, batch_size_strategy
        self._policy_network_train_steps, self._advantage_network_train_steps = policy_network_train_steps, advantage_network_train_steps
        self._num_iterations, self._num_traversals = num_iterations, num_traversals
        self._memory_capacity = int(memory_capacity)
        self._reinitialize_advantage_networks = reinitialize_advantage_networks
        self._learning_rate, self._print_nash_convs = learning_rate, print_nash_convs
        self._iteration, self._seed, self._samples_drawn = 1, int(seed), 0
        self.step_callback = None      # called as step_callback(iteration, player, advantage table) before a step's traversals

        self._tensors = self.tabular.infostate_tensors()
        tab = self.tabular.tables()
        dev = ctx.device
        self._legal = torch.from_numpy(tab["legal"].astype(np.int64)).to(dev)
        players = np.asarray(self.tabular.infostate_players()).astype(np.int64)
        self._rows_of = [torch.from_numpy(np.nonzero(players == p)[0]).to(dev) for p in range(self._num_players)]

        res_seed = (self._seed ^ RESERVOIR_SALT) & (2 ** 64 - 1)
        self._advantage_memories = [ReservoirBuffer(ctx, self._num_actions, self._memory_capacity, res_seed, p)
                                    for p in range(self._num_players)]
        self._strategy_memories = ReservoirBuffer(ctx, self._num_actions, self._memory_capacity, res_seed, self._num_players)
        self._advantage_networks = [MLP(self._embedding_size, list(advantage_network_layers), self._num_actions, None, seed + p).to(dev)
                                    for p in range(self._num_players)]
        self._policy_network = MLP(self._embedding_size, list(policy_network_layers), self._num_actions, nn.Softmax(-1), seed).to(dev)
        self._loss_policy = nn.MSELoss()
        self._loss_advantages = nn.MSELoss(reduction="mean")
        self._optimizer_policy = None
        self._optimizer_advantages = [None] * self._num_players
        self._reinitialize_policy_network()
        for p in range(self._num_players):
            self._reinitialize_advantage_network(p)

    @property
    def advantage_buffers(self):
        return self._advantage_memories

    @property
    def strategy_buffer(self):
        return self._strategy_memories

    @property
    def iteration(self):
        return self._iteration

    def _reinitialize_advantage_network(self, player):
        self._advantage_networks[player].reset()
        self._optimizer_advantages[player] = torch.optim.Adam(self._advantage_networks[player].parameters(), lr=self._learning_rate)

    def _reinitialize_policy_network(self):
        self._policy_network.reset()
        self._optimizer_policy = torch.optim.Adam(self._policy_network.parameters(), lr=self._learning_rate)

    @torch.inference_mode()
    def advantage_table(self):
        """[I, A] float32: row i is the advantage network of infostate i's player on its tensor."""
        table = torch.empty((self.tabular.num_infostates, self._num_actions), dtype=torch.float32, device=self.ctx.device)
        for p, rows in enumerate(self._rows_of):
            if len(rows):
                table[rows] = self._advantage_networks[p](self._tensors[rows])
        return table

    def traverse(self, player):
        """The step's num_traversals traversals for `player`; returns (advantage rows, strategy rows) appended."""
        table = self.advantage_table()
        if self.step_callback is not None:
            self.step_callback(self._iteration, player, table)
        first = ((self._iteration - 1) * self._num_players + player) * self._num_traversals
        return self.tabular.deep_cfr_traverse(table, player, self._iteration, self._seed, self._num_traversals, first,
                                              self._advantage_memories[player], self._strategy_memories)

    def solve(self):
        """Returns (policy network, advantage losses per player and iteration, policy loss), as the reference does."""
        advantage_losses = collections.defaultdict(list)
        for _ in range(self._num_iterations):
            if self._print_nash_convs:
                policy_loss = self._learn_strategy_network()
                print(f"NashConv @ {self._iteration} = {self.nash_conv()} | Policy loss = {policy_loss}")
                self._reinitialize_policy_network()
            for p in range(self._num_players):
                self.traverse(p)
                if self._reinitialize_advantage_networks:
                    self._reinitialize_advantage_network(p)
                advantage_losses[p].append(self._learn_advantage_network(p))
            self._iteration += 1
        policy_loss = self._learn_strategy_network()
        return self._policy_network, advantage_losses, policy_loss

    def _batch(self, memory, batch_size):
        if batch_size:
            if batch_size > len(memory):
                return None
            self._samples_drawn += 1
            return memory.sample(batch_size, self._seed ^ SAMPLE_SALT, self._samples_drawn)
        return memory.filled() if len(memory) else None

    def _train(self, network, optimizer, loss_fn, memory, batch_size, steps):
        loss = None
        for _ in range(steps):
            batch = self._batch(memory, batch_size)
            if batch is None:
                return None
            info, iteration, target = batch
            optimizer.zero_grad()
            weight = iteration.to(torch.float32).sqrt().unsqueeze(1)          # sqrt(iteration)-weighted MSE
            outputs = network(self._tensors[info.long()])
            loss = loss_fn(weight * outputs, weight * target)
            loss.backward()
            optimizer.step()
        return None if loss is None else loss.detach().item()

    def _learn_advantage_network(self, player):
        return self._train(self._advantage_networks[player], self._optimizer_advantages[player], self._loss_advantages,
                           self._advantage_memories[player], self._batch_size_advantage, self._advantage_network_train_steps)

    def _learn_strategy_network(self):
        return self._train(self._policy_network, self._optimizer_policy, self._loss_policy, self._strategy_memories,
                           self._batch_size_strategy, self._policy_network_train_steps)

    @torch.inference_mode()
    def policy_table(self):
        """[I, Amax] float64 (NumPy), column k the k-th legal action of the infostate — the layout of
        TabularSolver.evaluate_policy(which="table").  The policy network's softmax runs over all action ids; a row
        here is its restriction to the legal ids, renormalised (the reference hands the unnormalised restriction on)."""
        probs = self._policy_network(self._tensors).to(torch.float64)
        legal = self._legal >= 0
        table = torch.where(legal, probs.gather(1, self._legal.clamp(min=0)), torch.zeros((), dtype=torch.float64, device=probs.device))
        total = table.sum(1, keepdim=True)
        uniform = legal.to(torch.float64) / legal.sum(1, keepdim=True).clamp(min=1)
        table = torch.where(total > 0, table / total.clamp(min=torch.finfo(torch.float64).tiny), uniform)
        return table.cpu().numpy()

    def evaluate(self):
        return self.tabular.evaluate_policy(which="table", table=self.policy_table())

    def nash_conv(self):
        return self.evaluate()["nash_conv"]


__all__ = ["DeepCFRSolver", "ReservoirBuffer", "MLP"]
