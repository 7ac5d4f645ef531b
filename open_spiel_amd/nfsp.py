"""Neural Fictitious Self-Play (open_spiel/python/pytorch/nfsp.py with dqn.py inside it; Heinrich & Silver,
https://arxiv.org/abs/1603.01121) with the self-play on the device: the episodes, the epsilon-greedy and average-policy
action choices, the DQN transitions, the supervised rows, the replay ring and the reservoirs.

The networks do not change between two learning steps, so one forward pass over all infostate tensors — an [I, A] table
of Q values and an [I, A] table of average-policy probabilities — stands for every per-decision forward pass of the
reference, and one TabularSolver.nfsp_collect call plays a whole chunk of episodes and appends every row of it.  The
networks, their losses and optimisers are torch's; a buffer row names its infostates by index and the tensors the
reference stores with each row are gathered from TabularSolver.infostate_tensors() when a batch is formed (for the next
state of a final transition: zeros and an all-false mask, which is what reaches the reference's loss).

What is pinned against the reference (tests/golden/make_nfsp_vectors.py) is the device's part: given the two tables,
every row, its position, every draw and every buffer slot are the reference's, bit for bit, for the device's random
streams.  Deliberate differences: the networks and epsilon are frozen within a chunk of `episodes_per_step` episodes
(the reference moves them every `learn_every` steps of an agent, in the middle of an episode); the updates a chunk
owes are made after it.  With anticipatory_param=1 this is DQN self-play."""
import ctypes as C
import math

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

from ._abi import OsgError, check, describe, lib
from .deep_cfr import RESERVOIR_SALT, SAMPLE_SALT, ReservoirBuffer
from .engine import TabularSolver

ILLEGAL_ACTION_LOGITS_PENALTY = torch.finfo(torch.float).min
DQN_SEED = 42   # NFSP.__init__ does not hand its seed on: the Q networks are built with DQN's default


class TransitionRing:
    """dqn.ReplayBuffer on the device: `capacity` rows of (infostate index int32, action int32, reward float32, next
    infostate index int32 — -1 at the end of an episode —, final uint8).  The row with entry index n goes to slot
    n % capacity."""

    def __init__(self, ctx, capacity):
        self.ctx, self.capacity = ctx, int(capacity)
        h = C.c_void_p()
        check(lib().osg_transition_ring_create(ctx._h, self.capacity, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                lib().osg_transition_ring_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _sizes(self):
        size, entry, cap = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().osg_transition_ring_sizes(self._h, C.byref(size), C.byref(entry), C.byref(cap)))
        return size.value, entry.value

    def __len__(self):
        return self._sizes()[0]

    @property
    def entry_index(self):
        return self._sizes()[1]

    def clear(self):
        check(lib().osg_transition_ring_clear(self._h))

    def _tensor(self, t, dtype, m, what):
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (m,) or not t.is_contiguous()
                or t.device != self.ctx.device):
            raise OsgError(f"TransitionRing.{what}: expected a contiguous {dtype} tensor of shape ({m},) on {self.ctx.device}")
        return t.data_ptr()

    def append(self, info, action, reward, next_info, final):
        """len(info) sequential appends in row order (device tensors [m]: int32, int32, float32, int32, uint8)."""
        m = int(info.shape[0])
        check(lib().osg_transition_ring_append(self._h, m, self._tensor(info, torch.int32, m, "append"),
                                               self._tensor(action, torch.int32, m, "append"), self._tensor(reward, torch.float32, m, "append"),
                                               self._tensor(next_info, torch.int32, m, "append"), self._tensor(final, torch.uint8, m, "append")))

    def sample_slots(self, num_samples, seed, stream=0):
        """num_samples distinct filled slots [int64, device]: the smallest keys Rng(seed, slot, stream).next()."""
        if num_samples > len(self):
            raise ValueError(f"{num_samples} elements could not be sampled from size {len(self)}")
        slots = torch.empty(int(num_samples), dtype=torch.int64, device=self.ctx.device)
        check(lib().osg_transition_ring_sample(self._h, int(seed) & (2 ** 64 - 1), int(stream), int(num_samples), slots.data_ptr()))
        return slots

    def rows(self, slots):
        """(info int32, action int32, reward float32, next_info int32, final uint8), each [m], of the given slots."""
        m = int(slots.shape[0])
        dev = self.ctx.device
        out = [torch.empty(m, dtype=d, device=dev) for d in (torch.int32, torch.int32, torch.float32, torch.int32, torch.uint8)]
        check(lib().osg_transition_ring_rows(self._h, self._tensor(slots, torch.int64, m, "rows"), m, *[t.data_ptr() for t in out]))
        return tuple(out)

    def sample(self, num_samples, seed, stream=0):
        return self.rows(self.sample_slots(num_samples, seed, stream))

    def filled(self):
        """Every filled row in slot order."""
        return self.rows(torch.arange(len(self), dtype=torch.int64, device=self.ctx.device))


class MLP(nn.Module):
    """dqn.MLP: Linear + ReLU per hidden size, then a Linear layer; torch.manual_seed(seed) before the layers are made."""

    def __init__(self, input_size, hidden_sizes, output_size, seed=42):
        super().__init__()
        torch.manual_seed(seed)
        layers, width = [], input_size
        for size in hidden_sizes:
            layers.append(nn.Sequential(nn.Linear(width, size), nn.ReLU()))
            width = size
        layers.append(nn.Linear(width, output_size))
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


def exponential_schedule(start_e, end_e, duration):
    return lambda t: end_e + (start_e - end_e) * math.exp(-1.0 * min(t, duration) / duration)


def linear_schedule(start_e, end_e, duration):
    slope = (end_e - start_e) / duration
    return lambda t: max(slope * t + start_e, end_e)


def _optimizer(name, params, lr, allowed):
    makers = {"adam": torch.optim.Adam, "rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}
    if name not in allowed:
        raise ValueError("Not implemented, choose from " + ", ".join(repr(a) for a in allowed) + ".")
    return makers[name](params, lr=lr)


class NFSPSolver:
    """The P NFSP agents of the reference's self-play loop (examples/kuhn_nfsp.py) over a game string, with the reference's
    keyword names and defaults — NFSP's own and the DQN ones it forwards — and `episodes_per_step`, the episodes one
    step() plays between two rounds of learning.  `tabular` may hand in an existing TabularSolver of the game (any
    kind: its tables are not touched).

    step(): one forward pass of every player's Q network and average-policy network over its infostates gives the two
    [I, A] tables; epsilon is the schedule at each player's DQN step counter; one nfsp_collect call plays the episodes
    and appends the rows; then, per player, the updates the reference would have made in those steps are made:
    floor(after / learn_every) - floor(before / learn_every) updates of the average network on the NFSP agent's counter
    (while its reservoir holds rows; each also updates the Q network if it falls in an AVERAGE_POLICY episode, as the
    reference's does), as many of the Q network on the DQN agent's counter, and a soft target update per multiple of
    update_target_network_every on that counter.  As in the reference, seed reaches the average networks only (seed + 1)
    and gradient_clipping the average network's update only: NFSP does not hand either on to its DQN agent.

    Not served: board games and simultaneous-move games, checkpoint files, user-supplied buffer classes."""

    def __init__(self, ctx, game, hidden_layers_sizes, reservoir_buffer_capacity, anticipatory_param, batch_size=128,
                 rl_learning_rate=0.01, sl_learning_rate=0.01, min_buffer_size_to_learn=1000, learn_every=64, optimizer_str="sgd",
                 gradient_clipping=None, seed=42, replay_buffer_capacity=10000, update_target_network_every=1000,
                 weight_update_coeff=0.995, discount_factor=1.0, epsilon_start=1.0, epsilon_end=0.1, epsilon_decay_duration=int(1e6),
                 epsilon_decay_schedule_str="exp", loss_str="mse", huber_loss_parameter=1.0, episodes_per_step=1024, device=None,
                 tabular=None):
        self.ctx, self.game_string = ctx, game
        if device is not None and torch.device(device) != ctx.device:
            raise OsgError(f"NFSPSolver: the networks live on the context's device {ctx.device}")
        desc = describe(game)
        self.tabular = tabular if tabular is not None else TabularSolver(ctx, game)
        P, A = desc.num_players, self.tabular.amax
        if desc.num_distinct_actions != A:
            raise OsgError("NFSPSolver: the table's width is not the game's number of distinct actions")
        if isinstance(hidden_layers_sizes, int):
            hidden_layers_sizes = [hidden_layers_sizes]
        assert 0 <= discount_factor <= 1 and 0 <= weight_update_coeff < 1
        assert epsilon_start > 0 and epsilon_end >= 0 and epsilon_start >= epsilon_end
        self._num_players, self._num_actions = P, A
        self._batch_size, self._learn_every = int(batch_size), int(learn_every)
        self._min_buffer_size_to_learn = int(min_buffer_size_to_learn)
        self._anticipatory_param = float(anticipatory_param)
        self._update_target_network_every, self._tau = int(update_target_network_every), float(weight_update_coeff)
        self._discount_factor = float(discount_factor)
        self._gradient_norm_clipping = gradient_clipping
        self._episodes_per_step, self._seed = int(episodes_per_step), int(seed)
        if loss_str == "mse":
            self._rl_loss = F.mse_loss
        elif loss_str == "huber":
            self._rl_loss = lambda x, y: F.smooth_l1_loss(x, y, beta=huber_loss_parameter)
        else:
            raise ValueError("Not implemented, choose from 'mse', 'huber'.")
        if epsilon_decay_schedule_str == "exp":
            self.epsilon_schedule = exponential_schedule(epsilon_start, epsilon_end, epsilon_decay_duration)
        elif epsilon_decay_schedule_str == "linear":
            self.epsilon_schedule = linear_schedule(epsilon_start, epsilon_end, epsilon_decay_duration)
        else:
            raise ValueError("Not implemented, choose from 'linear', 'exp'.")

        dev = ctx.device
        self._tensors = self.tabular.infostate_tensors()
        legal = torch.from_numpy(self.tabular.tables()["legal"].astype(np.int64)).to(dev)        # [I, Amax] ids, -1 padded
        self._legal = legal
        self._legal_mask = (F.one_hot(legal.clamp(min=0), A) * (legal >= 0).unsqueeze(-1)).sum(1) > 0      # [I, A] by action id
        players = np.asarray(self.tabular.infostate_players()).astype(np.int64)
        self._rows_of = [torch.from_numpy(np.nonzero(players == p)[0]).to(dev) for p in range(P)]

        size = desc.info_size
        hidden = list(hidden_layers_sizes)
        self._q_networks = [MLP(size, hidden, A, DQN_SEED).to(dev) for _ in range(P)]
        self._target_q_networks = [MLP(size, hidden, A, DQN_SEED).to(dev) for _ in range(P)]
        for target, net in zip(self._target_q_networks, self._q_networks):
            target.load_state_dict(net.state_dict())
        self._avg_networks = [MLP(size, hidden, A, self._seed + 1).to(dev) for _ in range(P)]
        self._rl_optimizers = [_optimizer(optimizer_str, n.parameters(), rl_learning_rate, ("adam", "rmsprop", "sgd")) for n in self._q_networks]
        self._sl_optimizers = [_optimizer(optimizer_str, n.parameters(), sl_learning_rate, ("adam", "sgd")) for n in self._avg_networks]

        res_seed = (self._seed ^ RESERVOIR_SALT) & (2 ** 64 - 1)
        self._replay_buffers = [TransitionRing(ctx, replay_buffer_capacity) for _ in range(P)]
        self._reservoir_buffers = [ReservoirBuffer(ctx, A, reservoir_buffer_capacity, res_seed, p) for p in range(P)]
        self._episodes = 0
        self._samples_drawn = 0
        self.dqn_steps = [0] * P          # DQN._iteration of every player
        self.nfsp_steps = [0] * P         # NFSP._iteration
        self.updates = [[0, 0, 0] for _ in range(P)]   # Q-network updates, average-network updates, target copies made
        self.last_rl_loss = [None] * P
        self.last_sl_loss = [None] * P
        self.last_totals = None

    @property
    def replay_buffers(self):
        return self._replay_buffers

    @property
    def reservoir_buffers(self):
        return self._reservoir_buffers

    @property
    def episodes(self):
        return self._episodes

    @property
    def loss(self):
        return list(zip(self.last_sl_loss, self.last_rl_loss))

    # ---- the tables ---------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def tables(self):
        """(q [I, A] float32, avg [I, A] float32): row i from the networks of infostate i's player; avg is the softmax
        over the legal logits (_act), exactly zero at illegal ids."""
        I, A = self._tensors.shape[0], self._num_actions
        q = torch.empty((I, A), dtype=torch.float32, device=self.ctx.device)
        logits = torch.empty_like(q)
        for p, rows in enumerate(self._rows_of):
            if len(rows):
                q[rows] = self._q_networks[p](self._tensors[rows])
                logits[rows] = self._avg_networks[p](self._tensors[rows])
        logits = torch.where(self._legal_mask, logits, torch.full_like(logits, ILLEGAL_ACTION_LOGITS_PENALTY))
        return q, F.softmax(logits, dim=-1).contiguous()

    def epsilons(self):
        return [self.epsilon_schedule(t) for t in self.dqn_steps]

    # ---- one chunk ----------------------------------------------------------------------------------------------------------
    def step(self):
        """Plays episodes_per_step episodes, then learns; returns the call's totals [P, 4] (transitions, supervised
        rows, DQN-agent steps, NFSP-agent steps per player)."""
        q, avg = self.tables()
        E, L = self._episodes_per_step, self._learn_every
        totals = self.tabular.nfsp_collect(q, avg, self.epsilons(), self._anticipatory_param, self._seed, E, self._episodes,
                                           self._replay_buffers, self._reservoir_buffers)
        self._episodes += E
        self.last_totals = totals
        staged = self.tabular.nfsp_staged()
        for p in range(self._num_players):
            before_n, before_d = self.nfsp_steps[p], self.dqn_steps[p]
            after_n, after_d = before_n + int(totals[p, 3]), before_d + int(totals[p, 2])
            self.nfsp_steps[p], self.dqn_steps[p] = after_n, after_d
            sl_updates = after_n // L - before_n // L if len(self._reservoir_buffers[p]) else 0
            rl_updates = after_d // L - before_d // L
            if sl_updates:      # those that fall in an AVERAGE_POLICY episode update the Q network too (nfsp.py:313-317)
                off = staged["ring_offsets"][p * E:(p + 1) * E + 1]
                end = before_n + torch.cumsum(off[1:] - off[:-1] + 1, 0)
                start = torch.cat([end.new_tensor([before_n]), end[:-1]])
                average = ((staged["modes"] >> p) & 1) == 0
                rl_updates += int(((end // L - start // L) * average).sum().item())
            for _ in range(sl_updates):
                self.last_sl_loss[p] = self._learn_average(p)
                self.updates[p][1] += 1
            for _ in range(rl_updates):
                self.last_rl_loss[p] = self._learn_q(p)
                self.updates[p][0] += 1
            for _ in range(after_d // self._update_target_network_every - before_d // self._update_target_network_every):
                self._copy_weights(p)
                self.updates[p][2] += 1
        return totals

    def _ready(self, buffer):
        return len(buffer) >= self._batch_size and len(buffer) >= self._min_buffer_size_to_learn

    def _learn_q(self, p):
        """DQN.learn (dqn.py:501-569)."""
        ring = self._replay_buffers[p]
        if not self._ready(ring):
            return None
        self._samples_drawn += 1
        info, action, reward, next_info, final = ring.sample(self._batch_size, self._seed ^ SAMPLE_SALT, self._samples_drawn)
        live = final == 0
        nxt = next_info.clamp(min=0).long()
        next_states = self._tensors[nxt] * live.unsqueeze(1)
        next_mask = self._legal_mask[nxt] & live.unsqueeze(1)
        q_values = self._q_networks[p](self._tensors[info.long()])
        target_q = self._target_q_networks[p](next_states).detach()
        max_next_q = target_q.masked_fill(~next_mask, ILLEGAL_ACTION_LOGITS_PENALTY).max(dim=1)[0]
        target = (reward + live * self._discount_factor * max_next_q).detach()
        predictions = q_values.gather(-1, action.long().unsqueeze(-1)).squeeze(-1)
        loss = self._rl_loss(predictions, target)
        self._rl_optimizers[p].zero_grad()
        loss.backward()
        self._rl_optimizers[p].step()
        return loss.item()

    def _learn_average(self, p):
        """NFSP._learn (nfsp.py:364-409): cross-entropy of the masked logits against the stored probabilities."""
        memory = self._reservoir_buffers[p]
        if not self._ready(memory):
            return None
        self._samples_drawn += 1
        info, _, probs = memory.sample(self._batch_size, self._seed ^ SAMPLE_SALT, self._samples_drawn)
        info = info.long()
        logits = self._avg_networks[p](self._tensors[info])
        logits = torch.where(self._legal_mask[info], logits, torch.full_like(logits, ILLEGAL_ACTION_LOGITS_PENALTY))
        loss = F.cross_entropy(logits, probs).mean()
        self._sl_optimizers[p].zero_grad()
        loss.backward()
        if self._gradient_norm_clipping is not None:
            nn.utils.clip_grad_norm_(self._avg_networks[p].parameters(), self._gradient_norm_clipping)
        self._sl_optimizers[p].step()
        return loss.item()

    @torch.no_grad()
    def _copy_weights(self, p):
        tau = self._tau
        for target, param in zip(self._target_q_networks[p].parameters(), self._q_networks[p].parameters()):
            target.data.copy_(tau * param.data + (1.0 - tau) * target.data)

    # ---- policies -----------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def policy_table(self, mode="average"):
        """[I, Amax] float64 (NumPy), column k the k-th legal action of the infostate — the layout of
        TabularSolver.evaluate_policy(which="table").  "average": the average-policy network's masked softmax;
        "best_response": the greedy policy of the Q network (the first legal id on a tie)."""
        q, avg = self.tables()
        legal = self._legal >= 0
        ids = self._legal.clamp(min=0)
        zero = torch.zeros((), dtype=torch.float64, device=q.device)
        if mode == "average":
            table = torch.where(legal, avg.to(torch.float64).gather(1, ids), zero)
            table = table / table.sum(1, keepdim=True)
        elif mode == "best_response":
            values = torch.where(legal, q.gather(1, ids), torch.full_like(q, -float("inf")))
            table = F.one_hot(values.argmax(1), num_classes=q.shape[1]).to(torch.float64)
        else:
            raise ValueError("mode: 'average' or 'best_response'")
        return table.cpu().numpy()

    def evaluate(self, mode="average"):
        return self.tabular.evaluate_policy(which="table", table=self.policy_table(mode))

    def nash_conv(self, mode="average"):
        return self.evaluate(mode)["nash_conv"]


__all__ = ["NFSPSolver", "TransitionRing", "MLP"]
