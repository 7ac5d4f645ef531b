"""Batched State API over the HIP engine (host-side mirror of pyspiel.State).

The reference exposes one state at a time (`state.legal_actions_mask()`,
`state.apply_action(a)`, `state.is_terminal()`, `state.returns()`,
`state.observation_tensor(p)`; open_spiel/python/pybind11/pyspiel.cc:356-474).
`StateBatch` keeps those names and meanings, vectorised over N states that live
struct-of-arrays in HBM.  PyTorch is plumbing only (device buffers, streams,
torch.distributed); every rule evaluation runs in libosg_hip.so.
"""
import ctypes as C
import os
import warnings

import numpy as np
import torch

from . import _abi
from ._abi import OsgError, check, lib

TERMINAL_PLAYER = -4
CHANCE_PLAYER = -1


def _bad_tensor_message(t, dtype, numel, what, device):
    """Why `t` is not a buffer StateBatch hands to a kernel (StateBatch._checked; the native step raises the same text)."""
    if not isinstance(t, torch.Tensor):
        return f"{what}: expected a torch tensor on {device}"
    return (f"{what}: need a contiguous {dtype} tensor of {numel} elements on {device}, "
            f"got {t.dtype} {tuple(t.shape)} on {t.device}"
            f"{'' if t.is_contiguous() else ' (non-contiguous)'}")


def _import_native_step():
    """open_spiel_amd._osg_step_fast (csrc/host/osg_step_fast.cc): StateBatch.step's tensor checks and its osg_step
    call in one native call.  None under OSG_STEP_PY=1 (an A/B switch: step() runs its Python body, _step_py), or when
    the extension does not import; then step() runs the Python body and this warns once."""
    if os.environ.get("OSG_STEP_PY") == "1":
        return None
    try:
        from . import _osg_step_fast
    except ImportError as e:
        warnings.warn(f"open_spiel_amd._osg_step_fast did not import ({e}); StateBatch.step runs its Python body "
                      "(build it with `make -C open_spiel_amd/csrc`)", RuntimeWarning)
        return None
    return _osg_step_fast


_native_step = _import_native_step()


def _ptr(t):
    """Device / host pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


class Context:
    """One per (process, device): binds the engine to a HIP stream."""

    def __init__(self, device=0, stream=None):
        if not torch.cuda.is_available():
            raise OsgError("no MI355X visible (torch.cuda.is_available() is False): the engine "
                           "has no CPU fallback")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self.torch_stream = stream
        h = C.c_void_p()
        check(lib().osg_ctx_create(device, C.c_void_p(stream.cuda_stream), 0, C.byref(h)))
        self._h = h

    def synchronize(self):
        check(lib().osg_ctx_synchronize(self._h))

    def trim(self):
        """Free what the context caches between calls (the MCTS node pool, the staging buffer)."""
        check(lib().osg_ctx_trim(self._h))

    def set_stream(self, stream):
        """Issue every later call of this context's objects on `stream` (a torch.cuda.Stream of the same device),
        e.g. the stream a graph is being captured on; returns the stream that was bound before."""
        before = self.torch_stream
        check(lib().osg_ctx_set_stream(self._h, C.c_void_p(stream.cuda_stream)))
        self.torch_stream = stream
        return before

    def close(self):
        if self._h:
            lib().osg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Game:
    """Static description of a game string (pyspiel.Game subset)."""

    def __init__(self, game_string):
        self.game_string = game_string
        self.desc = _abi.describe(game_string)

    def num_distinct_actions(self):
        return self.desc.num_distinct_actions

    def max_chance_outcomes(self):
        return self.desc.max_chance_outcomes

    def num_players(self):
        return self.desc.num_players

    def max_game_length(self):
        return self.desc.max_game_length

    def min_utility(self):
        return self.desc.min_utility

    def max_utility(self):
        return self.desc.max_utility

    def observation_tensor_shape(self):
        return [self.desc.obs_shape[i] for i in range(self.desc.obs_rank)]

    def observation_tensor_size(self):
        return self.desc.obs_size

    def information_state_tensor_shape(self):
        return [self.desc.info_shape[i] for i in range(self.desc.info_rank)]

    def information_state_tensor_size(self):
        return self.desc.info_size

    def __str__(self):
        return self.desc.canonical.decode()

    def new_initial_states(self, ctx, n):
        return StateBatch(ctx, self.game_string, n)

    def solve(self, ctx, depth_limit=-1, include_terminals=True, max_states=1 << 26):
        """Every reachable position and its game-theoretic value (algorithms.get_all_states + value_iteration) for
        tic_tac_toe, connect_four and hex without the swap move: a SolvedGame.  depth_limit / include_terminals as
        get_all_states; a game with more than max_states positions raises OsgError."""
        return SolvedGame(ctx, self.game_string, depth_limit, include_terminals, max_states)


class StateBatch:
    """N states of one game in HBM (all start at Game::NewInitialState())."""

    def __init__(self, ctx, game_string, n):
        h = C.c_void_p()
        check(lib().osg_batch_create(ctx._h, game_string.encode(), int(n), C.byref(h)))
        self._adopt(ctx, game_string, h, owner=None)

    @classmethod
    def borrowed(cls, ctx, game_string, handle, owner):
        """A StateBatch over an osg_batch that `owner` owns (kept alive as long as the view is): close() only lets go."""
        self = cls.__new__(cls)
        self._adopt(ctx, game_string, C.c_void_p(handle), owner)
        return self

    def _adopt(self, ctx, game_string, h, owner):
        self.ctx = ctx
        self.game_string = game_string
        self._owner = owner   # None: the batch is this object's to destroy
        self.n = int(lib().osg_batch_size(h))
        self._h = h
        self._hraw = h.value  # the osg_batch* as an int for the native step (0 once closed)
        self.desc = _abi.GameDesc()
        check(lib().osg_batch_describe(self._h, C.byref(self.desc)))
        self.num_players = self.desc.num_players
        self.num_distinct_actions = self.desc.num_distinct_actions
        self._cmb = self.desc.compact_mask_bytes
        self._device_index = ctx.device.index
        if _native_step is not None and not _native_step.bound():
            _native_step.bind(OsgError, _bad_tensor_message, torch.uint8, torch.device,
                              C.cast(lib().osg_step, C.c_void_p).value, C.cast(lib().osg_last_error, C.c_void_p).value)

    def __len__(self):
        return self.n

    def close(self):
        """Free the states now; step() on a closed batch (as source or destination) raises."""
        if self._h:
            if self._owner is None:
                lib().osg_batch_destroy(self._h)
            self._owner = None
            self._h = None
            self._hraw = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.ctx.device)

    def _checked(self, t, dtype, numel, what):
        """A caller-supplied device buffer handed to a kernel by raw pointer: right dtype, on this
        context's device, contiguous, exactly `numel` elements — anything else would read or write
        out of bounds silently."""
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or t.device != self.ctx.device \
                or not t.is_contiguous() or t.numel() != numel:
            raise OsgError(_bad_tensor_message(t, dtype, numel, what, self.ctx.device))
        return t

    # -- State::Clone / reset ------------------------------------------------
    def reset(self):
        check(lib().osg_batch_reset(self._h))

    def clone(self):
        other = StateBatch(self.ctx, self.game_string, self.n)
        check(lib().osg_batch_copy(other._h, self._h))
        return other

    def gather(self, index):
        """New batch with state i = self[index[i]] (Clone() of chosen states)."""
        idx = torch.as_tensor(index, dtype=torch.int64, device=self.ctx.device).contiguous()
        other = StateBatch(self.ctx, self.game_string, idx.numel())
        check(lib().osg_batch_gather(other._h, self._h, _ptr(idx), 0))
        return other

    def raw_words(self):
        """The SoA image [state_words, n] as a numpy array (debug / fixtures)."""
        dt = np.uint64 if self.desc.state_word_bytes == 8 else np.uint32
        out = np.empty((self.desc.state_words, self.n), dt)
        check(lib().osg_batch_download(self._h, out.ctypes.data))
        return out

    def load_raw_words(self, words):
        dt = np.uint64 if self.desc.state_word_bytes == 8 else np.uint32
        w = np.ascontiguousarray(words, dt)
        assert w.shape == (self.desc.state_words, self.n)
        check(lib().osg_batch_upload(self._h, w.ctypes.data))

    def set_cells(self, index, cells):
        """State `index` := the position with these cells ('.', 'x', 'o'; tic_tac_toe: cell a = action a; connect_four:
        cell r * cols + c with row 0 the bottom row) — TicTacToeState(game, struct) / ConnectFourState(game, struct | string)
        (osg_batch_set_cells: built on the device with the game's own rules)."""
        text = cells.encode() if isinstance(cells, str) else bytes(cells)
        check(lib().osg_batch_set_cells(self._h, int(index), text, len(text)))

    # -- State::LegalActionsMask ---------------------------------------------
    def legal_actions_mask_bits(self):
        """[n, mask_words] int32 bit-packed legal mask (chance outcomes at chance nodes)."""
        out = self._dev((self.n, self.desc.mask_words), torch.int32)
        check(lib().osg_legal_mask(self._h, _ptr(out), 0))
        return out

    def legal_actions_bool(self):
        """[n, A] bool, True where action a is legal for the player to move: the bit mask against a row of powers of
        two (two small launches; legal_actions_mask() builds the reference's 0 / 1 layout with six)."""
        bits = self.legal_actions_mask_bits()
        A = self.desc.num_distinct_actions
        if getattr(self, "_pow2", None) is None:
            a = torch.arange(A, device=self.ctx.device)
            self._pow2 = (torch.ones_like(a, dtype=torch.int64) << (a % 32)).to(torch.int32)   # bit 31 wraps to the sign bit
            self._word = (a // 32).to(torch.int64)
        words = bits if bits.shape[1] == 1 else bits.index_select(1, self._word)
        return (words & self._pow2) != 0

    def legal_actions_mask(self):
        """[n, max(A, C)] uint8, one entry per action id (State::LegalActionsMask)."""
        bits = self.legal_actions_mask_bits()
        width = max(self.desc.num_distinct_actions, self.desc.max_chance_outcomes)
        shifts = torch.arange(32, device=bits.device, dtype=torch.int32)
        expanded = ((bits.unsqueeze(-1) >> shifts) & 1).reshape(self.n, -1)
        return expanded[:, :width].to(torch.uint8)

    # -- State::ApplyAction ----------------------------------------------------
    def apply_actions(self, actions, check_legal=True):
        """Apply actions[i] to state i (-1 = leave untouched).  Illegal actions raise."""
        a = torch.as_tensor(actions, dtype=torch.int32, device=self.ctx.device).contiguous()
        if a.numel() != self.n:
            raise OsgError("apply_actions: need one action per state")
        illegal = C.c_int64(0)
        check(lib().osg_apply(self._h, _ptr(a), 0, C.byref(illegal) if check_legal else None))
        if check_legal and illegal.value:
            raise OsgError(f"{illegal.value} illegal action(s) in apply_actions")

    # -- IsTerminal / CurrentPlayer / Returns ------------------------------------
    def status(self, want_returns=True):
        cur = self._dev((self.n,), torch.int8)
        term = self._dev((self.n,), torch.uint8)
        rets = self._dev((self.n, self.num_players), torch.float64) if want_returns else None
        check(lib().osg_status_query(self._h, _ptr(cur), _ptr(term), _ptr(rets), 0))
        return cur, term, rets

    def current_player(self):
        return self.status(False)[0]

    def is_terminal(self):
        return self.status(False)[1].bool()

    def returns(self):
        return self.status(True)[2]

    def chance_outcome_probs(self):
        """[n, max_chance_outcomes] float64: ChanceOutcomes() probabilities by outcome id."""
        out = self._dev((self.n, max(self.desc.max_chance_outcomes, 1)), torch.float64)
        check(lib().osg_chance_probs(self._h, _ptr(out), 0))
        return out

    # -- tensors -----------------------------------------------------------------
    def observation_tensor(self, player=-1, out=None):
        if out is None:
            out = self._dev((self.n, self.desc.obs_size), torch.float32)
        else:
            self._checked(out, torch.float32, self.n * self.desc.obs_size, "observation_tensor(out=)")
        check(lib().osg_observation(self._h, int(player), 0, _ptr(out), 0))
        return out

    def information_state_tensor(self, player=-1, out=None):
        if out is None:
            out = self._dev((self.n, self.desc.info_size), torch.float32)
        else:
            self._checked(out, torch.float32, self.n * self.desc.info_size, "information_state_tensor(out=)")
        check(lib().osg_observation(self._h, int(player), 1, _ptr(out), 0))
        return out

    def observation_string(self, index, player):
        """State::ObservationString(player) of state `index` (host formatter over the packed words)."""
        buf = C.create_string_buffer(1024)
        rc = lib().osg_observation_string(self._h, int(index), int(player), buf, 1024)
        if rc < 0:
            check(rc)
        return buf.value.decode()

    def state_string(self, index):
        """State::ToString() of state `index`."""
        buf = C.create_string_buffer(1024)
        rc = lib().osg_state_string(self._h, int(index), buf, 1024)
        if rc < 0:
            check(rc)
        return buf.value.decode()

    def action_string(self, index, player, action):
        """State::ActionToString(player, action) for state `index` (player -1 = chance)."""
        buf = C.create_string_buffer(64)
        rc = lib().osg_action_string(self._h, int(index), int(player), int(action), buf, 64)
        if rc < 0:
            check(rc)
        return buf.value.decode()

    def information_state_string(self, index, player):
        """State::InformationStateString(player) of state `index` (kuhn_poker / leduc_poker)."""
        buf = C.create_string_buffer(1024)
        rc = lib().osg_information_state_string(self._h, int(index), int(player), buf, 1024)
        if rc < 0:
            check(rc)
        return buf.value.decode()

    # -- the fused step -------------------------------------------------------------
    def step_buffers(self):
        mask = self._dev((self.n, self.desc.compact_mask_bytes), torch.uint8)
        status = self._dev((self.n,), torch.uint8)
        return mask, status

    def step(self, actions_u8, dst=None, mask=None, status=None, want_mask=True):
        """Fused legality check + ApplyAction + status + successor legal mask.

        actions_u8: [n] uint8 device tensor (0xFF = skip).  dst: destination batch
        (default: in place).  Returns (mask bytes [n, compact_mask_bytes], status [n]).
        want_mask=False (hex boards of up to 128 cells): the successor's mask row is not written — on a hex
        board it is ~occupied of the successor record; returns (None, status).
        The checks of the caller's buffers and the launch are one native call (_osg_step_fast); _step_py is the same
        step in Python (OSG_STEP_PY=1).
        """
        if _native_step is None:
            return self._step_py(actions_u8, dst, mask, status, want_mask)
        if dst is None:
            dst = self
        if not want_mask:
            mask = None
            if status is None:
                status = self._dev((self.n,), torch.uint8)
        elif mask is None or status is None:
            mask, status = self.step_buffers()
        _native_step.step(self._hraw, dst._hraw, self.n, dst.n, self.game_string, dst.game_string,
                          actions_u8, mask, status, self._cmb, self._device_index)
        return mask, status

    def _step_py(self, actions_u8, dst=None, mask=None, status=None, want_mask=True):
        if dst is None:
            dst = self
        if not self._h or not dst._h:
            raise OsgError("step: the batch or its destination is closed")
        if not want_mask:
            mask = None
            if status is None:
                status = self._dev((self.n,), torch.uint8)
            else:
                self._checked(status, torch.uint8, self.n, "step(status=)")
        elif mask is None or status is None:
            mask, status = self.step_buffers()
        else:
            self._checked(mask, torch.uint8, self.n * self.desc.compact_mask_bytes, "step(mask=)")
            self._checked(status, torch.uint8, self.n, "step(status=)")
        self._checked(actions_u8, torch.uint8, self.n, "step(actions_u8)")
        if dst.n != self.n or dst.game_string != self.game_string:
            raise OsgError("step(dst=): destination batch of a different game or size")
        check(lib().osg_step(self._h, dst._h, _ptr(actions_u8), None if mask is None else _ptr(mask), _ptr(status)))
        return mask, status

    # -- random play ------------------------------------------------------------------
    def random_steps(self, seed, steps, counters=None, index_offset=0):
        """`steps` uniformly random env steps per state with auto-reset; returns the
        [2] uint64-as-int64 device counters (steps applied, episodes finished)."""
        if counters is None:
            counters = torch.zeros(2, dtype=torch.int64, device=self.ctx.device)
        check(lib().osg_random_steps(self._h, int(seed), int(index_offset), int(steps), _ptr(counters)))
        return counters

    def synth(self, seed, depth_mod, index_offset=0):
        """SURVEY.md 8(d) synthetic inputs (osg_synth_batch): state i becomes the initial state advanced by
        depth_i = draw mod depth_mod random legal moves on the counter stream (seed, index_offset + i), never
        terminal; returns (actions [n] uint8 — one random legal action per state —, depth [n] int32).  The CPU
        oracle regenerates the same batch from (seed, index range, depth_mod)."""
        actions = self._dev((self.n,), torch.uint8)
        depth = self._dev((self.n,), torch.int32)
        check(lib().osg_synth_batch(self._h, int(seed), int(index_offset), int(depth_mod), _ptr(actions), _ptr(depth)))
        return actions, depth

    def rollout(self, seed, n_rollouts, index_offset=0, want_steps=False):
        """RandomRolloutEvaluator: SUM of Returns() over n_rollouts playouts per root."""
        total = self._dev((self.n, self.num_players), torch.float64)
        steps = self._dev((self.n,), torch.int32) if want_steps else None
        check(lib().osg_rollout(self._h, int(seed), int(index_offset), int(n_rollouts), _ptr(total),
                                _ptr(steps), 0))
        return (total, steps) if want_steps else total

    def mcts_search(self, uct_c=2.0, max_simulations=1024, n_rollouts=1, solve=False, max_nodes=0,
                    seed=0, index_offset=0, layout=0, puct=False):
        """MCTSBot.mcts_search for every root.  layout: 0 auto, 1 lane per root, 2 wave per root;
        puct: ChildSelectionPolicy.PUCT instead of UCT."""
        A = self.num_distinct_actions
        cfg = _abi.MctsCfg(uct_c, max_simulations, n_rollouts, int(solve), max_nodes, seed, index_offset,
                           int(layout), 1 if puct else 0)
        best = self._dev((self.n,), torch.int32)
        visits = self._dev((self.n, A), torch.int32)
        reward = self._dev((self.n, A), torch.float64)
        outcome = self._dev((self.n, A), torch.int8)
        stats = self._dev((self.n, 4), torch.float64)
        check(lib().osg_mcts_search(self._h, C.byref(cfg), _ptr(best), _ptr(visits), _ptr(reward),
                                    _ptr(outcome), _ptr(stats), 0))
        return dict(best_action=best, child_visits=visits, child_reward=reward, child_outcome=outcome,
                    root_stats=stats)

    def alpha_beta_search(self, depth_limit=-1, maximizing_player=None, leaf_value=None, max_nodes=1 << 22,
                          on_host=False):
        """algorithms.minimax.alpha_beta_search for every root, node for node (tic_tac_toe, connect_four, hex up to
        128 cells).  depth_limit < 0: unlimited; maximizing_player None: the player to move at each root;
        leaf_value: the constant a `value_function=lambda s: c` would return at the depth limit (None: no value
        function); max_nodes: node budget per root.  Returns (value f64, best_action i32, nodes i64, status u8), on the
        device unless on_host.  status 0 done, 1 depth limit reached with no leaf value (the reference's
        NotImplementedError), 2 budget exhausted — reported per root, never raised; value is NaN there."""
        cfg = _abi.AbCfg(int(depth_limit), -1 if maximizing_player is None else int(maximizing_player),
                         0 if leaf_value is None else 1, 0.0 if leaf_value is None else float(leaf_value), int(max_nodes))
        if on_host:
            value, best = torch.empty(self.n, dtype=torch.float64), torch.empty(self.n, dtype=torch.int32)
            nodes, status = torch.empty(self.n, dtype=torch.int64), torch.empty(self.n, dtype=torch.uint8)
        else:
            value, best = self._dev((self.n,), torch.float64), self._dev((self.n,), torch.int32)
            nodes, status = self._dev((self.n,), torch.int64), self._dev((self.n,), torch.uint8)
        check(lib().osg_alpha_beta_search(self._h, C.byref(cfg), _ptr(value), _ptr(best), _ptr(nodes), _ptr(status),
                                          1 if on_host else 0))
        return value, best, nodes, status


    def ismcts_search(self, uct_c=2.0, max_simulations=1024, n_rollouts=1, max_world_samples=0, final_policy_type=2,
                      puct=False, max_nodes=0, seed=0, index_offset=0, want_tree=False):
        """ISMCTSBot.step_with_policy (python/algorithms/ismcts.py) with RandomRolloutEvaluator(n_rollouts) for every
        root of a kuhn_poker or leduc_poker batch; every root must be a decision node.  max_world_samples 0: unlimited;
        final_policy_type 1 NORMALIZED_VISITED_COUNT, 2 MAX_VISIT_COUNT, 3 MAX_VALUE (or the enum of open_spiel_amd.ismcts);
        max_nodes 0: as many as the search can create.  Returns device tensors: policy [n, A] f64, sampled_action [n]
        i32, child_visits [n, A] i32, child_return_sum [n, A] f64, expansion_rank [n, A] i32 (-1: never expanded),
        nodes [n] i32 and status [n] u8 (0 done, 1 root never visited, 2 table full, 3 bad record; the policy is NaN
        where it is not 0) — statuses are reported per root, never raised.
        want_tree: True or an iterable of root indices adds "draws" [n] int64 (host) and "trees" {root: ismcts_tree(root)}."""
        A = self.num_distinct_actions
        cfg = _abi.IsmctsCfg(float(uct_c), int(max_simulations), int(n_rollouts), int(max_world_samples),
                             int(getattr(final_policy_type, "value", final_policy_type)), 2 if puct else 1, int(max_nodes),
                             int(seed), int(index_offset))
        out = dict(policy=self._dev((self.n, A), torch.float64), sampled_action=self._dev((self.n,), torch.int32),
                   child_visits=self._dev((self.n, A), torch.int32), child_return_sum=self._dev((self.n, A), torch.float64),
                   expansion_rank=self._dev((self.n, A), torch.int32), nodes=self._dev((self.n,), torch.int32),
                   status=self._dev((self.n,), torch.uint8))
        check(lib().osg_ismcts_search(self._h, C.byref(cfg), *[_ptr(out[k]) for k in (
            "policy", "sampled_action", "child_visits", "child_return_sum", "expansion_rank", "nodes", "status")], 0))
        if want_tree is not False and want_tree is not None:
            draws = np.empty(self.n, np.int64)
            check(lib().osg_ismcts_tree_sizes(self._h, None, draws.ctypes.data))
            out["draws"] = torch.from_numpy(draws)
            out["trees"] = {int(r): self.ismcts_tree(r) for r in (range(self.n) if want_tree is True else want_tree)}
        return out

    def ismcts_tree(self, root):
        """Root `root`'s tree of this context's last ismcts_search over this batch, nodes in creation order (node 0 is the
        root's): dict(player [k], key [k] — the InformationStateString the node stands for —, total_visits [k], and
        [k, 3] by action visits, return_sum, rank (the insertion rank of the action's child, -1: never expanded))."""
        sizes = np.empty(self.n, np.int32)
        check(lib().osg_ismcts_tree_sizes(self._h, sizes.ctypes.data, None))
        k = int(sizes[int(root)])
        tree = dict(player=np.zeros(k, np.int32), total_visits=np.zeros(k, np.int32), visits=np.zeros((k, 3), np.int32),
                    return_sum=np.zeros((k, 3), np.float64), rank=np.full((k, 3), -1, np.int32), key=[])
        if k:
            states = StateBatch(self.ctx, self.game_string, k)
            check(lib().osg_ismcts_tree_download(self._h, int(root), k, states._h, *[tree[name].ctypes.data for name in (
                "player", "total_visits", "visits", "return_sum", "rank")]))
            tree["key"] = [states.information_state_string(i, int(tree["player"][i])) for i in range(k)]
            states.close()
        return tree


class SolvedGame:
    """The positions of a game level by level (a level = the positions after that many plies), within a level
    ascending by the canonical key, and what the backward pass found at each (osg_solve_* of include/osg_abi.h).

    states         StateBatch of the n positions in result order (position 0 is the initial state)
    values         [n] f64: the value for player 0 (value_iteration's dict, by position)
    optimal_mask   [n, mask_words] i32 bit-packed: the legal actions whose child has the position's value
    distance       [n] i32: plies to the end under optimal play (a win as fast, a loss or draw as slow as possible)
    level_offsets  [levels + 1] i64;  num_terminals
    edge_off [n + 1] i64, edge_action [edges] i32, edge_child [edges] i64 (-1: a child the limits left out)
    All tensors live on the context's device."""

    def __init__(self, ctx, game_string, depth_limit=-1, include_terminals=True, max_states=1 << 26):
        self.ctx = ctx
        self.game_string = game_string
        self._h = None
        h = C.c_void_p()
        check(lib().osg_solve_create(ctx._h, game_string.encode(), int(depth_limit), 1 if include_terminals else 0,
                                     int(max_states), C.byref(h)))
        self._h = h
        n, levels, edges, terminals = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64()
        check(lib().osg_solve_sizes(h, C.byref(n), C.byref(levels), C.byref(edges), C.byref(terminals)))
        self.n, self.num_levels, self.num_edges, self.num_terminals = n.value, levels.value, edges.value, terminals.value
        dev = ctx.device
        offs = np.empty(self.num_levels + 1, np.int64)
        check(lib().osg_solve_level_offsets(h, offs.ctypes.data))
        self.level_offsets = torch.from_numpy(offs).to(dev)
        self.states = StateBatch(ctx, game_string, self.n)
        check(lib().osg_solve_states(h, self.states._h))
        words = self.states.desc.mask_words
        self.values = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.optimal_mask = torch.empty((self.n, words), dtype=torch.int32, device=dev)
        self.distance = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.edge_off = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        self.edge_action = torch.empty(self.num_edges, dtype=torch.int32, device=dev)
        self.edge_child = torch.empty(self.num_edges, dtype=torch.int64, device=dev)
        check(lib().osg_solve_values(h, _ptr(self.values), 0))
        check(lib().osg_solve_optimal(h, _ptr(self.optimal_mask), _ptr(self.distance), 0))
        check(lib().osg_solve_edges(h, _ptr(self.edge_off), _ptr(self.edge_action), _ptr(self.edge_child), 0))
        ctx.synchronize()

    def __len__(self):
        return self.n

    def close(self):
        if self._h:
            lib().osg_solve_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lookup(self, batch):
        """[len(batch)] i64 on the device: the index of each state of `batch` in the result, -1 if it is not there."""
        out = torch.empty(batch.n, dtype=torch.int64, device=self.ctx.device)
        check(lib().osg_solve_lookup(self._h, batch._h, _ptr(out), 0))
        return out

    def state_strings(self):
        """State::ToString() of every position, in result order (host; small games)."""
        return [self.states.state_string(i) for i in range(self.n)]

    def value_dict(self):
        """value_iteration's {str(state): value} (host; small games)."""
        return dict(zip(self.state_strings(), self.values.cpu().tolist()))


class TabularSolver:
    """CFRSolver / CFRPlusSolver / external-sampling MCCFR on the device.

    Mirrors pyspiel.CFRSolver(game).evaluate_and_update_policy() /
    average_policy() (open_spiel/python/pybind11/policy.cc:224-333).
    """

    def __init__(self, ctx, game_string, alternating_updates=True, linear_averaging=False,
                 regret_matching_plus=False, mccfr=False, general_kernel=False, epsilon=0.6, replicas=1,
                 random_initial_regrets=False, seed=0, replica_offset=0, discounting=None):
        """mccfr: False (CFR family), True / "external" (ES-MCCFR) or "outcome" (OS-MCCFR, `epsilon`).
        discounting: None, or (alpha, beta, gamma) of Discounted CFR (see set_discounting)."""
        self.ctx = ctx
        self.game_string = game_string
        solver = {False: 0, True: 1, "external": 1, "outcome": 2}[mccfr]
        cfg = _abi.CfrCfg(int(alternating_updates), int(linear_averaging), int(regret_matching_plus),
                          solver, float(epsilon), {False: 0, True: 1, "grid": 2, "path": 3, "split": 4, "sub": 5}[general_kernel], int(replicas),
                          int(random_initial_regrets), int(seed), int(replica_offset))
        self.replicas = int(replicas)
        h = C.c_void_p()
        check(lib().osg_cfr_create(ctx._h, game_string.encode(), C.byref(cfg), C.byref(h)))
        self._h = h
        sizes = (C.c_int64 * 6)()
        check(lib().osg_cfr_sizes(self._h, sizes))
        (self.num_histories, self.num_chance, self.num_decision, self.num_terminal,
         self.num_infostates, self.amax) = [int(v) for v in sizes]
        self.discounting = None
        if discounting is not None:
            self.set_discounting(*discounting)

    def set_discounting(self, alpha=1.5, beta=0, gamma=2, enabled=True):
        """Discounted CFR (discounted_cfr.py:190-209) for the iterations that follow: after each player's pass of
        iteration t its regrets are multiplied by t**alpha / (t**alpha + 1) (>= 0) or t**beta / (t**beta + 1) (< 0), and
        with linear_averaging the average-policy term is weighted by t**gamma.  Needs alternating updates and no RM+."""
        check(lib().osg_cfr_set_discounting(self._h, 1 if enabled else 0, float(alpha), float(beta), float(gamma)))
        self.discounting = (alpha, beta, gamma) if enabled else None

    def __del__(self):
        try:
            if self._h:
                lib().osg_cfr_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def evaluate_and_update_policy(self, iters=1):
        check(lib().osg_cfr_iterate(self._h, int(iters)))

    def evaluate_and_update_policy_cfr_br(self, iters=1):
        """CFRBRSolver.evaluate_and_update_policy (cfr_br.cc:48-83): every player's regret / average-policy pass
        runs against the other players' best responses to the current policy.  The solver must have been
        created as plain CFR (no linear averaging, no RM+)."""
        check(lib().osg_cfr_br_iterate(self._h, int(iters)))

    def set_average_type(self, full):
        """ES-MCCFR AverageType (external_sampling_mccfr.h:48): False kSimple, True kFull."""
        check(lib().osg_mccfr_set_average_type(self._h, 1 if full else 0))

    def mccfr_full_average(self, weight=1.0):
        """FullUpdateAverage (external_sampling_mccfr.cc:188-231) on the tables as they are."""
        check(lib().osg_mccfr_full_average(self._h, C.c_double(weight)))

    def mccfr_sample_uniforms(self, player, uniforms):
        """One UpdateRegrets(root, player, rng) whose draws are `uniforms` in visiting order (the sequence the
        reference's std::mt19937 + uniform_real_distribution would give); returns how many were used.  The
        deltas are left in mccfr_delta_tables(): fold with mccfr_apply_deltas()."""
        u = np.ascontiguousarray(uniforms, np.float64)
        used = C.c_int32(0)
        check(lib().osg_mccfr_sample_uniforms(self._h, int(player), u.ctypes.data, int(u.size), C.byref(used)))
        return used.value

    def reset(self):
        check(lib().osg_cfr_reset(self._h))

    def select_replica(self, r):
        """Which of the `replicas` independent solvers tables() / evaluate_policy() look at."""
        check(lib().osg_cfr_select_replica(self._h, int(r)))

    @property
    def iteration(self):
        return lib().osg_cfr_iteration(self._h)

    def last_kernel(self):
        """The kernel family the last iterate / sample call launched (diagnostic, osg_cfr_last_kernel)."""
        return lib().osg_cfr_last_kernel(self._h).decode()

    def last_eval_kernel(self):
        """The form the last policy evaluation took (diagnostic, osg_cfr_last_eval_kernel)."""
        return lib().osg_cfr_last_eval_kernel(self._h).decode()

    def run_mccfr(self, seed, trajectories, first_trajectory=0):
        """One mini-batch of external-sampling traversals, folded into the tables."""
        check(lib().osg_mccfr_iterate(self._h, int(seed), int(first_trajectory), int(trajectories)))

    def mccfr_sample(self, seed, trajectories, first_trajectory=0):
        """Traversals only: deltas stay in mccfr_delta_tables() (all-reduce them, then
        mccfr_apply_deltas())."""
        check(lib().osg_mccfr_sample(self._h, int(seed), int(first_trajectory), int(trajectories)))

    def load_tables(self, regrets=None, cum_policy=None, cur_policy=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (regrets, cum_policy, cur_policy)]
        for a in arrs:
            assert a is None or a.shape == (self.num_infostates, self.amax)
        check(lib().osg_cfr_upload_tables(self._h, *[None if a is None else a.ctypes.data for a in arrs]))

    def _wrap(self, ptr, shape):
        """Zero-copy torch view of device fp64 memory owned by the solver."""
        holder = type("Holder", (), {})()
        holder.__cuda_array_interface__ = {
            "shape": tuple(shape), "typestr": "<f8", "data": (ptr, False), "version": 2, "strides": None}
        return torch.as_tensor(holder, device=self.ctx.device)

    def device_tables(self):
        """(regrets, cumulative policy, current policy) as [I, Amax] device views."""
        r, c, p = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().osg_cfr_table_ptrs(self._h, C.byref(r), C.byref(c), C.byref(p)))
        shape = (self.num_infostates, self.amax)
        return self._wrap(r.value, shape), self._wrap(c.value, shape), self._wrap(p.value, shape)

    def mccfr_delta_flat(self):
        """Both MCCFR delta tables as ONE [2, I, Amax] device view (they are adjacent in the
        solver's allocation), so a multi-GPU job needs a single all-reduce per mini-batch."""
        r, c = C.c_void_p(), C.c_void_p()
        check(lib().osg_mccfr_delta_ptrs(self._h, C.byref(r), C.byref(c)))
        n = self.num_infostates * self.amax
        if c.value != r.value + 8 * n:
            raise OsgError("delta tables are not adjacent")
        return self._wrap(r.value, (2, self.num_infostates, self.amax))

    def mccfr_delta_tables(self):
        flat = self.mccfr_delta_flat()
        return flat[0], flat[1]

    def mccfr_apply_deltas(self):
        check(lib().osg_mccfr_apply_deltas(self._h))

    def mccfr_new_delta_buffer(self):
        """A caller-owned [2, I, Amax] fp64 device buffer (regret deltas | average-policy deltas) for
        mccfr_sample_into / mccfr_apply_deltas_from: two of them double-buffer the exchange step."""
        return torch.zeros((2, self.num_infostates, self.amax), dtype=torch.float64, device=self.ctx.device)

    def _delta_buffer_ptr(self, buf, what):
        want = (2, self.num_infostates, self.amax)
        if (not isinstance(buf, torch.Tensor) or buf.dtype != torch.float64 or tuple(buf.shape) != want
                or not buf.is_contiguous() or buf.device != self.ctx.device):
            raise OsgError(f"{what}: expected a contiguous float64 tensor of shape {want} on {self.ctx.device}")
        return buf.data_ptr()

    def mccfr_sample_into(self, buf, seed, trajectories, first_trajectory=0):
        """Traversals only, deltas left in the caller's buffer (osg_mccfr_sample_into)."""
        check(lib().osg_mccfr_sample_into(self._h, int(seed), int(first_trajectory), int(trajectories),
                                          self._delta_buffer_ptr(buf, "mccfr_sample_into")))

    def mccfr_apply_deltas_from(self, buf):
        check(lib().osg_mccfr_apply_deltas_from(self._h, self._delta_buffer_ptr(buf, "mccfr_apply_deltas_from")))

    def tables(self):
        I, A = self.num_infostates, self.amax
        nact = np.zeros(I, np.int32)
        legal = np.zeros((I, A), np.int32)
        out = {k: np.zeros((I, A), np.float64) for k in ("regrets", "cum_policy", "cur_policy", "avg_policy")}
        check(lib().osg_cfr_tables(self._h, nact.ctypes.data, legal.ctypes.data, out["regrets"].ctypes.data,
                                   out["cum_policy"].ctypes.data, out["cur_policy"].ctypes.data,
                                   out["avg_policy"].ctypes.data))
        keys = []
        buf = C.create_string_buffer(512)
        for i in range(I):
            check(min(lib().osg_cfr_infostate_key(self._h, i, buf, 512), 0))
            keys.append(buf.value.decode())
        out.update(keys=keys, nact=nact, legal=legal)
        return out

    def infostate_tensors(self, device=True):
        """[I, info_size] float32: information_state_tensor(player of the infostate) of every infostate, in this
        solver's infostate order (a torch tensor on the device, or a NumPy array)."""
        E = _abi.describe(self.game_string).info_size
        if device:
            out = torch.empty((self.num_infostates, E), dtype=torch.float32, device=self.ctx.device)
            check(lib().osg_cfr_infostate_tensors(self._h, out.data_ptr(), 0))
            return out
        out = np.zeros((self.num_infostates, E), np.float32)
        check(lib().osg_cfr_infostate_tensors(self._h, out.ctypes.data, 1))
        return out

    def deep_cfr_traverse(self, advantages, player, iteration, seed, trajectories, first_trajectory=0,
                          advantage_buffer=None, strategy_buffer=None):
        """`trajectories` Deep CFR traversals for `player` (deep_cfr.py _traverse_game_tree) against `advantages`, an
        [I, Amax] float32 device tensor of advantage-network outputs by action id.  The sampled advantages go to
        advantage_buffer and the opponents' strategies to strategy_buffer (deep_cfr.ReservoirBuffer, or None) in the
        reference's append order; the solver's own tables are not touched.  Returns (advantage rows, strategy rows)."""
        want = (self.num_infostates, self.amax)
        if (not isinstance(advantages, torch.Tensor) or advantages.dtype != torch.float32 or tuple(advantages.shape) != want
                or not advantages.is_contiguous() or advantages.device != self.ctx.device):
            raise OsgError(f"deep_cfr_traverse: expected a contiguous float32 tensor of shape {want} on {self.ctx.device}")
        counts = (C.c_int64 * 2)()
        check(lib().osg_deep_cfr_traverse(self._h, advantages.data_ptr(), int(player), int(iteration), int(seed),
                                          int(first_trajectory), int(trajectories),
                                          None if advantage_buffer is None else advantage_buffer._h,
                                          None if strategy_buffer is None else strategy_buffer._h, counts))
        return int(counts[0]), int(counts[1])

    def deep_cfr_staged(self):
        """The rows of the last deep_cfr_traverse in append order: a dict of device tensors adv_offsets / strat_offsets
        [T + 1] int64, adv_info / strat_info [R] int32, adv_values / strat_values [R, Amax] float32, draws [T] int32, and
        `bounds`, the most advantage / strategy rows one trajectory can append."""
        sizes = (C.c_int64 * 5)()
        check(lib().osg_deep_cfr_staged(self._h, sizes, None, None, None, None, None, None, None))
        T, na, ns = int(sizes[0]), int(sizes[1]), int(sizes[2])
        dev = self.ctx.device
        out = dict(adv_offsets=torch.zeros(T + 1, dtype=torch.int64, device=dev), adv_info=torch.empty(na, dtype=torch.int32, device=dev),
                   adv_values=torch.empty((na, self.amax), dtype=torch.float32, device=dev),
                   strat_offsets=torch.zeros(T + 1, dtype=torch.int64, device=dev), strat_info=torch.empty(ns, dtype=torch.int32, device=dev),
                   strat_values=torch.empty((ns, self.amax), dtype=torch.float32, device=dev),
                   draws=torch.empty(T, dtype=torch.int32, device=dev))
        check(lib().osg_deep_cfr_staged(self._h, None, *[out[k].data_ptr() for k in (
            "adv_offsets", "adv_info", "adv_values", "strat_offsets", "strat_info", "strat_values", "draws")]))
        self.ctx.synchronize()
        out["bounds"] = (int(sizes[3]), int(sizes[4]))
        return out

    def nfsp_collect(self, q_values, avg_probs, epsilon, anticipatory, seed, episodes, first_episode=0, rings=None,
                     reservoirs=None):
        """`episodes` NFSP self-play episodes (nfsp.py / dqn.py under the loop of examples/kuhn_nfsp.py) against
        q_values and avg_probs, [I, Amax] float32 device tensors by action id (the Q-network outputs and the average
        policy's probabilities, zero at illegal ids).  epsilon / anticipatory: a number or one per player.  Player p's
        DQN transitions go to rings[p] (nfsp.TransitionRing) and the supervised rows of its BEST_RESPONSE decisions to
        reservoirs[p] (deep_cfr.ReservoirBuffer) in the reference's append order; a list or an entry may be None.
        Returns an int64 array [P, 4]: transitions, supervised rows, DQN-agent steps, NFSP-agent steps per player."""
        P = _abi.describe(self.game_string).num_players
        want = (self.num_infostates, self.amax)
        for t in (q_values, avg_probs):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != want or not t.is_contiguous()
                    or t.device != self.ctx.device):
                raise OsgError(f"nfsp_collect: expected contiguous float32 tensors of shape {want} on {self.ctx.device}")
        eps = np.ascontiguousarray(np.broadcast_to(np.asarray(epsilon, np.float64), (P,)))
        ant = np.ascontiguousarray(np.broadcast_to(np.asarray(anticipatory, np.float64), (P,)))

        def handles(bufs):
            if bufs is None:
                return None
            if len(bufs) != P:
                raise OsgError(f"nfsp_collect: expected {P} buffers (entries may be None)")
            return (C.c_void_p * P)(*[None if b is None else b._h for b in bufs])

        totals = np.zeros((P, 4), np.int64)
        check(lib().osg_nfsp_collect(self._h, q_values.data_ptr(), avg_probs.data_ptr(), eps.ctypes.data, ant.ctypes.data,
                                     int(seed) & (2 ** 64 - 1), int(first_episode), int(episodes), handles(rings),
                                     handles(reservoirs), totals.ctypes.data))
        return totals

    def nfsp_staged(self):
        """The rows of the last nfsp_collect in sequence order (player by player, a player's rows by episode, then by
        time): a dict of device tensors ring_offsets / sl_offsets [P * E + 1] int64 (entry p * E + j: the first row of
        player p in episode j), ring_info / ring_action / ring_next [R] int32, ring_reward [R] float32, ring_final [R]
        uint8, sl_info [S] int32, sl_probs [S, Amax] float32, draws / modes [E] int32 (bit p of modes: BEST_RESPONSE),
        and `bounds`, the most rows of either kind an episode can give each player."""
        P = _abi.describe(self.game_string).num_players
        sizes = (C.c_int64 * (4 + max(P, 8)))()
        check(lib().osg_nfsp_staged(self._h, sizes, *([None] * 11)))
        E, nr, ns = int(sizes[0]), int(sizes[1]), int(sizes[2])
        dev = self.ctx.device
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)   # noqa: E731
        out = dict(ring_offsets=torch.zeros(P * E + 1, dtype=torch.int64, device=dev), ring_info=i32(nr), ring_action=i32(nr),
                   ring_reward=torch.empty(nr, dtype=torch.float32, device=dev), ring_next=i32(nr),
                   ring_final=torch.empty(nr, dtype=torch.uint8, device=dev),
                   sl_offsets=torch.zeros(P * E + 1, dtype=torch.int64, device=dev), sl_info=i32(ns),
                   sl_probs=torch.empty((ns, self.amax), dtype=torch.float32, device=dev), draws=i32(E), modes=i32(E))
        check(lib().osg_nfsp_staged(self._h, None, *[out[k].data_ptr() for k in (
            "ring_offsets", "ring_info", "ring_action", "ring_reward", "ring_next", "ring_final", "sl_offsets", "sl_info",
            "sl_probs", "draws", "modes")]))
        self.ctx.synchronize()
        out["bounds"] = tuple(int(sizes[4 + p]) for p in range(P))
        return out

    def evaluate_policy(self, which="average", table=None):
        """NashConv / exploitability / expected returns / best-response values of a policy on the
        device (algorithms::NashConv, Exploitability, ExpectedReturns, TabularBestResponse).
        which: "average" | "current" | "table" (then `table` is an [I, Amax] array in this
        solver's infostate order)."""
        code = {"average": 0, "current": 1, "table": 2}[which]
        P = _abi.describe(self.game_string).num_players
        ev, br = np.zeros(P), np.zeros(P)
        nc, ex = C.c_double(0), C.c_double(0)
        tab = None
        if code == 2:
            tab = np.ascontiguousarray(table, np.float64)
            assert tab.shape == (self.num_infostates, self.amax)
        check(lib().osg_cfr_evaluate_policy(self._h, code, None if tab is None else tab.ctypes.data,
                                            ev.ctypes.data, br.ctypes.data, C.byref(nc), C.byref(ex)))
        return dict(nash_conv=nc.value, exploitability=ex.value, expected_returns=ev, best_response_values=br)

    def nash_conv(self):
        return self.evaluate_policy()["nash_conv"]

    def exploitability(self):
        return self.evaluate_policy()["exploitability"]

    def action_values(self, which="average", table=None, responder=None, device=False, layout="legal"):
        """Per-infostate action values and reaches of a policy on the device (action_value.TreeWalkCalculator; with
        `responder`, the profile of action_value_vs_best_response.Calculator: that player best-responds, two-player
        games only).  which / table as for evaluate_policy.  Returns a dict: root_values [P], action_values and
        cf_reach_by_value [I, Amax], weighted_values [I, Amax, P], reach, cf_reach, chance_reach, player_reach [I], and
        with a responder best_response_value and best_index [I] (-1 at the other players' rows): osg_cfr_action_values
        in include/osg_abi.h has the definitions.  device=False: numpy arrays.  device=True: torch fp64 tensors on
        the context's device, enqueued on its stream with no host round trip, and `table` may be a device tensor.
        layout "legal": columns are the row's legal actions ascending; "action_id": action_values and
        cf_reach_by_value are [I, num_distinct_actions] indexed by action id, zeros at illegal ids (the reference's
        shape)."""
        code = {"average": 0, "current": 1, "table": 2}[which]
        if layout not in ("legal", "action_id"):
            raise OsgError(f"action_values: layout must be 'legal' or 'action_id', not {layout!r}")
        I, A = self.num_infostates, self.amax
        P = _abi.describe(self.game_string).num_players
        b = -1 if responder is None else int(responder)
        shapes = dict(root_values=(P,), action_values=(I, A), cf_reach=(I,), player_reach=(I,), reach=(I,),
                      chance_reach=(I,), cf_reach_by_value=(I, A), weighted_values=(I, A, P))
        if b >= 0:
            shapes.update(best_response_value=(1,), best_index=(I,))
        tab = None
        if code == 2:
            if device:
                tab = torch.as_tensor(table, dtype=torch.float64, device=self.ctx.device).contiguous()
            else:
                tab = np.ascontiguousarray(table, np.float64)
            if tuple(tab.shape) != (I, A):
                raise OsgError(f"action_values: expected a table of shape {(I, A)}")
        if device:
            res = {k: torch.zeros(shape, dtype=torch.int32 if k == "best_index" else torch.float64, device=self.ctx.device)
                   for k, shape in shapes.items()}
            addr = lambda t: t.data_ptr()
        else:
            res = {k: np.zeros(shape, np.int32 if k == "best_index" else np.float64) for k, shape in shapes.items()}
            addr = lambda a: a.ctypes.data
        out = _abi.ActionValuesOut(**{k: addr(v) for k, v in res.items()})
        check(lib().osg_cfr_action_values(self._h, code, None if tab is None else addr(tab), b, 0 if device else 1,
                                          C.byref(out)))
        if b >= 0:
            res["best_response_value"] = res["best_response_value"][0] if device else float(res["best_response_value"][0])
        if layout == "action_id":
            n_ids = _abi.describe(self.game_string).num_distinct_actions
            nact, legal = np.zeros(I, np.int32), np.zeros((I, A), np.int32)
            check(lib().osg_cfr_tables(self._h, nact.ctypes.data, legal.ctypes.data, None, None, None, None))
            rows, cols = np.nonzero(np.arange(A)[None, :] < nact[:, None])
            ids = legal[rows, cols]
            for k in ("action_values", "cf_reach_by_value"):
                if device:
                    wide = torch.zeros((I, n_ids), dtype=torch.float64, device=self.ctx.device)
                    r, c, d = (torch.as_tensor(x, device=self.ctx.device, dtype=torch.int64) for x in (rows, cols, ids))
                    wide[r, d] = res[k][r, c]
                else:
                    wide = np.zeros((I, n_ids))
                    wide[rows, ids] = res[k][rows, cols]
                res[k] = wide
        return res

    def action_values_vs_best_response(self, player, which="average", table=None):
        """action_value_vs_best_response.Calculator(game)(player, policy, info_states) for `player`'s information
        states in this solver's order: `player` plays the policy, the opponent best-responds.  Returns a dict:
        exploitability (the best responder's value), values_vs_br [n, num_distinct_actions] (indexed by action id,
        zeros at illegal ids), counterfactual_reach_probs_vs_br [n], player_reach_probs_vs_br [n], and rows [n], the
        solver's infostate indices of `player`'s rows."""
        player = int(player)
        P = _abi.describe(self.game_string).num_players
        if P != 2:   # action_value_vs_best_response.py:67
            raise OsgError(f"action_values_vs_best_response: only supports 2-player games ({P} players)")
        if player not in (0, 1):
            raise OsgError(f"action_values_vs_best_response: no player {player}")
        res = self.action_values(which, table, responder=1 - player, layout="action_id")
        rows = np.nonzero(res["best_index"] < 0)[0]
        return dict(exploitability=res["best_response_value"], values_vs_br=res["action_values"][rows],
                    counterfactual_reach_probs_vs_br=res["cf_reach"][rows], player_reach_probs_vs_br=res["player_reach"][rows],
                    rows=rows)

    def _table_stack(self, tables, device, what):
        """`tables` as a contiguous fp64 [K, I, Amax] stack: numpy, or with device=True a tensor on the context's device."""
        I, A = self.num_infostates, self.amax
        if device:
            stack = torch.as_tensor(tables, dtype=torch.float64, device=self.ctx.device).contiguous()
        else:
            stack = np.ascontiguousarray(tables, np.float64)
        if stack.ndim != 3 or tuple(stack.shape[1:]) != (I, A) or stack.shape[0] < 1:
            raise OsgError(f"{what}: expected a stack of tables of shape [K >= 1, {I}, {A}], not {tuple(stack.shape)}")
        return stack

    def infostate_players(self):
        """[I] int32: the player who acts at each information state, in this solver's row order."""
        return np.array([lib().osg_cfr_infostate_player(self._h, i) for i in range(self.num_infostates)], np.int32)

    def profile_returns(self, tables, profiles, device=False):
        """The expected returns of every listed profile of a population (expected_game_score.policy_value, one tree walk
        per profile in the reference): `tables` is a stack [K, I, Amax] of policy tables in this solver's layout,
        "policy k of player p" table k's rows at p's infostates; `profiles` is [M, P] int, player q of profile m
        follows table profiles[m, q].  Returns [M, P].  device=False: numpy in and out.  device=True: torch tensors
        (tables fp64, profiles int32) on the context's device, enqueued on its stream with no host round trip; there an
        index out of range is found on the device: the call writes nothing and the next population call raises.
        osg_cfr_profile_returns in include/osg_abi.h has the definitions and the limits."""
        P = _abi.describe(self.game_string).num_players
        stack = self._table_stack(tables, device, "profile_returns")
        if device:
            prof = torch.as_tensor(profiles, device=self.ctx.device).to(torch.int32).contiguous()
        else:
            prof = np.ascontiguousarray(profiles)
            if prof.dtype.kind not in "iu":
                raise OsgError("profile_returns: profiles must be integers")
            prof = np.ascontiguousarray(prof, np.int32)
        if prof.ndim != 2 or prof.shape[1] != P:
            raise OsgError(f"profile_returns: expected profiles of shape [M, {P}], not {tuple(prof.shape)}")
        M = int(prof.shape[0])
        if device:
            out = torch.zeros((M, P), dtype=torch.float64, device=self.ctx.device)
            addr = lambda t: t.data_ptr()
        else:
            out = np.zeros((M, P))
            addr = lambda a: a.ctypes.data
        check(lib().osg_cfr_profile_returns(self._h, addr(stack), int(stack.shape[0]), addr(prof), M, 0 if device else 1, addr(out)))
        return out

    def payoff_tensors(self, tables, populations=None, device=False):
        """The meta-game of a population in psro_v2's `meta_games` convention: a list of P arrays of shape
        [K_0, ..., K_{P-1}], out[q][i_0, ..., i_{P-1}] the return of player q when every player p follows its i_p-th
        policy.  populations[p] lists the tables (indices into `tables`) that are player p's policies; default: every
        table for every player.  One profile_returns call over the cartesian product."""
        P = _abi.describe(self.game_string).num_players
        stack = self._table_stack(tables, device, "payoff_tensors")
        if populations is None:
            populations = [range(int(stack.shape[0]))] * P
        pops = [np.asarray(list(p), np.int32) for p in populations]
        if len(pops) != P or any(p.ndim != 1 or len(p) < 1 for p in pops):
            raise OsgError(f"payoff_tensors: expected {P} non-empty lists of table indices")
        grid = np.stack(np.meshgrid(*pops, indexing="ij"), axis=-1).reshape(-1, P).astype(np.int32)
        if device:
            grid = torch.as_tensor(grid, device=self.ctx.device)
        ret = self.profile_returns(stack, grid, device=device)
        shape = [len(p) for p in pops]
        return [ret[:, q].reshape(shape) for q in range(P)]

    def aggregate_policies(self, tables, weights, epsilon=1e-40, device=False):
        """policy_aggregator.PolicyAggregator(game, epsilon).aggregate for all players at once: the [I, Amax] behavioural
        policy that is realization-equivalent to every player p mixing the tables of the stack [K, I, Amax] with
        weights[p] ([P, K], >= 0 and finite).  A table of weight 0 contributes nothing; a row no table reaches is
        uniform.  device as for profile_returns.  osg_cfr_aggregate_policies in include/osg_abi.h has the definition."""
        P = _abi.describe(self.game_string).num_players
        stack = self._table_stack(tables, device, "aggregate_policies")
        K = int(stack.shape[0])
        if device:
            w = torch.as_tensor(weights, dtype=torch.float64, device=self.ctx.device).contiguous()
            out = torch.zeros((self.num_infostates, self.amax), dtype=torch.float64, device=self.ctx.device)
            addr = lambda t: t.data_ptr()
        else:
            w = np.ascontiguousarray(weights, np.float64)
            out = np.zeros((self.num_infostates, self.amax))
            addr = lambda a: a.ctypes.data
        if tuple(w.shape) != (P, K):
            raise OsgError(f"aggregate_policies: expected weights of shape {(P, K)}, not {tuple(w.shape)}")
        check(lib().osg_cfr_aggregate_policies(self._h, addr(stack), K, addr(w), float(epsilon), 0 if device else 1, addr(out)))
        return out

    def average_policy(self):
        t = self.tables()
        return {k: [(int(t["legal"][i, a]), float(t["avg_policy"][i, a])) for a in range(t["nact"][i])]
                for i, k in enumerate(t["keys"])}


class DCFRSolver(TabularSolver):
    """discounted_cfr.DCFRSolver(game, alpha=3/2, beta=0, gamma=2) on the device: alternating updates, linear
    averaging, no RM+, regrets discounted after every player's pass (Brown & Sandholm 2019)."""

    def __init__(self, ctx, game_string, alpha=1.5, beta=0, gamma=2, **kw):
        super().__init__(ctx, game_string, alternating_updates=True, linear_averaging=True, regret_matching_plus=False,
                         discounting=(alpha, beta, gamma), **kw)


class LCFRSolver(DCFRSolver):
    """discounted_cfr.LCFRSolver(game): Linear CFR = DCFR with alpha = beta = gamma = 1."""

    def __init__(self, ctx, game_string, **kw):
        super().__init__(ctx, game_string, alpha=1, beta=1, gamma=1, **kw)


class XFPSolver(TabularSolver):
    """fictitious_play.XFPSolver(game) on the device: extensive-form fictitious play (Heinrich, Lanctot and Silver 2015,
    Algorithm 1).  XFP has no parameters.  The average policy lives in the solver's current-policy table (uniform at the
    start); every iteration mixes every player's best response to it into it (osg_xfp_iterate in include/osg_abi.h has
    the arithmetic).  The trajectory depends on argmax decisions: where the reference's best response sits on an exact
    or rounding-level tie, feed that iteration's best response through update().
    general_kernel: as for TabularSolver (True: the general per-iteration form where the fused kernel applies; "grid":
    the best response by a launch per level).  The reference's save_oracles and get_empirical_metagame are out of
    scope: no best response is kept beyond its iteration."""

    def __init__(self, ctx, game_string, general_kernel=False):
        super().__init__(ctx, game_string, alternating_updates=True, linear_averaging=False, regret_matching_plus=False,
                         general_kernel=general_kernel)

    def iteration(self):
        """XFPSolver.iteration() (fictitious_play.py:165-168).  The reference's method takes the name of TabularSolver's
        counter property; the counter is `iterations` here, as the reference calls its own."""
        self.iterate(1)

    @property
    def iterations(self):
        """Fictitious-play iterations done so far (osg_cfr_iteration)."""
        return lib().osg_cfr_iteration(self._h)

    def iterate(self, iters=1):
        check(lib().osg_xfp_iterate(self._h, int(iters)))

    def best_responses(self):
        """Every player's best response to the average policy: ([I] int32 indices among each row's legal actions, [P]
        best-response values)."""
        best = np.zeros(self.num_infostates, np.int32)
        values = np.zeros(_abi.describe(self.game_string).num_players)
        check(lib().osg_cfr_best_response(self._h, 1, None, best.ctypes.data, values.ctypes.data))
        return best, values

    def _best_index(self, best_index):
        best = np.ascontiguousarray(best_index, np.int32)
        if best.shape != (self.num_infostates,):
            raise OsgError(f"best_index: expected {self.num_infostates} indices, one per information state")
        return best

    def update(self, best_index):
        """The averaging half of one iteration with the caller's best responses (osg_xfp_update)."""
        best = self._best_index(best_index)
        check(lib().osg_xfp_update(self._h, best.ctypes.data))

    def reaches(self, best_index=None):
        """(avg_reach [I], br_reach [I]) the next update would use; best_index None: the device's own best responses."""
        best = None if best_index is None else self._best_index(best_index)
        avg, br = np.zeros(self.num_infostates), np.zeros(self.num_infostates)
        check(lib().osg_xfp_reaches(self._h, None if best is None else best.ctypes.data, avg.ctypes.data, br.ctypes.data))
        return avg, br

    def evaluate_and_update_policy(self, iters=1):
        raise OsgError("XFPSolver: iterate() / iteration() advance fictitious play; a CFR iteration would overwrite the average policy")

    evaluate_and_update_policy_cfr_br = evaluate_and_update_policy

    def evaluate_policy(self, which="current", table=None):
        return super().evaluate_policy(which, table)

    def nash_conv(self):
        return self.evaluate_policy("current")["nash_conv"]

    def exploitability(self):
        return self.evaluate_policy("current")["exploitability"]

    def average_policy_tables(self):
        """XFPSolver.average_policy_tables(): per player, {infostate string: {action: probability}}."""
        t = self.tables()
        out = [{} for _ in range(_abi.describe(self.game_string).num_players)]
        for i, k in enumerate(t["keys"]):
            player = lib().osg_cfr_infostate_player(self._h, i)
            out[player][k] = {int(t["legal"][i, a]): float(t["cur_policy"][i, a]) for a in range(t["nact"][i])}
        return out

    def average_policy(self):
        t = self.tables()
        return {k: [(int(t["legal"][i, a]), float(t["cur_policy"][i, a])) for a in range(t["nact"][i])]
                for i, k in enumerate(t["keys"])}


class MMDSolver(TabularSolver):
    """mmd_dilated.MMDDilatedEnt(game, alpha, stepsize) on the device: magnetic mirror descent over the sequence form with
    dilated entropy (Sokota et al. 2023).  With alpha > 0 the LAST iterate converges linearly to the alpha-reduced
    normal-form QRE; with alpha = 0 it is mirror descent-ascent and the average converges to a Nash equilibrium.  The
    policy lives in the current-policy table, the average sequences in the cumulative-policy table (osg_mmd_set_params in
    include/osg_abi.h; csrc/osg_mmd.h has the arithmetic).
    alpha, stepsize: scalars or one value per replica (a sweep: replica r runs with its own pair); stepsize None is the
    reference's default alpha / max|payoff|**2.  general_kernel=True forces the launch-per-level form (one replica)."""

    def __init__(self, ctx, game_string, alpha, stepsize=None, replicas=1, general_kernel=False):
        super().__init__(ctx, game_string, alternating_updates=True, linear_averaging=False, regret_matching_plus=False,
                         general_kernel=general_kernel, replicas=replicas)
        self.set_params(alpha, stepsize)

    def _per_replica(self, value, what):
        v = np.atleast_1d(np.asarray(value, np.float64))
        if v.shape == (1,):
            v = np.repeat(v, self.replicas)
        if v.ndim != 1:
            raise OsgError(f"MMDSolver: {what} must be a scalar or a sequence")
        return np.ascontiguousarray(v)

    def default_stepsize(self, alpha):
        out = C.c_double(0)
        check(lib().osg_mmd_default_stepsize(self._h, C.c_double(float(alpha)), C.byref(out)))
        return out.value

    def set_params(self, alpha, stepsize=None):
        """The parameters of the update_sequences() calls that follow; the state is kept (annealing)."""
        a = self._per_replica(alpha, "alpha")
        if stepsize is None:
            e = np.array([self.default_stepsize(v) for v in a], np.float64)
        else:
            e = self._per_replica(stepsize, "stepsize")
        if e.size != a.size:
            raise OsgError("MMDSolver: alpha and stepsize differ in length")
        check(lib().osg_mmd_set_params(self._h, int(a.size), a.ctypes.data, e.ctypes.data))
        self.alpha, self.stepsize = a.copy(), e.copy()

    def iterate(self, iters=1):
        check(lib().osg_mmd_iterate(self._h, int(iters)))

    def update_sequences(self):
        """MMDDilatedEnt.update_sequences() (mmd_dilated.py:261-281)."""
        self.iterate(1)

    def get_gap(self):
        """MMDDilatedEnt.get_gap() of the selected replica: the saddle-point gap of the regularised game (alpha > 0)."""
        out = C.c_double(0)
        check(lib().osg_mmd_gap(self._h, C.byref(out)))
        return out.value

    def _sequences(self, which):
        x = np.zeros((self.num_infostates, self.amax), np.float64)
        check(lib().osg_mmd_sequences(self._h, which, x.ctypes.data))
        return x

    def current_sequences(self):
        """[I, Amax]: the sequence value of every (infostate, action) under the current policy."""
        return self._sequences(0)

    def get_avg_sequences(self):
        return self._sequences(1)

    def _policy_dict(self, name):
        t = self.tables()
        return {k: [(int(t["legal"][i, a]), float(t[name][i, a])) for a in range(t["nact"][i])]
                for i, k in enumerate(t["keys"])}

    def get_policies(self):
        """get_policies(): the current behavioural policy, {infostate string: [(action, probability)]}."""
        return self._policy_dict("cur_policy")

    def get_avg_policies(self):
        """get_avg_policies(): the average sequences row-normalised (sequence_form_utils.py:284-322)."""
        return self._policy_dict("avg_policy")

    def evaluate_and_update_policy(self, iters=1):
        raise OsgError("MMDSolver: iterate() / update_sequences() advance mirror descent; a CFR iteration would overwrite its tables")

    evaluate_and_update_policy_cfr_br = evaluate_and_update_policy

    def evaluate_policy(self, which="current", table=None):
        return super().evaluate_policy(which, table)

    def nash_conv(self):
        return self.evaluate_policy("current")["nash_conv"]

    def exploitability(self):
        return self.evaluate_policy("current")["exploitability"]


class EFRSolver(TabularSolver):
    """efr.EFRSolver(game, deviations_name) on the device: extensive-form regret minimization (Morrill et al. 2021).  The
    deviation set decides which hindsight-rationality class the empirical play approaches; `blind cf` is CFR with
    simultaneous updates.  The current policy lives in the current-policy table and the reach-weighted cumulative policy
    in the cumulative-policy table, so tables(), evaluate_policy(), nash_conv() and action_values() are the inherited
    ones; the regrets are per (information state, deviation) (osg_efr_set_deviations in include/osg_abi.h; csrc/osg_efr.h
    has the arithmetic).  kuhn_poker and leduc_poker with any served number of players, one replica.
    form: None (by tree size), "resident" (one launch of one workgroup per call) or "levels" (a launch per phase)."""

    DEVIATION_SETS = {
        "blind action": 0, "informed action": 1, "blind cf": 2, "blind counterfactual": 2, "informed cf": 3,
        "informed counterfactual": 3, "bps": 4, "blind partial sequence": 4, "cfps": 5, "cf partial sequence": 5,
        "counterfactual partial sequence": 5, "csps": 6, "casual partial sequence": 6, "tips": 7,
        "twice informed partial sequence": 7, "bhv": 8, "single target behavioural": 8, "behavioural": 8}

    def __init__(self, ctx, game_string, deviations_name, form=None, replicas=1):
        self._h = None
        self._check_arguments(deviations_name, form)
        super().__init__(ctx, game_string, alternating_updates=False, linear_averaging=False, regret_matching_plus=False,
                         replicas=replicas)
        self.set_deviations(deviations_name, form)

    @classmethod
    def _check_arguments(cls, deviations_name, form):
        if deviations_name not in cls.DEVIATION_SETS:   # efr.py:490-494, the message as the reference words it
            raise ValueError("Unsupported Deviation Set Passed              As Constructor Argument")
        if form not in (None, "resident", "levels"):
            raise OsgError(f"EFRSolver: form must be None, 'resident' or 'levels', not {form!r}")

    def set_deviations(self, deviations_name, form=None):
        """Builds the tables of another deviation set (or kernel form) on the same tree and starts over: uniform policy,
        R = 0, counter 0 (osg_efr_set_deviations)."""
        self._check_arguments(deviations_name, form)
        check(lib().osg_efr_set_deviations(self._h, self.DEVIATION_SETS[deviations_name], {None: 0, "resident": 1, "levels": 2}[form]))
        self.deviations_name = deviations_name
        self.external_only = self.DEVIATION_SETS[deviations_name] in (0, 2, 4)
        sizes = (C.c_int64 * 5)()
        check(lib().osg_efr_sizes(self._h, sizes))
        self.num_deviations, self.max_deviations, self.memory, self._state_doubles, self.depths = [int(v) for v in sizes]

    def evaluate_and_update_policy(self, iters=1):
        """_EFRSolver.evaluate_and_update_policy() (efr.py:424-433), `iters` times."""
        check(lib().osg_efr_iterate(self._h, int(iters)))

    def evaluate_and_update_policy_cfr_br(self, iters=1):
        raise OsgError("EFRSolver: evaluate_and_update_policy() advances EFR; a CFR-BR iteration would overwrite its tables")

    def deviation_counts(self):
        """dict(total=, max_per_infostate=, memory=): deviations of the set on this game, and L."""
        return dict(total=self.num_deviations, max_per_infostate=self.max_deviations, memory=self.memory)

    def deviations(self):
        """The deviation tables (osg_efr_deviations): dict of offsets [I + 1], target, source, weights_none, y_slot [D],
        weights, memory, cells [D, L]."""
        D, L = self.num_deviations, self.memory
        out = dict(offsets=np.zeros(self.num_infostates + 1, np.int32), target=np.zeros(D, np.int8), source=np.zeros(D, np.int8),
                   weights_none=np.zeros(D, np.int8), weights=np.zeros((D, L), np.int8), memory=np.zeros((D, L), np.int8),
                   y_slot=np.zeros(D, np.int32), cells=np.zeros((D, L), np.int32))
        check(lib().osg_efr_deviations(self._h, *[out[k].ctypes.data for k in
                                                  ("offsets", "target", "source", "weights_none", "weights", "memory", "y_slot", "cells")]))
        return out

    def regret_state(self):
        """The checkpointable regret state (osg_efr_regrets): R per deviation, then the carried y values."""
        state = np.zeros(self._state_doubles, np.float64)
        check(lib().osg_efr_regrets(self._h, state.ctypes.data))
        return state

    def load_regret_state(self, state):
        state = np.ascontiguousarray(state, np.float64)
        if state.shape != (self._state_doubles,):
            raise OsgError(f"load_regret_state: expected {self._state_doubles} doubles")
        check(lib().osg_efr_upload_regrets(self._h, state.ctypes.data))

    def set_iteration(self, iteration):
        check(lib().osg_cfr_set_iteration(self._h, int(iteration)))

    def return_cumulative_regret(self):
        """{infostate string: [cumulative regret by deviation index]} (efr.py:121-132)."""
        R = self.regret_state()[:self.num_deviations]
        off = self.deviations()["offsets"]
        return {k: R[off[i]:off[i + 1]].tolist() for i, k in enumerate(self.tables()["keys"])}

    def current_policy(self):
        """[I, Amax]: the current policy table, columns the row's legal actions ascending."""
        return self.tables()["cur_policy"]

    def average_policy(self):
        """[I, Amax]: the average policy table (efr.py:144-163), a row the regret pass never reached uniform."""
        return self.tables()["avg_policy"]
