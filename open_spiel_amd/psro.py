"""Policy-space response oracles (Lanctot et al. 2017; open_spiel/python/algorithms/psro_v2/) with exact best responses
on the kuhn_poker / leduc_poker trees: the population, the payoff tensors' new cells, the aggregation of a meta-strategy
into one behavioural policy and the best responses to it all run on the device (TabularSolver.profile_returns,
aggregate_policies, osg_cfr_best_response), and so do psro_v2's "prd" and "rm" meta-solvers (projected replicator
dynamics and regret matching, meta_solvers.py: every iteration of a solve in one launch) and its default, "alpharank" (the
sweep over the infinite-alpha noise, of which the MARGINALS are played); a meta-solver passed as a callable runs on the
host.  Out of scope: strategy selectors other than "add every player's best response", sampled
meta-game estimation (sims_per_entry), reinforcement-learning oracles, the LP Nash solver ("nash"; pass one as a
callable), "uniform_biased" and joint meta-strategies (psro_v2 hands alpha-rank's joint distribution to its rectified /
joint training; here its marginals are played)."""
import functools
import itertools

import numpy as np
import torch

from . import _abi, meta_solvers
from ._abi import OsgError, check, lib
from .engine import TabularSolver

DEVICE_META_SOLVERS = {"prd": meta_solvers.projected_replicator_dynamics, "rm": meta_solvers.regret_matching,
                       "alpharank": meta_solvers.alpharank_strategy}


def uniform_meta_solver(payoff_tensors):
    """psro_v2's uniform strategy: every policy of a player's population with the same weight."""
    return [np.full(k, 1.0 / k) for k in payoff_tensors[0].shape]


class PSROSolver:
    """PSRO / double oracle on the device.  `meta_solver`: "uniform"; "prd" or "rm", projected replicator dynamics or
    regret matching on the device with `meta_solver_kwargs` under the reference's names (prd_iterations, prd_dt,
    prd_gamma / iterations, gamma, average_over_last_n_strategies, ...; its defaults otherwise); "alpharank", the marginals
    of alpha-rank's swept distribution on the device; or any callable that takes
    the payoff tensors (a list of P arrays [K_0, ..., K_{P-1}], psro_v2's `meta_games`) and returns P weight vectors, the
    reference's meta-solvers among them.  `initial`: "uniform", or an [I, Amax] policy table in the solver's layout: every player's
    first policy.  With the uniform meta-solver and the uniform initial policy this is fictitious play with kept
    oracles: the aggregate after t iterations is XFPSolver's average policy, up to argmax ties.

    The population is a stack of tables on the device (grown geometrically); every iteration appends ONE table whose
    rows are the one-hot best responses of all players, and player p's population is a list of indices into the stack."""

    def __init__(self, ctx, game_string, meta_solver="uniform", initial="uniform", meta_solver_kwargs=None):
        self.ctx = ctx
        self.game_string = game_string
        self.solver = TabularSolver(ctx, game_string)
        self.num_players = _abi.describe(game_string).num_players
        I, A = self.solver.num_infostates, self.solver.amax
        if meta_solver_kwargs and not (isinstance(meta_solver, str) and meta_solver in DEVICE_META_SOLVERS):
            raise OsgError("PSROSolver: meta_solver_kwargs go with meta_solver 'prd', 'rm' or 'alpharank'")
        if meta_solver == "uniform":
            meta_solver = uniform_meta_solver
        elif isinstance(meta_solver, str) and meta_solver in DEVICE_META_SOLVERS:
            meta_solver = functools.partial(DEVICE_META_SOLVERS[meta_solver], ctx, **dict(meta_solver_kwargs or {}))
        if not callable(meta_solver):
            raise OsgError(f"PSROSolver: meta_solver must be 'uniform', 'prd', 'rm', 'alpharank' or a callable, not {meta_solver!r}")
        self._meta_solver = meta_solver
        self._nact = np.zeros(I, np.int32)
        check(lib().osg_cfr_tables(self.solver._h, self._nact.ctypes.data, None, None, None, None, None))
        if isinstance(initial, str):
            if initial != "uniform":
                raise OsgError(f"PSROSolver: initial must be 'uniform' or a policy table, not {initial!r}")
            first = np.where(np.arange(A)[None, :] < self._nact[:, None], 1.0 / self._nact[:, None], 0.0)
        else:
            first = np.ascontiguousarray(initial, np.float64)
            if first.shape != (I, A):
                raise OsgError(f"PSROSolver: expected an initial table of shape {(I, A)}")
        self._stack = torch.zeros((8, I, A), dtype=torch.float64, device=ctx.device)
        self._stack[0] = torch.as_tensor(first, device=ctx.device)
        self._tables = 1
        self._populations = [[0] for _ in range(self.num_players)]
        self._tensors = [t.cpu().numpy() for t in self.solver.payoff_tensors(self._stack[:1], device=True)]
        self._last_weights = None
        self._last_values = None
        self.iterations = 0

    # ---- the population ----
    def _append(self, table):
        if self._tables == self._stack.shape[0]:
            grown = torch.zeros((2 * self._stack.shape[0],) + tuple(self._stack.shape[1:]), dtype=torch.float64, device=self.ctx.device)
            grown[:self._tables] = self._stack
            self._stack = grown
        self._stack[self._tables] = table
        self._tables += 1
        return self._tables - 1

    def _weight_matrix(self, meta_strategies):
        """[P, tables] on the device: player p's weights at its population's indices (a shorter vector covers the
        population's first policies), zero elsewhere."""
        W = np.zeros((self.num_players, self._tables))
        if len(meta_strategies) != self.num_players:
            raise OsgError(f"PSROSolver: expected {self.num_players} weight vectors")
        for p, w in enumerate(meta_strategies):
            w = np.asarray(w, np.float64).reshape(-1)
            if len(w) > len(self._populations[p]):
                raise OsgError(f"PSROSolver: player {p} has {len(self._populations[p])} policies, not {len(w)}")
            W[p, self._populations[p][:len(w)]] = w
        return torch.as_tensor(W, device=self.ctx.device)

    def policies(self):
        """Per player, its population as an array [K_p, I, Amax] (player p's policies are the tables' rows at p's infostates)."""
        return [self._stack[self._populations[p]].cpu().numpy() for p in range(self.num_players)]

    def table_stack(self):
        """The stack of tables on the device, [tables, I, Amax], and per player the indices of its policies."""
        return self._stack[:self._tables], [list(p) for p in self._populations]

    def meta_games(self):
        """The payoff tensors, psro_v2's get_meta_game(): P arrays [K_0, ..., K_{P-1}]."""
        return [t.copy() for t in self._tensors]

    def meta_strategies(self):
        """The meta-solver's answer on the current payoff tensors: P weight vectors."""
        ms = [np.asarray(w, np.float64).reshape(-1) for w in self._meta_solver(self.meta_games())]
        if [len(w) for w in ms] != [len(p) for p in self._populations]:
            raise OsgError("PSROSolver: the meta-solver must return one weight per policy of every player")
        return ms

    def last_meta_strategies(self):
        """The weights the latest iteration's best responses answered (one fewer per player than there are policies now)."""
        return None if self._last_weights is None else [w.copy() for w in self._last_weights]

    def last_best_response_values(self):
        """[P]: every player's best-response value against the mixture of the latest iteration."""
        return None if self._last_values is None else self._last_values.copy()

    def aggregate(self, meta_strategies=None, device=False):
        """The behavioural policy [I, Amax] realization-equivalent to the meta-strategy (default: meta_strategies())."""
        ms = self.meta_strategies() if meta_strategies is None else meta_strategies
        out = self.solver.aggregate_policies(self._stack[:self._tables], self._weight_matrix(ms), device=True)
        return out if device else out.cpu().numpy()

    def evaluate(self, meta_strategies=None):
        """evaluate_policy of the aggregate: nash_conv, exploitability, expected_returns, best_response_values."""
        return self.solver.evaluate_policy("table", self.aggregate(meta_strategies))

    def nash_conv(self, meta_strategies=None):
        return self.evaluate(meta_strategies)["nash_conv"]

    # ---- one iteration ----
    def iteration(self):
        """Meta-solver, aggregation, every player's best response to the aggregate, one new table, the new cells."""
        P = self.num_players
        weights = self.meta_strategies()
        mixture = self.aggregate(weights)
        best = np.zeros(self.solver.num_infostates, np.int32)
        values = np.zeros(P)
        check(lib().osg_cfr_best_response(self.solver._h, 2, mixture.ctypes.data, best.ctypes.data, values.ctypes.data))
        rows = torch.zeros(tuple(self._stack.shape[1:]), dtype=torch.float64, device=self.ctx.device)
        rows[torch.arange(len(best), device=self.ctx.device), torch.as_tensor(best, device=self.ctx.device, dtype=torch.int64)] = 1.0
        new = self._append(rows)
        old = [len(p) for p in self._populations]
        for p in range(P):
            self._populations[p].append(new)
        # the new cells: every profile that names a new policy for at least one player
        cells = np.array([c for c in itertools.product(*[range(k + 1) for k in old]) if any(c[p] == old[p] for p in range(P))], np.int64)
        profiles = np.stack([np.asarray(self._populations[p], np.int32)[cells[:, p]] for p in range(P)], axis=1)
        ret = self.solver.profile_returns(self._stack[:self._tables], torch.as_tensor(profiles, device=self.ctx.device), device=True).cpu().numpy()
        grown = []
        for q in range(P):
            t = np.zeros([k + 1 for k in old])
            t[tuple(slice(0, k) for k in old)] = self._tensors[q]
            t[tuple(cells.T)] = ret[:, q]
            grown.append(t)
        self._tensors = grown
        self._last_weights, self._last_values = weights, values
        self.iterations += 1

    def iterate(self, iters=1):
        for _ in range(int(iters)):
            self.iteration()
