"""PSRO's meta-strategy solvers on the device: psro_v2's "prd" (open_spiel/python/algorithms/
projected_replicator_dynamics.py) and "rm" (regret_matching.py), with the reference's keyword names and defaults.  A solve
is one launch of osg_meta_solve — every iteration, a workgroup per meta-game — and solve_meta_games takes a batch: many
meta-games of one shape, or a sweep of dt / gamma / iterations over copies of one.  csrc/osg_meta_solver.h fixes the order
of every sum; the reference's go through BLAS, so it is matched within rounding (1e-12 on the recorded cases), not bit for
bit.  Regret matching amplifies rounding once a regret changes sign: beyond a few hundred iterations two correct
implementations drift apart.

Alpha-rank, psro_v2's default meta-solver (open_spiel/python/egt/alpharank.py), is here too: alpharank_compute,
sweep_pi_vs_epsilon, alpharank_strategy and get_alpharank_marginals under the reference's names and defaults, and the
batched solve_alpharank over osg_alpharank.  Its stationary distributions come from a Grassmann-Taksar-Heyman
elimination (csrc/osg_alpharank.h) instead of the reference's eigen-solve: no negative masses, small masses accurate to
a relative 8 n 2^-53, and no "Expected 1 stationary distribution" where the chain is irreducible."""
import ctypes as C

import numpy as np
import torch

from . import _abi
from ._abi import OsgError, check, lib

METHODS = {"prd": 0, "rm": 1}
FORMS = {None: 0, "auto": 0, "lds": 1, "global": 2}


def _per_problem(value, B, dtype, name):
    a = np.asarray(value, dtype)
    if a.ndim == 0:
        return np.full(B, a)
    if a.shape != (B,):
        raise OsgError(f"solve_meta_games: {name} must be a scalar or have one entry per problem ({B}), not shape {a.shape}")
    return a


def solve_meta_games(ctx, tensors, method, iterations=int(1e5), dt=1e-3, gamma=1e-6, window=None, use_approx=False,
                     initial=None, return_last=False, form=None, device=False):
    """The batched form.  tensors [B, P, K_0 .. K_{P-1}]: B meta-games of one shape, each P payoff tensors.  method "prd"
    or "rm"; iterations, dt, gamma: scalars, or arrays [B] (then every problem runs its own: one launch for a sweep).
    window: average_over_last_n_strategies (None: the whole trajectory).  initial [B, sum K_p] or None (uniform).
    form: None (by size), "lds" or "global".  Returns the averaged strategies [B, sum K_p], player after player, and with
    return_last the last iterate as well.  device=True: tensors and initial are float64 torch tensors on the context's
    device, and so are the results, which are enqueued on its stream; otherwise NumPy arrays."""
    if method not in METHODS:
        raise OsgError(f"solve_meta_games: method must be 'prd' or 'rm', not {method!r}")
    if form not in FORMS:
        raise OsgError(f"solve_meta_games: form must be None, 'lds' or 'global', not {form!r}")
    if device:
        t = torch.as_tensor(tensors, dtype=torch.float64, device=ctx.device).contiguous()
        addr = lambda x: x.data_ptr()
        empty = lambda shape: torch.empty(shape, dtype=torch.float64, device=ctx.device)
    else:
        t = np.ascontiguousarray(tensors, np.float64)
        addr = lambda x: x.ctypes.data
        empty = lambda shape: np.empty(shape, np.float64)
    if t.ndim < 3 or t.shape[1] != t.ndim - 2:
        raise OsgError(f"solve_meta_games: expected tensors of shape [B, P, K_0 .. K_(P-1)], not {tuple(t.shape)}")
    B, P = int(t.shape[0]), int(t.shape[1])
    shape = np.array(t.shape[2:], np.int32)
    SK = int(shape.sum())
    shared = all(np.ndim(x) == 0 for x in (iterations, dt, gamma))
    n_cfgs = 1 if shared else B
    its, dts, gammas = (_per_problem(x, n_cfgs, kind, name) for x, kind, name in
                        ((iterations, np.int64, "iterations"), (dt, np.float64, "dt"), (gamma, np.float64, "gamma")))
    if n_cfgs and not (np.abs(its) < 2**31).all():
        raise OsgError("solve_meta_games: iterations does not fit 32 bits")
    cfgs = (_abi.MetaCfg * max(n_cfgs, 1))()
    for b in range(n_cfgs):
        cfgs[b].method, cfgs[b].window, cfgs[b].use_approx, cfgs[b].form = METHODS[method], int(window or 0), int(bool(use_approx)), FORMS[form]
        cfgs[b].iterations, cfgs[b].dt, cfgs[b].gamma = int(its[b]), float(dts[b]), float(gammas[b])
    init = None
    if initial is not None:
        init = (torch.as_tensor(initial, dtype=torch.float64, device=ctx.device).contiguous() if device
                else np.ascontiguousarray(initial, np.float64))
        if tuple(init.shape) != (B, SK):
            raise OsgError(f"solve_meta_games: expected initial strategies of shape {(B, SK)}, not {tuple(init.shape)}")
    average = empty((B, SK))
    last = empty((B, SK)) if return_last else None
    check(lib().osg_meta_solve(ctx._h, P, shape.ctypes.data, B, addr(t), C.cast(cfgs, C.c_void_p), n_cfgs,
                               None if init is None else addr(init), addr(average), None if last is None else addr(last),
                               0 if device else 1))
    return (average, last) if return_last else average


def _solve_one(ctx, payoff_tensors, method, initial, **kwargs):
    t = np.stack([np.asarray(x, np.float64) for x in payoff_tensors])
    shape = t.shape[1:]
    if initial:
        if len(initial) != len(shape) or [len(s) for s in initial] != list(shape):
            raise OsgError(f"meta-solver: the initial strategies must be one vector per player, of lengths {list(shape)}")
        initial = np.concatenate([np.asarray(s, np.float64) for s in initial])[None]
    else:
        initial = None
    flat = solve_meta_games(ctx, t[None], method, initial=initial, **kwargs)[0]
    return [np.array(x) for x in np.split(flat, np.cumsum(shape)[:-1])]


def projected_replicator_dynamics(ctx, payoff_tensors, prd_initial_strategies=None, prd_iterations=int(1e5), prd_dt=1e-3,
                                  prd_gamma=1e-6, average_over_last_n_strategies=None, use_approx=False, **unused_kwargs):
    """projected_replicator_dynamics.projected_replicator_dynamics on the device: P weight vectors."""
    return _solve_one(ctx, payoff_tensors, "prd", prd_initial_strategies, iterations=prd_iterations, dt=prd_dt, gamma=prd_gamma,
                      window=average_over_last_n_strategies, use_approx=use_approx)


def regret_matching(ctx, payoff_tensors, initial_strategies=None, iterations=int(1e5), gamma=1e-6,
                    average_over_last_n_strategies=None, **unused_kwargs):
    """regret_matching.regret_matching on the device: P weight vectors."""
    return _solve_one(ctx, payoff_tensors, "rm", initial_strategies, iterations=iterations, gamma=gamma,
                      window=average_over_last_n_strategies)


# ---- alpha-rank (open_spiel/python/egt/alpharank.py; psro_v2's default meta-solver) ----
AR_MODES = {"finite": 0, "infinite": 1, "sweep": 2}


def solve_alpharank(ctx, tensors, mode="sweep", m=50, alpha=100.0, eps=None, min_iters=10, max_iters=100, single_population=False,
                    form=None, chunk=0, device=False):
    """The batched form of alpha-rank: one call of osg_alpharank.  tensors [B, P, K_0 .. K_{P-1}]: B meta-games of one
    shape, each P payoff tensors; with single_population [B, 1, K, K] (or [B, K, K]): one square table each.  mode:
    "finite" (alpha, m), "infinite" (eps = inf_alpha_eps) or "sweep" (eps = warm_start_epsilon, None: 0.5; min_iters,
    max_iters).  mode, m, alpha and eps: scalars, or sequences [B] (then every problem runs its own: a sweep over alpha or
    m is one call).  form: None (by size), "lds" or "global"; chunk: epsilons per launch (0: the library's choice).
    Returns a dict: pi [B, n], marginals [B, sum K_p], eps [B], iterations [B], status [B] (0; 1: the chain is not
    irreducible in floating point, pi is NaN; 2: the sweep did not stop before max_iters).  device=True: tensors is a float64
    torch tensor on the context's device and so are the results; otherwise NumPy arrays."""
    if form not in FORMS:
        raise OsgError(f"solve_alpharank: form must be None, 'lds' or 'global', not {form!r}")
    if device:
        t = torch.as_tensor(tensors, dtype=torch.float64, device=ctx.device).contiguous()
        addr = lambda x: x.data_ptr()
        empty = lambda shape, kind=torch.float64: torch.empty(shape, dtype=kind, device=ctx.device)
        i32 = torch.int32
    else:
        t = np.ascontiguousarray(tensors, np.float64)
        addr = lambda x: x.ctypes.data
        empty = lambda shape, kind=np.float64: np.empty(shape, kind)
        i32 = np.int32
    if single_population:
        if t.ndim == 3:
            t = t[:, None]
        if t.ndim != 4 or t.shape[1] != 1:
            raise OsgError(f"solve_alpharank: a single population takes tensors of shape [B, 1, K, K], not {tuple(t.shape)}")
        P = 1
    else:
        if t.ndim < 4 or t.shape[1] != t.ndim - 2:
            raise OsgError(f"solve_alpharank: expected tensors of shape [B, P, K_0 .. K_(P-1)] with P >= 2, not {tuple(t.shape)}")
        P = int(t.shape[1])
    B = int(t.shape[0])
    shape = np.array(t.shape[2:], np.int32)
    n = int(shape[0]) if P == 1 else int(shape.prod())
    SK = int(shape[0]) if P == 1 else int(shape.sum())
    eps = 0.0 if eps is None else eps
    shared = all(np.ndim(x) == 0 for x in (m, alpha, eps)) and isinstance(mode, str)
    n_cfgs = 1 if shared else B
    modes = [mode] * n_cfgs if isinstance(mode, str) else list(mode)
    if len(modes) != n_cfgs or any(x not in AR_MODES for x in modes):
        raise OsgError(f"solve_alpharank: mode must be 'finite', 'infinite' or 'sweep' (or one of them per problem), not {mode!r}")
    ms, alphas, epss = (_per_problem(x, n_cfgs, kind, name) for x, kind, name in
                        ((m, np.int64, "m"), (alpha, np.float64, "alpha"), (eps, np.float64, "eps")))
    if n_cfgs and not (np.abs(ms) < 2**31).all():
        raise OsgError("solve_alpharank: m does not fit 32 bits")
    cfgs = (_abi.AlphaRankCfg * max(n_cfgs, 1))()
    for b in range(n_cfgs):
        cfgs[b].mode, cfgs[b].m, cfgs[b].alpha, cfgs[b].eps = AR_MODES[modes[b]], int(ms[b]), float(alphas[b]), float(epss[b])
        cfgs[b].min_iters, cfgs[b].max_iters, cfgs[b].form, cfgs[b].chunk = int(min_iters), int(max_iters), FORMS[form], int(chunk)
    out = dict(pi=empty((B, n)), marginals=empty((B, SK)), eps=empty((B,)), iterations=empty((B,), i32), status=empty((B,), i32))
    check(lib().osg_alpharank(ctx._h, P, shape.ctypes.data, B, addr(t), C.cast(cfgs, C.c_void_p), n_cfgs, addr(out["pi"]),
                              addr(out["marginals"]), addr(out["eps"]), addr(out["iterations"]), addr(out["status"]), 0 if device else 1))
    return out


def _alpharank_one(ctx, payoff_tensors, **kwargs):
    """One meta-game through solve_alpharank; status 1 and 2 raise what the reference raises."""
    tables = [np.asarray(x, np.float64) for x in payoff_tensors]
    out = solve_alpharank(ctx, np.stack(tables)[None], single_population=len(tables) == 1, **kwargs)
    status = int(out["status"][0])
    if status == 1:
        raise ValueError("Expected 1 stationary distribution, but the chain is not irreducible in floating point "
                         "(a fixation probability underflowed to 0, or a payoff is not finite)")
    if status == 2:
        raise RuntimeError(f"AlphaRank stationary distribution not found after {int(out['iterations'][0]) + 1} iterations of "
                           "pi_vs_epsilon sweep")
    return out


def alpharank_compute(ctx, payoff_tensors, m=50, alpha=100, use_inf_alpha=False, inf_alpha_eps=0.01):
    """alpharank.compute on the device: pi over the profiles (their ids: the row-major index).  A list of one [K, K] table
    is the single-population chain with the local selection model.  rhos and rho_m are not returned."""
    if use_inf_alpha:
        return _alpharank_one(ctx, payoff_tensors, mode="infinite", eps=inf_alpha_eps)["pi"][0]
    return _alpharank_one(ctx, payoff_tensors, mode="finite", m=m, alpha=alpha)["pi"][0]


def sweep_pi_vs_epsilon(ctx, payoff_tensors, warm_start_epsilon=None, return_epsilon=False, min_iters=10, max_iters=100):
    """alpharank.sweep_pi_vs_epsilon on the device (its error-free path: the elimination does not fail where the
    reference's eigen-solve does, so no epsilon is ever raised again)."""
    out = _alpharank_one(ctx, payoff_tensors, mode="sweep", eps=warm_start_epsilon, min_iters=min_iters, max_iters=max_iters)
    return (out["pi"][0], float(out["eps"][0])) if return_epsilon else out["pi"][0]


def get_alpharank_marginals(payoff_tensors, pi):
    """psro_v2/utils.get_alpharank_marginals: per player the sum of pi over the other players' axes (on the host)."""
    if len(payoff_tensors) == 1:
        return np.asarray(pi, np.float64)
    shape = np.shape(payoff_tensors[0])
    joint = np.asarray(pi, np.float64).reshape(shape)
    return [joint.sum(axis=tuple(q for q in range(len(shape)) if q != p)) for p in range(len(shape))]


def alpharank_strategy(ctx, payoff_tensors, return_joint=False, **unused_kwargs):
    """psro_v2/utils.alpharank_strategy on payoff tensors: the swept distribution's marginals, one vector per player
    (computed on the device in the header's order of sums), and with return_joint the joint distribution [K_0 .. K_{P-1}]
    as well.  remove_epsilon_negative_probs has nothing to do here: the elimination never produces a negative mass."""
    tables = [np.asarray(x, np.float64) for x in payoff_tensors]
    out = _alpharank_one(ctx, tables, mode="sweep")
    if len(tables) == 1:
        marginals = [np.array(out["marginals"][0])]
    else:
        marginals = [np.array(x) for x in np.split(out["marginals"][0], np.cumsum(tables[0].shape)[:-1])]
    if return_joint:
        return marginals, (np.array(out["pi"][0]) if len(tables) == 1 else np.array(out["pi"][0]).reshape(tables[0].shape))
    return marginals
