"""PSRO's meta-strategy solvers on the device: psro_v2's "prd" (open_spiel/python/algorithms/
projected_replicator_dynamics.py) and "rm" (regret_matching.py), with the reference's keyword names and defaults.  A solve
is one launch of osg_meta_solve — every iteration, a workgroup per meta-game — and solve_meta_games takes a batch: many
meta-games of one shape, or a sweep of dt / gamma / iterations over copies of one.  csrc/osg_meta_solver.h fixes the order
of every sum; the reference's go through BLAS, so it is matched within rounding (1e-12 on the recorded cases), not bit for
bit.  Regret matching amplifies rounding once a regret changes sign: beyond a few hundred iterations two correct
implementations drift apart."""
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
