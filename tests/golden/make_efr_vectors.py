#!/usr/bin/env python3
"""Golden runs of extensive-form regret minimization, produced by RUNNING the reference's own
open_spiel/python/algorithms/efr.py (imported unmodified from where it lies) over the genuine games
(oracle/_ref/libspiel_ref.so through oracle/pyspiel_over_capi.py).  Run in the build container (needs the reference
sources; CPU only, about two minutes):

    python tests/golden/make_efr_vectors.py

Output: tests/golden/efr_vectors.npz (np.savez_compressed).  `runs` lists the run names "<game>|<deviation set>"; the
arrays of run number r carry the prefix "r<r>/":

  keys_bytes / keys_len     the information-state strings in the reference's node order (first DFS visit)
  player [I] int8, nact [I] int32, legal [I, 3] int32 (-1 padded)
  own_len [I] int32         earlier own decisions on the way to the infostate
  own_info [I, L] int32     their infostates (indices into keys), own_action [I, L] int32 the actions played there,
  own_legal [I, L, 3] int32 the legal actions there (-1 padded)
  dev_count [I] int32       deviations per infostate; the deviations of all infostates follow one another:
  dev_target, dev_source (-1: external), dev_external [D] int8
  dev_weights [D, L] int8   the 0/1 memory weights (-1 padding; all -1 with dev_weights_none: the reference's `None`)
  dev_memory [D, L] int8    the remembered actions (-1 padding)
  checkpoints [C] int32     iterations after which the state was recorded:
  R [C, D]                  cumulative regret per deviation (0 where the reference has no entry yet)
  cur, cum, avg [C, I, 3]   current, cumulative and average policy by ACTION ID (0 at an illegal id)
  unvisited [T] int32       per iteration, the infostates whose members the regret pass all skipped (their y values are
                            carried into the policy pass instead of being reset)
  min_abs_R, min_z, min_sv_ratio   the smallest nonzero |R| at the checkpoints, and the smallest positive z and kept sigma / sigma_max
                            over ALL iterations

"tree/<game>/parent, kind (0 chance, 1 decision, 2 terminal), action, prob, info, returns [H(, P)]": the game tree depth
first (a parent before its children, children in action order), `info` an index into the keys, `prob` the chance
probability of the edge from the parent.

"cfr/<game>/avg|cur|cum [I, 3]": the reference cfr.py's _CFRSolver(alternating_updates=False, linear_averaging=False,
regret_matching_plus=False) after the `blind cf` run's last checkpoint, same row order.

Regret-matching unit cases ("rm/"): A [n], external_only [n], nkeys [n], key_target / key_source [n, 9] (-1 padding;
source -1: external), y [n, 9], out [n, 3], rank [n] (-1: no solve), sv [n, 3] (NaN padding).

A checkpoint is kept only if the reference's own run reaches the same tables (within 1e-12) whichever LAPACK driver
solves its least-squares systems (gelsd, scipy's default; gelsy; gelss).  A solution component that is 0 in exact
arithmetic is rounding noise of either sign, the clip makes it exactly 0 or leaves 1e-17, and the walk's `reach == 0` test
(and with it whether an infostate's y is reset or carried) can then go either way.  A run ends before its first
checkpoint that does not pass (the generator prints which).

Asserted here: every singular value of every solve is >= 1e-6 sigma_max or dropped by scipy's rule (<= eps sigma_max);
the smallest nonzero |R| at every checkpoint and the smallest positive z anywhere are >= 1e-9 — so no max(0, .), no z > 0 and no rank decision can
turn on a rounding difference.

Consumers: tests/efr_cases.py and through it test_efr_goldens.py, test_efr_native.py (CPU), test_z27_gpu_efr.py.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = os.environ.get("OSG_REFERENCE_ROOT", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden", "efr_vectors.npz")

ALL_SETS = ["blind action", "informed action", "blind cf", "informed cf", "bps", "cfps", "csps", "tips", "bhv"]
RUNS = ([("kuhn_poker", d, [1, 2, 3, 5, 10, 20]) for d in ALL_SETS]
        + [("kuhn_poker(players=3)", d, [1, 2, 5, 10]) for d in ("blind cf", "csps", "tips", "bhv")]
        + [("leduc_poker", d, [1, 2, 4]) for d in ("blind cf", "informed cf", "cfps", "csps", "tips", "bhv")])
MIN_R = 1e-9
MIN_Z = 1e-9
MIN_SV = 1e-6
NOISE = 1e-12
EPS = np.finfo(np.float64).eps


def reference_modules():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import reference_py
    if not reference_py.sources_present():
        raise RuntimeError("needs the reference sources")
    reference_py.build()
    import pyspiel_over_capi
    pyspiel = pyspiel_over_capi.install(reference_py)
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    from open_spiel.python.algorithms import cfr, efr
    return pyspiel, efr, cfr


class SolveLog:
    """Stands in for scipy.linalg inside efr.py: lstsq is scipy's own, its rank and singular values are kept."""

    def __init__(self, linalg):
        self._linalg = linalg
        self.last = None
        self.min_ratio = np.inf
        self.driver = None   # another LAPACK driver for the replays that test a run's robustness

    def lstsq(self, a, b):
        if self.driver is not None:
            return self._linalg.lstsq(a, b, lapack_driver=self.driver)
        x, res, rank, sv = self._linalg.lstsq(a, b)
        kept = sv[sv > EPS * sv[0]]
        assert len(kept) == rank
        for s in sv:
            assert s >= MIN_SV * sv[0] or s <= EPS * sv[0], f"a singular value near the rank rule: {sv}"
        self.min_ratio = min(self.min_ratio, kept[-1] / sv[0])
        self.last = (rank, sv.copy())
        return x, res, rank, sv


def run(efr, game, name, checkpoints, log):
    min_z = [np.inf]

    class Probe(efr.EFRSolver):
        def _regret_matching(self, node):
            z = sum(node.y_values.values())
            if z > 0:
                min_z[0] = min(min_z[0], z)
            return super()._regret_matching(node)

    solver = Probe(game, name)
    nodes = solver._info_state_nodes
    keys = list(nodes)
    index_to_key = {n.index_in_tabular_policy: i for i, n in enumerate(nodes.values())}
    I = len(keys)
    L = max(1, max(len(n.history) for n in nodes.values()))
    player = np.zeros(I, np.int8)
    legal = np.full((I, 3), -1, np.int32)
    nact = np.zeros(I, np.int32)
    own_len = np.zeros(I, np.int32)
    own_info = np.full((I, L), -1, np.int32)
    own_action = np.full((I, L), -1, np.int32)
    own_legal = np.full((I, L, 3), -1, np.int32)
    dev_count = np.zeros(I, np.int32)
    dev = []
    key_player = {}

    key_index = {k: i for i, k in enumerate(keys)}
    tree = []   # depth-first: (parent, kind 0 chance / 1 decision / 2 terminal, edge action, edge chance probability, infostate, returns)

    def walk(state, parent, action, prob):
        me = len(tree)
        if state.is_terminal():
            tree.append((parent, 2, action, prob, -1, list(state.returns())))
            return
        if state.is_chance_node():
            tree.append((parent, 0, action, prob, -1, [0.0] * game.num_players()))
            for o, p in state.chance_outcomes():
                walk(state.child(o), me, o, p)
            return
        k = state.information_state_string(state.current_player())
        key_player.setdefault(k, state.current_player())
        tree.append((parent, 1, action, prob, key_index[k], [0.0] * game.num_players()))
        for a in state.legal_actions():
            walk(state.child(a), me, a, 0.0)

    walk(game.new_initial_state(), -1, -1, 0.0)
    for i, (k, n) in enumerate(nodes.items()):
        player[i] = key_player[k]
        nact[i] = len(n.legal_actions)
        legal[i, :nact[i]] = n.legal_actions
        own_len[i] = len(n.history)
        assert len(n.history) == len(n.current_history_probs)
        for j, (la, idx) in enumerate(n.current_history_probs):
            own_info[i, j] = index_to_key[idx]
            own_action[i, j] = n.history[j]
            own_legal[i, j, :len(la)] = la
        dev_count[i] = len(n.relizable_deviations)
        for d in n.relizable_deviations:
            t = d.local_swap_transform
            w = np.full(L, -1, np.int8)
            m = np.full(L, -1, np.int8)
            none = d.prior_actions_weight is None
            if not none:
                assert len(d.prior_actions_weight) == len(n.history)
                for j, x in enumerate(d.prior_actions_weight):
                    assert x in (0, 1)
                    w[j] = int(x)
            for j, x in enumerate(d.prior_memory_actions):
                assert x == int(x)
                m[j] = int(x)
            assert d.use_unmodified_history
            dev.append((t.target_action, -1 if t.source_action is None else t.source_action, int(t.source_action is None), none, w, m))
    D = len(dev)
    off = np.concatenate([[0], np.cumsum(dev_count)])
    R, cur, cum, avg, unvisited = [], [], [], [], []
    min_r = np.inf

    def regrets(nodes=nodes):
        r = np.zeros(D)
        for i, n in enumerate(nodes.values()):
            for d, v in n.cumulative_regret.items():
                r[off[i] + d] = float(np.asarray(v).reshape(-1)[0])
        return r

    def cumulative(nodes=nodes):
        c = np.zeros((I, 3))
        for i, n in enumerate(nodes.values()):
            for a, v in n.cumulative_policy.items():
                c[i, a] = v
        return c

    def table(tab):
        out = np.zeros((I, 3))
        for i, n in enumerate(nodes.values()):
            row = tab.action_probability_array[n.index_in_tabular_policy]
            out[i, :len(row)] = row
        return out

    # A checkpoint whose smallest nonzero |R| is below MIN_R moves to the next iteration where it is not.
    pending, taken, it = sorted(checkpoints), [], 0
    while pending:
        it += 1
        assert it <= max(checkpoints) + 30, f"{name}: no admissible iteration for checkpoint {pending[0]}"
        # the regret pass and the policy pass of evaluate_and_update_policy, with a look between them
        solver._compute_cumulative_immediate_regret_for_player(
            solver._root_node, policies=None, reach_probabilities=np.ones(game.num_players() + 1), player=None)
        unvisited.append(sum(1 for n in nodes.values() if len(n.y_values) > 0))
        solver._update_current_policy(solver._root_node, solver._current_policy)
        solver._iteration += 1
        if it < pending[0]:
            continue
        r = regrets()
        smallest = np.min(np.abs(r[r != 0])) if np.any(r != 0) else np.inf
        if smallest < MIN_R:
            continue
        min_r = min(min_r, smallest)
        pending.pop(0)
        pending = [max(c, it + 1) for c in pending]
        taken.append(it)
        R.append(r)
        cur.append(table(solver.current_policy()))
        cum.append(cumulative())
        avg.append(table(solver.average_policy()).copy())
    # The reference clips the least-squares solution at 0 and its walk tests reaches with == 0.  A component that is 0 in
    # exact arithmetic leaves LAPACK as rounding noise of either sign: clipped to exactly 0 or kept as 1e-17, and that can
    # decide whether a subtree is entered (and an infostate's y reset or carried).  A checkpoint is kept only if the
    # reference's own run arrives at the same tables whichever LAPACK driver solves (gelsd, its default; gelsy; gelss);
    # the run ends before the first that does not.
    kept = len(taken)
    for driver in ("gelsy", "gelss"):
        log.driver = driver
        other = efr.EFRSolver(game, name)
        done = 0
        for c, upto in enumerate(taken[:kept]):
            for _ in range(upto - done):
                other.evaluate_and_update_policy()
            done = upto
            diff = max(np.max(np.abs(regrets(other._info_state_nodes) - R[c])), np.max(np.abs(table(other.current_policy()) - cur[c])),
                       np.max(np.abs(cumulative(other._info_state_nodes) - cum[c])))
            if diff > NOISE:
                kept = c
                break
        log.driver = None
    assert kept >= 1, f"{name}: no checkpoint survives the rounding noise of the solves"
    if kept < len(taken):
        print(f"   {name}: checkpoints {taken[kept:]} depend on the LAPACK driver (rounding noise in a clipped solution) and are left out")
    checkpoints, R, cur, cum, avg = taken[:kept], R[:kept], cur[:kept], cum[:kept], avg[:kept]
    assert min_r >= MIN_R, f"{name}: a regret of {min_r}"
    assert min_z[0] >= MIN_Z, f"{name}: a z of {min_z[0]}"
    kb = [k.encode() for k in keys]
    return dict(
        keys_bytes=np.frombuffer(b"".join(kb), np.uint8), keys_len=np.array([len(k) for k in kb], np.int32), player=player,
        nact=nact, legal=legal, own_len=own_len, own_info=own_info, own_action=own_action, own_legal=own_legal,
        dev_count=dev_count, dev_target=np.array([d[0] for d in dev], np.int8), dev_source=np.array([d[1] for d in dev], np.int8),
        dev_external=np.array([d[2] for d in dev], np.int8), dev_weights_none=np.array([d[3] for d in dev], np.int8),
        dev_weights=np.array([d[4] for d in dev], np.int8), dev_memory=np.array([d[5] for d in dev], np.int8),
        checkpoints=np.array(checkpoints, np.int32), R=np.array(R), cur=np.array(cur), cum=np.array(cum), avg=np.array(avg),
        unvisited=np.array(unvisited, np.int32), min_abs_R=np.float64(min_r), min_z=np.float64(np.asarray(min_z[0]).reshape(-1)[0]),
        min_sv_ratio=np.float64(log.min_ratio)), keys, nodes, dict(
            parent=np.array([t[0] for t in tree], np.int32), kind=np.array([t[1] for t in tree], np.int8),
            action=np.array([t[2] for t in tree], np.int32), prob=np.array([t[3] for t in tree], np.float64),
            info=np.array([t[4] for t in tree], np.int32), returns=np.array([t[5] for t in tree], np.float64))


def cfr_equivalent(cfr, game, iters, keys, nodes):
    solver = cfr._CFRSolver(game, alternating_updates=False, linear_averaging=False, regret_matching_plus=False)
    for _ in range(iters):
        solver.evaluate_and_update_policy()
    out = {}
    avg = solver.average_policy()
    for name, tab in (("avg", avg), ("cur", solver.current_policy())):
        t = np.zeros((len(keys), 3))
        for i, k in enumerate(keys):
            row = tab.action_probability_array[tab.state_lookup[k]]
            t[i, :len(row)] = row
        out[name] = t
    c = np.zeros((len(keys), 3))
    for i, k in enumerate(keys):
        for a, v in solver._info_state_nodes[k].cumulative_policy.items():
            c[i, a] = v
    out["cum"] = c
    return out


def unit_cases(efr, log):
    rng = np.random.RandomState(2102)
    rows = []

    class Node:
        pass

    class Self:
        pass

    for A in (2, 3):
        ext = efr.return_all_external_deviations(A, [None], [])
        inn = efr.return_all_non_identity_internal_deviations(A, [None], [])
        for external_only, pool in ((True, ext), (False, inn), (False, inn + ext), (False, ext + inn)):
            for _ in range(48):
                mode = rng.randint(4)
                devs = [pool[j] for j in rng.permutation(len(pool))] if mode == 3 else list(pool)
                y = rng.uniform(0.0, 1.0, len(devs)) * 10.0 ** rng.randint(-3, 3)
                if mode == 0:
                    y[rng.uniform(size=len(devs)) < 0.6] = 0.0
                elif mode == 1:   # a single positive weight
                    keep = rng.randint(len(devs))
                    y[np.arange(len(devs)) != keep] = 0.0
                if external_only:
                    devs = list(pool)   # (the shortcut reads every target's row)
                node = Node()
                node.legal_actions = list(range(A))
                node.y_values = {d: float(v) for d, v in zip(devs, y)}
                me = Self()
                me._external_only = external_only
                log.last = None
                pol = efr.EFRSolver._regret_matching(me, node)
                out = np.zeros(3)
                out[:A] = [pol[a] for a in range(A)]
                sv = np.full(3, np.nan)
                rank = -1
                if log.last is not None:
                    rank = log.last[0]
                    sv[:A] = log.last[1]
                kt = np.full(9, -1, np.int32)
                ks = np.full(9, -1, np.int32)
                yy = np.zeros(9)
                for j, d in enumerate(devs):
                    t = d.local_swap_transform
                    kt[j] = t.target_action
                    ks[j] = -1 if t.source_action is None else t.source_action
                    yy[j] = y[j]
                rows.append((A, int(external_only), len(devs), kt, ks, yy, out, rank, sv))
    deficient = sum(1 for r in rows if 0 <= r[7] < r[0])
    assert deficient >= 20, deficient
    return dict(A=np.array([r[0] for r in rows], np.int32), external_only=np.array([r[1] for r in rows], np.int8),
                nkeys=np.array([r[2] for r in rows], np.int32), key_target=np.array([r[3] for r in rows]),
                key_source=np.array([r[4] for r in rows]), y=np.array([r[5] for r in rows]), out=np.array([r[6] for r in rows]),
                rank=np.array([r[7] for r in rows], np.int32), sv=np.array([r[8] for r in rows])), deficient


def main(runs=None, path=None):
    """runs, path: another list in the form of RUNS and its file (tests/golden/make_solver_variant_vectors.py), without
    the regret-matching unit cases, which do not depend on the game."""
    variant = runs is not None
    runs, path = (RUNS if runs is None else runs), (path or GOLDEN)
    pyspiel, efr, cfr = reference_modules()
    log = SolveLog(efr.linalg)
    efr.linalg = log
    out = {"runs": np.array([f"{g}|{d}" for g, d, _ in runs])}
    t_all = time.time()
    for r, (game_string, name, checkpoints) in enumerate(runs):
        t0 = time.time()
        log.min_ratio = np.inf
        game = pyspiel.load_game(game_string)
        rec, keys, nodes, tree = run(efr, game, name, checkpoints, log)
        for k, v in tree.items():   # (the same for every run of a game)
            out[f"tree/{game_string}/{k}"] = v
        for k, v in rec.items():
            out[f"r{r}/{k}"] = v
        print(f"{game_string} | {name}: {len(rec['dev_target'])} deviations, at most {rec['dev_count'].max()} per infostate, "
              f"smallest |R| {rec['min_abs_R']:.3g}, z {rec['min_z']:.3g}, sigma ratio {rec['min_sv_ratio']:.3g}, "
              f"checkpoints {rec['checkpoints'].tolist()}, unvisited infostates per iteration {rec['unvisited'].tolist()}, {time.time() - t0:.1f} s", flush=True)
        if name == "blind cf":
            eq = cfr_equivalent(cfr, game, int(rec['checkpoints'][-1]), keys, nodes)
            for k, v in eq.items():
                out[f"cfr/{game_string}/{k}"] = v
            print(f"   against cfr.py: average policy differs by at most {np.max(np.abs(eq['avg'] - rec['avg'][-1])):.3g}", flush=True)
    if not variant:
        rm, deficient = unit_cases(efr, log)
        for k, v in rm.items():
            out[f"rm/{k}"] = v
        print(f"{len(rm['A'])} regret-matching cases, {deficient} rank-deficient")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", f"{time.time() - t_all:.0f} s of reference time")


if __name__ == "__main__":
    main()
