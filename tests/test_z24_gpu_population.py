"""Payoff-tensor cells, policy aggregation and PSRO on the device (osg_cfr_profile_returns, osg_cfr_aggregate_policies in
include/osg_abi.h; TabularSolver.profile_returns / payoff_tensors / aggregate_policies; PSROSolver) against what the
reference's own expected_game_score.py and policy_aggregator.py left in tests/golden/population_vectors.npz
(tests/golden/make_population_vectors.py).

Bound for every output against the reference, and for the identities between two different device computations (the
splice and multilinearity tests): 1e-12 absolute (population_cases.TOLERANCE).  A profile's returns have one order of
summation whatever else a call holds (open_spiel_amd/csrc/osg_population.h), so the same profile computed twice by the
device is compared with array_equal.  Every test prints the worst deviation it saw before it asserts.

Measured on an MI355X: the aggregated cells equal the reference's bit for bit; the returns deviate
by at most 1.8e-15 from the reference, by at most 3.4e-14 from evaluate_policy of the spliced table and 3.3e-15 from the
weighted payoff tensor."""
import hashlib

import numpy as np
import pytest

import action_value_cases as avc
import population_cases as pc

pytestmark = pytest.mark.gpu

PIN = pc.TOLERANCE
INVALID, UNSUPPORTED = -1, -2
SENTINEL = -777.25


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


@pytest.fixture(scope="module")
def v():
    return pc.load()


@pytest.fixture(scope="module")
def solvers(ctx, v):
    """(solver, order, player) per game, made once: order[device row] = the goldens' row, player [I] in device order."""
    import open_spiel_amd as osa
    made = {}

    def get(game, **kwargs):
        key = (game, tuple(sorted(kwargs.items())))
        if key not in made:
            s = osa.TabularSolver(ctx, game, **kwargs)
            dev = s.tables()
            keys = sorted(dev["keys"])
            assert bytes(v[f"{game}/keys_sha256"]) == hashlib.sha256("\n".join(keys).encode()).digest()
            where = {k: i for i, k in enumerate(keys)}
            order = np.array([where[k] for k in dev["keys"]])
            assert np.array_equal(dev["nact"], v[f"{game}/nact"][order])
            player = s.infostate_players()
            assert np.array_equal(player, v[f"{game}/player"][order])
            made[key] = (s, order, player)
        return made[key]
    return get


def _stack(v, game, kinds, order):
    """The tables of `kinds` in the device's row order."""
    return np.ascontiguousarray(pc.table_stack(kinds, v[f"{game}/nact"], int(v[f"{game}/amax"]), int(v["seed"]))[:, order])


def _wide_kinds(game):
    """The stack of the identity tests: four tables, three on the large game (81 profiles)."""
    return pc.KINDS[:3] if game == pc.LARGE_GAME else pc.KINDS


def _numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _device(ctx, x):
    import torch
    return torch.as_tensor(x, device=ctx.device)


def _mixture_value(tensors, weights):
    """sum over the profiles of prod_p weights[p][k_p] * tensors[q][k_0 .. k_{P-1}], per player q."""
    out = []
    for t in tensors:
        for w in weights:
            t = np.tensordot(np.asarray(w), t, axes=(0, 0))
        out.append(float(t))
    return np.array(out)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("game", pc.GAMES)
def test_every_golden_case(ctx, solvers, v, game, device):
    s, order, _ = solvers(game)
    back = np.argsort(order)
    stack = _stack(v, game, pc.kinds_of(v, game), order)
    give = (lambda x: _device(ctx, x)) if device else (lambda x: x)
    got = _numpy(s.profile_returns(give(stack), give(v[f"{game}/profiles"]), device=device))
    assert s.last_eval_kernel() == "k_pop_returns"
    worst = {"returns": float(np.abs(got - v[f"{game}/returns"]).max())}
    bound = {"returns": PIN}
    for name in pc.weights_of(v, game):
        agg = _numpy(s.aggregate_policies(give(stack), give(v[f"{game}/weights/{name}"]), epsilon=float(v["epsilon"]), device=device))[back]
        assert s.last_eval_kernel() == "k_pop_aggregate"
        if game == pc.LARGE_GAME:
            worst[f"aggregate/{name}_rows"] = float(np.abs(agg[::pc.ROW_STRIDE] - v[f"{game}/aggregate/{name}_rows"]).max())
            worst[f"aggregate/{name}_colsum"] = float(np.abs(agg.sum(axis=0) - v[f"{game}/aggregate/{name}_colsum"]).max())
            bound[f"aggregate/{name}_colsum"] = pc.colsum_tolerance(len(agg))
        else:
            worst[f"aggregate/{name}"] = float(np.abs(agg - v[f"{game}/aggregate/{name}"]).max())
    print(f"population {game} device={device}: worst |device - reference| " + " ".join(f"{k} {d:.3g}" for k, d in worst.items()))
    for name, d in worst.items():
        assert d <= bound.get(name, PIN), (game, name, d)


def _batch_independence(s, stack, nact, profiles, sizes, shift):
    """The same profiles alone, together, reversed, tiled to every size of `sizes` and behind `shift` unrelated tables."""
    A = stack.shape[2]
    base = s.profile_returns(stack, profiles)
    assert not np.isnan(base).any()
    for m, profile in enumerate(profiles):
        assert np.array_equal(s.profile_returns(stack, profile[None, :])[0], base[m]), ("alone", m)
    assert np.array_equal(s.profile_returns(stack, profiles[::-1])[::-1], base), "reversed"
    for n in sizes:
        pick = (np.arange(n) * 7 + 3) % len(profiles)
        assert np.array_equal(s.profile_returns(stack, profiles[pick]), base[pick]), ("tiled", n)
    front = np.stack([avc.policy_table("random", nact, A, 4000 + k) for k in range(shift)])
    assert np.array_equal(s.profile_returns(np.concatenate([front, stack]), profiles + shift), base), "shifted"
    return base


@pytest.mark.parametrize("game", ["kuhn_poker", "leduc_poker"])
def test_a_profiles_bits_do_not_depend_on_the_batch(ctx, solvers, v, game):
    s, order, _ = solvers(game)
    stack = _stack(v, game, pc.KINDS, order)
    profiles = pc.all_profiles(2, 4)
    # (1025 and 2049 besides: on 256 compute units the launch takes tiles of 1, 2, 4 and 8 profiles at 257, 1025, 2049, 4097)
    base = _batch_independence(s, stack, v[f"{game}/nact"][order], profiles, (1, 2, 63, 64, 65, 257, 1025, 2049, 4097), 13)
    # the device path and a solver made for another kernel family give the same bits as well
    assert np.array_equal(_numpy(s.profile_returns(_device(ctx, stack), _device(ctx, profiles), device=True)), base)
    other, order2, _ = solvers(game, general_kernel="grid")
    assert np.array_equal(order, order2) and np.array_equal(other.profile_returns(stack, profiles), base)
    w = pc.weight_matrix("seeded", 2, 4)
    agg = s.aggregate_policies(stack, w)
    assert np.array_equal(agg, other.aggregate_policies(stack, w))
    assert np.array_equal(agg, _numpy(s.aggregate_policies(_device(ctx, stack), _device(ctx, w), device=True)))


def test_a_profiles_bits_do_not_depend_on_the_batch_on_the_large_tree(solvers, v):
    s, order, _ = solvers(pc.LARGE_GAME)
    stack = _stack(v, pc.LARGE_GAME, pc.KINDS[:3], order)
    profiles = pc.all_profiles(3, 3)
    together = s.profile_returns(stack, profiles)                                     # 27
    pick = (np.arange(65) * 7 + 3) % 27
    assert np.array_equal(s.profile_returns(stack, profiles[pick]), together[pick])   # 65
    for m in (0, 5, 26):
        assert np.array_equal(s.profile_returns(stack, profiles[m:m + 1])[0], together[m])   # 1


@pytest.mark.parametrize("game", pc.GAMES)
def test_splice_identity_on_every_profile(solvers, v, game):
    """The profile's returns are the expected returns of the table spliced from the profile's tables, row by player."""
    s, order, player = solvers(game)
    P = int(v[f"{game}/num_players"])
    stack = _stack(v, game, _wide_kinds(game), order)
    profiles = pc.all_profiles(P, len(stack))
    got = s.profile_returns(stack, profiles)
    worst = 0.0
    for m, profile in enumerate(profiles):
        want = s.evaluate_policy("table", pc.splice(stack, profile, player))["expected_returns"]
        worst = max(worst, float(np.abs(got[m] - want).max()))
    print(f"splice identity {game}: {len(profiles)} profiles, worst |profile_returns - evaluate_policy| {worst:.3g}")
    assert worst <= PIN


@pytest.mark.parametrize("game", pc.GAMES)
def test_the_aggregate_is_worth_the_weighted_payoff_tensor(solvers, v, game):
    s, order, _ = solvers(game)
    P = int(v[f"{game}/num_players"])
    stack = _stack(v, game, _wide_kinds(game), order)
    tensors = s.payoff_tensors(stack)
    assert len(tensors) == P and all(t.shape == (len(stack),) * P for t in tensors)
    for name in ("uniform", "seeded"):
        w = pc.weight_matrix(name, P, len(stack))
        want = _mixture_value(tensors, w)
        got = s.evaluate_policy("table", s.aggregate_policies(stack, w))["expected_returns"]
        d = float(np.abs(got - want).max())
        print(f"multilinearity {game} {name}: worst |evaluate_policy(aggregate) - weighted tensor| {d:.3g}")
        assert d <= PIN, (game, name)


def test_payoff_tensors_follow_the_populations(solvers, v):
    s, order, _ = solvers("kuhn_poker(players=3)")
    stack = _stack(v, "kuhn_poker(players=3)", pc.KINDS, order)
    full = s.payoff_tensors(stack)
    pops = [[3, 1], [0], [2, 0, 1]]
    part = s.payoff_tensors(stack, pops)
    for q in range(3):
        assert part[q].shape == (2, 1, 3)
        assert np.array_equal(part[q], full[q][np.ix_(*pops)])


def test_refused_calls_write_nothing(ctx, solvers, v):
    import torch
    from open_spiel_amd import lib
    s, order, _ = solvers("kuhn_poker")
    stack = _stack(v, "kuhn_poker", pc.KINDS, order)
    profiles = pc.all_profiles(2, 4)
    weights = pc.weight_matrix("seeded", 2, 4)
    ret = np.full((16, 2), SENTINEL)
    agg = np.full(stack.shape[1:], SENTINEL)
    p = lambda a: a.ctypes.data

    def returns(tables=stack, n_tables=4, prof=profiles, n=16, out=ret):
        return lib().osg_cfr_profile_returns(s._h, None if tables is None else p(tables), n_tables, None if prof is None else p(prof), n, 1,
                                             None if out is None else p(out))

    def aggregate(tables=stack, n_tables=4, w=weights, eps=1e-40, out=agg):
        return lib().osg_cfr_aggregate_policies(s._h, None if tables is None else p(tables), n_tables, None if w is None else p(w), eps, 1,
                                                None if out is None else p(out))

    def bad(profile):
        b = profiles.copy()
        b[11] = profile
        return b

    def badw(x):
        w = weights.copy()
        w[1, 2] = x
        return w

    refused = [(returns(tables=None), INVALID), (returns(prof=None), INVALID), (returns(out=None), INVALID),
               (returns(n_tables=0), INVALID), (returns(prof=bad((4, 0))), INVALID), (returns(prof=bad((0, -1))), INVALID),
               (returns(n=(1 << 22) + 1), UNSUPPORTED), (returns(n_tables=1 << 30), UNSUPPORTED),
               (aggregate(tables=None), INVALID), (aggregate(w=None), INVALID), (aggregate(out=None), INVALID),
               (aggregate(n_tables=0), INVALID), (aggregate(w=badw(-1e-300)), INVALID), (aggregate(w=badw(np.nan)), INVALID),
               (aggregate(w=badw(np.inf)), INVALID), (aggregate(eps=-1e-300), INVALID), (aggregate(eps=np.nan), INVALID),
               (aggregate(n_tables=1 << 30), UNSUPPORTED)]
    assert [rc for rc, _ in refused] == [want for _, want in refused]
    assert (ret == SENTINEL).all() and (agg == SENTINEL).all()
    assert returns(n=(1 << 22) + 1) == UNSUPPORTED and b"limit" in lib().osg_last_error()
    assert returns(n_tables=1 << 30) == UNSUPPORTED and b"limit" in lib().osg_last_error()
    # with device memory the indices and the weights are checked on the device: nothing is written, the next call says so
    import open_spiel_amd as osa
    d_stack, d_ret = _device(ctx, stack), torch.full((16, 2), SENTINEL, dtype=torch.float64, device=ctx.device)
    d_agg = torch.full(stack.shape[1:], SENTINEL, dtype=torch.float64, device=ctx.device)
    d_bad, d_badw = _device(ctx, bad((0, 4))), _device(ctx, badw(-0.5))
    assert lib().osg_cfr_profile_returns(s._h, d_stack.data_ptr(), 4, d_bad.data_ptr(), 16, 0, d_ret.data_ptr()) == 0
    ctx.synchronize()
    assert (d_ret.cpu().numpy() == SENTINEL).all()
    with pytest.raises(osa.OsgError, match="profile index"):
        s.profile_returns(stack, profiles)
    assert lib().osg_cfr_aggregate_policies(s._h, d_stack.data_ptr(), 4, d_badw.data_ptr(), 1e-40, 0, d_agg.data_ptr()) == 0
    ctx.synchronize()
    assert (d_agg.cpu().numpy() == SENTINEL).all()
    with pytest.raises(osa.OsgError, match="weight"):
        s.aggregate_policies(stack, weights)
    # and the solver goes on
    assert returns() == 0 and aggregate() == 0
    assert np.abs(ret[[0, 5, 10]] - v["kuhn_poker/returns"][[0, 5, 10]]).max() <= PIN and np.abs(agg.sum(axis=1) - 1).max() <= PIN


def _last_policy_alone(tensors):
    out = [np.zeros(k) for k in tensors[0].shape]
    for w in out:
        w[-1] = 1.0
    return out


@pytest.mark.parametrize("game,iters", [("kuhn_poker", 10), ("kuhn_poker(players=3)", 5), ("leduc_poker", 5)])
def test_psro_keeps_its_tensors_and_its_best_responses_agree_with_them(ctx, game, iters):
    import open_spiel_amd as osa
    solver = osa.PSROSolver(ctx, game)
    P = solver.num_players
    assert [t.shape for t in solver.meta_games()] == [(1,) * P] * P
    worst_br, worst_nc, curve = 0.0, 0.0, []
    for it in range(iters):
        solver.iteration()
        n = it + 2
        games = solver.meta_games()
        stack, pops = solver.table_stack()
        assert stack.shape[0] == n and pops == [list(range(n))] * P
        fresh = solver.solver.payoff_tensors(stack, pops, device=True)
        for q in range(P):
            assert games[q].shape == (n,) * P and np.array_equal(games[q], fresh[q].cpu().numpy()), (game, it, q)
        w = solver.last_meta_strategies()
        assert [len(x) for x in w] == [n - 1] * P
        old = tuple(slice(0, n - 1) for _ in range(P))
        mixture = _mixture_value([t[old] for t in games], w)
        gains = []
        for p in range(P):   # the new policy of player p against the others' mixture, read off the new cells
            index = tuple(slice(n - 1, n) if q == p else slice(0, n - 1) for q in range(P))
            value = _mixture_value([games[p][index]], [np.ones(1) if q == p else w[q] for q in range(P)])[0]
            worst_br = max(worst_br, abs(value - solver.last_best_response_values()[p]))
            gains.append(value - mixture[p])
        nc = solver.nash_conv(w)
        worst_nc = max(worst_nc, abs(nc - sum(gains)))
        curve.append(nc)
    print(f"psro {game}: worst |best response - new cells| {worst_br:.3g}, |nash_conv - sum of gains| {worst_nc:.3g}; "
          "NashConv " + " ".join(f"{x:.4f}" for x in curve))
    assert worst_br <= PIN
    assert worst_nc <= 2 * P * PIN   # a sum of 2 P quantities, each within the bound
    assert curve[-1] < curve[0]


def test_psro_takes_a_callable_meta_solver(ctx):
    import open_spiel_amd as osa
    uniform, last = osa.PSROSolver(ctx, "kuhn_poker"), osa.PSROSolver(ctx, "kuhn_poker", meta_solver=_last_policy_alone)
    for _ in range(4):
        uniform.iteration()
        last.iteration()
    assert [np.array_equal(x, [0, 0, 0, 1]) for x in last.last_meta_strategies()] == [True, True]
    assert not all(np.array_equal(a, b) for a, b in zip(uniform.meta_games(), last.meta_games()))
    assert not np.array_equal(uniform.policies()[0], last.policies()[0])
    with pytest.raises(osa.OsgError):
        osa.PSROSolver(ctx, "kuhn_poker", meta_solver="nash")
