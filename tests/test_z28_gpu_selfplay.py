"""AlphaZero self-play on the device (osg_selfplay_*, osg_replay_*, osg_mcts_root_noise in include/osg_abi.h;
open_spiel_amd.alpha_zero) against the host program that runs the same header on the CPU
(tests/native/selfplay_host_test.cpp), the NumPy restatement of the reference's lines (tests/selfplay_cases.py), exact
distributions and the oracle's replay of every game.

Device against host noise (device log / cos / pow against libm): NOISE_REL_BOUND below is ten times the largest
relative difference measured on an MI355X; rows in which a Marsaglia-Tsang accept / reject flipped on a last-bit
difference differ grossly, are counted, and at most one row in 2^12 may be excluded
(tests/test_selfplay_host.py shows that cap holds for the host program with its logarithm moved by one ulp)."""
import numpy as np
import pytest

import sampling_stats as st
import selfplay_cases as sc

N_NOISE, NOISE_SEED, NOISE_SHAPES = sc.N_NOISE, sc.NOISE_SEED, sc.NOISE_SHAPES

pytestmark = pytest.mark.gpu

# measured on an MI355X over 2^16 rows of Dirichlet(0.3) on 9 actions: 0 gross rows, largest relative difference of a
# coordinate (against the row's largest) 7.8e-16; the bound is one order of magnitude above
NOISE_REL_BOUND = 7.8e-15
GROSS = 1e-6

GAMES = {7: "connect_four", 9: "tic_tac_toe", 81: "hex(board_size=9)", 361: "hex(board_size=19)"}


@pytest.fixture(scope="module")
def osa():
    import open_spiel_amd
    return open_spiel_amd


@pytest.fixture(scope="module")
def ctx(osa):
    return osa.Context(0)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("selfplay_gpu_io"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sc.build_host_test(str(tmp_path_factory.mktemp("selfplay_gpu") / "selfplay_host_test"))


def _bits32(t):
    return t.cpu().numpy().view(np.uint32)


def _selfplay(osa, ctx, game, n, capacity=64, **kw):
    envs = osa.StateBatch(ctx, game, n)
    buf = osa.ReplayBuffer(ctx, game, capacity)
    kw.setdefault("max_simulations", 2)
    kw.setdefault("uct_c", 1.4)
    return osa.SelfPlay(envs, buf, None, **kw), envs, buf


# ---- select -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", sc.ACTIONS)
@pytest.mark.parametrize("n", [sc.ROWS, 1])
def test_select_is_the_host_programs_bit_for_bit(osa, ctx, exe, workdir, A, n):
    import torch
    game = GAMES[A]
    for temperature in sc.TEMPERATURES:
        for drop in (sc.TEMPERATURE_DROP, 0):   # every row drawn / every row greedy at the first ply of a game
            case = sc.select_case(A, temperature, sc.ROWS)
            rows = slice(0, n) if n > 1 else slice(3, 4)
            case.update(rows=n, visits=case["visits"][rows], best=case["best"][rows], drop=drop,
                        move=np.zeros(n, np.int32), plyc=np.zeros(n, np.int64))
            (p64, p32, action, ok), = sc.host_select(exe, [case], workdir)
            sp, envs, buf = _selfplay(osa, ctx, game, n, temperature=temperature, temperature_drop=drop, seed=case["seed"],
                                      index_offset=case["offset"])
            # environments at different plies of their games: none, one or two moves played (the staging area starts out
            # as initial states, so only a copied record can match)
            idx = np.arange(n) if n > 1 else np.array([3])
            first = np.where(idx % 2 == 1, idx % min(A, 7), -1).astype(np.int32)
            second = np.where(idx % 4 == 3, (idx + 1) % min(A, 7), -1).astype(np.int32)
            envs.apply_actions(first)
            envs.apply_actions(second)
            initial = osa.StateBatch(ctx, game, n).raw_words()
            root_value = np.linspace(-1.0, 1.0, n) if n > 1 else np.array([0.3])
            policy, act = sp.select(torch.from_numpy(case["visits"]), torch.from_numpy(case["best"]), torch.from_numpy(root_value))
            staged = sp.staged(0)
            live = ok.astype(bool)
            if live.all():
                ctx.synchronize()
            else:
                with pytest.raises(osa.OsgError, match="illegal"):   # the zero-visit row is reported ...
                    ctx.synchronize()
            assert (_bits32(policy) == p32.view(np.uint32)).all(), (A, temperature, drop)
            assert (act.cpu().numpy() == action).all(), (A, temperature, drop)
            assert (act.cpu().numpy()[~live] == -1).all()
            if drop == 0:
                assert (action[live] == case["best"][live]).all()
            # ... and not recorded; every other row is staged as ply 0 of its game
            assert (_bits32(staged["policy"])[live] == p32.view(np.uint32)[live]).all()
            assert (staged["action"].cpu().numpy()[live] == action[live]).all()
            assert (staged["root_value"].cpu().numpy()[live] == root_value.astype(np.float32)[live]).all()
            plies_played = (first >= 0).astype(int) + (second >= 0).astype(int)
            assert (staged["player"].cpu().numpy()[live] == (plies_played % 2)[live]).all()
            assert (staged["states"].raw_words() == envs.raw_words())[:, live].all()
            assert (staged["states"].raw_words() == initial)[:, ~live].all()
            moved_on = plies_played > 0
            assert (envs.raw_words() != initial).any(0)[moved_on].all() and moved_on[live].any()
            assert (staged["length"].cpu().numpy() == 0).all() and (staged["ply_counter"].cpu().numpy() == 0).all()
            assert len(buf) == 0
            sp.close()


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_drawn_actions_follow_the_devices_own_policy(osa, ctx, temperature):
    import torch
    n = 1 << 16
    sp, envs, buf = _selfplay(osa, ctx, "tic_tac_toe", n, temperature=temperature, temperature_drop=4, seed=0xF4E9, index_offset=77)
    visits = np.tile(np.array([10, 12, 14, 16, 18, 20, 22, 24, 26], np.int32), (n, 1))
    policy, act = sp.select(torch.from_numpy(visits), torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.float64))
    ctx.synchronize()
    p = policy[0].cpu().numpy().astype(np.float64)
    assert (_bits32(policy) == _bits32(policy[:1])).all()
    want = sc.policy_target(visits[:1], temperature)[0]
    assert np.abs(p - want).max() < 1e-7
    z, x2, d = st.chi_square(st.counts_of(act.cpu().numpy(), 9), p / p.sum())
    print(f"T = {temperature}: chi-square z = {z:.3f} (X^2 = {x2:.2f}, d = {d})")
    assert st.accept(z)


# ---- root noise ---------------------------------------------------------------------------------------------------------
def _device_noise(osa, ctx, prior, mask, alpha, epsilon, seed, index_offset, sub, request=None):
    import torch
    p = torch.from_numpy(np.ascontiguousarray(prior, np.float64)).to(ctx.device)
    m = torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32)).to(ctx.device)
    r = None if request is None else torch.from_numpy(np.ascontiguousarray(request, np.uint8)).to(ctx.device)
    osa._abi.check(osa.lib().osg_mcts_root_noise(ctx._h, p.data_ptr(), m.data_ptr(), mask.shape[1],
                                                 None if r is None else r.data_ptr(), p.shape[0], p.shape[1],
                                                 float(alpha), float(epsilon), int(seed), int(index_offset), int(sub)))
    ctx.synchronize()
    return p.cpu().numpy()


def _compare_noise(dev, host):
    """(rows that differ grossly, largest relative difference of the others): per row, against its largest entry."""
    rel = np.abs(dev - host).max(1) / np.abs(host).max(1)
    gross = rel > GROSS
    return int(gross.sum()), float(rel[~gross].max()) if (~gross).any() else 0.0


def test_root_noise_touches_only_requested_rows_and_legal_columns(osa, ctx, exe, workdir):
    rng = np.random.default_rng(3)
    N, A = 257, 81
    mask = rng.integers(0, 1 << 32, (N, 3), dtype=np.uint64).astype(np.uint32)
    mask[:, 2] &= np.uint32((1 << (A - 64)) - 1)
    mask[:, 0] |= np.uint32(1)
    legal = ((mask[:, np.arange(A) // 32] >> (np.arange(A) % 32).astype(np.uint32)) & 1).astype(bool)
    prior = np.where(legal, rng.random((N, A)), -7.0)
    prior = np.where(legal, prior / np.where(legal, prior, 0).sum(1, keepdims=True), prior)
    request = rng.choice(np.array([0, 1, 2, 3, 5], np.uint8), N)
    request[:4] = [5, 1, 5, 2]
    at_root = request == 5
    out = _device_noise(osa, ctx, prior, mask, 0.3, 0.25, 11, 5, 2, request)
    assert (out[~at_root].view(np.uint64) == prior[~at_root].view(np.uint64)).all()
    assert (out[~legal] == -7.0).all()
    assert (out[at_root][legal[at_root]] != prior[at_root][legal[at_root]]).mean() > 0.99
    import math
    sums = np.array([math.fsum(row[l]) for row, l in zip(out[at_root], legal[at_root])])
    assert np.abs(sums - 1.0).max() <= 4 * np.finfo(np.float64).eps
    every = _device_noise(osa, ctx, prior, mask, 0.3, 0.25, 11, 5, 2, None)      # no request array: every row
    assert (every[at_root].view(np.uint64) == out[at_root].view(np.uint64)).all()
    assert (every[~at_root][legal[~at_root]] != prior[~at_root][legal[~at_root]]).mean() > 0.99
    same = _device_noise(osa, ctx, prior, mask, 0.3, 0.0, 11, 5, 2, None)
    assert (same.view(np.uint64) == prior.view(np.uint64)).all()                 # epsilon = 0 changes nothing
    again = _device_noise(osa, ctx, prior, mask, 0.3, 0.25, 11, 5, 2, request)
    assert (again.view(np.uint64) == out.view(np.uint64)).all()                  # the same seed: the same bits
    for i in (0, 2, 200, 256):
        alone = _device_noise(osa, ctx, prior[i:i + 1], mask[i:i + 1], 0.3, 0.25, 11, 5 + i, 2, None)
        assert (alone.view(np.uint64) == every[i:i + 1].view(np.uint64)).all()   # row i = row 0 at index_offset + i
    host = sc.host_noise(exe, prior, mask, 0.3, 0.25, 11, 5, 2, workdir)
    gross, rel = _compare_noise(every, host)
    print(f"device against host, mixed priors: {gross} gross rows of {N}, largest relative difference {rel:.3e}")
    assert gross == 0 and rel <= NOISE_REL_BOUND
    for bad in (dict(alpha=0.0), dict(alpha=float("nan")), dict(epsilon=1.5)):
        args = dict(alpha=0.3, epsilon=0.25)
        args.update(bad)
        with pytest.raises(osa.OsgError):
            _device_noise(osa, ctx, prior, mask, args["alpha"], args["epsilon"], 11, 5, 2, None)


@pytest.mark.parametrize("k,alpha", NOISE_SHAPES)
def test_root_noise_has_the_dirichlets_moments_and_marginal(osa, ctx, k, alpha):
    x = _device_noise(osa, ctx, np.zeros((N_NOISE, k)), sc.first_k_mask(N_NOISE, k, k), alpha, 1.0, NOISE_SEED, 0, 0)
    assert np.isfinite(x).all() and (x >= 0).all()
    res = sc.noise_statistics(x, k, alpha)
    print(k, alpha, res)
    assert res["ok"], res


def test_root_noise_agrees_with_the_host_program(osa, ctx, exe, workdir):
    k, alpha = 9, 0.3
    dev = _device_noise(osa, ctx, np.zeros((N_NOISE, k)), sc.first_k_mask(N_NOISE, k, k), alpha, 1.0, NOISE_SEED, 0, 0)
    host = sc.pure_noise(exe, k, alpha, N_NOISE, NOISE_SEED, workdir)
    gross, rel = _compare_noise(dev, host)
    print(f"device against host, Dirichlet({alpha}) on {k} actions: {gross} gross rows of {N_NOISE}, "
          f"largest relative difference of the others {rel:.3e}")
    assert gross <= N_NOISE >> 12
    assert rel <= NOISE_REL_BOUND


class _StubEvaluator:
    """Prior proportional to a + 1 over the legal actions, value `v` for player 0 — a pure function of the state."""
    needs_prior = True
    joint = False

    def __init__(self, v=0.0):
        self.v = v

    def evaluate(self, leaf, want_prior, want_value):
        import torch
        legal = leaf.legal_actions_bool().to(torch.float64)
        w = legal * torch.arange(1, legal.shape[1] + 1, device=legal.device, dtype=torch.float64)
        prior = w / w.sum(1, keepdim=True).clamp(min=1.0)
        value = torch.full((leaf.n, 1), self.v, dtype=torch.float64, device=legal.device)
        return prior, torch.cat([value, -value], dim=1)


def test_search_mixes_the_root_prior_on_the_device(osa, ctx, exe, workdir):
    from open_spiel_amd import mcts
    n, A = 5, 9
    roots = osa.StateBatch(ctx, "tic_tac_toe", n)
    kw = dict(max_simulations=4, uct_c=1.4, puct=True, seed=3, index_offset=10)   # (too few to reach the end of a game)
    plain = mcts.search(roots, _StubEvaluator(), **kw)["child_prior"].cpu().numpy()
    stub = np.arange(1, A + 1) / 45.0
    assert np.abs(plain - stub).max() < 1e-15
    res = mcts.search(roots, _StubEvaluator(), dirichlet_alpha=0.3, dirichlet_epsilon=0.25, noise_seed=77, noise_sub=3,
                      want_root_value=True, **kw)
    want = sc.host_noise(exe, np.tile(plain[0], (n, 1)), sc.first_k_mask(n, A, A), 0.3, 0.25, 77, 10, 3, workdir)
    got = res["child_prior"].cpu().numpy()
    gross, rel = _compare_noise(got, want)
    assert gross == 0 and rel <= NOISE_REL_BOUND, (gross, rel)
    assert len({row.tobytes() for row in got}) == n          # every root its own stream
    assert (res["root_value"].cpu().numpy() == 0.0).all()    # the stub's value, averaged
    assert "root_value" not in mcts.search(roots, _StubEvaluator(), **kw)
    # SelfPlay draws the noise on noise_seed(seed), not on the seed of its move draws
    from open_spiel_amd import alpha_zero
    sp = osa.SelfPlay(roots, osa.ReplayBuffer(ctx, "tic_tac_toe", 16), _StubEvaluator(), max_simulations=4, uct_c=1.4,
                      dirichlet_alpha=0.3, dirichlet_epsilon=0.25, seed=3, index_offset=10)
    got = sp.search(6)["child_prior"].cpu().numpy()
    for noise_seed, same in ((alpha_zero.noise_seed(3), True), (3, False)):
        want = sc.host_noise(exe, np.tile(plain[0], (n, 1)), sc.first_k_mask(n, A, A), 0.3, 0.25, noise_seed, 10, 6, workdir)
        gross, rel = _compare_noise(got, want)
        assert (gross == 0 and rel <= NOISE_REL_BOUND) == same, (noise_seed, gross, rel)


# ---- a full run ---------------------------------------------------------------------------------------------------------
# (the connect_four boards: the u64 records — the default board's two constant-folded words, a general one-word-per-colour
# board and a two-words-per-colour board above 64 bits — through select's copy, the scatter and the sample)
@pytest.mark.parametrize("game,n,capacity", [("tic_tac_toe", 64, 257), ("hex(board_size=3)", 33, 257),
                                             ("connect_four", 33, 65), ("connect_four(rows=4,columns=5,x_in_row=3)", 33, 65),
                                             ("connect_four(rows=8,columns=9,x_in_row=3)", 33, 65)])
def test_self_play_fills_the_ring_like_the_sequential_model(osa, ctx, oracle, game, n, capacity):
    import torch
    from open_spiel_amd import mcts
    drop, plies, seed, offset = 4, 40, 0xA11CE, 500
    envs = osa.StateBatch(ctx, game, n)
    buf = osa.ReplayBuffer(ctx, game, capacity)
    evaluator = mcts.RolloutEvaluator()
    sp = osa.SelfPlay(envs, buf, evaluator, max_simulations=32, uct_c=1.4, temperature=1.0, temperature_drop=drop,
                      puct=False, seed=seed, index_offset=offset)
    og = oracle.Game(game)
    A = envs.num_distinct_actions
    model = [og.new_initial_state() for _ in range(n)]
    trajectory = [[] for _ in range(n)]          # per environment: (words, player, policy bits, action)
    ring, games = sc.Ring(capacity), 0
    for step in range(plies):
        words = envs.raw_words()
        for i in range(n):     # the environments are where the oracle is after the logged actions
            assert envs.state_string(i) == str(model[i]), (step, i)
        # the same search once more, for the visit counts step() consumes
        again = mcts.search(envs.clone(), evaluator, max_simulations=32, uct_c=1.4, seed=sp.search_seed(step),
                            index_offset=offset, puct=False, want_root_value=True)
        out = sp.step()
        ctx.synchronize()
        visits = again["child_visits"].cpu().numpy()
        p64 = sc.policy_target(visits, 1.0)
        policy = out["policy"].cpu().numpy()
        assert (policy.view(np.uint32) == p64.astype(np.float32).view(np.uint32)).all(), step
        moved = np.array([len(t) for t in trajectory], np.int32)
        action = out["action"].cpu().numpy()
        want = sc.moves(p64, again["best_action"].cpu().numpy(), moved, np.full(n, step), drop, seed, offset)
        assert (action == want).all(), step     # the streams: Rng(seed, offset + env, plies played since creation)
        root_value = out["root_value"].cpu().numpy()
        assert (root_value == again["root_value"].cpu().numpy()).all() and (np.abs(root_value) <= 1.0).all()
        finished, returns = out["finished"].cpu().numpy(), out["returns"].cpu().numpy()
        for i in range(n):
            state = model[i]
            assert action[i] in state.legal_actions()
            trajectory[i].append((words[:, i].copy(), state.current_player(), policy[i].view(np.uint32).copy(), int(action[i]),
                                  np.float32(root_value[i]), str(state),
                                  np.asarray(state.observation_tensor(state.current_player()), np.float32),
                                  np.isin(np.arange(A), state.legal_actions())))
            state.apply_action(int(action[i]))
            assert bool(finished[i]) == state.is_terminal(), (step, i)
            if state.is_terminal():
                assert returns[i] == state.returns()[0]
                for row in trajectory[i]:
                    ring.append(row + (np.float32(state.returns()[0]),))   # value = returns[0] of the row's game
                trajectory[i] = []
                model[i] = og.new_initial_state()
                games += 1
            else:
                assert returns[i] == 0.0
        assert buf.total_seen == ring.total_seen and len(buf) == len(ring)
        if len(ring):
            rows = buf.rows(torch.arange(len(ring)))
            ring_words = buf.states.raw_words()[:, :len(ring)]
            got_words = rows["states"].raw_words()
            assert (got_words == ring_words).all()
            assert (ring_words == np.stack([r[0] for r in ring.data], 1)).all(), step
            assert (rows["player"].cpu().numpy() == np.array([r[1] for r in ring.data])).all()
            assert (_bits32(rows["policy"]) == np.stack([r[2] for r in ring.data])).all()
            assert (rows["action"].cpu().numpy() == np.array([r[3] for r in ring.data])).all()
            assert (rows["root_value"].cpu().numpy() == np.array([r[4] for r in ring.data])).all()
            assert (rows["value"].cpu().numpy() == np.array([r[8] for r in ring.data])).all()
    assert games > 3 and ring.total_seen > capacity       # the ring wrapped
    assert envs.desc.state_words * envs.desc.state_word_bytes == words.shape[0] * words.itemsize
    # every stored row's state string is the oracle's at that ply of the replayed game
    assert len(ring) == capacity
    for slot in range(capacity):
        assert buf.states.state_string(slot) == ring.data[slot][5], slot
    # sampling
    m = 1000
    index, states, policy, value = buf.sample_rows(m, seed=99, index_offset=7)
    want_index = st.VecRng(99, 7 + np.arange(m, dtype=np.int64), 0).below(len(buf))
    assert (index.cpu().numpy() == want_index).all()
    batch = buf.sample(m, seed=99, index_offset=7)
    gathered = buf.states.gather(index)
    assert torch.equal(batch.observation, gathered.observation_tensor(-1))
    assert torch.equal(batch.legals_mask, gathered.legal_actions_bool())
    picked = buf.rows(index)
    assert torch.equal(batch.policy, picked["policy"]) and torch.equal(batch.value, picked["value"])
    assert batch.observation.shape == (m, envs.desc.obs_size) and batch.legals_mask.shape == (m, A)
    # observation and legal mask are the oracle's for the player to move at the sampled row's position
    assert (batch.observation.cpu().numpy() == np.stack([ring.data[k][6] for k in want_index])).all()
    assert (batch.legals_mask.cpu().numpy() == np.stack([ring.data[k][7] for k in want_index])).all()
    assert (batch.value.cpu().numpy() == np.array([ring.data[k][8] for k in want_index])).all()
    ctx.synchronize()


def test_a_large_root_value_cuts_the_game_off(osa, ctx):
    n = 64
    envs = osa.StateBatch(ctx, "tic_tac_toe", n)
    buf = osa.ReplayBuffer(ctx, "tic_tac_toe", 257)
    sp = osa.SelfPlay(envs, buf, _StubEvaluator(0.9), max_simulations=4, uct_c=1.4, cutoff_value=0.5, seed=5)
    for step in range(3):
        out = sp.step()
        ctx.synchronize()
        assert bool(out["finished"].all())
        assert np.abs(out["root_value"].cpu().numpy() - 0.9).max() < 1e-12
        assert (out["returns"].cpu().numpy() == out["root_value"].cpu().numpy()).all()   # player 0 moved: + root_value
        assert buf.total_seen == n * (step + 1)
        assert (envs.raw_words() == osa.StateBatch(ctx, "tic_tac_toe", n).raw_words()).all()   # every game restarted
    import torch
    rows = buf.rows(torch.arange(len(buf)))
    assert np.abs(rows["value"].cpu().numpy() - 0.9).max() < 1e-6
    assert (rows["player"].cpu().numpy() == 0).all()
    # player 1 to move with the same evaluator: its root value is -0.9, and so are its returns; player 0's are + 0.9
    envs2 = osa.StateBatch(ctx, "tic_tac_toe", 4)
    envs2.apply_actions([4, 4, 0, 8])
    buf2 = osa.ReplayBuffer(ctx, "tic_tac_toe", 16)
    out = osa.SelfPlay(envs2, buf2, _StubEvaluator(0.9), max_simulations=4, uct_c=1.4, cutoff_value=0.5, seed=5).step()
    ctx.synchronize()
    assert np.abs(out["root_value"].cpu().numpy() + 0.9).max() < 1e-12 and bool(out["finished"].all())
    assert (out["returns"].cpu().numpy() == -out["root_value"].cpu().numpy()).all()


def test_self_play_with_a_network_evaluator_and_root_noise(osa, ctx):
    """The two search paths self-play can take with a network: one evaluator round per simulation (no noise), and the
    request / answer loop with the root noise mixed on the device."""
    import torch
    from open_spiel_amd import mcts

    def model(obs, legal):
        w = legal.to(torch.float32)
        return w / w.sum(1, keepdim=True).clamp(min=1.0), torch.zeros(obs.shape[0], device=obs.device)

    n = 64
    for alpha in (0.0, 0.3):
        envs = osa.StateBatch(ctx, "tic_tac_toe", n)
        buf = osa.ReplayBuffer(ctx, "tic_tac_toe", 4096)
        sp = osa.SelfPlay(envs, buf, mcts.VPNetEvaluator(model), max_simulations=16, uct_c=1.4, temperature_drop=2,
                          dirichlet_alpha=alpha, dirichlet_epsilon=0.25, seed=9)
        length, rows, policies = np.zeros(n, np.int64), 0, []
        for step in range(12):
            out = sp.step()
            ctx.synchronize()
            policy = out["policy"].cpu().numpy()
            assert np.abs(policy.sum(1) - 1.0).max() < 1e-6 and np.isfinite(out["root_value"].cpu().numpy()).all()
            policies.append(policy)
            length += 1
            done = out["finished"].cpu().numpy()
            rows += int(length[done].sum())
            length[done] = 0
            assert buf.total_seen == rows
        assert rows > 0
        if alpha == 0.0:
            plain = policies[0]
        else:   # the noise reaches the search: the first ply's visit counts differ from the plain run's, root by root
            assert (np.abs(policies[0] - plain).max(1) > 0).mean() > 0.5


def test_a_buffer_in_use_refuses_to_close(osa, ctx):
    envs = osa.StateBatch(ctx, "tic_tac_toe", 4)
    buf = osa.ReplayBuffer(ctx, "tic_tac_toe", 8)
    sp = osa.SelfPlay(envs, buf, None, max_simulations=2, uct_c=1.4)
    with pytest.raises(osa.OsgError, match="close it first"):
        buf.close()
    assert len(buf) == 0      # still usable
    sp.close()
    buf.close()
    with pytest.raises(osa.OsgError, match="closed"):
        osa.SelfPlay(envs, buf, None, max_simulations=2, uct_c=1.4)
    with pytest.raises(osa.OsgError, match="closed"):
        buf.sample(4, seed=1)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(osa, ctx):
    for game in ("kuhn_poker", "leduc_poker"):
        with pytest.raises(osa.OsgError, match="osg error -2"):
            osa.ReplayBuffer(ctx, game, 8)
    with pytest.raises(osa.OsgError):
        osa.ReplayBuffer(ctx, "tic_tac_toe", 0)
    envs = osa.StateBatch(ctx, "tic_tac_toe", 4)
    buf = osa.ReplayBuffer(ctx, "tic_tac_toe", 8)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(osa.OsgError, match="temperature"):
            osa.SelfPlay(envs, buf, None, max_simulations=8, uct_c=1.4, temperature=bad)
    with pytest.raises(osa.OsgError, match="max_simulations"):
        osa.SelfPlay(envs, buf, None, max_simulations=1, uct_c=1.4)
    with pytest.raises(osa.OsgError, match="empty"):
        buf.sample(4, seed=1)
    with pytest.raises(osa.OsgError):
        osa.SelfPlay(envs, osa.ReplayBuffer(ctx, "connect_four", 8), None, max_simulations=8, uct_c=1.4)
    # the C entry points themselves
    from open_spiel_amd import _abi
    import ctypes as C
    h = C.c_void_p()
    kuhn = osa.StateBatch(ctx, "kuhn_poker", 4)
    cfg = _abi.SelfPlayCfg(1.0, 2.0, 4, 0, 0, 0)
    assert osa.lib().osg_selfplay_create(kuhn._h, buf._h, C.byref(cfg), C.byref(h)) == -2
    states = osa.StateBatch(ctx, "tic_tac_toe", 4)
    assert osa.lib().osg_replay_sample(buf._h, 1, 0, 0, states._h, None, None, None) == -1
    assert osa.lib().osg_replay_sample(buf._h, 1, 0, 4, states._h, None, None, None) == -1   # empty
    ctx.synchronize()
