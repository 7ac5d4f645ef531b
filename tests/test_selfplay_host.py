"""The self-play arithmetic (open_spiel_amd/csrc/osg_selfplay.h, host + device) driven on the CPU by
tests/native/selfplay_host_test.cpp and held against the NumPy restatement of the reference's lines
(tests/selfplay_cases.py) and against exact distributions.  The program is stand-alone; it is built once plain and once
with the address and undefined-behaviour sanitizers and run as its own binary.

Largest fp64 deviation of the policy target from NumPy's at temperatures 0.25, 0.5 and 2 (printed by
test_policy_target_with_a_temperature): 5.6e-16 relative — two correct pows and two sum orders."""
import numpy as np
import pytest

import sampling_stats as st
import selfplay_cases as sc

N_NOISE, NOISE_SEED, NOISE_SHAPES = sc.N_NOISE, sc.NOISE_SEED, sc.NOISE_SHAPES


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("selfplay_io"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sc.build_host_test(str(tmp_path_factory.mktemp("selfplay") / "selfplay_host_test"))


@pytest.fixture(scope="module")
def sanitized_exe(tmp_path_factory):
    return sc.build_host_test(str(tmp_path_factory.mktemp("selfplay_san") / "selfplay_host_test_san"),
                              extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"))


@pytest.fixture(scope="module")
def selected(exe, workdir):
    cases = sc.select_cases()
    return cases, sc.host_select(exe, cases, workdir)


def test_policy_target_at_temperature_one_is_numpys_bit_for_bit(selected):
    cases, outs = selected
    seen = 0
    for c, (p64, p32, action, ok) in zip(cases, outs):
        if c["temperature"] != 1.0:
            continue
        want = sc.policy_target(c["visits"], 1.0)
        live = c["visits"].sum(1) > 0
        assert (ok.astype(bool) == live).all() and not live[5]
        assert (p64[live].view(np.uint64) == want[live].view(np.uint64)).all()
        assert (p32[live].view(np.uint32) == want[live].astype(np.float32).view(np.uint32)).all()
        assert (p64[~live] == 0).all() and (p64[live][c["visits"][live] == 0] == 0).all()
        seen += 1
    assert seen == len(sc.ACTIONS)


def test_policy_target_with_a_temperature(selected):
    """f32 policy within one f32 ulp of NumPy's: two correctly working fp64 pows and sum orders differ by a few 1e-16
    relative, far inside half an f32 ulp, so after rounding they differ by at most one."""
    cases, outs = selected
    worst = 0.0
    for c, (p64, p32, action, ok) in zip(cases, outs):
        if c["temperature"] == 1.0:
            continue
        want = sc.policy_target(c["visits"], c["temperature"])
        live = c["visits"].sum(1) > 0
        w32 = want[live].astype(np.float32)
        assert (w32 >= 0).all() and (p32[live] >= 0).all()
        ulps = np.abs(p32[live].view(np.int32).astype(np.int64) - w32.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (c["A"], c["temperature"], int(ulps.max()))
        pos = want[live] > 0
        assert ((p64[live] > 0) == pos).all()
        worst = max(worst, float(np.abs(p64[live][pos] / want[live][pos] - 1.0).max()))
    print(f"largest fp64 deviation of the policy target from NumPy's: {worst:.3e} relative")
    assert worst < 1e-14


def test_draw_action_is_the_restatements_over_the_programs_policy(selected):
    cases, outs = selected
    for c, (p64, p32, action, ok) in zip(cases, outs):
        live = ok.astype(bool)
        want = sc.moves(np.where(live[:, None], p64, 1.0), c["best"], c["move"], c["plyc"], c["drop"], c["seed"], c["offset"])
        assert (action[live] == want[live]).all(), (c["A"], c["temperature"])
        assert (action[~live] == -1).all()
        greedy = live & (c["move"] >= c["drop"])
        assert greedy.any() and (action[greedy] == c["best"][greedy]).all()
        drawn = live & ~greedy
        assert (c["visits"][drawn, action[drawn]] > 0).all()


def test_greedy_rows_consume_no_draw(exe, workdir):
    """The move of a drawn row depends on its stream; a greedy row's does not, whatever the stream."""
    c = sc.select_case(9, 1.0)
    other = dict(c, seed=c["seed"] + 1, plyc=c["plyc"] + 3)
    (_, _, a0, ok), (_, _, a1, _) = sc.host_select(exe, [c, other], workdir)
    live = ok.astype(bool)
    greedy = live & (c["move"] >= c["drop"])
    assert (a0[greedy] == a1[greedy]).all() and (a0[greedy] == c["best"][greedy]).all()
    assert (a0[live & ~greedy] != a1[live & ~greedy]).any()


def _ring_cases():
    rng = np.random.default_rng(7)
    cases = []
    for capacity in (1, 5, 257):
        flushes = []
        for f in range(12):
            lengths = rng.integers(1, 10, 33)
            finished = rng.random(33) < (0.0 if f in (0, 6) else 0.3)   # flushes with no finished environment
            flushes.append(np.where(finished, lengths, 0).astype(np.int32))
        flushes.append(np.full(33, 9, np.int32))   # 297 rows at once: larger than every capacity here
        flushes.append(np.where(rng.random(33) < 0.5, 3, 0).astype(np.int32))
        cases.append((capacity, flushes))
    return cases


def test_ring_slots_are_the_sequential_appends(exe, workdir):
    cases = _ring_cases()
    outs = sc.host_ring(exe, cases, workdir)
    for (capacity, flushes), per in zip(cases, outs):
        ring, held, row_id = sc.Ring(capacity), {}, 0
        for flen, (slots, total_seen, size) in zip(flushes, per):
            first = row_id
            for i, length in enumerate(flen):
                for t in range(length):
                    ring.append(row_id)
                    row_id += 1
            for g, slot in enumerate(slots):
                if slot >= 0:
                    assert (first + g) not in held.values()
                    held[int(slot)] = first + g
            written = [s for s in slots if s >= 0]
            assert len(written) == len(set(written)) == min(len(slots), capacity)   # no two rows of a flush share a slot
            assert (total_seen, size) == (ring.total_seen, len(ring))
            # the literal ring keeps its rows in slot order once it is full, and appends in order before
            assert [held[s] for s in range(len(ring))] == ring.data, (capacity, total_seen)


@pytest.mark.parametrize("k,alpha", NOISE_SHAPES)
def test_noise_has_the_dirichlets_moments_and_marginal(exe, workdir, k, alpha):
    x = sc.pure_noise(exe, k, alpha, N_NOISE, NOISE_SEED, workdir)
    assert np.isfinite(x).all() and (x >= 0).all()
    assert np.abs(np.array([float(np.sum(r)) for r in x[:512]]) - 1.0).max() <= 4 * np.finfo(np.float64).eps
    res = sc.noise_statistics(x, k, alpha)
    print(k, alpha, res)
    assert res["ok"], res
    assert (res["z"] is None) == (sc.dirichlet_first_cdf(k, alpha) is None)


@pytest.mark.parametrize("k,alpha", [(2, 0.5), (7, 0.3)])
def test_the_rules_reject_noise_without_the_small_alpha_step(exe, workdir, k, alpha):
    """The defect: gamma(alpha + 1) not scaled by u ^ (1 / alpha), i.e. Dirichlet(alpha + 1) — rejected at this N."""
    x = sc.pure_noise(exe, k, alpha, N_NOISE, NOISE_SEED, workdir, mode=1)
    res = sc.noise_statistics(x, k, alpha)
    print(k, alpha, res)
    assert not res["ok"]
    assert not res["means"]["ok"]
    if res["z"] is not None:
        assert not st.accept(res["z"])


def test_noise_mixes_only_the_legal_columns(exe, workdir):
    rng = np.random.default_rng(3)
    N, A = 64, 81
    mask = rng.integers(0, 1 << 32, (N, 3), dtype=np.uint64).astype(np.uint32)
    mask[:, 2] &= np.uint32((1 << (A - 64)) - 1)
    mask[:, 0] |= np.uint32(1)
    legal = ((mask[:, np.arange(A) // 32] >> (np.arange(A) % 32).astype(np.uint32)) & 1).astype(bool)
    prior = np.where(legal, rng.random((N, A)), -7.0)
    prior = np.where(legal, prior / np.where(legal, prior, 0).sum(1, keepdims=True), prior)
    out = sc.host_noise(exe, prior, mask, 0.3, 0.25, 11, 5, 2, workdir)
    assert (out[~legal] == -7.0).all()
    assert (out[legal] != prior[legal]).mean() > 0.99
    assert np.abs(np.where(legal, out, 0).sum(1) - 1.0).max() < 1e-14
    same = sc.host_noise(exe, prior, mask, 0.3, 0.0, 11, 5, 2, workdir)
    assert (same.view(np.uint64) == prior.view(np.uint64)).all()          # epsilon = 0 changes nothing
    again = sc.host_noise(exe, prior, mask, 0.3, 0.25, 11, 5, 2, workdir)
    assert (again.view(np.uint64) == out.view(np.uint64)).all()
    shifted = sc.host_noise(exe, prior[7:8], mask[7:8], 0.3, 0.25, 11, 5 + 7, 2, workdir)
    assert (shifted.view(np.uint64) == out[7:8].view(np.uint64)).all()    # row i = row 0 of a batch at index_offset + i


def test_a_last_bit_of_the_logarithm_flips_at_most_one_row_in_4096(exe, workdir):
    """The device's log differs from libm's in the last bits, and a Marsaglia-Tsang accept / reject that flips on such
    a difference changes a row grossly.  With the seed of the device comparison (tests/test_z28_gpu_selfplay.py) the host
    program run with every logarithm one ulp up or down stays within the cap the device test grants itself."""
    k, alpha = 9, 0.3
    base = sc.pure_noise(exe, k, alpha, N_NOISE, NOISE_SEED, workdir)
    for mode in (2, 3):
        other = sc.pure_noise(exe, k, alpha, N_NOISE, NOISE_SEED, workdir, mode=mode)
        rel = np.abs(other - base).max(1) / np.abs(base).max(1)
        gross = int((rel > 1e-6).sum())
        print(f"log {'+' if mode == 2 else '-'}1 ulp: {gross} gross rows of {N_NOISE}, largest other deviation "
              f"{rel[rel <= 1e-6].max():.3e}")
        assert gross <= N_NOISE >> 12


def test_noise_and_move_draws_never_share_a_stream():
    """A root's noise and its environment's move draw have the same stream (index_offset + env) and sub-stream (the
    ply): SelfPlay salts the noise's seed.  With one seed for both, the uniform that picks the move would be the first
    uniform behind the first legal action's noise."""
    from open_spiel_amd import alpha_zero
    env, ply = np.meshgrid(np.arange(4096, dtype=np.int64), np.arange(64, dtype=np.int64), indexing="ij")
    for seed in (0, 1, 0xA11CE, alpha_zero.NOISE_SALT, (1 << 64) - 1):
        salted = alpha_zero.noise_seed(seed)
        assert salted != seed and 0 <= salted < 1 << 64 and alpha_zero.noise_seed(salted) == seed
        move = st.VecRng(seed, 500 + env, ply)
        noise = st.VecRng(salted, 500 + env, ply)
        assert (move.s != noise.s).all()
        assert (move.unit() != noise.unit()).all()                      # z of the move against u1 of the first normal


def test_the_same_program_is_clean_under_the_sanitizers(sanitized_exe, exe, workdir):
    cases = sc.select_cases(rows=33)
    for a, b in zip(sc.host_select(sanitized_exe, cases, workdir), sc.host_select(exe, cases, workdir)):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    ring = _ring_cases()
    for a, b in zip(sc.host_ring(sanitized_exe, ring, workdir), sc.host_ring(exe, ring, workdir)):
        for (s0, t0, z0), (s1, t1, z1) in zip(a, b):
            assert (s0 == s1).all() and (t0, z0) == (t1, z1)
    x = sc.pure_noise(sanitized_exe, 7, 0.3, 4096, NOISE_SEED, workdir)
    assert x.tobytes() == sc.pure_noise(exe, 7, 0.3, 4096, NOISE_SEED, workdir).tobytes()
