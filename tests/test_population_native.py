"""The payoff-tensor cells and the aggregated policies as the kernels compute them (open_spiel_amd/csrc/osg_population.h,
host + device) driven on the CPU: tests/native/population_host_test.cpp runs the header's functions in the kernels' orders
over every case of tests/golden/population_vectors.npz whose tree action_value_vectors.npz carries (the four small games)
and compares every return and every aggregated cell with what the reference's own expected_game_score.py and
policy_aggregator.py computed, within 1e-12 absolute.  The same program is built once more with the address and
undefined-behaviour sanitizers, as a stand-alone binary, and run."""
import subprocess

import pytest

import action_value_cases as avc
import population_cases as pc


@pytest.fixture(scope="module")
def vectors():
    return pc.load(), avc.load()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pc.build_host_test(str(tmp_path_factory.mktemp("pop") / "population_host_test"))


@pytest.fixture(scope="module")
def sanitized_exe(tmp_path_factory):
    return pc.build_host_test(str(tmp_path_factory.mktemp("pop_san") / "population_host_test_san"),
                              extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"))


def _run(program, vectors, tmp_path, game):
    v, av = vectors
    profiles, aggregates = pc.write_cases(v, av, game, tmp_path / "cases.bin")
    P = int(v[f"{game}/num_players"])
    assert profiles == len(pc.RECORDED_KINDS[game]) ** P and aggregates == len(pc.RECORDED_WEIGHTS[game])
    r = subprocess.run([program, str(tmp_path / "cases.bin"), repr(pc.TOLERANCE)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith(f"ok: {profiles} profiles, {aggregates} aggregates") and "FAILED" not in r.stdout
    assert r.stdout.count("largest deviation") == 1 + aggregates


@pytest.mark.parametrize("game", pc.SMALL_GAMES)
def test_header_functions_reproduce_every_recorded_case(exe, vectors, tmp_path, game):
    _run(exe, vectors, tmp_path, game)


@pytest.mark.parametrize("game", pc.SMALL_GAMES)
def test_the_same_program_is_clean_under_the_sanitizers(sanitized_exe, vectors, tmp_path, game):
    _run(sanitized_exe, vectors, tmp_path, game)
