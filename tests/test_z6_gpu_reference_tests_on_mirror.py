"""The reference's own C++ unit tests for the hot path, run against the MI355X host mirror on the device.

oracle/Makefile.mirror_tests (run by __graft_entry__.build()) compiles the reference's test SOURCES unmodified (read
where they lie in the reference tree, never copied) against open_spiel_amd/csrc/host/osg_spiel.h + libosg_hip.so; the
binaries land in oracle/_ref/mirror_tests/ (git-ignored, carried with the built tree like the rest of oracle/_ref/) and
are run here.  A test passes iff the binary
exits 0, i.e. every SPIEL_CHECK_* of the reference's own test held on the MI355X path:

* cfr_br_test.cc (as is): CFR-BR on kuhn/leduc reaches the reference's NashConv bounds; 3-player kuhn runs.
* mcts_test.cc: 8 of its 10 tests (catch and pig are outside the hot path): self-play through Bot/EvaluateBots,
  the three MCTS-Solver known answers, garbage collection under max_memory_mb=1, the wall-clock limit.
* external_sampling_mccfr_test.cc: kuhn (1000 iterations, NashConv < 0.05), leduc (1000, < 2.5), 3-player kuhn,
  the Serialize/Deserialize round trip at 1e-15 — liars_dice left out.
* outcome_sampling_mccfr_test.cc: kuhn (10000, < 0.17), leduc (10000, < 3.07), serialization — liars_dice left out.
* cfr_test.cc: 11 of its tests (goofspiel / matrix games through LoadGameAsTurnBased left out): Kuhn CFR and CFR+ reach
  the Nash value and exploitability <= 0.05, the 3- / 4-player Kuhn and leduc NashConv bounds, the table and solver
  serialization round trips.
* tabular_exploitability_test.cc (as is): exploitability / NashConv of the optimal, uniform and first-action policies
  on kuhn and leduc equal the reference's constants (0, 0.4583333333333335, 2.373611111111111, 0.916666666666667,
  4.747222222222222, 1, 2), the illegal-action regression.
* best_response_test.cc: 13 of 14 (the .efg one left out): best-response actions against five policies and the
  best-response value of EVERY history against the reference's golden tables.
* hex_test.cc and kuhn_poker_test.cc (as is) and leduc_poker_test.cc (the configurations the engine offers: 2 and 3
  players), each linked with the reference's tests/basic_tests.cc compiled unmodified: RandomSimTest — hundreds of
  random games checking Clone, serialization round trips, legal-action masks, sorted / unique actions, every
  player's tensors and strings at every state, returns — plus undo, ResampleFromInfostate, the single_tensor
  observer, GetAllStates (54 kuhn states), the always-X policies, board orientation and the swap rule.
* basic_tests.cc on tic_tac_toe and connect_four with the arguments of tic_tac_toe_test.cc / connect_four_test.cc:
  RandomSimTest, FastLoss, arbitrary board sizes.
* tic_tac_toe_test.cc (as is) and connect_four_test.cc (round 5; every test but the half of TestPermissiveValidation whose
  position names a mover the stone count contradicts): the JSON struct API — ToStruct / ToJson with the reference's
  exact JSON text, the struct types from JSON, ActionToStruct / StructToActions / ApplyActionStruct /
  ValidateActionStruct, NewInitialState from a struct, a board string and JSON, ConnectFourGameParams, LoadGame(params),
  LoadGameFromJson.
"""
import os
import subprocess

import pytest

import reference_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILT = os.path.join(ROOT, "oracle", "_ref", "mirror_tests")
BINARIES = ["reference_cfr_br_test", "reference_mcts_test_on_mirror", "reference_es_mccfr_test_on_mirror",
            "reference_os_mccfr_test_on_mirror", "reference_cfr_test_on_mirror", "reference_tabular_exploitability_test",
            "reference_best_response_test_on_mirror", "reference_hex_test", "reference_kuhn_poker_test",
            "reference_leduc_poker_test_on_mirror", "reference_basic_tests_boards_on_mirror", "reference_tic_tac_toe_test",
            "reference_connect_four_test_on_mirror", "reference_get_all_states_test",
            "reference_get_legal_actions_map_test_on_mirror"]


def _built(binary):
    """The binary as __graft_entry__.build() left it (the GPU tests never rebuild: the reference tree is not read here)."""
    path = os.path.join(BUILT, binary)
    if not os.access(path, os.X_OK):
        pytest.fail(f"{path} missing: run __graft_entry__.build() where the reference tree exists before shipping")
    return path


def test_reference_test_sources_compile_against_the_mirror():
    """CPU half: where the reference tree exists, its test sources compile and link against the mirror."""
    if not reference_py.sources_present():
        pytest.skip("no reference tree here: the binaries are built where it exists and carried prebuilt")
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.mirror_tests",
                           "REF=" + reference_py.REFERENCE_ROOT])
    for b in BINARIES + SLOW_BINARIES + [e[0] for e in EXAMPLES]:
        assert os.access(os.path.join(BUILT, b), os.X_OK), b


# the reference's example programs (open_spiel/examples/*.cc), compiled unmodified as well: (binary, arguments, a line of output)
EXAMPLES = [
    ("reference_example_cfr_example", [], "Iteration 999 exploitability=0.0009"),          # kuhn_poker, 1000 iterations
    # (mcts_example.cc:48-49 seeds from the clock when --seed is 0: a fixed seed — the random opponent is std::mt19937, the
    #  search draws from the engine's counter streams — makes the two games reproducible: the search wins both; the exact
    #  games are asserted below, so a weaker search — draws against the random player — fails)
    ("reference_example_mcts_example", ["--num_games=2", "--max_simulations=1000", "--quiet=true", "--seed=11"], "Overall wins: 2,0"),
    ("reference_example_example", ["--game=connect_four", "--seed=7"], "Final return to player 0 is"),
    # (with --show_infostate example.cc:139-141 hands an EMPTY span to InformationStateTensor: fatal in the reference too)
    ("reference_example_example", ["--game=leduc_poker", "--seed=3", "--show_legals=true"], "Final return to player 1 is"),
    ("reference_example_benchmark_game", ["--game=hex", "--sims=20", "--attempts=2"], "Benchmark: game: hex, num_sims: 20."),
    # count_all_states.cc over GetAllHistories: the census of kuhn_poker and leduc_poker (9 457 histories, 936 infostates)
    ("reference_example_count_all_states", [],
     "Game: kuhn_poker, num_histories: 58, num_terminal_histories: 30, num_chance_nodes: 4, num_nonterminal_states: 12, num_terminal_states: 30"),
    ("reference_example_count_all_states", ["--game_string=leduc_poker"], "Game: leduc_poker, num_histories: 9457, num_terminal_histories: 5520"),
    ("reference_example_shared_library_example", ["kuhn_poker(players=3)"], "Final return to player 2 is"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("binary,args,expect", EXAMPLES)
def test_reference_example_program_runs_on_the_mirror(binary, args, expect):
    path = _built(binary)
    r = subprocess.run([path] + args, capture_output=True, text=True, timeout=600)
    print((r.stdout + r.stderr)[-1500:])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert expect in r.stdout + r.stderr
    if binary == "reference_example_mcts_example":   # x (the search) against the uniform random player, seed 11
        out = r.stdout + r.stderr
        assert "Returns: 1,-1 Game actions: x(1,1) o(0,1) x(1,0) o(0,0) x(1,2)" in out
        assert "Returns: 1,-1 Game actions: x(1,1) o(0,0) x(2,2) o(1,2) x(2,0) o(0,2) x(2,1)" in out
        assert "Overall returns: 2,-2" in out and "Number of distinct games played: 2" in out


SLOW_BINARIES = ["reference_evaluate_bots_test"]   # 200 000 episodes through one-state batches: 142 s on an MI355X


@pytest.mark.gpu
@pytest.mark.skipif(not os.environ.get("OSG_SLOW_TESTS"), reason="142 s: set OSG_SLOW_TESTS=1 (passed on the device: profiles/r03_slow_reference_tests.log)")
@pytest.mark.parametrize("binary", SLOW_BINARIES)
def test_slow_reference_unit_test_passes_on_the_mirror(binary):
    test_reference_unit_test_passes_on_the_mirror(binary)


@pytest.mark.gpu
@pytest.mark.parametrize("binary", BINARIES)
def test_reference_unit_test_passes_on_the_mirror(binary):
    path = _built(binary)
    r = subprocess.run([path], capture_output=True, text=True, timeout=1200)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
