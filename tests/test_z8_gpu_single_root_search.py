"""The one-root search of MCTSBot (osg_mcts_tree_* with RandomRolloutEvaluator in the launch): the two-wavefront form
(lane 0 walks the tree, a second wavefront plays each leaf's playouts in parallel) must build exactly the tree of the
one-lane form — same counter streams, integer returns summed in another order (the lane form is what the oracle's
MCTSBot replays draw for draw in tests/test_gpu_mcts.py and tests/test_z5_gpu_mcts_evaluator.py; mcts.cc:353-467)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys
sys.path.insert(0, ROOT)
from open_spiel_amd import pyspiel_hip as pyspiel
out = {}
for game_string, moves, sims, n_rollouts, solve, uct_c in CASES:
    game = pyspiel.load_game(game_string)
    state = game.new_initial_state()
    for a in moves:
        state.apply_action(a)
    bot = pyspiel.MCTSBot(game, pyspiel.RandomRolloutEvaluator(n_rollouts, 7), uct_c, sims, 50, solve, 0x5EED, False)
    rows = []
    def walk(node, depth):
        rows.append([depth, int(node.action), int(node.player), int(node.explore_count), float(node.total_reward),
                     [float(x) for x in node.outcome]])
        for c in node.children:
            walk(c, depth + 1)
    for _ in range(2):                       # two searches with one bot: the second one's streams start at search 1
        walk(bot.mcts_search(state), 0)
    out[game_string + str(moves) + str(uct_c)] = rows
print("TREES " + json.dumps(out))
'''

CASES = [
    ("tic_tac_toe", [], 400, 20, True, 2.0),
    ("tic_tac_toe", [4, 0, 8], 300, 7, True, 2.0),
    ("connect_four", [3, 3, 2], 300, 70, False, 2.0),        # more playouts than one round of lanes... (70 > 64)
    ("hex(board_size=5)", [12, 6], 200, 5, True, 2.0),
    ("kuhn_poker", [0, 1], 150, 9, False, 2.0),              # chance inside the playouts
    ("leduc_poker", [0, 3, 1], 150, 4, False, 2.0),
    ("hex(board_size=13)", [84, 70], 60, 3, False, 2.0),     # 167 children per node: the sequential expansion, nine-bit fields unused
    ("hex(board_size=19)", [180], 30, 2, False, 2.0),        # 360 children: the nine-bit action / child-count fields
    # round 6: the lockstep form's arg-max goes through an fp32 filter with an exact fallback; exploration constants at
    # which single precision cannot separate the children (values apart by less than its resolution), overflows
    # (1e30 * sqrt: +inf in fp32) or carries nothing (0) must still build the one-lane form's tree
    ("tic_tac_toe", [], 400, 20, True, 1e-9),
    ("tic_tac_toe", [4], 400, 3, False, 0.0),
    ("tic_tac_toe", [], 300, 20, True, 1e30),
    ("connect_four", [3, 3], 400, 5, True, 1e-5),
    ("connect_four", [], 300, 2, False, 0.37),
]


def _trees(coop):
    env = dict(os.environ, OSG_MCTS_COOP="1" if coop else "0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    code = f"ROOT={ROOT!r}\nCASES={CASES!r}\n" + CHILD
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TREES ")][-1]
    return json.loads(line[6:])


def _one_root_search_in_the_launch(ctx, game, moves, sims, n_rollouts, max_nodes, seed, offset):
    """osg_mcts_tree_* for ONE root with the playouts in the launch (flag 4), the whole search in one advance."""
    import ctypes as C
    import torch
    import open_spiel_amd as osa
    from open_spiel_amd import _abi
    from open_spiel_amd._abi import check, lib
    roots = osa.StateBatch(ctx, game, 1)
    for a in moves:
        roots.apply_actions(torch.tensor([a], dtype=torch.int32))
    leaf = osa.StateBatch(ctx, game, 1)
    A = roots.num_distinct_actions
    request = torch.zeros(1, dtype=torch.uint8, device=ctx.device)
    cfg = _abi.MctsCfg(2.0, sims, n_rollouts, 0, max_nodes, seed, offset, 1, 0)
    tree = C.c_void_p()
    check(lib().osg_mcts_tree_create(roots._h, C.byref(cfg), 4, C.byref(tree)))
    try:
        counts = (C.c_int64 * 4)()
        check(lib().osg_mcts_tree_advance(tree, leaf._h, None, None, request.data_ptr(), sims, counts))
        assert counts[1] == 0 and counts[2] == 0 and counts[3] == 0, "the search finished inside the launch"
        best = torch.zeros(1, dtype=torch.int32, device=ctx.device)
        visits = torch.zeros((1, A), dtype=torch.int32, device=ctx.device)
        reward = torch.zeros((1, A), dtype=torch.float64, device=ctx.device)
        outcome = torch.zeros((1, A), dtype=torch.int8, device=ctx.device)
        stats = torch.zeros((1, 4), dtype=torch.float64, device=ctx.device)
        check(lib().osg_mcts_tree_results(tree, best.data_ptr(), visits.data_ptr(), reward.data_ptr(), outcome.data_ptr(),
                                          None, stats.data_ptr()))
        ctx.synchronize()
        nodes = lib().osg_mcts_tree_nodes(tree, 0)
    finally:
        lib().osg_mcts_tree_destroy(tree)
    return dict(best=int(best[0]), visits=visits[0].cpu().numpy(), reward=reward[0].cpu().numpy(),
                outcome=outcome[0].cpu().numpy(), stats=stats[0].cpu().numpy(), nodes=int(nodes))


@pytest.mark.parametrize("game,moves,sims,n_rollouts,max_nodes,two_wavefronts", [
    ("tic_tac_toe", [], 300, 5, 40, True),                          # the compaction happens inside LDS
    # a tree that outgrows the 6 144 nodes kept in LDS before it is collected: the remap pass reads counts and parents on
    # both sides of the LDS / pool boundary and the compaction writes into LDS.  (The root has 167 children and a node is
    # expanded at its second visit: a search of fewer than ~170 simulations never leaves the root's children and has
    # nothing to collect; with 400 the oracle's tree passes 8 000 nodes.)  The two-wavefront form needs more than one
    # playout per leaf; with one, the same search runs in the one-lane form
    ("hex(board_size=13)", [84, 70], 400, 2, 8000, True),
    ("hex(board_size=13)", [84, 70], 400, 1, 8000, False),
])
def test_one_root_search_under_a_node_budget_replay_parity(oracle, game, moves, sims, n_rollouts, max_nodes, two_wavefronts):
    """GarbageCollect (mcts.cc:441-482) in the one-root search with the playouts in the launch: in the two-wavefront
    form the tree's first nodes live in LDS and are reached through index-picking proxies, so the compaction runs on LDS;
    on a tree that has outgrown the LDS part it also reads the nodes that live in the pool.  The oracle's MCTSBot at the same max_nodes_
    with every draw from the device's counter streams must give IDENTICAL root statistics, node count and simulations."""
    import open_spiel_amd as osa
    assert os.environ.get("OSG_MCTS_COOP", "1") != "0"
    assert two_wavefronts == (n_rollouts > 1)          # osg_mcts_tree_advance: one root, flag 4, n_rollouts > 1
    ctx = osa.Context(0)
    seed, offset = 0x6C6C6563, 4242
    got = _one_root_search_in_the_launch(ctx, game, moves, sims, n_rollouts, max_nodes, seed, offset)
    st = oracle.Game(game).new_initial_state()
    for a in moves:
        st.apply_action(int(a))
    want = st.mcts_search(2.0, sims, n_rollouts, -max_nodes, False, 0, counter_root=offset, counter_seed=seed)
    free = st.mcts_search(2.0, sims, n_rollouts, 4096, False, 0, counter_root=offset, counter_seed=seed)
    # a collection happened, by the oracle's own numbers: fewer nodes in use than its search without a budget keeps
    assert want["nodes"] < free["nodes"], (want["nodes"], free["nodes"])
    assert free["nodes"] > max_nodes
    assert got["stats"][0] == want["root_visits"], "root visits"
    assert got["stats"][3] == want["root_visits"] == sims, "simulations (each one visits the root)"
    assert got["nodes"] == got["stats"][1] == want["nodes"], "nodes in use"
    assert sorted(want["children"][:, 0].astype(int).tolist()) == np.nonzero(got["outcome"] != 3)[0].tolist()
    for a, cnt, tot, _ in want["children"]:
        a = int(a)
        assert got["visits"][a] == cnt, f"action {a}: visits {got['visits'][a]} vs {cnt}"
        assert got["reward"][a] == tot, f"action {a}: reward {got['reward'][a]} vs {tot}"
    assert got["best"] == want["best_action"]


def test_two_wavefront_one_root_search_builds_the_tree_of_the_one_lane_form():
    import __graft_entry__ as ge
    ge.build()
    coop, plain = _trees(True), _trees(False)
    assert coop.keys() == plain.keys()
    for key in coop:
        a, b = coop[key], plain[key]
        assert len(a) == len(b) and len(a) > 10, key
        for ra, rb in zip(a, b):
            assert ra[:4] == rb[:4], (key, ra, rb)                       # depth, action, player, visits
            assert ra[4] == rb[4], (key, ra, rb)                         # total reward: bit for bit
            assert np.array_equal(np.array(ra[5]), np.array(rb[5]), equal_nan=True), (key, ra, rb)
