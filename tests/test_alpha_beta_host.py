"""The search loop of the alpha-beta kernel (open_spiel_amd/csrc/osg_alpha_beta.h: AbSearch, host + device) driven on the
CPU: tests/native/alpha_beta_host_test.cpp instantiates it with array models of tic_tac_toe and connect_four written
from the rules in the test itself, and checks value (bit for bit), best_action, nodes and status of every tic_tac_toe and
connect_four case of tests/golden/minimax_vectors.npz — results of the reference's own minimax.py — plus the two edges of
the node budget: the tic_tac_toe initial position needs 18 297 nodes, so max_nodes = 18297 finishes and 18296 gives status 2."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 1 << 22


def _case_line(maxp, budget, value, best, nodes, status, history):
    bits = struct.unpack("<Q", struct.pack("<d", float(value)))[0]
    h = [int(a) for a in history if a >= 0]
    return f"{maxp} {budget} {bits:x} {best} {nodes} {status} {len(h)} " + " ".join(map(str, h))


def _geometry(game):
    if game == "tic_tac_toe":
        return game, 3, 3
    assert game.startswith("connect_four")
    params = dict(kv.split("=") for kv in game[len("connect_four("):-1].split(",")) if "(" in game else {}
    return "connect_four", int(params.get("rows", 6)), int(params.get("columns", 7))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ab") / "alpha_beta_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w",
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "alpha_beta_host_test.cpp"), "-o", path])
    return path


def test_host_instantiation_equals_the_reference_on_every_ttt_and_c4_golden(exe, tmp_path):
    lines, cases, sets = [], 0, 0
    with np.load(os.path.join(ROOT, "tests", "golden", "minimax_vectors.npz")) as z:
        names = sorted({k.split("/")[0] for k in z.files})
        for name in names:
            game = bytes(z[f"{name}/game"]).decode()
            if not game.startswith(("tic_tac_toe", "connect_four")):
                continue
            short, rows, cols = _geometry(game)
            n = len(z[f"{name}/status"])
            lines.append(f"set {short} {rows} {cols} {int(z[f'{name}/depth_limit'])} {int(z[f'{name}/leaf_mode'])} "
                         f"{float(z[f'{name}/leaf_value'])!r} {n}")
            for i in range(n):
                lines.append(_case_line(int(z[f"{name}/maximizing_player"][i]), BUDGET, z[f"{name}/value"][i],
                                        int(z[f"{name}/best_action"][i]), int(z[f"{name}/nodes"][i]),
                                        int(z[f"{name}/status"][i]), z[f"{name}/histories"][i]))
            cases += n
            sets += 1
    assert sets >= 10 and cases >= 4000
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.startswith(f"ok: {cases} cases in {sets} sets")


def test_node_budget_edges(exe, tmp_path):
    with np.load(os.path.join(ROOT, "tests", "golden", "minimax_vectors.npz")) as z:
        assert not (z["ttt_full/histories"][0] >= 0).any()   # case 0 is the initial position
        value, best, nodes = z["ttt_full/value"][0], int(z["ttt_full/best_action"][0]), int(z["ttt_full/nodes"][0])
    assert (value, best, nodes) == (0.0, 0, 18297)
    path = tmp_path / "edges.txt"
    path.write_text("set tic_tac_toe 3 3 -1 0 0.0 3\n" +
                    _case_line(-1, 18297, value, best, nodes, 0, []) + "\n" +
                    _case_line(-1, 18296, float("nan"), -1, 0, 2, []) + "\n" +
                    _case_line(-1, 1, float("nan"), -1, 0, 2, []) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.startswith("ok: 3 cases in 1 sets")
