"""The averaging arithmetic of extensive-form fictitious play as the kernels run it (open_spiel_amd/csrc/osg_xfp.h, host +
device) driven on the CPU: tests/native/xfp_host_test.cpp feeds every recorded best response of
tests/golden/xfp_vectors.npz — the trajectories of the reference's own fictitious_play.py — through xfp_reach and
xfp_update_row; both reaches and the policy after every iteration must equal the recorded ones bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = {"kuhn_poker": 120, "kuhn_poker(players=3)": 40, "leduc_poker": 25}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("xfp") / "xfp_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-w", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "xfp_host_test.cpp"), "-o", path])
    return path


@pytest.mark.parametrize("game", list(GAMES))
def test_header_functions_reproduce_every_recorded_iteration(exe, tmp_path, game):
    with np.load(os.path.join(ROOT, "tests", "golden", "xfp_vectors.npz")) as z:
        v = {k[len(game) + 1:]: z[k] for k in z.files if k.startswith(game + "/")}
    T, I, A = v["policy"].shape
    assert T == GAMES[game]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.array([I, A, int(v["player"].max()) + 1, T], np.int32).tobytes())
        for name in ("nact", "player", "pred_info", "pred_action"):
            f.write(np.ascontiguousarray(v[name], np.int32).tobytes())
        for t in range(T):
            f.write(np.ascontiguousarray(v["br"][t], np.int32).tobytes())
            for name in ("avg_reach", "br_reach", "policy"):
                f.write(np.ascontiguousarray(v[name][t], np.float64).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.startswith(f"ok: {T} iterations, {I} infostates, {int(v['nact'].sum()) * T} cells")
