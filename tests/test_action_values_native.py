"""The per-infostate action values as the kernels compute them (open_spiel_amd/csrc/osg_action_values.h, host +
device) driven on the CPU: tests/native/action_values_host_test.cpp runs the header's functions in the kernels' two
orders over every case of tests/golden/action_value_vectors.npz that carries its tree (the four small games) and
compares every output with what the reference's own action_value.py computed, within 1e-12 absolute (values are at most
13 in magnitude and a sum has a few hundred terms: honest rounding stays below about 1e-13; measured largest deviations:
DESIGN.md section 10)."""
import subprocess

import pytest

import action_value_cases as avc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return avc.build_host_test(str(tmp_path_factory.mktemp("av") / "action_values_host_test"))


@pytest.mark.parametrize("game", avc.SMALL_GAMES)
def test_header_functions_reproduce_every_recorded_case(exe, tmp_path, game):
    v = avc.load()
    listed = avc.write_cases(v, game, tmp_path / "cases.bin")
    assert len(listed) == (7 if game in avc.TWO_PLAYER else 3)
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), repr(avc.TOLERANCE)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.rstrip().endswith(f"ok: {len(listed)} cases")
    assert r.stdout.count("largest deviation") == len(listed) and "FAILED" not in r.stdout
    assert r.stdout.count("agree bit for bit") == len(listed)
