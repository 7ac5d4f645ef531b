"""Extensive-form regret minimization as the kernels run it (open_spiel_amd/csrc/osg_efr.h, host + device) driven on the
CPU: tests/native/efr_host_test.cpp builds the deviation tables with the header's builder, compares them with the
reference's exactly, and runs whole iterations with the header's functions over every run of
tests/golden/efr_vectors.npz — the trajectories of the reference's own efr.py — with the items of every phase in both
orders (the same bits), comparing R, the current, cumulative and average policy at every checkpoint within
efr_cases.TOLERANCE.  It prints the largest deviation per run.  The regret-matching unit cases go through the header's
efr_regret_match with the rank LAPACK found."""
import subprocess

import numpy as np
import pytest

import efr_cases as ec


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ec.build_host_test(str(tmp_path_factory.mktemp("efr") / "efr_host_test"))


@pytest.mark.parametrize("r", range(len(ec.run_ids())), ids=ec.run_ids())
def test_header_functions_reproduce_every_recorded_checkpoint(exe, tmp_path, r):
    v = ec.load()
    ec.write_case(v, r, tmp_path / "case.bin")
    p = subprocess.run([exe, "run", str(tmp_path / "case.bin"), repr(ec.TOLERANCE), str(tmp_path / "state.bin")],
                       capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert p.stdout.rstrip().endswith(f"ok: {len(v[f'r{r}/checkpoints'])} checkpoints")
    assert "largest deviation" in p.stdout and "FAILED" not in p.stdout and "deviation tables" in p.stdout


def test_header_regret_matching_on_the_unit_cases(exe, tmp_path):
    v = ec.load()
    n = ec.write_unit_cases(v, tmp_path / "rm.bin")
    p = subprocess.run([exe, "rm", str(tmp_path / "rm.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.fromfile(tmp_path / "out.bin", np.float64).reshape(n, 5)
    assert np.array_equal(got[:, 4].astype(np.int32), v["rm/rank"])
    largest = 0.0
    for j in range(n):
        A = int(v["rm/A"][j])
        largest = max(largest, float(np.max(np.abs(got[j, :A] - v["rm/out"][j, :A]))))
    print(f"{n} cases, largest deviation {largest:.3g}")
    assert largest <= ec.TOLERANCE
