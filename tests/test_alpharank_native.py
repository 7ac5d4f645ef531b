"""Alpha-rank as the kernels compute it (open_spiel_amd/csrc/osg_alpharank.h, host + device) driven on the CPU:
tests/native/alpharank_host_test.cpp runs the header's functions in the kernels' order, with the matrix in both of the
kernels' layouts, on every case of tests/alpharank_cases.py.  With infinite alpha and for the sweep its entries, pi,
marginals, epsilon, iterations and status must be the NumPy restatement's bit for bit (alpharank_cases.solve); with finite
alpha, where libm's exp and NumPy's may differ in the last place, pi lies within the case's bound; and every pi lies
within the entrywise relative bound of the exact one (alpharank_cases.bound).  The same program is built once more with
the address and undefined-behaviour sanitizers, as a stand-alone binary, and run."""
import subprocess

import pytest

import alpharank_cases as ac


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("alpharank_cases") / "cases.bin"
    ac.write_cases(ac.CASES, ac.restated(), ac.load(), path)
    return str(path)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ac.build_host_test(str(tmp_path_factory.mktemp("alpharank") / "alpharank_host_test"))


@pytest.fixture(scope="module")
def sanitized_exe(tmp_path_factory):
    return ac.build_host_test(str(tmp_path_factory.mktemp("alpharank_san") / "alpharank_host_test_san"),
                              extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"))


def _run(program, cases_file):
    r = subprocess.run([program, cases_file], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith(f"ok: {len(ac.CASES)} cases, both layouts, bit-equal to the restatement") and "FAILED" not in r.stdout
    assert r.stdout.count("largest relative deviation") == 1


def test_header_functions_reproduce_every_case(exe, cases_file):
    _run(exe, cases_file)


def test_the_same_program_is_clean_under_the_sanitizers(sanitized_exe, cases_file):
    _run(sanitized_exe, cases_file)
