"""The exact Nash meta-solver as the kernel computes it (open_spiel_amd/csrc/osg_nash_lp.h, host + device) on the CPU:
tests/native/nash_lp_host_test.cpp runs the header's functions in the kernel's arrangement and through nl_solve on every
case of nash_lp_cases.CASES.  Both must give the NumPy restatement's x, y, v and pivot count bit for bit; the program is
built once more with the address and undefined-behaviour sanitizers, as a stand-alone binary, and run.  The restatement's
answers pass the certificate against HiGHS."""
import subprocess

import pytest

import nash_lp_cases as nc


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("nash_lp_cases") / "cases.bin"
    nc.write_cases(path)
    return str(path)


@pytest.mark.parametrize("extra", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover")], ids=["plain", "sanitized"])
def test_header_functions_reproduce_the_restatement_bit_for_bit(tmp_path, cases_file, extra):
    exe = nc.build_host_test(str(tmp_path / "nash_lp_host_test"), extra=extra)
    r = subprocess.run([exe, cases_file], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith(f"ok: {len(nc.CASES)} cases, both arrangements, bit-equal to the restatement") and "FAILED" not in r.stdout


@pytest.mark.parametrize("name", list(nc.CASES))
def test_the_restatement_passes_the_certificate(name):
    x, y, v, pivots, status = nc.restated(name)
    assert pivots <= 1000   # (the cap of 20 000 is far away)
    nc.certify(nc.CASES[name], x, y, v, status, name)
