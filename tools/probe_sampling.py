#!/usr/bin/env python3
"""Every statistic of tests/test_z22_gpu_sampling_statistics.py with its bound and N, once (MI355X):

    python tools/probe_sampling.py > profiles/sampling_statistics.txt

Runs the test module's own helper calls — one pass over its cases in this process — and prints, under each case's
name, the lines the checks print before they assert: the X^2 scores, the worst |mean - exact| against its Bernstein /
Hoeffding bound, the aggregate sum of z^2, the sample counts.  Ends with one line that counts the cases; if a check
fails, the test runner's whole report follows instead.  The exit status is that of the checks."""
import contextlib
import io
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Titles:
    cases = 0

    def pytest_runtest_logstart(self, nodeid, location):
        Titles.cases += 1
        print("\n@" + nodeid.split("::", 1)[1], flush=True)


if __name__ == "__main__":
    raw = io.StringIO()
    with contextlib.redirect_stdout(raw):
        rc = pytest.main([os.path.join(ROOT, "tests", "test_z22_gpu_sampling_statistics.py"), "-s", "-q", "--no-header",
                          "-p", "no:cacheprovider", "--tb=short"], plugins=[Titles()])
    if rc != 0:
        print(raw.getvalue())
        sys.exit(rc)
    for line in raw.getvalue().splitlines():   # the case names and what the checks printed; not the runner's progress marks
        if line.startswith("@"):
            print(line[1:])
        elif line.startswith("  "):
            print(line)
    print(f"{Titles.cases} cases, every statistic within its bound")
