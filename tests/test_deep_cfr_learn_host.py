"""CPU checks of the fused Deep CFR learner's LDS planner (csrc/osg_adam_plan.h) through a small stand-alone program.  (The
float64 restatement, tests/deep_cfr_learn_cases.py, is held against torch's autograd and Adam by every GPU case.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adam_plan") / "adam_plan_host_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"), os.path.join(ROOT, "tests", "native", "adam_plan_host_test.cpp"), "-o", exe])

    def run(widths, batch, limit=LDS_LIMIT):
        out = subprocess.check_output([exe, str(len(widths) - 1), *map(str, widths), str(batch), str(limit)], text=True)
        return [line.split() for line in out.splitlines()]
    return run


# the shapes the learner must serve on 160 KB: the reference example's, its tests', (128,) at 1024 rows, (64, 64)
MUST_SERVE = [([30, 64, 3], 256), ([11, 4, 2, 2], 32), ([11, 8, 4, 2], 32), ([11, 32, 16, 2], 32), ([11, 16, 8, 2], 32),
              ([30, 128, 3], 1024), ([30, 64, 64, 3], 256), ([256, 64, 16], 1024), ([30, 1, 1], 1)]


@pytest.mark.parametrize("widths,batch", MUST_SERVE + [([30, 128, 128, 3], 256)])
def test_the_plan_fits_is_aligned_and_disjoint_and_takes_the_tallest_tile(plan, widths, batch):
    lines = plan(widths, batch)
    assert lines[0][0] == "ok", lines
    lds, tile, tiles = (int(x) for x in lines[0][1:4])
    assert lds <= LDS_LIMIT and tile in (16, 32, 64, 128) and tiles == -(-batch // tile)
    assert all(int(l[1]) % 16 == 4 for l in lines if l[0] == "stride")     # 4 mod 16: the bank argument of osg_adam_plan.h
    bufs = sorted((int(l[1]), int(l[2])) for l in lines if l[0] == "buf")
    assert all(start % 4 == 0 for start, _ in bufs)                        # 16 bytes
    assert all(a + n <= b for (a, n), (b, _) in zip(bufs, bufs[1:])) and (bufs[-1][0] + bufs[-1][1]) * 4 <= lds
    # the tallest: one byte less than this form needs gives a lesser form or a lower tile
    assert plan(widths, batch, lds)[0][1:6] == lines[0][1:6]
    less = plan(widths, batch, lds - 1)[0]
    assert less[0] == "refused" or (int(less[2]), int(less[4]), int(less[5])) < (tile, *map(int, lines[0][4:6]))


def test_the_plan_refuses_with_a_reason_and_says_where_the_wide_network_lands(plan):
    for widths, batch in (([30, 256, 256, 3], 256), ([30, 129, 3], 8), ([257, 8, 3], 8), ([30, 8, 17], 8), ([30, 8, 3], 1025), ([30, 8, 3], 0)):
        line = plan(widths, batch)[0]
        assert line[0] == "refused" and len(line) > 3, line
    wide = plan([30, 128, 128, 3], 256)[0]
    assert wide[2:6] == ["32", "8", "0", "0"]       # (128, 128): tiles of 32 rows, no transposed copies, moments in global memory
    assert plan([30, 64, 3], 256)[0][2:6] == ["128", "2", "1", "1"] and plan([30, 128, 3], 1024)[0][2] == "64"
    assert plan([30, 64, 3], 17)[0][2] == "32" and plan([30, 64, 3], 1)[0][2] == "16"   # no taller than the batch needs
    assert plan([30, 64, 3], 256, 20 * 1024)[0][0] == "refused"
