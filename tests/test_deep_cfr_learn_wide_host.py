"""CPU checks of the wide fused Deep CFR learner's planner (csrc/osg_adam_wide_plan.h) through a small stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adam_wide_plan") / "adam_wide_plan_host_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"), os.path.join(ROOT, "tests", "native", "adam_wide_plan_host_test.cpp"), "-o", exe])

    def run(widths, batch, limit=LDS_LIMIT):
        out = subprocess.check_output([exe, str(len(widths) - 1), *map(str, widths), str(batch), str(limit)], text=True)
        return [line.split() for line in out.splitlines()]
    return run


@pytest.mark.parametrize("widths,batch", [([30, 256, 256, 3], 256), ([30, 256, 256, 3], 1024), ([30, 512, 3], 1024), ([11, 129, 2], 17),
                                          ([30, 20, 3], 17), ([256, 512, 512, 16], 1024), ([30, 1, 1], 1)])
def test_the_plan_fits_is_aligned_and_disjoint_and_covers_the_batch(plan, widths, batch):
    lines = plan(widths, batch)
    assert lines[0][0] == "ok", lines
    lds, R, G, scratch, params, partial_stride, piece = (int(x) for x in lines[0][1:8])
    assert lds <= LDS_LIMIT and R % 16 == 0 and R >= 16 and 1 <= G <= 64 and G * R >= batch > (G - 1) * R
    assert all(int(l[1]) % 16 == 4 for l in lines if l[0] == "stride")     # 4 mod 16: the bank argument of osg_adam_wide_plan.h
    bufs = sorted((int(l[1]), int(l[2])) for l in lines if l[0] == "buf")
    assert all(start % 4 == 0 for start, _ in bufs)                        # 16 bytes
    assert all(a + n <= b for (a, n), (b, _) in zip(bufs, bufs[1:])) and (bufs[-1][0] + bufs[-1][1]) * 4 <= lds
    assert params == sum(o * i + o for i, o in zip(widths, widths[1:])) + 2 * widths[-2]
    assert partial_stride >= params + 2 and scratch >= 256 + 4 * G * partial_stride and G * piece >= params   # the slices cover every parameter
    assert plan(widths, batch) == lines                                    # a pure function of its arguments
    assert plan(widths, batch, lds)[0] == lines[0]                         # ... which takes the most rows that fit


def test_the_plan_refuses_with_a_reason_and_says_where_the_default_network_lands(plan):
    for widths, batch, limit in (([30, 513, 3], 8, LDS_LIMIT), ([30, 8, 3], 1025, LDS_LIMIT), ([30, 8, 3], 0, LDS_LIMIT), ([30, 8, 17], 8, LDS_LIMIT),
                                 ([30, 256, 256, 3], 256, 20 * 1024)):
        line = plan(widths, batch, limit)[0]
        assert line[0] == "refused" and len(line) > 3, line
    assert plan([30, 256, 256, 3], 256)[0][2:4] == ["32", "8"] and plan([30, 256, 256, 3], 1024)[0][2:4] == ["32", "32"]
    assert plan([30, 20, 3], 65)[0][2:4] == ["64", "2"] and plan([30, 20, 3], 17)[0][2:4] == ["32", "1"]   # no more rows than the batch needs
