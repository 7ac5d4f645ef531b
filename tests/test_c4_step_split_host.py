"""The body of k_step_c4std2 / k_step_c4std as the kernels run it (open_spiel_amd/csrc/step/osg_c4_step_split.h:
c4_place + c4_finish on the planes' 32-bit halves, the o plane final between the two) against c4_fused_step
(osg_c4_step.h) on the CPU: bit-identical planes, mask and status on every move of 200 000 random games played to
the end, with "no action", an action >= 7 and a move into every full column fed to every position and finished
games stepped again.  The program fails if it met no win in one of the four directions, no draw at 42 stones or no
full-column refusal.  Run once as built for speed and once under -fsanitize=undefined (a plain host program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=undefined", "-fno-sanitize-recover"]],
                         ids=["plain", "ubsan"])
def test_split_step_equals_the_fused_step(tmp_path, flags):
    exe = str(tmp_path / "c4_step_split_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-w", *flags,
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "c4_step_split_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert r.stdout.startswith("ok: 200000 games") and "runtime error" not in r.stderr
