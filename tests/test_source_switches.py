"""No compile-time A/B switches in the native sources: a preprocessor conditional that names an OSG_* macro is either a
header's include guard or one of the instrumentation builds below, whose results are those of the shipped build.
A kernel experiment is compared as two library builds (OSG_VARIANT_LIB), not kept behind a -D flag.

Nor launch ladders written in the preprocessor: which template instantiation a launch takes is chosen by the functions
of osg_internal.h (for_game, for_hex, with_bool, with_int), so the only function-like OSG_* macros are the error return
and the instrumentation hook."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_spiel_amd", "csrc")
INSTRUMENTATION = {"OSG_PHASE_TIMING", "OSG_MCTS_PROFILE"}
CONDITIONAL = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")
DIRECTIVE = re.compile(r"^\s*#\s*(\w+)\s*(\w*)")
FUNCTION_MACROS = {"OSG_HIP", "OSG_PROF"}
FUNCTION_MACRO = re.compile(r"^\s*#\s*define\s+(OSG_\w+)\(")


def _include_guard(lines):
    """NAME when the file's first two directives are `#ifndef NAME` / `#define NAME`."""
    directives = [m.groups() for m in map(DIRECTIVE.match, lines) if m][:2]
    if len(directives) == 2 and directives[0][0] == "ifndef" and directives[1] == ("define", directives[0][1]):
        return directives[0][1]
    return None


def _sources():
    sources = [p for ext in ("hip", "h", "cc", "cpp") for p in glob.glob(os.path.join(CSRC, "**", f"*.{ext}"), recursive=True)]
    assert sources
    return sorted(sources)


def test_no_osg_switches_in_preprocessor_conditionals():
    found = []
    for path in _sources():
        with open(path) as f:
            lines = f.read().splitlines()
        allowed = INSTRUMENTATION | {_include_guard(lines)}
        for no, line in enumerate(lines, 1):
            m = CONDITIONAL.match(line)
            if m and set(re.findall(r"\bOSG_\w+", m.group(1))) - allowed:
                found.append(f"{os.path.relpath(path, ROOT)}:{no}: {line.strip()}")
    assert not found, "compile-time switches on OSG_* macros:\n" + "\n".join(found)


def test_no_function_like_osg_macros():
    found = []
    for path in _sources():
        with open(path) as f:
            for no, line in enumerate(f.read().splitlines(), 1):
                m = FUNCTION_MACRO.match(line)
                if m and m.group(1) not in FUNCTION_MACROS:
                    found.append(f"{os.path.relpath(path, ROOT)}:{no}: {line.strip()}")
    assert not found, "launch ladders as macros (use for_game / for_hex / with_bool / with_int):\n" + "\n".join(found)
