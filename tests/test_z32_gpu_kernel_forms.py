"""Which launch form every tabular entry point takes under every osg_cfr_cfg.kernel value and evaluation switch, against
the forms recorded in tests/golden/kernel_forms.json from the library BEFORE the choice moved behind the choosers of
csrc/osg_cfr_internal.h (eval_form, eval_form_for_kernel_option, cfr_iterate_form, cfr_br_iterate_form): the matrix the
family tests leave unpinned.

  games           kuhn_poker, leduc_poker (3-player leduc_poker: tests/test_gpu_cfr.py and tests/test_z13_gpu_dcfr.py)
  general_kernel  False, True, "grid", "path", "split", "sub"
  environment     none; OSG_EVAL_JOBS=0; OSG_EVAL_GRID=1; OSG_EVAL_GRID=0; OSG_EVAL_JOBS=0 with OSG_EVAL_GRID=1
                  (set on the live process: the library reads both at every call)
  calls           CALLS below, in that order, each group on a fresh solver

After each call (last_kernel(), last_eval_kernel()) is recorded, or the leading "osg error N" of a refusal (of the call, or
of the solver's construction: every call of the group then records it).  A call that names no kernel leaves what the
group's earlier calls named — or "" on a fresh solver, which is why CFR-BR starts a group of its own: its one-workgroup
loop and plain k_cfr name none.  Only names and error codes are read.

Recording (from a library built of the tree before a change, on the device):
  OSG_VARIANT_LIB=<that libosg_hip.so> python tests/test_z32_gpu_kernel_forms.py tests/golden/kernel_forms.json

One test per (game, environment): 6 general_kernel values x 4 solvers.  Measured on an MI355X: 0.15 - 0.17 s per
leduc_poker test, 0.04 - 0.05 s per kuhn_poker test, 3.6 s for the file (1.8 s of it the context)."""
import contextlib
import json
import os
import re
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_forms.json")
GAMES = ["kuhn_poker", "leduc_poker"]
KERNELS = [False, True, "grid", "path", "split", "sub"]
SWITCHES = ("OSG_EVAL_JOBS", "OSG_EVAL_GRID")
ENVIRONMENTS = {
    "none": {},
    "jobs0": {"OSG_EVAL_JOBS": "0"},
    "grid1": {"OSG_EVAL_GRID": "1"},
    "grid0": {"OSG_EVAL_GRID": "0"},
    "jobs0-grid1": {"OSG_EVAL_JOBS": "0", "OSG_EVAL_GRID": "1"},
}
# (solver class, [(name of the call, the call)]): a fresh solver per group
CALLS = [
    ("TabularSolver", [("evaluate_and_update_policy(1)", lambda s: s.evaluate_and_update_policy(1)),
                       ("nash_conv()", lambda s: s.nash_conv())]),
    ("TabularSolver", [("evaluate_and_update_policy_cfr_br(1)", lambda s: s.evaluate_and_update_policy_cfr_br(1)),
                       ("action_values()", lambda s: s.action_values()),
                       ("action_values(responder=0)", lambda s: s.action_values(responder=0))]),
    ("XFPSolver", [("XFPSolver.iterate(1)", lambda s: s.iterate(1))]),
    ("DCFRSolver", [("DCFRSolver.evaluate_and_update_policy(1)", lambda s: s.evaluate_and_update_policy(1))]),
]


@contextlib.contextmanager
def switches(values):
    before = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            if k in values:
                os.environ[k] = values[k]
            else:
                os.environ.pop(k, None)
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _refusal(e):
    m = re.match(r"osg error -?\d+", str(e))
    if not m:
        raise e
    return m.group(0)


def forms_of(ctx, game, kernel):
    """{name of the call: [last_kernel, last_eval_kernel] or "osg error N"} of one (game, general_kernel) under the
    environment as it stands."""
    import open_spiel_amd as osa
    out = {}
    for cls, calls in CALLS:
        try:
            solver = getattr(osa, cls)(ctx, game, general_kernel=kernel)
        except osa.OsgError as e:
            out.update({name: _refusal(e) for name, _ in calls})
            continue
        for name, call in calls:
            try:
                call(solver)
                out[name] = [solver.last_kernel(), solver.last_eval_kernel()]
            except osa.OsgError as e:
                out[name] = _refusal(e)
    return out


def record(ctx):
    return {game: {label: {str(kernel): forms_of_under(ctx, game, kernel, values) for kernel in KERNELS}
                   for label, values in ENVIRONMENTS.items()} for game in GAMES}


def forms_of_under(ctx, game, kernel, values):
    with switches(values):
        return forms_of(ctx, game, kernel)


@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("label", list(ENVIRONMENTS))
@pytest.mark.parametrize("game", GAMES)
def test_kernel_forms(ctx, golden, game, label):
    names = [name for _, calls in CALLS for name, _ in calls]
    assert sorted(golden[game][label]) == sorted(str(k) for k in KERNELS)
    for kernel in KERNELS:
        want = golden[game][label][str(kernel)]
        assert sorted(want) == sorted(names)
        got = forms_of_under(ctx, game, kernel, ENVIRONMENTS[label])
        for name in names:
            assert got[name] == want[name], f"{game} general_kernel={kernel!r} {label}: {name}"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import open_spiel_amd as osa
    forms = record(osa.Context(0))
    with open(sys.argv[1], "w") as f:   # one line per (game, environment, general_kernel)
        games = [f' "{game}": {{\n' + ",\n".join(
            f'  "{label}": {{\n' + ",\n".join(f'   "{k}": {json.dumps(v, sort_keys=True)}' for k, v in sorted(by_kernel.items())) + "\n  }"
            for label, by_kernel in sorted(by_label.items())) + "\n }" for game, by_label in sorted(forms.items())]
        f.write("{\n" + ",\n".join(games) + "\n}\n")
