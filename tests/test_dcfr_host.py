"""Discounted CFR, the parts that need no device: the two C-ABI entry points are declared, exported and bound; the
factors osg_cfr_discount_factors returns — the ones the kernels are handed — equal the reference's Python expressions
(discounted_cfr.py:184,203-208) bit for bit; and the Python entry points carry the reference's defaults."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the exponents as the reference passes them: DCFRSolver's defaults (a float and two ints), LCFRSolver's ints, floats
PARAMETER_SETS = {"D": (3 / 2, 0, 2), "L": (1, 1, 1), "X": (1.5, 0.5, 3)}
ITERATIONS = [1, 2, 3, 10, 1000, 10**6]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import open_spiel_amd
    return open_spiel_amd


def _factors(lib, alpha, beta, gamma, t):
    out = (C.c_double * 3)()
    rc = lib.osg_cfr_discount_factors(alpha, beta, gamma, t, out)
    return rc, list(out)


def test_entry_points_are_declared_exported_and_bound(built):
    from open_spiel_amd import _abi
    header = open(os.path.join(ROOT, "include", "osg_abi.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    handle = C.CDLL(_abi.LIB_PATH)
    for name in ("osg_cfr_set_discounting", "osg_cfr_discount_factors"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/osg_abi.h"
        assert name in _abi.SIGNATURES
        assert hasattr(handle, name), f"libosg_hip.so does not export {name}"
    assert _abi.SIGNATURES["osg_cfr_set_discounting"] == (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double])
    assert _abi.SIGNATURES["osg_cfr_discount_factors"][1][:4] == [C.c_double, C.c_double, C.c_double, C.c_int]
    # the layout of osg_cfr_cfg did not change for it
    assert [f[0] for f in _abi.CfrCfg._fields_] == [
        "alternating_updates", "linear_averaging", "regret_matching_plus", "solver", "epsilon", "kernel", "replicas",
        "random_initial_regrets", "seed", "replica_offset"]
    assert C.sizeof(_abi.CfrCfg) == 56


@pytest.mark.parametrize("name", list(PARAMETER_SETS))
@pytest.mark.parametrize("t", ITERATIONS)
def test_factors_equal_the_reference_expressions_bit_for_bit(built, name, t):
    alpha, beta, gamma = PARAMETER_SETS[name]
    rc, got = _factors(built.lib(), alpha, beta, gamma, t)
    assert rc == 0
    want = [t**alpha / (t**alpha + 1), t**beta / (t**beta + 1), float(t**gamma)]
    assert [x.hex() for x in got] == [float(x).hex() for x in want], (name, t, got, want)


@pytest.mark.parametrize("bad", [(-1.0, 0, 2), (1.5, -0.5, 2), (1.5, 0, -2.0), (math.nan, 0, 2), (1.5, math.inf, 2),
                                 (1.5, 0, -math.inf)])
def test_factors_refuse_bad_exponents(built, bad):
    rc, _ = _factors(built.lib(), *bad, 5)
    assert rc == -1   # OSG_ERR_INVALID
    assert "finite and non-negative" in built.lib().osg_last_error().decode()


@pytest.mark.parametrize("t", [0, -3])
def test_factors_refuse_iterations_below_one(built, t):
    rc, _ = _factors(built.lib(), 1.5, 0, 2, t)
    assert rc == -1
    assert "count from 1" in built.lib().osg_last_error().decode()


def test_python_entry_points_carry_the_reference_defaults(built):
    import open_spiel_amd as osa
    from open_spiel_amd import engine
    assert osa.DCFRSolver is engine.DCFRSolver and osa.LCFRSolver is engine.LCFRSolver
    assert issubclass(engine.DCFRSolver, engine.TabularSolver) and issubclass(engine.LCFRSolver, engine.TabularSolver)
    sig = inspect.signature(engine.DCFRSolver.__init__)
    assert [(k, sig.parameters[k].default) for k in ("alpha", "beta", "gamma")] == [("alpha", 1.5), ("beta", 0), ("gamma", 2)]
    assert inspect.signature(engine.TabularSolver.__init__).parameters["discounting"].default is None
    assert callable(engine.TabularSolver.set_discounting)

    made = []

    def fake_init(self, ctx, game_string, **kw):   # what the thin classes hand to TabularSolver
        made.append(kw)

    real = engine.TabularSolver.__init__
    engine.TabularSolver.__init__ = fake_init
    try:
        engine.DCFRSolver(None, "kuhn_poker", replicas=4, seed=7, general_kernel="grid")
        engine.LCFRSolver(None, "kuhn_poker")
    finally:
        engine.TabularSolver.__init__ = real
    assert made[0] == dict(alternating_updates=True, linear_averaging=True, regret_matching_plus=False,
                           discounting=(1.5, 0, 2), replicas=4, seed=7, general_kernel="grid")
    assert made[1] == dict(alternating_updates=True, linear_averaging=True, regret_matching_plus=False, discounting=(1, 1, 1))
