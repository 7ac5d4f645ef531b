"""Extensive-form fictitious play, the parts that need no device: the three C-ABI entry points are declared, exported and
bound with the stated signatures, the layout of osg_cfr_cfg did not change for them, and XFPSolver is exported with the
reference's surface."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "osg_xfp_iterate": (r"osg_cfr\s*\*\s*s\s*,\s*int\s+iters", [C.c_void_p, C.c_int]),
    "osg_xfp_update": (r"osg_cfr\s*\*\s*s\s*,\s*const\s+int32_t\s*\*\s*h_best_index", [C.c_void_p, C.c_void_p]),
    "osg_xfp_reaches": (r"osg_cfr\s*\*\s*s\s*,\s*const\s+int32_t\s*\*\s*h_best_index\s*,\s*double\s*\*\s*h_avg_reach\s*,"
                        r"\s*double\s*\*\s*h_br_reach", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import open_spiel_amd
    return open_spiel_amd


def test_entry_points_are_declared_exported_and_bound(built):
    from open_spiel_amd import _abi
    header = open(os.path.join(ROOT, "include", "osg_abi.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    handle = C.CDLL(_abi.LIB_PATH)
    for name, (params, argtypes) in SIGNATURES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, params), header), f"{name} is not declared as stated"
        assert _abi.SIGNATURES[name] == (C.c_int, argtypes)
        assert hasattr(handle, name), f"libosg_hip.so does not export {name}"
    # the layout of osg_cfr_cfg did not change for it
    assert [f[0] for f in _abi.CfrCfg._fields_] == [
        "alternating_updates", "linear_averaging", "regret_matching_plus", "solver", "epsilon", "kernel", "replicas",
        "random_initial_regrets", "seed", "replica_offset"]
    assert C.sizeof(_abi.CfrCfg) == 56


def test_the_header_states_the_kernel_names(built):
    header = open(os.path.join(ROOT, "include", "osg_abi.h")).read()
    for name in ("k_xfp_small", "k_xfp<k_policy_eval>", "k_xfp<k_eval_jobs>", "k_xfp<k_geval>", "k_xfp_update"):
        assert f'"{name}"' in header, name
    source = open(os.path.join(ROOT, "open_spiel_amd", "csrc", "osg_cfr_xfp.hip")).read()
    for name in ("k_xfp_small", "k_xfp<k_policy_eval>", "k_xfp<k_eval_jobs>", "k_xfp<k_geval>", "k_xfp_update"):
        assert f'"{name}"' in source, name


def test_xfp_solver_is_exported_with_the_reference_surface(built):
    import open_spiel_amd as osa
    from open_spiel_amd import engine
    assert osa.XFPSolver is engine.XFPSolver and issubclass(engine.XFPSolver, engine.TabularSolver)
    params = inspect.signature(engine.XFPSolver.__init__).parameters
    assert list(params)[:3] == ["self", "ctx", "game_string"]
    # XFP has no parameters: beyond the game only the kernel-form switch of the cross-checks
    assert [k for k in params if k not in ("self", "ctx", "game_string")] == ["general_kernel"]
    for name in ("iteration", "iterate", "best_responses", "update", "reaches", "average_policy", "average_policy_tables",
                 "nash_conv", "exploitability"):
        assert callable(getattr(engine.XFPSolver, name)), name
    assert inspect.signature(engine.XFPSolver.reaches).parameters["best_index"].default is None
    assert inspect.signature(engine.XFPSolver.evaluate_policy).parameters["which"].default == "current"

    made = []

    def fake_init(self, ctx, game_string, **kw):   # what the thin class hands to TabularSolver
        made.append(kw)

    real = engine.TabularSolver.__init__
    engine.TabularSolver.__init__ = fake_init
    try:
        engine.XFPSolver(None, "kuhn_poker")
        engine.XFPSolver(None, "leduc_poker", general_kernel="grid")
    finally:
        engine.TabularSolver.__init__ = real
    plain = dict(alternating_updates=True, linear_averaging=False, regret_matching_plus=False)
    assert made == [dict(plain, general_kernel=False), dict(plain, general_kernel="grid")]
