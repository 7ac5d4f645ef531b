"""tests/golden/minimax_vectors.npz (tests/golden/make_minimax_vectors.py): the sets the device tests compare against are
there with consistent shapes; where the reference sources are present, re-running the reference's own minimax.py over a
seeded sample of every set reproduces the file exactly; the C-ABI entry is declared, bound and exported; and a program
that calls algorithms::AlphaBetaSearch through include/open_spiel/algorithms/minimax.h compiles against the mirror."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = ("game", "histories", "depth_limit", "leaf_mode", "leaf_value", "maximizing_player", "value", "best_action", "nodes", "status")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_minimax_vectors", os.path.join(GOLDEN, "make_minimax_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def vectors():
    path = os.path.join(GOLDEN, "minimax_vectors.npz")
    assert os.path.getsize(path) < (1 << 20)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_every_set_is_recorded_with_consistent_shapes(gen, vectors):
    assert set(vectors) == {f"{name}/{f}" for name in gen.SETS for f in FIELDS}
    for name, spec in gen.SETS.items():
        s = {f: vectors[f"{name}/{f}"] for f in FIELDS}
        n = len(s["status"])
        assert n == (spec["first"] if "opp" in spec else spec["n"] + len(spec.get("fixed", []))), name
        assert bytes(s["game"]).decode() == spec["game"]
        assert s["histories"].dtype == np.int16 and s["histories"].shape[0] == n
        assert int(s["depth_limit"]) == spec["depth"] and int(s["leaf_mode"]) == (0 if spec["leaf"] is None else 1)
        assert float(s["leaf_value"]) == (spec["leaf"] or 0.0)
        for f, dt in (("maximizing_player", np.int8), ("value", np.float64), ("best_action", np.int32), ("nodes", np.int64),
                      ("status", np.uint8)):
            assert s[f].dtype == dt and s[f].shape == (n,), (name, f)
        done = s["status"] == 0
        assert set(np.unique(s["status"])) <= {0, 1} and (spec["leaf"] is None or done.all())
        assert np.isnan(s["value"][~done]).all() and (s["best_action"][~done] == -1).all()
        assert (s["nodes"][done] >= 1).all() and np.isfinite(s["value"][done]).all()
        plies = (s["histories"] >= 0).sum(axis=1)
        assert ((s["histories"] >= 0) == (np.arange(s["histories"].shape[1])[None, :] < plies[:, None])).all()   # padded at the end
        if "opp" in spec:
            assert np.array_equal(s["maximizing_player"], 1 - plies % 2)
            assert np.array_equal(s["histories"], vectors[f"{spec['opp']}/histories"][:n, :s["histories"].shape[1]])
        else:
            assert (s["maximizing_player"] == -1).all()
        assert (plies >= spec.get("min_plies", 0)).all()


def test_the_recorded_results_are_the_known_ones(vectors):
    """The reference's own test positions (minimax_test.cc: 0, 1, -1) and node counts of known trees."""
    v = vectors
    assert v["ttt_full/value"][:3].tolist() == [0.0, 1.0, -1.0]
    assert v["ttt_full/histories"][1, :2].tolist() == [4, 1] and v["ttt_full/histories"][2, :4].tolist() == [5, 4, 3, 8]
    assert (int(v["ttt_full/best_action"][0]), int(v["ttt_full/nodes"][0]), int(v["ttt_full/nodes"][1])) == (0, 18297, 383)
    assert (float(v["ttt_d1_c0/value"][0]), int(v["ttt_d1_c0/nodes"][0])) == (0.0, 10)
    assert v["ttt_d3_none/status"][0] == 1
    assert int(v["c4_d6_c0/nodes"][0]) == 1249 and v["c4_d8_c0/nodes"][:2].tolist() == [12574, 15224]
    assert (float(v["c4_5x5_d10_c025/value"][0]), int(v["c4_5x5_d10_c025/nodes"][0])) == (0.25, 17131)
    assert (float(v["hex3_full/value"][0]), int(v["hex3_full/best_action"][0]), int(v["hex3_full/nodes"][0])) == (1.0, 2, 11703)
    assert int(v["hex4_d6_c0/nodes"][0]) == 8417
    # sets that mix finished roots with roots that reach the depth limit without a leaf value, and terminal roots
    for name in ("ttt_d1_none", "ttt_d2_none", "ttt_d3_none"):
        assert 0 < int((v[f"{name}/status"] == 1).sum()) < len(v[f"{name}/status"])
    assert ((v["ttt_full/nodes"] == 1) & (v["ttt_full/best_action"] == -1)).sum() > 50


@pytest.mark.parametrize("name", [
    "ttt_full", "ttt_full_opp", "ttt_d1_none", "ttt_d2_none", "ttt_d3_none", "ttt_d1_c0", "ttt_d4_c025",
    "c4_d6_c0", "c4_d6_c0_opp", "c4_d8_c0", "c4_5x5_d10_c025", "c4_8x8_d5_c0",
    "hex3_full", "hex3_full_opp", "hex4_d6_c0", "hex4_full_6plus", "hex5_swap_d4_c0", "hex9_d3_c0"])
def test_rerunning_the_reference_reproduces_a_sample(gen, vectors, reference, name):
    if not reference.sources_present():
        pytest.skip("needs the reference sources")
    n = len(vectors[f"{name}/status"])
    # a seeded sample among the cheaper half of the set (the file records what every case cost), and case 0
    cheap = np.argsort(vectors[f"{name}/nodes"], kind="stable")[:max(1, n // 2)]
    sample = sorted({0} | set(np.random.RandomState(len(name)).choice(cheap, size=min(12, len(cheap)), replace=False).tolist()))
    again = gen.reference_set(name, sample)
    for f in FIELDS:
        want = vectors[f"{name}/{f}"]
        if f == "histories":
            want = want[sample][:, :again[f].shape[1]]
            assert (vectors[f"{name}/{f}"][sample][:, again[f].shape[1]:] == -1).all()
        elif f in ("maximizing_player", "value", "best_action", "nodes", "status"):
            want = want[sample]
        assert np.array_equal(again[f], want, equal_nan=(f == "value")), (name, f)


def test_the_abi_entry_is_declared_bound_and_exported():
    from open_spiel_amd import _abi
    assert "osg_alpha_beta_search" in _abi.SIGNATURES
    assert [f[0] for f in _abi.AbCfg._fields_] == ["depth_limit", "maximizing_player", "leaf_mode", "leaf_value", "max_nodes"]
    with open(os.path.join(ROOT, "include", "osg_abi.h")) as f:
        header = f.read()
    assert "int osg_alpha_beta_search(const osg_batch* roots, const osg_ab_cfg* cfg, double* value, int32_t* best_action," in header
    assert "minimax.cc" in header
    import __graft_entry__ as ge
    ge.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T osg_alpha_beta_search" in out
    assert ctypes.sizeof(_abi.AbCfg) == 32


def test_a_program_calling_alpha_beta_search_compiles_against_the_mirror(tmp_path):
    """Compile only (running needs the device: tests/test_z14_gpu_minimax.py)."""
    import __graft_entry__ as ge
    ge.build()
    lib_dir = os.path.join(ROOT, "open_spiel_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "minimax_on_mirror_test.cpp"),
                           "-o", str(tmp_path / "minimax_on_mirror_test"), "-L", lib_dir, "-losg_hip", f"-Wl,-rpath,{lib_dir}"])
