"""Extensive-form regret minimization against the reference's own efr.py (tests/golden/efr_vectors.npz, made by
tests/golden/make_efr_vectors.py): the restatement of open_spiel_amd/csrc/osg_efr.h in tests/efr_cases.py — the header's
items in the header's orders, in Python floats — builds the reference's deviation tables exactly and reproduces every
checkpoint (R per deviation, current, cumulative and average policy) within efr_cases.TOLERANCE (100 x the measured
largest deviation of the host program; module docstring of efr_cases), and every regret-matching unit case with the
rank LAPACK found.  The `blind cf` runs equal the reference cfr.py's simultaneous-update CFR."""
import numpy as np
import pytest

import efr_cases as ec


def _tables_equal_the_reference(v, r, T):
    assert np.array_equal(np.diff(T["dev_off"]), v[f"r{r}/dev_count"])
    assert np.array_equal(T["target"], v[f"r{r}/dev_target"])
    assert np.array_equal(T["source"], v[f"r{r}/dev_source"])
    assert np.array_equal(np.array(T["source"]) < 0, v[f"r{r}/dev_external"] == 1)
    none = v[f"r{r}/dev_weights_none"]
    assert np.array_equal(T["none"], none)
    assert np.array_equal(np.array(T["weights"]), v[f"r{r}/dev_weights"])
    # (with the `None` weights the reference holds zeros or the history as memory, and reads neither)
    assert np.array_equal(np.array(T["memory"])[none == 0], v[f"r{r}/dev_memory"][none == 0])


@pytest.mark.parametrize("r", range(len(ec.run_ids())), ids=ec.run_ids())
def test_restatement_reproduces_tables_and_every_checkpoint(r):
    v = ec.load()
    _, game, name = ec.runs(v)[r]
    lay = ec.layout(v, r, game)
    assert ec.keys_of(v, r) == ec.keys_of(v, [q for q, g, _ in ec.runs(v) if g == game][0])
    T = ec.build_tables(lay, ec.TYPES.index(name))
    _tables_equal_the_reference(v, r, T)
    s = ec.State(lay, T)
    done, largest = 0, 0.0
    for c, upto in enumerate(v[f"r{r}/checkpoints"]):
        while done < upto:
            ec.iterate(lay, T, s)
            done += 1
        got = dict(R=np.array(s.R), cur=np.array(s.pol), cum=np.array(s.cum), avg=s.average(lay))
        for k, mine in got.items():
            want = v[f"r{r}/R"][c] if k == "R" else ec.by_legal(v, r, v[f"r{r}/{k}"][c])
            d = float(np.max(np.abs(mine - want)))
            largest = max(largest, d)
            assert d <= ec.TOLERANCE, f"{k} after {upto} iterations deviates by {d}"
    print(f"{game} | {name}: largest deviation {largest:.3g}")
    if name == "blind cf":
        for k in ("avg", "cur", "cum"):
            want = ec.by_legal(v, r, v[f"cfr/{game}/{k}"])
            d = float(np.max(np.abs(got[k] - want)))
            print(f"   against cfr.py, {k}: {d:.3g}")
            assert d <= ec.TOLERANCE


def test_every_regret_matching_case_with_the_rank_equal():
    v = ec.load()
    n = len(v["rm/A"])
    assert n >= 300
    largest, deficient = 0.0, 0
    for j in range(n):
        A, nk = int(v["rm/A"][j]), int(v["rm/nkeys"][j])
        keys = [int(v["rm/key_target"][j, k]) | ((int(v["rm/key_source"][j, k]) + 1) << 4) for k in range(nk)]
        row, rank = ec.regret_match(A, keys, [float(x) for x in v["rm/y"][j, :nk]], bool(v["rm/external_only"][j]))
        assert rank == v["rm/rank"][j], f"case {j}: rank {rank}, LAPACK found {v['rm/rank'][j]} (singular values {v['rm/sv'][j]})"
        deficient += 0 <= rank < A
        d = float(np.max(np.abs(np.array(row) - v["rm/out"][j, :A])))
        largest = max(largest, d)
        assert d <= ec.TOLERANCE, f"case {j} deviates by {d}"
    assert deficient >= 20
    print(f"{n} cases, {deficient} rank-deficient, largest deviation {largest:.3g}")
