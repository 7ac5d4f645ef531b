"""StateBatch.step's native fast path (open_spiel_amd/_osg_step_fast, csrc/host/osg_step_fast.cc) against the same
step in Python (StateBatch._step_py): the extension is built and used, gives bit-identical successors, masks and
status words, and refuses every argument the Python body refuses, with the same text, before anything is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- CPU --------------------------------------------------------------------------------------------------------------
def test_extension_imports_and_engine_uses_it():
    from open_spiel_amd import _osg_step_fast, engine
    if os.environ.get("OSG_STEP_PY") == "1":
        assert engine._native_step is None
    else:
        assert engine._native_step is _osg_step_fast


def test_osg_step_py_switch_selects_the_python_body():
    code = ("import open_spiel_amd.engine as e; import sys; "
            "sys.exit(0 if (e._native_step is None) == (sys.argv[1] == '1') else 1)")
    for value in ("1", "0"):
        env = dict(os.environ, OSG_STEP_PY=value)
        assert subprocess.run([sys.executable, "-c", code, value], cwd=ROOT, env=env).returncode == 0, value


def test_refusals_before_any_launch_match_the_python_text():
    """CPU tensors and non-tensors are refused by the native checks before osg_step is reached (no device needed)."""
    import ctypes as C
    import torch
    from open_spiel_amd import _osg_step_fast as fast
    from open_spiel_amd import engine
    from open_spiel_amd._abi import OsgError, lib
    fast.bind(OsgError, engine._bad_tensor_message, torch.uint8, torch.device,
              C.cast(lib().osg_step, C.c_void_p).value, C.cast(lib().osg_last_error, C.c_void_p).value)
    assert fast.bound()
    n, dev = 8, torch.device("cuda", 0)
    cpu = torch.zeros(n, dtype=torch.uint8)
    fake_h = 1   # never dereferenced: every call below is refused first
    for args, what, t, numel in (
            ((cpu, None, cpu), "step(status=)", cpu, n),
            ((cpu, cpu, cpu), "step(mask=)", cpu, 2 * n),
            ((np.zeros(n, np.uint8), None, cpu), "step(status=)", cpu, n)):
        with pytest.raises(OsgError) as e:
            fast.step(fake_h, fake_h, n, n, "connect_four", "connect_four", *args, 2, 0)
        assert str(e.value) == engine._bad_tensor_message(t, torch.uint8, numel, what, dev)
    with pytest.raises(OsgError, match="closed"):
        fast.step(0, fake_h, n, n, "connect_four", "connect_four", cpu, None, cpu, 2, 0)
    with pytest.raises(TypeError):
        fast.step(fake_h, fake_h, n)


# -- GPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import open_spiel_amd as osa
    return osa.Context(0)


def _start(ctx, game, n, seed):
    import open_spiel_amd as osa
    b = osa.StateBatch(ctx, game, n)
    b.random_steps(seed, 3)
    return b


def _actions(b, ply, n):
    import torch
    width = max(b.desc.num_distinct_actions, b.desc.max_chance_outcomes)
    g = torch.Generator().manual_seed(1000 + ply)
    a = torch.randint(0, width, (n,), generator=g, dtype=torch.int64)
    a[torch.rand(n, generator=g) < 0.05] = 255                       # skips
    return a.to(torch.uint8)


CASES = [  # (game, n, want_mask, side arrays offset by one byte)
    ("tic_tac_toe", 1000, True, False),
    ("connect_four", 4096, True, False),       # k_step_c4std2
    ("connect_four", 1001, True, False),       # odd: k_step_c4std
    ("connect_four", 4096, True, True),        # odd side-array addresses: k_step_c4std
    ("connect_four(rows=8,columns=8)", 512, True, False),
    ("hex(board_size=9)", 512, False, False),
    ("kuhn_poker", 600, True, False),
    ("leduc_poker", 600, True, False),
]


def _side(n, cmb, offset, want_mask):
    """(actions, mask, status) device buffers; with offset, each starts one byte into its allocation."""
    import torch
    o = 1 if offset else 0
    a = torch.empty(n + o, dtype=torch.uint8, device="cuda")[o:]
    m = torch.empty(n * cmb + o, dtype=torch.uint8, device="cuda")[o:] if want_mask else None
    s = torch.empty(n + o, dtype=torch.uint8, device="cuda")[o:]
    return a, m, s


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("game,n,want_mask,offset", CASES)
def test_fast_path_matches_python_body(ctx, game, n, want_mask, offset, in_place):
    fast_src = _start(ctx, game, n, 7)
    py_src = fast_src.clone()
    fast_dst, py_dst = (fast_src, py_src) if in_place else (fast_src.clone(), py_src.clone())
    cmb = fast_src.desc.compact_mask_bytes
    for ply in range(12):
        acts = _actions(fast_src, ply, n)
        if offset or ply % 2:    # the caller's buffers ...
            fa, fm, fs = _side(n, cmb, offset, want_mask)
            pa, pm, ps = _side(n, cmb, offset, want_mask)
            fa.copy_(acts)
            pa.copy_(acts)
            m1, s1 = fast_src.step(fa, dst=fast_dst, mask=fm, status=fs, want_mask=want_mask)
            m2, s2 = py_src._step_py(pa, dst=py_dst, mask=pm, status=ps, want_mask=want_mask)
            assert s1 is fs and m1 is fm
        else:                    # ... or the ones step() allocates
            a = acts.cuda()
            m1, s1 = fast_src.step(a, dst=fast_dst, want_mask=want_mask)
            m2, s2 = py_src._step_py(a, dst=py_dst, want_mask=want_mask)
        ctx.synchronize()
        assert np.array_equal(fast_dst.raw_words(), py_dst.raw_words()), ply
        assert np.array_equal(s1.cpu().numpy(), s2.cpu().numpy()), ply
        if want_mask:
            assert np.array_equal(m1.cpu().numpy().reshape(-1), m2.cpu().numpy().reshape(-1)), ply
        else:
            assert m1 is None and m2 is None
        if not in_place:          # next ply from the successors
            fast_src, fast_dst = fast_dst, fast_src
            py_src, py_dst = py_dst, py_src


def _both_raise(src, dst, *args, **kw):
    """step() and _step_py() refuse the call with the same OsgError text."""
    import open_spiel_amd as osa
    with pytest.raises(osa.OsgError) as fast:
        src.step(*args, dst=dst, **kw)
    with pytest.raises(osa.OsgError) as py:
        src._step_py(*args, dst=dst, **kw)
    assert str(fast.value) == str(py.value)
    return str(fast.value)


@pytest.mark.gpu
def test_invalid_arguments_raise_and_leave_both_batches_unchanged(ctx):
    import torch
    import open_spiel_amd as osa
    n = 64
    src = _start(ctx, "connect_four", n, 3)
    dst = _start(ctx, "connect_four", n, 4)
    a8 = _actions(src, 0, n).cuda()
    mask, status = src.step_buffers()
    before = src.raw_words(), dst.raw_words()
    bad_actions = [
        a8.to(torch.int32),                                              # wrong dtype
        a8.cpu(),                                                        # a CPU tensor
        a8[:-1],                                                         # wrong numel
        torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2],       # non-contiguous
        a8.cpu().numpy(),                                                # not a tensor
    ]
    for bad in bad_actions:
        assert "step(actions_u8)" in _both_raise(src, dst, bad, mask=mask, status=status)
    assert "step(mask=)" in _both_raise(src, dst, a8, mask=mask[:-1], status=status)
    assert "step(mask=)" in _both_raise(src, dst, a8, mask=mask.view(torch.int8), status=status)
    assert "step(status=)" in _both_raise(src, dst, a8, mask=mask, status=status.cpu())
    assert "step(status=)" in _both_raise(src, dst, a8, status=status[:-1], want_mask=False)
    for other in (osa.StateBatch(ctx, "connect_four", n // 2), osa.StateBatch(ctx, "tic_tac_toe", n),
                  osa.StateBatch(ctx, "connect_four(rows=8,columns=8)", n)):
        assert "dst=" in _both_raise(src, other, a8, mask=mask, status=status)
    ctx.synchronize()
    assert np.array_equal(src.raw_words(), before[0]) and np.array_equal(dst.raw_words(), before[1])

    closed = _start(ctx, "connect_four", n, 5)
    closed.close()
    closed.close()                                 # (idempotent)
    assert "closed" in _both_raise(closed, dst, a8, mask=mask, status=status)
    assert "closed" in _both_raise(src, closed, a8, mask=mask, status=status)
    ctx.synchronize()
    assert np.array_equal(src.raw_words(), before[0]) and np.array_equal(dst.raw_words(), before[1])


@pytest.mark.gpu
def test_native_error_code_carries_the_library_message(ctx):
    """A refusal by osg_step itself (a non-hex game without a mask) raises OsgError with osg_last_error()."""
    import torch
    import open_spiel_amd as osa
    b = osa.StateBatch(ctx, "connect_four", 64)
    a8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(osa.OsgError) as fast:
        b.step(a8, want_mask=False)
    with pytest.raises(osa.OsgError) as py:
        b._step_py(a8, want_mask=False)
    assert str(fast.value) == str(py.value) and "osg error" in str(fast.value) and "d_mask may be NULL" in str(fast.value)
