"""Shared by the solve tests: the goldens of tests/golden/solve_vectors.npz (tests/golden/make_solve_vectors.py) and
the reference's board strings."""
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "solve_vectors.npz")
SEP = "\x1e"

_cache = {}


def load():
    if "v" not in _cache:
        _cache["v"] = np.load(GOLDEN)
    return _cache["v"]


def solve_cases():
    return str(load()["cases"]).split("\n")


def enum_cases():
    return str(load()["enum_cases"]).split("\n")


def field(case, name):
    a = load()[f"{case}/{name}"]
    return a if a.ndim else a.item()


def keys(case):
    """The sorted state strings of a case that keeps them, else None."""
    return str(load()[f"{case}/keys"]).split(SEP) if f"{case}/keys" in load().files else None


def sha256_of(sorted_strings):
    return hashlib.sha256(SEP.join(sorted_strings).encode()).hexdigest()


def stones(s):
    return s.count("x") + s.count("o")


def ttt_string(cells):
    """TicTacToeState::ToString (tic_tac_toe.cc:150-160): three rows of three cells."""
    return "\n".join(cells[3 * r:3 * r + 3] for r in range(3))


def hex_string(cells, rows, cols):
    """HexState::ToString (hex.cc:331-360): row r indented by r spaces, a space after every cell."""
    return "\n".join(" " * r + "".join(c + " " for c in cells[r * cols:(r + 1) * cols]) for r in range(rows))


def build_host_test(exe):
    """tests/native/solve_host_test.cpp as a plain executable with the address and undefined-behaviour sanitizers."""
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O1", "-g", "-w",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "solve_host_test.cpp"), "-o", exe])
    return exe


def render_strings(game_kind, raw, rows, cols):
    """State::ToString() of every state of a batch from its raw SoA words ([state_words, n], StateBatch.raw_words()) —
    what osg_state_string prints one state at a time, for the cases with 10^5 states.  connect_four
    (connect_four.cc:212-222: rows from the top, a newline after each) or hex (hex.cc:342-359)."""
    n = raw.shape[1]
    cells = np.full((n, rows, cols), ord("."), np.uint8)
    if game_kind == "connect_four":
        wide = (rows + 1) * cols > 64
        for r in range(rows):
            for c in range(cols):
                bit = c * (rows + 1) + r
                if wide:
                    x, o = raw[bit // 64], raw[2 + bit // 64]
                else:
                    x, o = raw[0], raw[1]
                cells[:, rows - 1 - r, c] = np.where((x >> np.uint64(bit % 64)) & np.uint64(1), ord("x"),
                                                     np.where((o >> np.uint64(bit % 64)) & np.uint64(1), ord("o"), ord(".")))
        text = np.concatenate([cells, np.full((n, rows, 1), ord("\n"), np.uint8)], axis=2).reshape(n, -1)
    else:
        nw = (rows * cols + 31) // 32   # words per plane: black at [0, nw), white at [nw, 2 nw); only bits below the
        for r in range(rows):           # cell count are read (a folded record keeps meta bits above them)
            for c in range(cols):
                cell = r * cols + c
                black, white, bit = raw[cell // 32], raw[nw + cell // 32], np.uint32(cell % 32)
                cells[:, r, c] = np.where((black >> bit) & np.uint32(1), ord("x"),
                                          np.where((white >> bit) & np.uint32(1), ord("o"), ord(".")))
        parts = []
        for r in range(rows):
            if r:
                parts.append(np.full((n, 1), ord("\n"), np.uint8))
                parts.append(np.full((n, r), ord(" "), np.uint8))
            row = np.full((n, cols, 2), ord(" "), np.uint8)
            row[:, :, 0] = cells[:, r, :]
            parts.append(row.reshape(n, -1))
        text = np.concatenate(parts, axis=1)
    text = np.ascontiguousarray(text)
    return [bytes(t).decode() for t in text]
