"""The scalar side of the plane form of the dense gap loop (abd_dense.hpp: dense_walk_planes; abd_planes.hpp:
abd_plane_first_pair, abd_row_off_next) on the CPU: for every row length G in 1 .. 70 and every piece [g0, g1) of it, every
gap a mask fetch touches lies inside the row's abd_plane_gaps(G) gaps, every gap is handed its own masks, and every refill of a
row buffer reads the row it is meant to, by its running offset."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plane_fetch_harness.cpp")
INC = os.path.join(ROOT, "abdpymc_amd", "csrc")

G_ALL = range(1, 71)
# one row in the offset's unit: the split panels' 64 cells, the pair panel's bytes at N = 70 and at the bench's N = 10 000
ROW_STEPS = [64, 70 * 16, 10000 * 16]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("plane_fetch") / "libplane_fetch_harness.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-fvisibility-inlines-hidden", "-Wl,-Bsymbolic", "-I", INC, SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    ip, llp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    lib.plane_fetch_gaps.argtypes = [C.c_int]
    lib.plane_fetch_first_pair.argtypes = [C.c_int]
    lib.plane_fetch_row_off_next.argtypes = [C.c_uint, C.c_uint, C.c_uint]
    lib.plane_fetch_row_off_next.restype = C.c_uint
    lib.plane_fetch_piece.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint, ip, llp]
    lib.plane_fetch_piece.restype = C.c_longlong
    lib.plane_fetch_all_pieces.argtypes = [C.c_int, C.c_uint, llp]
    lib.plane_fetch_all_pieces.restype = C.c_longlong
    return lib


def test_the_index_functions(harness):
    for g0 in range(0, 72):
        assert harness.plane_fetch_first_pair(g0) == g0 + (g0 & 1)
    for step in ROW_STEPS:
        for last in (0, 1, 2, 5):
            off = 0
            for r in range(1, 9):  # row r from row r - 1: min(r, last) rows in
                off = harness.plane_fetch_row_off_next(off, step, last * step)
                assert off == min(r, last) * step
    # the largest offsets a dense cohort can have (N * 16 * (G + 2) < 2^32): no wrap below the clamp
    step, last = 10_000_000 * 16, 24
    assert harness.plane_fetch_row_off_next((last - 1) * step, step, last * step) == last * step
    assert harness.plane_fetch_row_off_next(last * step, step, last * step) == last * step


@pytest.mark.parametrize("row_step", ROW_STEPS)
def test_every_piece_of_every_row(harness, row_step):
    out = (C.c_longlong * 4)()
    for G in G_ALL:
        bad = harness.plane_fetch_all_pieces(G, row_step, out)
        pieces, fetches, max_gap, clamped = out[0], out[1], out[2], out[3]
        assert bad == 0, f"G = {G}: {bad} violations"
        assert pieces == G * (G + 1) // 2
        # the last fetch of a row reads the pair after the last pair walked: gaps G, G + 1 if G is even, G - 1, G if it is odd
        assert max_gap == (G + 1 if G % 2 == 0 else G)
        assert 0 <= max_gap < harness.plane_fetch_gaps(G)
        assert fetches >= 2 * pieces
        assert (clamped > 0) == (G > 1)  # (a piece of two gaps or more ends with refills aimed past its last row)


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 7, 64, 65, 70])
def test_the_fetch_schedule_of_a_piece(harness, G):
    """the trace of single pieces against the schedule written out here: the pair that holds the first even gap, the single
    gap of an odd start, then behind every gap of a pair the same gap of the next pair"""
    out = (C.c_longlong * 4)()
    for g0 in range(G):
        for g1 in range(g0 + 1, G + 1):
            trace = np.full(g1 - g0 + 5, 10 ** 6, dtype=np.int32)
            bad = harness.plane_fetch_piece(G, g0, g1, 64, trace.ctypes.data_as(C.POINTER(C.c_int)), out)
            assert bad == 0
            f = g0 + (g0 & 1)
            want = [f, f + 1]
            left = g1 - g0
            if g0 & 1:
                want.append(g0)
                left -= 1
            for _ in range(left // 2):
                want += [f + 2, f + 3]
                f += 2
            assert out[0] == len(want) and out[2] == g1 - g0
            assert trace[:len(want)].tolist() == want
            assert out[1] == max(want) and max(want) <= G + 1
            assert out[3] == 2 * (left // 2) + (g0 & 1)


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    exe = tmp_path / "plane_fetch_harness"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-DPLANE_FETCH_HARNESS_MAIN", "-I", INC, SRC, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "plane fetch harness ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
