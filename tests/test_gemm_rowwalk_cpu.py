"""CPU: the GEMM epilogue's row walk (row_walk_begin / row_walk_advance / mfma32_row_step in gvx_kernels.h) against the division
formula it replaces, through gvx_debug_gemm_row_walk - the same three functions the kernel calls, compiled for the host.

A lane of the 32 x 32 MFMA tile holds 16 rows of an M tile: first + (q & 3) + 8 * (q >> 2) for q = 0..15, where first = m_begin +
(tile and wave offsets, multiples of 32) + 4 * (lane >> 5).  The kernel divides once, at `first`, and walks from there; for every
row the walk must give (m // R, m % R) and the offset (m // R) * s1 + (m % R) * s0 of the RowMap.  No device is touched."""
import ctypes as C

import pytest

from genvox_amd import _lib

ROWS = [(q & 3) + 8 * (q >> 2) for q in range(16)]


@pytest.fixture(scope="module")
def walk():
    fn = _lib.load().gvx_debug_gemm_row_walk
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_long, C.c_long, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def run(R, s1, s0, first):
        off, grp, idx = (C.c_long * 16)(), (C.c_int * 16)(), (C.c_int * 16)()
        assert fn(R, s1, s0, first, off, grp, idx) == 0, (R, s1, s0, first)
        return list(zip(off, grp, idx))
    return run


def _want(R, s1, s0, first):
    return [((m // R) * s1 + (m % R) * s0, m // R, m % R) for m in (first + d for d in ROWS)]


def _firsts(R, m_begin):
    """First rows of a lane: both halves of the wave (4 * h), M tiles and waves at multiples of 32, and - whatever R is - every
    residue of the first row mod R (rows m_begin + 32 * t + 4 * h reach all of them only for odd R: the rest is walked from plain
    consecutive first rows, which the kernel's m_begin may produce as well)."""
    out = {m_begin + 32 * t + 4 * h for t in range(0, 9) for h in (0, 1)}
    out |= {m_begin + x for x in range(min(R, 900) + 33)}
    out |= {m_begin + 32 * t + 4 * h for t in (100, 799, 25599 // 32) for h in (0, 1)}
    return sorted(out)


@pytest.mark.parametrize("m_begin", [0, 128, 24576, 77])
@pytest.mark.parametrize("R", [1, 2, 3, 5, 31, 32, 33, 800])
def test_walk_equals_division_conv_maps(walk, R, m_begin):
    """Convolution outputs: R frames per sequence, s0 = C channels, s1 = (R + 4) C (halo rows between the groups); and the plain
    forms with s1 = 0 (one group would do, but the map is free to have many) and a row stride that is no multiple of anything."""
    for s1, s0 in ((0, 512), (0, 85), ((R + 4) * 512, 512), ((R + 4) * 80, 80), (7, 3 * R + 11)):
        for first in _firsts(R, m_begin):
            assert walk(R, s1, s0, first) == _want(R, s1, s0, first), (R, s1, s0, first)


@pytest.mark.parametrize("B", [1, 3, 5, 32, 33])
def test_walk_equals_division_blocked_output(walk, B):
    """The Prenet's output map: rows are (t, b) time-major, R = B rows per step, the step's block is [K / 8][B][8] floats - s0 = 8
    (one row of a k-group block), s1 = the floats of one step (256 columns: 32 k-group blocks of c_nblk = 8 B)."""
    c_nblk = 8 * B
    s1, s0 = 32 * c_nblk, 8
    for m_begin in (0, 128, 24576):
        for first in _firsts(B, m_begin):
            assert walk(B, s1, s0, first) == _want(B, s1, s0, first), (B, first)


def test_walk_with_negative_and_large_strides(walk):
    """Offsets are 64-bit: a map whose offsets pass 2^31 floats, and one whose group stride is smaller than a group (s1 < R s0)."""
    for R, s1, s0 in ((800, 804 * 4096, 4096), (5, 3, 1 << 33), (33, -17, 2)):
        for first in (0, 4, R - 1, R, 32 * 20000 + 4, 2 ** 31 - 64):
            assert walk(R, s1, s0, first) == _want(R, s1, s0, first), (R, s1, s0, first)


def test_bad_arguments_are_refused(walk):
    fn = _lib.load().gvx_debug_gemm_row_walk
    off, grp, idx = (C.c_long * 16)(), (C.c_int * 16)(), (C.c_int * 16)()
    assert fn(0, 0, 1, 0, off, grp, idx) != 0 and fn(4, 0, 1, -1, off, grp, idx) != 0 and fn(4, 0, 1, 0, None, grp, idx) != 0
