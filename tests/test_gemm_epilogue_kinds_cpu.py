"""CPU: which compile-time epilogue kind a GEMM launch takes (gemm_epilogue_of in gemm_f32.hip, through gvx_debug_gemm_epilogue -
the function launch_gemm asks; host arithmetic, no device).  tests/test_gemm_epilogue_gpu.py compares the kinds' outputs with
the parent's epilogue; this pins that the launches it makes are of the kind it means to compare."""
import ctypes as C

import pytest

from genvox_amd import _lib

PARENT, GENERAL, PLAIN, BIAS = 0, 1, 2, 3
ROW_MAJOR_TILES = (4111, 2311, 4113, 2211, 2212, 2222, 4212)
HAS_PLAIN = {2211, 2212, 4212}                 # the Winograd products' shapes
HAS_BIAS = {2211, 2212, 4212, 4113, 2311}      # pre_gate, the LSTM input GEMM, the memory projection; the mel / gate projection


@pytest.fixture(scope="module")
def kind():
    lib = _lib.load()
    fn = lib.gvx_debug_gemm_epilogue
    fn.restype, fn.argtypes = C.c_int, [C.c_int] * 7
    return lambda tile, kmajor=0, bias=0, act=0, keep=0, row_len=0, halo=0: fn(tile, kmajor, bias, act, keep, row_len, halo)


@pytest.fixture()
def switch():
    fn = _lib.load().gvx_debug_gemm_parent_epilogue
    fn.restype, fn.argtypes = C.c_int, [C.c_int]
    was = fn(-1)
    yield fn
    fn(was)


def test_special_kinds_only_where_instantiated(kind, switch):
    switch(0)
    for tile in ROW_MAJOR_TILES:
        assert kind(tile) == (PLAIN if tile in HAS_PLAIN else GENERAL), tile
        assert kind(tile, bias=1) == (BIAS if tile in HAS_BIAS else GENERAL), tile
    for tile in (2212, 2222):   # the K-major form (weight gradients): general only
        assert kind(tile, kmajor=1) == GENERAL and kind(tile, kmajor=1, bias=1) == GENERAL
    assert kind(1234) == GENERAL   # no such shape: nothing special (launch_gemm refuses it)


def test_any_extra_means_general(kind, switch):
    switch(0)
    for tile in ROW_MAJOR_TILES:
        for bias in (0, 1):
            assert kind(tile, bias=bias, act=1) == GENERAL and kind(tile, bias=bias, act=2) == GENERAL
            assert kind(tile, bias=bias, keep=1) == GENERAL and kind(tile, bias=bias, row_len=1) == GENERAL
            assert kind(tile, bias=bias, halo=2) == GENERAL
            assert kind(tile, bias=bias, act=2, row_len=1, halo=2) == GENERAL


def test_switch_selects_the_parent_epilogue_everywhere(kind, switch):
    assert switch(1) in (0, 1) and switch(-1) == 1
    for tile in ROW_MAJOR_TILES:
        assert kind(tile) == PARENT and kind(tile, bias=1) == PARENT and kind(tile, bias=1, act=2, row_len=1, halo=2) == PARENT
    assert kind(2222, kmajor=1) == PARENT
    assert switch(0) == 1 and switch(-1) == 0
    assert kind(4212) == PLAIN


def test_bad_arguments(kind):
    assert kind(0) == -1 and kind(4212, halo=-1) == -1
