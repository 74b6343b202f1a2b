"""CPU: the workspace size queries as the header promises them (include/genvox_amd.h, "Workspaces and scratch").  gvx_model_create
and every size query are host arithmetic: no device, no blob.

Grid: B in {1, 2, 31, 32, 33, 64}, L in {1, 5, 128, 129, 256, 257}, T in {1, 2, 800}, at the default and the reduced layer sizes.

What is pinned:
  * gvx_workspace_bytes_autoregressive(B, L, S) <= gvx_workspace_bytes(B, L, S) and gvx_postnet_workspace_bytes(B, T) <=
    gvx_workspace_bytes(B, L, T): both are promises of the header;
  * every size is a positive multiple of 256 and does not shrink when T grows with B and L fixed;
  * the size is NOT monotone in B or in L: the region of Prenet gate contributions exists only for shapes whose plan uses it
    (make_ws_plan, pre_gate), so 33 rows need less than 32 and 257 tokens less than 256 at the default sizes.  A caller that keeps
    "the larger workspace" by comparing sizes across shapes without calling the query for the shape at hand is wrong, and the two
    pairs below are there to say so;
  * refused shapes give 0, as the header lists them.  gvx_dtw_workspace_bytes gives 0 for a refused shape AND for a shape that needs
    no workspace (its tables fit the LDS): gvx_dtw_uses_lds_tables tells the two apart (-1 / 1), and both are pinned.
"""
import ctypes as C
import itertools

import pytest

from genvox_amd import _lib
from genvox_amd.tacotron2 import dims_from_configs
from tests.helpers import BPTT_DEFAULT, BPTT_L_LIMIT, bptt_args_for_plan, create_handle, fwd_configs

BS, LS, TS = (1, 2, 31, 32, 33, 64), (1, 5, 128, 129, 256, 257), (1, 2, 800)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module", params=["def", "small"])
def handle(lib, request):
    h = create_handle(lib, dims_from_configs(*fwd_configs(request.param)))
    yield request.param, h
    lib.gvx_model_destroy(h)


def test_sizes_are_multiples_of_256_and_the_smaller_queries_are_smaller(lib, handle):
    _, h = handle
    for B, L, T in itertools.product(BS, LS, TS):
        full, ar, post = lib.gvx_workspace_bytes(h, B, L, T), lib.gvx_workspace_bytes_autoregressive(h, B, L, T), lib.gvx_postnet_workspace_bytes(h, B, T)
        for n in (full, ar, post):
            assert n > 0 and n % 256 == 0, (B, L, T, full, ar, post)
        assert ar <= full and post <= full, (B, L, T, full, ar, post)


def test_sizes_do_not_shrink_with_T(lib, handle):
    _, h = handle
    for B, L in itertools.product(BS, LS):
        for query in (lambda T: lib.gvx_workspace_bytes(h, B, L, T), lambda T: lib.gvx_workspace_bytes_autoregressive(h, B, L, T),
                      lambda T: lib.gvx_postnet_workspace_bytes(h, B, T)):
            sizes = [query(T) for T in TS]
            assert sizes == sorted(sizes), (B, L, sizes)


def test_the_size_is_not_monotone_in_rows_or_tokens(lib):
    """Default layer sizes: 32 rows of 128 tokens run beside the resident attention kernel and carry T x B x 4A floats of Prenet gate
    contributions; 33 rows do not.  256 tokens do, 257 do not.  (The figures themselves are not pinned, the order is.)"""
    h = create_handle(lib, dims_from_configs(*fwd_configs("def")))
    try:
        assert lib.gvx_workspace_bytes(h, 33, 128, 800) < lib.gvx_workspace_bytes(h, 32, 128, 800)
        assert lib.gvx_workspace_bytes(h, 32, 257, 800) < lib.gvx_workspace_bytes(h, 32, 256, 800)
        # the autoregressive amount leaves that region out: monotone on the same pairs
        assert lib.gvx_workspace_bytes_autoregressive(h, 33, 128, 800) > lib.gvx_workspace_bytes_autoregressive(h, 32, 128, 800)
        assert lib.gvx_workspace_bytes_autoregressive(h, 32, 257, 800) > lib.gvx_workspace_bytes_autoregressive(h, 32, 256, 800)
    finally:
        lib.gvx_model_destroy(h)


def test_refused_shapes_give_zero(lib, handle):
    _, h = handle
    for B, L, T in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5)):
        assert lib.gvx_workspace_bytes(h, B, L, T) == 0 and lib.gvx_workspace_bytes_autoregressive(h, B, L, T) == 0, (B, L, T)
    assert lib.gvx_workspace_bytes(None, 1, 1, 1) == 0 and lib.gvx_postnet_workspace_bytes(None, 1, 1) == 0
    assert lib.gvx_postnet_workspace_bytes(h, 0, 5) == 0 and lib.gvx_postnet_workspace_bytes(h, 5, 0) == 0


def test_conv_train_queries_refuse_what_the_calls_refuse(lib):
    ok = (3, 8, 24, 5, 3)
    assert lib.gvx_conv_train_saved_bytes(*ok) > 0 and lib.gvx_conv_train_workspace_bytes(*ok) > 0
    assert lib.gvx_conv_train_saved_bytes(1, 8, 8, 1, 3) > 0 and lib.gvx_conv_train_workspace_bytes(1, 8, 8, 1, 3) > 0   # B * T == 1 is served
    for what, shape in (("B = 0", (0, 8, 24, 5, 3)), ("T = 0", (3, 8, 24, 0, 3)), ("Cin % 8", (3, 7, 24, 5, 3)), ("Cout % 8", (3, 8, 20, 5, 3)),
                        ("Cin = 0", (3, 0, 24, 5, 3)), ("even k", (3, 8, 24, 5, 4)), ("k = 0", (3, 8, 24, 5, 0)), ("k < 0", (3, 8, 24, 5, -1)),
                        ("B * T above 2^30", (1 << 16, 8, 24, 1 << 15, 3))):
        assert lib.gvx_conv_train_saved_bytes(*shape) == 0 and lib.gvx_conv_train_workspace_bytes(*shape) == 0, what


def test_decoder_bptt_query_stops_at_the_lds_limit(lib):
    at = bptt_args_for_plan(2, BPTT_L_LIMIT, 2, BPTT_DEFAULT)
    past = bptt_args_for_plan(2, BPTT_L_LIMIT + 1, 2, BPTT_DEFAULT)
    assert BPTT_L_LIMIT + 1 == 665
    n = lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(at))
    assert n > 0 and n % 256 == 0
    assert lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(past)) == 0
    assert lib.gvx_train_decoder_bptt_workspace_bytes(None) == 0
    for B in (0, 33):
        assert lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(bptt_args_for_plan(B, 9, 2, BPTT_DEFAULT))) == 0, B


def test_dtw_query_zero_means_refused_or_not_needed(lib):
    frames, feats = 32768, 256                                               # GVX_DTW_MAX_FRAMES, GVX_DTW_MAX_FEATURES
    # tables in the LDS: no workspace
    assert lib.gvx_dtw_uses_lds_tables(1000, 1000, 13) == 1 and lib.gvx_dtw_workspace_bytes(2, 1000, 1000, 13) == 0
    # tables through the cache: a workspace, a multiple of 256, also at the limits themselves
    for shape in ((2, 3000, 3000, 80), (2, frames, frames, feats)):
        n = lib.gvx_dtw_workspace_bytes(*shape)
        assert lib.gvx_dtw_uses_lds_tables(*shape[1:]) == 0 and n > 0 and n % 256 == 0, shape
    for what, shape in (("Tp above the limit", (2, frames + 1, 10, 13)), ("Tg above the limit", (2, 10, frames + 1, 13)),
                        ("K above the limit", (2, 10, 10, feats + 1)), ("B = 0", (0, 3000, 3000, 80)), ("K = 0", (2, 3000, 3000, 0))):
        assert lib.gvx_dtw_workspace_bytes(*shape) == 0, what
        if shape[0] > 0:
            assert lib.gvx_dtw_uses_lds_tables(*shape[1:]) == -1, what
