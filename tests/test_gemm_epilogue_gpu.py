"""GPU: the compile-time epilogue kinds of the fp32 GEMM (EPI_PLAIN, EPI_BIAS, EPI_GENERAL in gemm_f32.hip) against the epilogue
the kernels had before them, kept as EPI_PARENT and selected with gvx_debug_gemm_parent_epilogue.  No value is computed
differently and no store goes elsewhere, so every comparison is bit equality - of the outputs, of a whole workspace that started
as 0xFF, and of the guard words around both.  Through the entry points of tests/test_gemm_gpu.py and
tests/test_winograd_conv_gpu.py: gvx_train_gemm_nt / _tn, gvx_postnet_forward, and one whole forward for the Prenet's keep masks
and blocked output.  tests/test_gemm_epilogue_kinds_cpu.py pins which kind each kind of launch takes."""
import contextlib
import ctypes as C

import pytest
import torch

from genvox_amd import _lib
from tests.helpers import GEMM_BRANCH_CASES, GemmCase, gemm_plan

pytestmark = pytest.mark.gpu

PARENT, GENERAL, PLAIN, BIAS = 0, 1, 2, 3
SENTINEL = 0x5A5A5A5A
GUARD_WORDS = 64   # 256 bytes: the guarded buffers keep their alignment


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    lib.gvx_debug_gemm_parent_epilogue.restype, lib.gvx_debug_gemm_parent_epilogue.argtypes = C.c_int, [C.c_int]
    lib.gvx_debug_gemm_epilogue.restype, lib.gvx_debug_gemm_epilogue.argtypes = C.c_int, [C.c_int] * 7
    return lib


@contextlib.contextmanager
def epilogue(lib, parent):
    was = lib.gvx_debug_gemm_parent_epilogue(1 if parent else 0)
    try:
        yield
    finally:
        lib.gvx_debug_gemm_parent_epilogue(was)


def _G():
    from tests import test_gemm_gpu as G
    return G


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- plain and bias-only products, every tile shape --------------------------------------------------------------------------
def _smallest(tile, split):
    return min((c for c in GEMM_BRANCH_CASES if c.tile == tile and (c.rows_big > 0) == split), key=lambda c: c.M * c.N * c.K)


TILE_CASES = [_smallest(t, False) for t in (4111, 2311, 4113, 2211, 2212, 4212)] + [
    _smallest(4212, True),                                  # two launches: rows_big on <4,2,1,2>, m_begin = rows_big on <2,2,1,1>
    # M no multiple of the tile, N no multiple of 32, the shortest K and a K with a tail, on a four-wave and the six-wave shape
    GemmCase(200, 130, 36, 0, None, 2211, 0, 1), GemmCase(131, 45, 4, 0, None, 2311, 0, 1), GemmCase(131, 45, 36, 0, None, 2311, 0, 1),
    GemmCase(132, 260, 33, 1, None, 2212, 0, 1),            # the K-major form: general only
]
HAS_PLAIN, HAS_BIAS = {2211, 2212, 4212}, {2211, 2212, 4212, 4113, 2311}


@pytest.mark.parametrize("c", TILE_CASES, ids=[f"{'tn' if c.kmajor else 'nt'}-{c.M}x{c.N}x{c.K}" for c in TILE_CASES])
def test_plain_and_bias_products_equal_the_parent_epilogue(lib, c):
    """call_gemm checks C's guard rows and padding columns itself; C, with and without a bias, must come out bit for bit."""
    G = _G()
    rc, tile, rows_big, _ = gemm_plan(lib, c.M, c.N, c.K, c.kmajor)
    assert (rc, tile, rows_big) == (0, c.tile, c.rows_big), c
    a, w, bias = G.make_operands(c, "rounded", 7000 + c.M + c.K)
    for use_bias in ([False] if c.kmajor else [False, True]):
        want_kind = GENERAL if c.kmajor else (BIAS if tile in HAS_BIAS else GENERAL) if use_bias else (PLAIN if tile in HAS_PLAIN else GENERAL)
        with epilogue(lib, False):
            assert lib.gvx_debug_gemm_epilogue(tile, c.kmajor, int(use_bias), 0, 0, 0, 0) == want_kind, (c, use_bias)
            new = G.call_gemm(lib, c, a, w, bias, True, use_bias=use_bias)
        with epilogue(lib, True):
            assert lib.gvx_debug_gemm_epilogue(tile, c.kmajor, int(use_bias), 0, 0, 0, 0) == PARENT
            old = G.call_gemm(lib, c, a, w, bias, True, use_bias=use_bias)
        assert bool(torch.isfinite(new).all()) and torch.equal(_bits(new), _bits(old)), (c, use_bias, int((_bits(new) != _bits(old)).sum()))
        if use_bias:   # (and the bias is in there: not the plain product again)
            with epilogue(lib, False):
                assert not torch.equal(new, G.call_gemm(lib, c, a, w, bias, True, use_bias=False)), c


# ---- convolution outputs: row_len, halo rows, sequence boundaries inside a wave's rows; the batched Winograd products -----------
@pytest.fixture(scope="module")
def small_postnet():
    return _G()._postnet_model(False)[0]   # 64 channels: 80 -> 64, three 64 -> 64 layers, 64 -> 80


def _postnet_raw(lib, model, mel, lens):
    """gvx_postnet_forward on exactly its workspace bytes, every byte 0xFF before the call, guard words around the workspace and
    around the output.  -> (output words, all workspace words with the guards)."""
    model._ensure_packed()
    B, _, T = mel.shape
    h, st = model._handle, torch.cuda.current_stream().cuda_stream
    n = lib.gvx_postnet_workspace_bytes(h, B, T)
    assert n % 4 == 0
    ws = torch.full((n // 4 + 2 * GUARD_WORDS,), -1, dtype=torch.int32, device="cuda")   # 0xFF bytes
    ws[:GUARD_WORDS] = SENTINEL
    ws[GUARD_WORDS + n // 4:] = SENTINEL
    ws[GUARD_WORDS:GUARD_WORDS + 256] = 0   # the status words of a model workspace are cleared once by the caller
    out = torch.full((mel.numel() + 2 * GUARD_WORDS,), SENTINEL, dtype=torch.int32, device="cuda")
    ml = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    rc = lib.gvx_postnet_forward(h, mel.data_ptr(), None if ml is None else ml.data_ptr(), B, T, out.data_ptr() + 4 * GUARD_WORDS,
                                 ws.data_ptr() + 4 * GUARD_WORDS, n, st)
    torch.cuda.synchronize()
    assert rc == 0, lib.gvx_last_error()
    for buf, body in ((ws, n // 4), (out, mel.numel())):
        assert bool((buf[:GUARD_WORDS] == SENTINEL).all()) and bool((buf[GUARD_WORDS + body:] == SENTINEL).all()), "guard words written"
    return out, ws


def _postnet_both(lib, model, mel, lens):
    with epilogue(lib, False):
        new = _postnet_raw(lib, model, mel, lens)
    with epilogue(lib, True):
        old = _postnet_raw(lib, model, mel, lens)
    for name, x, y in (("output", new[0], old[0]), ("workspace", new[1], old[1])):
        assert torch.equal(x, y), (name, tuple(mel.shape), lens, int((x != y).sum()))
    return new[0][GUARD_WORDS:GUARD_WORDS + mel.numel()].view(torch.float32).view(mel.shape)


@pytest.mark.parametrize("mode", [0, 2], ids=["direct", "winograd"])
@pytest.mark.parametrize("T", [1, 2, 5, 33, 130])
def test_convolution_outputs_equal_the_parent_epilogue(lib, small_postnet, mode, T):
    """B = 3 sequences of T frames: 3 T rows of tanh / row_len / halo output per layer (EPI_GENERAL), for T <= 5 all in one wave's
    32 rows, front and back halo rows of several sequences written by one block; for T = 33 and 130 a boundary inside a wave.
    Lengths: every row whole, and one row each of length T, 1 and 0.  Mode 2 runs the 64-channel layers as Winograd: eight
    products in one launch (EPI_PLAIN, grid.y = the slice) between the direct first and last layer."""
    model, G = small_postnet, _G()
    mel = G._mel(3, 80, T, 900 + T)
    model.set_winograd(mode)
    try:
        assert model.conv_plan(64, 64, 5) == (1 if mode else 0)
        whole = _postnet_both(lib, model, mel, None)
        ragged = _postnet_both(lib, model, mel, [T, 1, 0])
    finally:
        model.set_winograd(1)
    assert bool(torch.isfinite(whole).all()) and torch.equal(ragged[0], whole[0])
    assert bool((ragged[1, :, 1:] == 0).all()) and bool((ragged[2] == 0).all())   # behind row_len: zeros (the residual of a zeroed mel)


def test_batched_winograd_products_equal_the_parent_epilogue(lib, small_postnet):
    """One batched product of 8 slices, M = 66 tiles of four frames (2 x 130 frames), C = 64: <2,2,1,1>, EPI_PLAIN, two row
    tiles per slice, the second one mostly outside M."""
    model, G = small_postnet, _G()
    assert lib.gvx_debug_gemm_epilogue(2211, 0, 0, 0, 0, 0, 0) == PLAIN
    model.set_winograd(2)
    try:
        assert model.conv_plan(64, 64, 5) == 1
        for lens in (None, [130, 67]):
            _postnet_both(lib, model, G._mel(2, 80, 130, 977), lens)
    finally:
        model.set_winograd(1)


# ---- the Prenet: keep masks and the k-group-blocked output (R = B rows per step), inside a whole forward -----------------------
def test_forward_with_keep_masks_equals_the_parent_epilogue(lib):
    """B = 3, default layer sizes: the Prenet's two GEMMs (ReLU, keep mask, rows (t, b) into [K / 8][B][8] blocks: a group of
    the row map every three rows), the encoder's ReLU convolutions, pre_gate, the LSTM input GEMM and the projections, all in
    one teacher-forced forward.  A model per setting: nothing launched under one setting is replayed under the other."""
    from genvox_amd import weights as gw
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
    from genvox_amd.tacotron2 import Tacotron2

    mc, ac, tc = Tacotron2Config(), AudioConfig(filter_length=1024, log_func="np.log"), TextConfig(n_tokens=40)
    sd = gw.generate_state_dict(mc, ac, tc, seed=0)
    B, L, T = 3, 12, 5
    inp = gw.synthetic_inputs(B, L, T, tc.n_tokens, ac.n_mels, seed=5)
    batch = {k: torch.from_numpy(v) for k, v in inp.items()}
    masks = torch.from_numpy(gw.prenet_keep_masks((T + 1) * B, mc.prenet_dim))
    assert 0 < int(masks.sum()) < masks.numel()
    outs = []
    for parent in (False, True):
        with epilogue(lib, parent):
            assert lib.gvx_debug_gemm_epilogue(4212, 0, 1, 0, 0, 0, 0) == (PARENT if parent else BIAS)
            model = Tacotron2(mc, ac, tc)
            model.load_state_dict(sd)
            model = model.to("cuda:0")
            got = model.forward({**batch, "prenet_keep_masks": masks})
            torch.cuda.synchronize()
            model.check_status()
            outs.append({k: v.clone() for k, v in got.items()})
    assert set(outs[0]) == set(outs[1]) and len(outs[0]) >= 4
    for k in outs[0]:
        assert bool(torch.isfinite(outs[0][k]).all()) and torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), k
