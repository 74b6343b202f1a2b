"""Shared helpers for the parity tests (fixture loading, weight sets, mask unpacking)."""
import collections
import ctypes as C
import functools
import os

import numpy as np
import torch

from genvox_amd import weights as gw
from tests.golden.cases import AR_CASES, AUDIO_CASE, TF_CASES, case_configs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3  # BASELINE.json north_star: mels within 1e-3 (fp32) of the reference


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=4)
def _state_dict_cached(dims_key, weight_seed, peaky):
    case = {**TF_CASES, **AR_CASES}[dims_key]
    mc, ac, tc = case_configs(case)
    return gw.generate_state_dict(mc, ac, tc, seed=weight_seed, peaky_attention=peaky)


def case_state_dict(name):
    case = {**TF_CASES, **AR_CASES}[name]
    return _state_dict_cached(name, case["weight_seed"], case.get("peaky", False))


def unpack_masks(packed, shape):
    n = int(np.prod(shape[1:]))
    bits = np.unpackbits(packed, axis=1)[:, :n]
    return torch.from_numpy(np.ascontiguousarray(bits.reshape(shape)))


def tf_batch(fx):
    return {k: torch.from_numpy(fx[k]) for k in ("token_padded", "token_lengths", "mel_padded", "gate_padded", "mel_lengths")}


def max_abs_diff(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0


# ---- the dense fp32 GEMM (genvox_amd/csrc/gemm_f32.hip): the shapes tests/test_gemm_gpu.py runs, each with the branch of
# launch_gemm it is there for.  tests/test_host_cpu.py pins every line against gvx_debug_gemm_plan on the CPU, so a retuned
# threshold fails there and the cases get re-aimed instead of silently losing a branch. --------------------------------------
# tile: <WR,WC,TM,TN> as four digits; rows_big > 0: the two-launch split (rows [0, rows_big) on `tile`, the rest on <2,2,1,1>);
# scratch: None (NULL), "full" (room for 8 partial tiles) or the number of partial tiles the scratch holds; pieces: K pieces that
# run (1 = no split-K).  kmajor: gvx_train_gemm_tn (K = rows) instead of gvx_train_gemm_nt.
GemmCase = collections.namedtuple("GemmCase", "M N K kmajor scratch tile rows_big pieces")


def _nt(M, N, K, tile, rows_big=0, scratch=None, pieces=1):
    return GemmCase(M, N, K, 0, scratch, tile, rows_big, pieces)


def _tn(M, N, rows, tile, scratch=None, pieces=1):
    return GemmCase(M, N, rows, 1, scratch, tile, 0, pieces)


GEMM_BRANCH_CASES = [
    # N <= 32 -> <4,1,1,1>
    _nt(1, 1, 4, 4111), _nt(130, 32, 36, 4111), _nt(257, 24, 100, 4111),
    # 32 < N <= 96, at most 4096 rows -> <2,3,1,1> (six waves)
    _nt(65, 33, 44, 2311), _nt(568, 80, 2560, 2311), _nt(4096, 96, 400, 2311),
    # N <= 96, more than 4096 rows -> <4,1,1,3>
    _nt(4097, 81, 400, 4113), _nt(4229, 96, 36, 4113),
    # fewer than 192 tiles of 128 x 128 -> <2,2,1,1>
    _nt(63, 97, 68, 2211), _nt(200, 130, 4, 2211), _nt(4096, 512, 2560, 2211),
    # 192 <= tiles < 384 -> <2,2,1,2>
    _nt(6200, 512, 80, 2212),
    # >= 384 tiles, remainder of the last round 0 or > 64 -> <4,2,1,2> alone
    _nt(16384, 512, 256, 4212), _nt(12803, 512, 36, 4212),
    # remainder 1..64 -> <4,2,1,2> on the rows of the full rounds, <2,2,1,1> from m_begin = rows_big
    _nt(25600, 512, 400, 4212, 24576), _nt(25563, 512, 80, 4212, 24576), _nt(33000, 130, 80, 4212, 32768),
]
# every K % 32 (the k tail of the last k-tile), K around 32, 64 and 2560, row-major and K-major
GEMM_KTAIL_CASES = (
    [_nt(200, 130, 32 + r, 2211) for r in range(0, 32, 4)] + [_nt(257, 24, 64 + r, 4111) for r in range(0, 32, 4)]
    + [_nt(130, 100, 2560 + r, 2211) for r in range(0, 32, 4)]
    + [_tn(132, 260, k0 + r, 2212) for k0 in (32, 64, 2560) for r in range(0, 32, 4)])
# split-K: scratch given, fewer than 256 tiles of 64 x 128, K >= 512
GEMM_SPLITK_CASES = [
    _nt(32, 4096, 2560, 2211, scratch="full", pieces=8), _nt(32, 80, 2560, 2311, scratch="full", pieces=8),
    _nt(64, 16, 1024, 4111, scratch="full", pieces=4), _nt(200, 512, 4096, 2211, scratch="full", pieces=8),
    _nt(32, 4096, 516, 2211, scratch="full", pieces=2),     # pieces of 320 and 196
    _nt(32, 4096, 2052, 2211, scratch="full", pieces=7),    # 8 wanted: pieces of 320, the seventh is 132 long
    _nt(32, 4096, 2560, 2211, scratch=3, pieces=3),         # the scratch holds 3 partial tiles: pieces of 896, 896, 768
    _nt(32, 4096, 2560, 2211, scratch=1, pieces=1),         # room for one: no split
    _nt(32, 4096, 2560, 2211, scratch=None, pieces=1),
    _tn(132, 260, 6400, 2212, scratch="full", pieces=8), _tn(132, 260, 6401, 2212, scratch="full", pieces=8),
    _tn(4, 4, 517, 2212, scratch="full", pieces=2), _tn(512, 2560, 1000, 2212, scratch="full", pieces=3),
]
# K-major (gvx_train_gemm_tn): <2,2,1,2> below 384 tiles of 128 x 128, <2,2,2,2> from there on; rows that are no multiple of 4
GEMM_KMAJOR_CASES = (
    [_tn(4, 4, rows, 2212) for rows in (1, 3, 31, 32, 33, 6400, 6401)] + [_tn(132, 260, rows, 2212) for rows in (1, 3, 31, 33, 6400)]
    + [_tn(1536, 4096, rows, 2222) for rows in (1, 33, 6401)] + [_tn(2560, 2560, rows, 2222) for rows in (3, 32, 6400)])
GEMM_CASES = GEMM_BRANCH_CASES + GEMM_KTAIL_CASES + GEMM_SPLITK_CASES + GEMM_KMAJOR_CASES
# the reduced table of the GVX_GEMM_8W=0 run: there <2,2,2,2> takes the place of <4,2,1,2>
GEMM_8W_CASES = [c for c in GEMM_BRANCH_CASES if c.tile == 4212]


def gemm_scratch_bytes(case):
    """Bytes of split-K scratch the case hands to the entry point (None: a NULL scratch)."""
    if case.scratch is None:
        return None
    return (8 if case.scratch == "full" else case.scratch) * case.M * case.N * 4


def gemm_plan(lib, M, N, K, kmajor=0, scratch_bytes=None):
    """(status, tile, rows_big, k_pieces) of gvx_debug_gemm_plan: how gvx_train_gemm_nt / _tn would run the product.  Host
    arithmetic only - no device, no model handle; the export is in neither the public header nor _lib.SIGNATURES."""
    fn = lib.gvx_debug_gemm_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 5 + [C.c_size_t] + [C.POINTER(C.c_int)] * 3
    tile, rows_big, pieces = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = fn(M, N, K, kmajor, scratch_bytes is not None, scratch_bytes or 0, C.byref(tile), C.byref(rows_big), C.byref(pieces))
    return rc, tile.value, rows_big.value, pieces.value
