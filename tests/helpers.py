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


# ---- back-propagation through the decoder loop (gvx_train_decoder_bptt, genvox_amd/csrc/train_bptt_decoder.hip): the shapes
# tests/test_bptt_gpu.py runs, each with the branch of bptt_attention_kernel / bptt_chunks / bptt_plan it is there for.
# tests/test_host_cpu.py pins every line against gvx_debug_bptt_plan on the CPU. --------------------------------------------------
# sizes = (A, D, E, P, a, F, kl).  lengths: "full" (every row L), "ragged" (rows from 1 to L, both present when B >= 2), "short"
# (every row shorter than L).  plan = (G, CH, chunks that hold positions, passes over the energies, over the dense-gradient
# groups, over the convolution-gradient items, query / v in registers, Na, Nd) as gvx_debug_bptt_plan reports it.
BpttCase = collections.namedtuple("BpttCase", "name B L T sizes lengths plan")
BPTT_DEFAULT = (1024, 1024, 512, 256, 128, 32, 31)
BPTT_ODD = (40, 56, 48, 20, 24, 12, 5)        # E + A = 88, A + E + D = 144: padded product columns; 512 % 24 != 0
BPTT_EVEN = (32, 32, 32, 16, 16, 8, 3)        # 64 and 96 columns: no padding


def _bp(name, B, L, T, sizes, lengths, plan):
    return BpttCase(name, B, L, T, sizes, lengths, plan)


_DEF_N = (1536, 2560)
_ODD_N = (96, 160)
BPTT_CASES = [
    # default layer sizes.  One chunk and T = 1 (ya0 and w_prev both NULL, no products launch of the attention cell)
    _bp("def_1x1x1", 1, 1, 1, BPTT_DEFAULT, "full", (1, 1, 1, 1, 1, 1, 1) + _DEF_N),
    _bp("def_2x5x3", 2, 5, 3, BPTT_DEFAULT, "ragged", (2, 3, 2, 1, 1, 1, 1) + _DEF_N),
    # L = 33: G = 8, CH = 5, the eighth chunk is empty; kl = 31 reaches three chunks to each side
    _bp("def_3x33x4", 3, 33, 4, BPTT_DEFAULT, "ragged", (8, 5, 7, 1, 1, 1, 1) + _DEF_N),
    _bp("def_32x128x3", 32, 128, 3, BPTT_DEFAULT, "ragged", (8, 16, 8, 1, 1, 1, 1) + _DEF_N),
    # CH a = 32 x 128 = 4096: the last L of one energy pass; 257, 300: the reload of the second pass
    _bp("def_5x256x3", 5, 256, 3, BPTT_DEFAULT, "ragged", (8, 32, 8, 1, 1, 1, 1) + _DEF_N),
    _bp("def_3x257x3", 3, 257, 3, BPTT_DEFAULT, "ragged", (8, 33, 8, 2, 1, 1, 1) + _DEF_N),
    _bp("def_2x300x3", 2, 300, 3, BPTT_DEFAULT, "short", (8, 38, 8, 2, 1, 1, 1) + _DEF_N),
    # near the LDS limit, and the largest L the argument check accepts (162580 of 163840 bytes; 665 needs 164128)
    _bp("def_2x600x2", 2, 600, 2, BPTT_DEFAULT, "ragged", (8, 75, 8, 3, 1, 1, 1) + _DEF_N),
    _bp("def_1x664x2", 1, 664, 2, BPTT_DEFAULT, "full", (8, 83, 8, 3, 1, 1, 1) + _DEF_N),
] + [
    # L = 1 .. 4: one chunk; 5 .. 28: fewer than eight (CH = 4 at 8, 28; 3 at 9); 29, 31, 32: eight chunks of 4
    _bp("odd_L%d" % L, 3, L, 3, BPTT_ODD, "ragged", plan + _ODD_N)
    for L, plan in ((1, (1, 1, 1, 1, 1, 1, 0)), (2, (1, 2, 1, 1, 1, 1, 0)), (3, (1, 3, 1, 1, 1, 1, 0)), (4, (1, 4, 1, 1, 1, 1, 0)),
                    (5, (2, 3, 2, 1, 1, 1, 0)), (8, (2, 4, 2, 1, 1, 1, 0)), (9, (3, 3, 3, 1, 1, 1, 0)), (28, (7, 4, 7, 1, 1, 1, 0)),
                    (29, (8, 4, 8, 1, 1, 1, 0)), (31, (8, 4, 8, 1, 1, 1, 0)), (32, (8, 4, 8, 1, 1, 1, 0)))
] + [
    # every row shorter than L (the last chunk holds only padding), all rows full
    _bp("odd_short", 4, 9, 3, BPTT_ODD, "short", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    _bp("odd_full", 4, 9, 3, BPTT_ODD, "full", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    # T = 1, T = 2 (one products launch of the attention cell), the longest T of the table
    _bp("odd_T1", 3, 9, 1, BPTT_ODD, "ragged", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    _bp("odd_T2", 3, 9, 2, BPTT_ODD, "ragged", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    _bp("odd_T6", 3, 9, 6, BPTT_ODD, "ragged", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    # B = 1, 2, 31, 32 (3 above)
    _bp("odd_B1", 1, 9, 2, BPTT_ODD, "full", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    _bp("odd_B2", 2, 9, 2, BPTT_ODD, "ragged", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    _bp("odd_B31", 31, 9, 2, BPTT_ODD, "ragged", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    _bp("odd_B32", 32, 9, 2, BPTT_ODD, "ragged", (3, 3, 3, 1, 1, 1, 0) + _ODD_N),
    # attention dim, filters, kernel size.  a = 1 / F = 1 / kl = 1; a = 16 (divides 512) with the product columns unpadded
    _bp("a1_F1_kl1", 3, 9, 3, (32, 32, 32, 16, 1, 1, 1), "ragged", (3, 3, 3, 1, 1, 1, 1, 64, 96)),
    _bp("a16_F8_kl3", 3, 9, 3, BPTT_EVEN, "ragged", (3, 3, 3, 1, 1, 1, 1, 64, 96)),
    # a = 100 (512 % 100 != 0): halo of kl = 31 over three chunks of 5; CH a = 42 x 100 > 4096: second energy pass with per-item q / v
    _bp("a100_F32_kl31", 3, 33, 3, (40, 56, 48, 20, 100, 32, 31), "ragged", (8, 5, 7, 1, 1, 1, 0, 96, 160)),
    _bp("a100_L330", 2, 330, 2, (40, 56, 48, 20, 100, 32, 31), "ragged", (8, 42, 8, 2, 1, 1, 0, 96, 160)),
    # a = 256 fills the dense-gradient pass exactly (a x 4 groups = 2 x 512); F x 2 x kl = 2112 > 2048: second pass of the
    # convolution gradient; CH a = 17 x 256 > 4096: second energy pass with a | 512
    _bp("a256_F32_kl33", 3, 40, 3, (32, 32, 32, 16, 256, 32, 33), "ragged", (8, 5, 8, 1, 1, 2, 1, 64, 96)),
    _bp("a256_L136", 2, 136, 2, (32, 32, 32, 16, 256, 32, 33), "ragged", (8, 17, 8, 2, 1, 2, 1, 64, 96)),
    # padded product columns at large layer sizes (E + A = 1544 -> 1568, A + E + D = 2584 -> 2592)
    _bp("big_odd_N", 2, 12, 2, (1032, 1040, 512, 256, 128, 32, 31), "ragged", (3, 4, 3, 1, 1, 1, 1, 1568, 2592)),
]
BPTT_BY_NAME = {c.name: c for c in BPTT_CASES}
# the 32-row cases whose rows 0 .. 4 are recomputed as a call of their own (bit-equal: no summation order depends on B)
BPTT_ROW_CASES = ["def_32x128x3", "odd_B32"]
# handed over once more with a dense [T][B][E] copy of the contexts (ctx_ts = B E, ctx_bs = E)
BPTT_STRIDE_CASES = ["def_3x33x4", "odd_L9", "a100_F32_kl31"]
BPTT_L_LIMIT = 664   # default layer sizes: the largest L gvx_train_decoder_bptt accepts (the attention launch's 160 KiB of LDS)

# encoder BiLSTM walk (gvx_train_encoder_lstm_bptt / _resident): plan = (workgroups per direction, LDS bytes, the resident entry
# point takes the resident walk, trips of the kernels' loop over batch rows)
EncBpttCase = collections.namedtuple("EncBpttCase", "name B L H lengths plan")
ENC_BPTT_CASES = [
    # H = 8 (two workgroups per direction, the scalar h_prev loop: H % 32 != 0), L = 1, B = 1
    EncBpttCase("H8_1x1", 1, 1, 8, "full", (2, 1024, 1, 1)),
    EncBpttCase("H8_3x2", 3, 2, 8, "ragged", (2, 1024, 1, 1)),
    EncBpttCase("H8_64x150", 64, 150, 8, "short", (2, 1024, 1, 2)),
    EncBpttCase("H24_3x21", 3, 21, 24, "ragged", (6, 3072, 1, 1)),
    EncBpttCase("H24_32x21", 32, 21, 24, "full", (6, 3072, 1, 1)),
    # B = 33, 64: the second trip of `for (b = b0; b < B; b += 32)`
    EncBpttCase("H24_33x21", 33, 21, 24, "ragged", (6, 3072, 1, 2)),
    EncBpttCase("H24_64x21", 64, 21, 24, "short", (6, 3072, 1, 2)),
    # default size
    EncBpttCase("H256_1x150", 1, 150, 256, "full", (64, 32768, 1, 1)),
    EncBpttCase("H256_3x21", 3, 21, 256, "ragged", (64, 32768, 1, 1)),
    EncBpttCase("H256_32x150", 32, 150, 256, "ragged", (64, 32768, 1, 1)),
    EncBpttCase("H256_33x21", 33, 21, 256, "ragged", (64, 32768, 1, 2)),
    EncBpttCase("H256_64x2", 64, 2, 256, "full", (64, 32768, 1, 2)),
    # H = 384: the last size of the resident walk (192 workgroups, 48 KiB); 392: the launch per step from both entry points
    EncBpttCase("H384_3x21", 3, 21, 384, "ragged", (96, 49152, 1, 1)),
    EncBpttCase("H384_33x2", 33, 2, 384, "short", (96, 49152, 1, 2)),
    EncBpttCase("H392_3x21", 3, 21, 392, "ragged", (98, 50176, 0, 1)),
    EncBpttCase("H392_1x1", 1, 1, 392, "full", (98, 50176, 0, 1)),
]


def bptt_lengths(kind, B, L):
    """Token lengths of a case, longest first (as the collate function sorts a batch)."""
    if kind == "full" or L == 1:
        return [L] * B
    if kind == "short":
        return sorted((max(1, (L - 1) - (i * 7) % max(1, L - 1)) for i in range(B)), reverse=True)
    if B == 1:
        return [L]
    return sorted([L, 1] + [1 + (i * 5 + 3) % L for i in range(B - 2)], reverse=True)


def bptt_args_for_plan(B, L, T, sizes):
    """An argument block with the case's sizes and non-null dummy pointers: for the host-only queries, which never dereference."""
    from genvox_amd import _lib

    a = _lib.gvx_bptt_decoder_args()
    a.B, a.L, a.T = B, L, T
    a.A, a.D, a.E, a.P, a.a, a.F, a.kl = sizes
    a.att_scale = a.dec_scale = 1.0
    for n, t in _lib.gvx_bptt_decoder_args._fields_:
        if t is C.c_void_p:
            setattr(a, n, 256)
    return a


def bptt_plan(lib, args):
    """(status, [G, CH, chunks, energy passes, dense passes, conv passes, q in registers, Na, Nd, LDS bytes]) of
    gvx_debug_bptt_plan.  Host arithmetic only; the export is in neither the public header nor _lib.SIGNATURES."""
    fn = lib.gvx_debug_bptt_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    out = (C.c_int * 10)()
    rc = fn(C.byref(args) if args is not None else None, out)
    return rc, list(out)


def enc_bptt_plan(lib, B, H, resident):
    """(status, [workgroups per direction, LDS bytes, resident walk taken, row trips]) of gvx_debug_enc_bptt_plan."""
    fn = lib.gvx_debug_enc_bptt_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int)]
    out = (C.c_int * 4)()
    rc = fn(B, H, 1 if resident else 0, out)
    return rc, list(out)


# ---- the training-mode convolution layer (gvx_conv_bn_act_train_forward / _backward, genvox_amd/csrc/train_conv.hip): the shapes
# tests/test_conv_train_gpu.py runs, each group with the branch it is there for.  tests/test_host_cpu.py pins every line against
# gvx_debug_conv_train_plan on the CPU, so a retuned threshold fails there and the cases get re-aimed. ---------------------------------
# act: none / relu / tanh.  p: None (keep = NULL), else the dropout probability handed over with a keep mask (0.0: a mask, scale 1).
# running: running_mean / running_var given.  offset: size of the channel means of the pre-BatchNorm values (through the bias).
# plan = (forward tile, forward rows_big, data-gradient tile, data-gradient rows_big, weight-gradient tile, K pieces of the weight
# gradient, length of a piece or 0) as gvx_debug_conv_train_plan reports it; tiles as the four digits of <WR,WC,TM,TN>.
ConvTrainCase = collections.namedtuple("ConvTrainCase", "name B Cin Cout T k act p plan running offset")


def _cv(name, B, Cin, Cout, T, k, act, p, plan, running=True, offset=0.0):
    return ConvTrainCase(name, B, Cin, Cout, T, k, act, p, plan, running, offset)


CONV_TRAIN_CASES = [
    # T against the halo (pad = 0 .. 3 rows: T = 1, 2 are shorter than it) and against the K-major loader's (group, index) increments
    # under wmap = {R = T, ...}: every k a new group (T = 1), a quad of k across groups (T = 2, 3), several groups per k-tile of 32
    # (T < 32), T around 32 and 64; B = 1 is one group.  Fewer than 512 rows: the weight gradient in one piece
    _cv("t_37x1_8to24_k5", 37, 8, 24, 1, 5, "none", None, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_1x1_24to40_k7", 1, 24, 40, 1, 7, "relu", 0.5, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_50x2_40to8_k5", 50, 40, 8, 2, 5, "tanh", 0.0, (4111, 0, 2311, 0, 2212, 1, 0)),
    _cv("t_1x2_24to24_k5", 1, 24, 24, 2, 5, "none", 0.9, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_33x3_8to40_k7", 33, 8, 40, 3, 7, "relu", None, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_1x3_40to24_k3", 1, 40, 24, 3, 3, "tanh", 0.5, (4111, 0, 2311, 0, 2212, 1, 0)),
    _cv("t_19x4_8to24_k3", 19, 8, 24, 4, 3, "none", 0.0, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_13x5_24to40_k5", 13, 24, 40, 5, 5, "relu", 0.9, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_1x5_40to8_k7", 1, 40, 8, 5, 7, "tanh", None, (4111, 0, 2311, 0, 2212, 1, 0)),
    _cv("t_11x7_24to24_k7", 11, 24, 24, 7, 7, "none", 0.5, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_9x7_8to40_k1", 9, 8, 40, 7, 1, "relu", 0.0, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_5x31_40to24_k5", 5, 40, 24, 31, 5, "tanh", 0.9, (4111, 0, 2311, 0, 2212, 1, 0)),
    _cv("t_5x32_8to24_k3", 5, 8, 24, 32, 3, "none", None, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_1x32_24to40_k5", 1, 24, 40, 32, 5, "relu", 0.5, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_5x33_40to8_k7", 5, 40, 8, 33, 7, "tanh", 0.0, (4111, 0, 2311, 0, 2212, 1, 0)),
    _cv("t_3x63_24to24_k5", 3, 24, 24, 63, 5, "none", 0.9, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_3x64_8to40_k1", 3, 8, 40, 64, 1, "relu", None, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_1x64_40to24_k5", 1, 40, 24, 64, 5, "tanh", 0.5, (4111, 0, 2311, 0, 2212, 1, 0)),
    _cv("t_3x65_8to24_k5", 3, 8, 24, 65, 5, "none", 0.0, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("t_1x65_24to40_k7", 1, 24, 40, 65, 7, "relu", 0.9, (2311, 0, 4111, 0, 2212, 1, 0)),
    # split-K weight gradient, few tiles: from 512 rows on, one more piece per 256 rows up to 8.  T = 1 (600 groups); T = 3, 5, 37, 50,
    # 27, 59, 89: every piece begins inside a sequence (kchunk % T != 0); T = 64, 128, 96, 512, 2048: at a sequence's first frame or in
    # the only sequence.  rows = 511 | 512, 513 (320 + 193) | 767 (2 pieces of 384, the last 383) | 768 | 2047 (7 pieces of 320, the
    # last 127) | 2048 (8 of 256)
    _cv("sk_600x1_40to8_k5", 600, 40, 8, 1, 5, "tanh", None, (4111, 0, 2311, 0, 2212, 2, 320)),
    _cv("sk_171x3_24to24_k3", 171, 24, 24, 3, 3, "none", 0.5, (4111, 0, 4111, 0, 2212, 2, 320)),
    _cv("sk_103x5_8to40_k5", 103, 8, 40, 5, 5, "relu", 0.0, (2311, 0, 4111, 0, 2212, 2, 320)),
    _cv("sk_14x37_40to24_k5", 14, 40, 24, 37, 5, "tanh", 0.9, (4111, 0, 2311, 0, 2212, 2, 320)),
    _cv("sk_11x50_8to24_k7", 11, 8, 24, 50, 7, "none", None, (4111, 0, 4111, 0, 2212, 2, 320)),
    _cv("sk_8x64_24to40_k5", 8, 24, 40, 64, 5, "relu", 0.5, (2311, 0, 4111, 0, 2212, 2, 256)),
    _cv("sk_4x128_40to8_k3", 4, 40, 8, 128, 3, "tanh", 0.0, (4111, 0, 2311, 0, 2212, 2, 256)),
    _cv("sk_7x73_24to24_k5", 7, 24, 24, 73, 5, "none", 0.9, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("sk_1x512_8to40_k5", 1, 8, 40, 512, 5, "relu", None, (2311, 0, 4111, 0, 2212, 2, 256)),
    _cv("sk_19x27_40to24_k5", 19, 40, 24, 27, 5, "tanh", 0.5, (4111, 0, 2311, 0, 2212, 2, 320)),
    _cv("sk_13x59_8to24_k3", 13, 8, 24, 59, 3, "none", 0.0, (4111, 0, 4111, 0, 2212, 2, 384)),
    _cv("sk_12x64_24to40_k5", 12, 24, 40, 64, 5, "relu", 0.9, (2311, 0, 4111, 0, 2212, 3, 256)),
    _cv("sk_8x96_40to8_k1", 8, 40, 8, 96, 1, "tanh", None, (4111, 0, 2311, 0, 2212, 3, 256)),
    _cv("sk_23x89_24to24_k5", 23, 24, 24, 89, 5, "none", 0.5, (4111, 0, 4111, 0, 2212, 7, 320)),
    _cv("sk_16x128_8to40_k5", 16, 8, 40, 128, 5, "relu", 0.0, (2311, 0, 4111, 0, 2212, 8, 256)),
    _cv("sk_1x2048_40to24_k3", 1, 40, 24, 2048, 3, "tanh", 0.9, (4111, 0, 2311, 0, 2212, 8, 256)),
    # the 160-tile shape 512 x 2560: whole up to 767 rows, 3 pieces from 768 (2047: 704 + 704 + 639), 8 from 2048
    _cv("sk_13x59_512to512_k5", 13, 512, 512, 59, 5, "none", None, (2211, 0, 2211, 0, 2212, 1, 0)),
    _cv("sk_12x64_512to512_k5", 12, 512, 512, 64, 5, "relu", 0.5, (2211, 0, 2211, 0, 2212, 3, 256)),
    _cv("sk_23x89_512to512_k5", 23, 512, 512, 89, 5, "tanh", 0.0, (2211, 0, 2211, 0, 2212, 3, 704)),
    _cv("sk_16x128_512to512_k5", 16, 512, 512, 128, 5, "none", 0.9, (2211, 0, 2211, 0, 2212, 8, 256)),
    # rows against the walk of bn_stats_kernel / col_reduce_kernel (32 row lanes, four rows each per trip: 128 rows, then a tail loop)
    # and Cout against its 32 columns per workgroup (8: a quarter block; 40, 136: a partial last block); rows = 1, 2: the unbiased
    # factor's guard and rows / (rows - 1) = 2
    _cv("r_1x1_8to8_k3", 1, 8, 8, 1, 3, "relu", None, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x1_24to40_k3", 1, 24, 40, 1, 3, "tanh", 0.5, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x1_8to136_k3", 1, 8, 136, 1, 3, "none", 0.0, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_2x1_8to8_k3", 2, 8, 8, 1, 3, "relu", 0.9, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_2x1_24to40_k3", 2, 24, 40, 1, 3, "tanh", None, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_2x1_8to136_k3", 2, 8, 136, 1, 3, "none", 0.5, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x31_8to8_k3", 1, 8, 8, 31, 3, "relu", 0.0, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x31_24to40_k3", 1, 24, 40, 31, 3, "tanh", 0.9, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x31_8to136_k3", 1, 8, 136, 31, 3, "none", None, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_4x8_8to8_k3", 4, 8, 8, 8, 3, "relu", 0.5, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_4x8_24to40_k3", 4, 24, 40, 8, 3, "tanh", 0.0, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_4x8_8to136_k3", 4, 8, 136, 8, 3, "none", 0.9, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_3x11_8to8_k3", 3, 8, 8, 11, 3, "relu", None, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_3x11_24to40_k3", 3, 24, 40, 11, 3, "tanh", 0.5, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_3x11_8to136_k3", 3, 8, 136, 11, 3, "none", 0.0, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x127_8to8_k3", 1, 8, 8, 127, 3, "relu", 0.9, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x127_24to40_k3", 1, 24, 40, 127, 3, "tanh", None, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x127_8to136_k3", 1, 8, 136, 127, 3, "none", 0.5, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_2x64_8to8_k3", 2, 8, 8, 64, 3, "relu", 0.0, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_2x64_24to40_k3", 2, 24, 40, 64, 3, "tanh", 0.9, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_2x64_8to136_k3", 2, 8, 136, 64, 3, "none", None, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_3x43_8to8_k3", 3, 8, 8, 43, 3, "relu", 0.5, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_3x43_24to40_k3", 3, 24, 40, 43, 3, "tanh", 0.0, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_3x43_8to136_k3", 3, 8, 136, 43, 3, "none", 0.9, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_5x51_8to8_k3", 5, 8, 8, 51, 3, "relu", None, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_5x51_24to40_k3", 5, 24, 40, 51, 3, "tanh", 0.5, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_5x51_8to136_k3", 5, 8, 136, 51, 3, "none", 0.0, (2211, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x257_8to8_k3", 1, 8, 8, 257, 3, "relu", 0.9, (4111, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x257_24to40_k3", 1, 24, 40, 257, 3, "tanh", None, (2311, 0, 4111, 0, 2212, 1, 0)),
    _cv("r_1x257_8to136_k3", 1, 8, 136, 257, 3, "none", 0.5, (2211, 0, 4111, 0, 2212, 1, 0)),
    # the model's own layers at the benchmark's training shape 32 x 200 (<4,1,1,3> for 80 channels above 4096 rows, <2,2,1,2>, the
    # elementwise kernels' grid-stride loops: 6400 x 512 > 4096 x 256), once at 32 x 800 (<4,2,1,2> plus the second launch of 64 x 64
    # tiles from row 24576 = sequence 30, frame 576), at one utterance of 568 frames and at 3 x 50 (<2,3,1,1> for the data gradient)
    _cv("m_32x200_80to512_k5", 32, 80, 512, 200, 5, "tanh", 0.5, (2212, 0, 4113, 0, 2212, 8, 832)),
    _cv("m_32x200_512to512_k5", 32, 512, 512, 200, 5, "relu", 0.5, (2212, 0, 2212, 0, 2212, 8, 832)),
    _cv("m_32x200_512to80_k5", 32, 512, 80, 200, 5, "none", 0.5, (4113, 0, 2212, 0, 2212, 6, 1088)),
    _cv("m_32x800_512to512_k5", 32, 512, 512, 800, 5, "tanh", 0.5, (4212, 24576, 4212, 24576, 2212, 8, 3200)),
    _cv("m_1x568_512to512_k5", 1, 512, 512, 568, 5, "tanh", 0.5, (2211, 0, 2211, 0, 2212, 1, 0)),
    _cv("m_3x50_80to512_k5", 3, 80, 512, 50, 5, "tanh", 0.5, (2211, 0, 2311, 0, 2212, 1, 0)),
    _cv("m_1x568_512to80_k5", 1, 512, 80, 568, 5, "none", None, (2311, 0, 2211, 0, 2212, 2, 320)),
    # 12 x 36 = 432 tiles of 128 x 128 in the weight gradient: the <2,2,2,2> K-major tile under a two-level map (the model never
    # reaches it; the code can)
    _cv("big_2x37_512to1536_k9", 2, 512, 1536, 37, 9, "tanh", 0.5, (2211, 0, 2211, 0, 2222, 1, 0)),
    # options on small shapes: no running statistics; channel means of order 1e3 (forward and backward)
    _cv("norun_5x13_24to40_k5", 5, 24, 40, 13, 5, "tanh", 0.5, (2311, 0, 4111, 0, 2212, 1, 0), running=False),
    _cv("norun_7x80_8to24_k3", 7, 8, 24, 80, 3, "relu", None, (4111, 0, 4111, 0, 2212, 2, 320), running=False),
    _cv("off_5x31_24to40_k5", 5, 24, 40, 31, 5, "tanh", 0.5, (2311, 0, 4111, 0, 2212, 1, 0), offset=1000.0),
    _cv("off_9x64_40to24_k3", 9, 40, 24, 64, 3, "relu", None, (4111, 0, 2311, 0, 2212, 2, 320), offset=1000.0),
    _cv("off_3x3_8to136_k5", 3, 8, 136, 3, 5, "none", 0.0, (2211, 0, 4111, 0, 2212, 1, 0), offset=1000.0),
]
CONV_TRAIN_BY_NAME = {c.name: c for c in CONV_TRAIN_CASES}
# run once more with dx = NULL (everything else bit-equal) and with x_wgrad given (only dw changes, bit-equal elsewhere)
CONV_TRAIN_OPTION_CASES = ["t_50x2_40to8_k5", "t_5x33_40to8_k7", "sk_103x5_8to40_k5"]
# B sequences of T frames against one sequence of B T frames: the same rows, other halos - the row maps' R matters
CONV_TRAIN_REGROUP_CASES = ["t_13x5_24to40_k5", "sk_14x37_40to24_k5", "sk_600x1_40to8_k5"]
CONV_TRAIN_BIG = "m_32x800_512to512_k5"   # its float64 reference is 2 x 10^11 flops on the CPU: one such case


def conv_train_plan(lib, B, Cin, Cout, T, k):
    """(status, (forward tile, rows_big, data-gradient tile, rows_big, weight-gradient tile, K pieces, piece length)) of
    gvx_debug_conv_train_plan.  Host arithmetic only; the export is in neither the public header nor _lib.SIGNATURES."""
    fn = lib.gvx_debug_conv_train_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    out = (C.c_int * 8)(*([-1] * 8))
    rc = fn(B, Cin, Cout, T, k, out)
    return rc, (out[0], out[1], out[2], out[3], out[4], out[6], out[7]), out[5]


# ---- the forward recurrences (gvx_decoder_teacher_forced(_train), gvx_decoder_autoregressive, gvx_encoder_lstm_forward,
# gvx_encoder_forward): the cases tests/test_forward_loops_gpu.py runs, each with the plan it is there for.
# tests/test_host_cpu.py pins every line against gvx_debug_decoder_plan / gvx_debug_encoder_resident on the CPU, and both sides of
# every threshold of plan_teacher_forced / plan_autoregressive, so a retuned plan fails there and the cases get re-aimed. -----------
# dims: a key of FWD_DIMS.  env: GVX_* variables set while the handle is created (read_knobs reads them once).  setter: an export
# called as setter(handle, 0) afterwards.  lengths: as bptt_lengths.  mode (teacher-forced): 0 inference, 1 training call with the
# whole tape, 2 training call with a partial tape; drop: hidden-state dropout on (p_att 0.2, p_dec 0.5) in a training call.
# plan: teacher-forced (kind, pa_layout, tile_layout, rows64, pre_gate, timeout_check, side_stream, graph);
#       autoregressive (kind, split_h, fold, graph);  encoder: (resident,).
# What the argument checks refuse of the shapes one would list (pinned in tests/test_host_cpu.py, FWD_REFUSED_DIMS): channel sizes
# that are no multiple of 8 - n_mels 79 and 83, att_dim 1, prenet_dim 20 - are GVX_ERR_UNSUPPORTED at gvx_model_create, so the
# padded projection stride is run at n_mels 72 / 88 and the odd layer sizes with P = 24, a = 8.
FwdCase = collections.namedtuple("FwdCase", "name dims env setter B L T lengths mode drop plan")
FWD_DIMS = {
    "def": dict(model={}, n_mels=80),
    "small": dict(model=dict(symbols_embedding_dim=32, encoder_embedding_dim=32, encoder_kernel_size=3, encoder_n_convolutions=2,
                             decoder_rnn_dim=64, attention_rnn_dim=48, prenet_dim=24, attention_dim=16, attention_location_n_filters=8,
                             attention_location_kernel_size=7, postnet_embedding_dim=40, postnet_kernel_size=5, postnet_n_convolutions=3),
                  n_mels=24),   # SMALL of tests/golden/cases.py (kl = 7)
    # the odd set of the BPTT table on multiples of 8: E + A = 88, A + E + D = 144 (padded product columns), kl = 5
    "odd": dict(model=dict(symbols_embedding_dim=48, encoder_embedding_dim=48, encoder_kernel_size=3, encoder_n_convolutions=1,
                           decoder_rnn_dim=56, attention_rnn_dim=40, prenet_dim=24, attention_dim=24, attention_location_n_filters=12,
                           attention_location_kernel_size=5, postnet_embedding_dim=16, postnet_kernel_size=3, postnet_n_convolutions=1),
                n_mels=16),
    "a8_F1_kl1": dict(model=dict(symbols_embedding_dim=32, encoder_embedding_dim=32, encoder_kernel_size=3, encoder_n_convolutions=1,
                                 decoder_rnn_dim=32, attention_rnn_dim=32, prenet_dim=16, attention_dim=8, attention_location_n_filters=1,
                                 attention_location_kernel_size=1, postnet_embedding_dim=16, postnet_kernel_size=3, postnet_n_convolutions=1),
                      n_mels=16),
    "p128": dict(model=dict(prenet_dim=128), n_mels=80),
    "mels72": dict(model={}, n_mels=72),    # PS() 76, PSB() 80
    "mels88": dict(model={}, n_mels=88),    # PS() 92, PSB() 96: the resident autoregressive pair stops at n_mels 80
    "att16": dict(model=dict(attention_dim=16), n_mels=80),
    "att256": dict(model=dict(attention_dim=256), n_mels=80),
    "dec512": dict(model=dict(decoder_rnn_dim=512), n_mels=80),   # E / 4 != D / 8: no fold
}
FWD_REFUSED_DIMS = [dict(n_mels=79), dict(n_mels=83), dict(attention_dim=1), dict(prenet_dim=20)]
_PA0 = "gvx_model_set_persistent_attention"


def _tf(name, B, L, T, plan, dims="def", env=None, setter=None, lengths="ragged", mode=0, drop=False):
    return FwdCase(name, dims, env or {}, setter, B, L, T, lengths, mode, drop, plan)


_K2L1 = (2, 1, 1, 0, 1, 1, 1, 0)
_K2L2 = (2, 2, 2, 0, 1, 1, 1, 0)
_K2L2_224 = (2, 2, 1, 0, 1, 1, 1, 0)
_K1L1, _K1L2, _K1R64 = (1, 1, 1, 0, 1, 1, 1, 1), (1, 2, 2, 0, 1, 1, 1, 1), (1, 3, 3, 1, 1, 1, 1, 1)
_K0 = lambda lay, pre=0: (0, lay, lay, 0, pre, pre, 0, 1)
_R64 = {"GVX_TF_ROWS64": "1"}
TF_CASES_FWD = (
    # kind 2, layout 1 (224 workgroups beside <= 32 attention workgroups); L = 2, 15, 16: the halo of kl = 31 wider than the row
    [_tf("k2_%dx%dx%d" % s, *s, _K2L1, lengths=ln) for s, ln in (((1, 1, 1), "full"), ((1, 128, 3), "full"), ((2, 5, 4), "ragged"), ((3, 33, 6), "ragged"),
                                                                  ((17, 127, 5), "ragged"), ((31, 128, 3), "short"), ((32, 128, 12), "ragged"),
                                                                  ((32, 1, 2), "full"), ((3, 2, 3), "ragged"), ((3, 15, 3), "ragged"), ((3, 16, 3), "full"))]
    # kind 2, layout 2 on the 192-workgroup deal (B <= 2 or B > 16)
    + [_tf("k2_%dx%dx%d" % s, *s, _K2L2) for s in ((1, 129, 3), (2, 256, 3), (17, 129, 3), (32, 190, 4), (32, 256, 3))]
    # ... on the 224-workgroup deal (3 .. 16 rows), and the same shapes sent back to 192 workgroups
    + [_tf("k2_%dx%dx%d" % s, *s, _K2L2_224) for s in ((3, 129, 3), (16, 190, 5), (16, 256, 3))]
    + [_tf("k2_long192_%dx%dx%d" % s, *s, _K2L2, env={"GVX_TF_LONG_224": "0"}) for s in ((3, 129, 3), (16, 190, 5), (16, 256, 3))]
    # kind 1: the weight-streaming launch per step beside the resident attention kernel
    + [_tf("k1_5x77x4", 5, 77, 4, _K1L1, env={"GVX_TF_RESIDENT": "0"}), _tf("k1_32x128x3", 32, 128, 3, _K1L1, env={"GVX_TF_RESIDENT": "0"}),
       _tf("k1_4x200x3", 4, 200, 3, _K1L2, env={"GVX_TF_RESIDENT": "0"}), _tf("k1_32x256x3", 32, 256, 3, _K1L2, env={"GVX_TF_RESIDENT": "0"})]
    # ... on layout 3: 33 .. 64 rows in one call, two batch tiles per workgroup
    + [_tf("rows64_%dx%dx%d" % s, *s, _K1R64, env=_R64) for s in ((33, 21, 3), (40, 50, 4), (64, 1, 2), (64, 128, 3))]
    # kind 0 at the default sizes: L past 256, the handle that shares the chip, the two-launch attention, 33 .. 64 rows direct
    + [_tf("k0_2x257x3", 2, 257, 3, _K0(0)), _tf("k0_3x300x3", 3, 300, 3, _K0(0)),
       _tf("k0_pa0_5x40x4", 5, 40, 4, _K0(1), setter=_PA0), _tf("k0_pa0_32x128x3", 32, 128, 3, _K0(1), setter=_PA0),
       _tf("k0_split_4x60x3", 4, 60, 3, _K0(1), env={"GVX_ATTN_SPLIT": "1"}), _tf("k0_split_3x200x3", 3, 200, 3, _K0(2), env={"GVX_ATTN_SPLIT": "1"}),
       _tf("k0_40x30x3", 40, 30, 3, _K0(3)), _tf("k0_64x128x2", 64, 128, 2, _K0(3))]
    # one case per layout under each of the remaining knobs
    + [_tf("depth6_k1_6x90x3", 6, 90, 3, _K1L1, env={"GVX_PA_DEPTH": "6", "GVX_TF_RESIDENT": "0"}),
       _tf("depth6_k1_6x140x3", 6, 140, 3, _K1L2, env={"GVX_PA_DEPTH": "6", "GVX_TF_RESIDENT": "0"}),
       _tf("noprefetch_6x90x3", 6, 90, 3, _K0(1), env={"GVX_ATTN_PREFETCH": "0"}, setter=_PA0),
       _tf("noprefetch_6x140x3", 6, 140, 3, _K0(2), env={"GVX_ATTN_PREFETCH": "0"}, setter=_PA0),
       _tf("pool2_6x90x3", 6, 90, 3, _K2L1, env={"GVX_SIDE_POOL": "2"}), _tf("pool2_6x140x3", 6, 140, 3, _K2L2_224, env={"GVX_SIDE_POOL": "2"})]
    # other layer sizes: launches per step
    + [_tf("small_5x13x6", 5, 13, 6, _K0(1), dims="small"), _tf("small_33x9x2", 33, 9, 2, _K0(3), dims="small"),
       _tf("odd_3x33x4", 3, 33, 4, _K0(1), dims="odd"), _tf("odd_32x9x3", 32, 9, 3, _K0(1), dims="odd"),
       _tf("a8_F1_kl1_3x9x3", 3, 9, 3, _K0(1), dims="a8_F1_kl1")]
    + [_tf("small_kl7_L%d" % L, 3, L, 3, _K0(1), dims="small") for L in (1, 2, 3, 4)]
    + [_tf("mels72_4x20x3", 4, 20, 3, _K2L1, dims="mels72"), _tf("mels88_4x20x3", 4, 20, 3, _K2L1, dims="mels88"),
       # prenet_dim 128: the resident tile kernel at another Prenet width (k-group offsets of its weight fragments; these two cases
       # found it reading the fragments of prenet_dim 256 there), inference and training deals
       _tf("p128_4x20x3", 4, 20, 3, _K2L1, dims="p128"), _tf("p128_5x150x3", 5, 150, 3, _K2L2_224, dims="p128"),
       _tf("p128_20x150x3", 20, 150, 3, _K2L2, dims="p128"),
       _tf("p128_tr_drop_4x20x3", 4, 20, 3, _K2L1, dims="p128", mode=1, drop=True),
       _tf("p128_tr_drop_20x150x3", 20, 150, 3, _K2L2, dims="p128", mode=1, drop=True)]
)
_TR = dict(mode=1)
TF_TRAIN_CASES_FWD = (
    # whole tape on the resident kernel: both layouts, both deals; dropout off and on
    [_tf("tr_k2_4x30x4", 4, 30, 4, _K2L1, **_TR), _tf("tr_k2_drop_32x128x3", 32, 128, 3, _K2L1, drop=True, **_TR),
     _tf("tr_k2_drop_20x150x3", 20, 150, 3, _K2L2, drop=True, **_TR), _tf("tr_k2_2x256x3", 2, 256, 3, _K2L2, **_TR),
     _tf("tr_k2_drop_9x190x3", 9, 190, 3, _K2L2_224, drop=True, **_TR),
     # a partial tape, GVX_TRAIN_RESIDENT_LOOP=0: the launch per step beside the resident attention kernel (never replayed: the tape)
     _tf("tr_part_k1_drop_4x30x4", 4, 30, 4, (1, 1, 1, 0, 1, 1, 1, 0), mode=2, drop=True),
     _tf("tr_part_k1_5x200x3", 5, 200, 3, (1, 2, 2, 0, 1, 1, 1, 0), mode=2),
     _tf("tr_loop0_k1_drop_6x40x3", 6, 40, 3, (1, 1, 1, 0, 1, 1, 1, 0), env={"GVX_TRAIN_RESIDENT_LOOP": "0"}, drop=True, **_TR),
     # kind 0: L past 256, GVX_TRAIN_RESIDENT=0 (pre_gate stays: the shape could run beside the kernel in inference mode)
     _tf("tr_k0_drop_3x257x3", 3, 257, 3, (0, 0, 0, 0, 0, 0, 0, 0), drop=True, **_TR),
     _tf("tr_res0_k0_drop_6x40x3", 6, 40, 3, (0, 1, 1, 0, 1, 1, 0, 0), env={"GVX_TRAIN_RESIDENT": "0"}, drop=True, **_TR),
     _tf("tr_small_drop_4x9x5", 4, 9, 5, (0, 1, 1, 0, 0, 0, 0, 0), dims="small", drop=True, **_TR),
     _tf("tr_small_part_4x9x5", 4, 9, 5, (0, 1, 1, 0, 0, 0, 0, 0), dims="small", mode=2)]
)


def _ar(name, B, L, T, plan, dims="def", env=None, setter=None, lengths="ragged"):
    return FwdCase(name, dims, env or {}, setter, B, L, T, lengths, 0, False, plan)


_A2, _A1 = (2, 0, 1, 0), (1, 0, 1, 1)
AR_CASES_FWD = (
    # two resident kernels: layout 1 (1, 5, 32 rows; L 1, 77, 128), layout 2 (1, 16 rows; L 129, 256)
    [_ar("ar2_1x1", 1, 1, 8, _A2, lengths="full"), _ar("ar2_5x77", 5, 77, 12, _A2), _ar("ar2_32x128", 32, 128, 10, _A2),
     _ar("ar2_1x129", 1, 129, 8, _A2, lengths="full"), _ar("ar2_16x256", 16, 256, 8, _A2),
     # launches per step: 17 .. 32 rows of 129 .. 256 tokens, L past 256, and every knob that leaves the pair
     _ar("ar0_17x129", 17, 129, 8, (0, 1, 1, 1)), _ar("ar0_2x257", 2, 257, 8, (0, 1, 1, 1)),
     _ar("ar1_5x77", 5, 77, 20, _A1, env={"GVX_AR_RESIDENT": "1", "GVX_AR_RESIDENT_LOOP": "0"}),
     _ar("ar0_loop0_5x77", 5, 77, 20, (0, 1, 1, 1), env={"GVX_AR_RESIDENT_LOOP": "0"}),
     _ar("ar0_nosplit_5x77", 5, 77, 8, (0, 0, 1, 1), env={"GVX_AR_RESIDENT_LOOP": "0", "GVX_AR_SPLIT_H": "0"}),
     _ar("ar0_att16_3x40", 3, 40, 8, (0, 0, 1, 1), dims="att16"), _ar("ar0_att256_3x40", 3, 40, 8, (0, 0, 1, 1), dims="att256"),
     # fold off: 36 rows in one call, a size with E / 4 != D / 8
     _ar("ar0_36x30", 36, 30, 6, (0, 0, 0, 1)), _ar("ar0_dec512_3x40", 3, 40, 8, (0, 1, 0, 1), dims="dec512"),
     _ar("ar0_p128_4x50", 4, 50, 8, (0, 1, 1, 1), dims="p128"), _ar("ar0_mels88_4x50", 4, 50, 8, (0, 1, 1, 1), dims="mels88"),
     _ar("ar0_small_5x13", 5, 13, 20, (0, 0, 1, 1), dims="small")]
)
# both sides of every threshold of the two plan functions, default handle: (B, L) -> teacher-forced (kind, pa_layout, tile_layout),
# autoregressive kind
FWD_THRESHOLDS = {
    (2, 200): ((2, 2, 2), 2), (3, 200): ((2, 2, 1), 2), (16, 200): ((2, 2, 1), 2), (17, 200): ((2, 2, 2), 0),
    (32, 100): ((2, 1, 1), 2), (33, 100): ((0, 3, 3), 0), (64, 100): ((0, 3, 3), 0), (65, 100): ((0, 0, 0), 0),
    (5, 128): ((2, 1, 1), 2), (5, 129): ((2, 2, 1), 2), (5, 256): ((2, 2, 1), 2), (5, 257): ((0, 0, 0), 0),
}

# encoder recurrence (gvx_encoder_lstm_forward): the (B, L, H) of ENC_BPTT_CASES, so forward and backward share shapes, plus the
# launch-per-position loop at H = 256 by knob.  plan: 1 = the one resident launch (B <= 32, H = 256)
EncFwdCase = collections.namedtuple("EncFwdCase", "name B L H lengths env plan")
ENC_FWD_CASES = ([EncFwdCase(c.name, c.B, c.L, c.H, c.lengths, {}, 1 if (c.H == 256 and c.B <= 32) else 0) for c in ENC_BPTT_CASES]
                 + [EncFwdCase("H256_3x21_per_position", 3, 21, 256, "ragged", {"GVX_ENC_PERSISTENT": "0"}, 0),
                    EncFwdCase("H256_32x150_per_position", 32, 150, 256, "ragged", {"GVX_ENC_PERSISTENT": "0"}, 0)])
# gvx_encoder_forward whole (embedding, convolutions, recurrence), default sizes: L shorter than the kernel of 5, 128, 300
ENC_WHOLE_CASES = [(3, 1), (3, 2), (3, 4), (4, 128), (2, 300)]


def fwd_configs(dims_name, n_tokens=40):
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig

    d = FWD_DIMS[dims_name]
    return (Tacotron2Config(**d["model"]), AudioConfig(filter_length=1024, hop_length=256, n_mels=d["n_mels"], log_func="np.log"),
            TextConfig(n_tokens=n_tokens))


def enc_fwd_configs(H):
    """A model whose encoder BiLSTM has H units per direction; everything around it as small as the dims checks allow."""
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig

    if H == 256:
        return fwd_configs("def")
    m = dict(FWD_DIMS["a8_F1_kl1"]["model"], symbols_embedding_dim=2 * H, encoder_embedding_dim=2 * H)
    return Tacotron2Config(**m), AudioConfig(filter_length=1024, hop_length=256, n_mels=16, log_func="np.log"), TextConfig(n_tokens=40)


def create_handle(lib, dims, env=None, setter=None):
    """gvx_model_create under `env` (restored afterwards), then setter(handle, 0).  Host only: no blob is bound."""
    h = C.c_void_p()
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rc = lib.gvx_model_create(C.byref(dims), C.byref(h))
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert rc == 0, (rc, lib.gvx_last_error())
    if setter:
        assert getattr(lib, setter)(h, 0) == 0
    return h


def decoder_plan(lib, handle, mode, B, L):
    """(status, teacher-forced plan (8 fields), autoregressive plan (4 fields)) of gvx_debug_decoder_plan.  Host arithmetic only; the
    export is in neither the public header nor _lib.SIGNATURES."""
    fn = lib.gvx_debug_decoder_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 12)(*([-1] * 12))
    rc = fn(handle, mode, B, L, out)
    return rc, tuple(out[:8]), tuple(out[8:])


def graph_replays(lib, handle):
    fn = lib.gvx_debug_graph_replays
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p]
    return int(fn(handle))


def encoder_resident(lib, handle, B):
    fn = lib.gvx_debug_encoder_resident
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int]
    return int(fn(handle, B))


# ---- the whole training step (Tacotron2._forward_train + training.train_backward + train_step): the cases
# tests/test_train_step_gpu.py runs against the float64 autograd of tests/train_ref64.py, each with what it is there for.
# tests/test_host_cpu.py pins every line's chunk list and, through gvx_teacher_forced_loop_kind / gvx_teacher_forced_rows_per_call and
# the training plan of gvx_debug_decoder_plan, the decoder loop each chunk is meant to reach. ---------------------------------------
# dims: a key of TRAIN_STEP_DIMS.  Token lengths as bptt_lengths("ragged"): rows from L down to 1; mel lengths as
# train_step_mel_lengths: one row of T frames, one of 1 frame (B >= 2).  forced: None, "resident_off"
# (gvx_model_set_resident_kernels(handle, 0)) or "enc_walk_per_step" (model._enc_bptt_resident = False).
# chunks: the row ranges of the recurrent part.  kinds: per chunk (loop kind of the training call, loop kind of an inference call).
TrainStepCase = collections.namedtuple("TrainStepCase", "name dims B L T mask_padding forced chunks kinds why")
TRAIN_STEP_DIMS = dict(FWD_DIMS, unusual=dict(
    model=dict(symbols_embedding_dim=48, encoder_embedding_dim=48, encoder_kernel_size=5, encoder_n_convolutions=2, decoder_rnn_dim=56,
               attention_rnn_dim=40, prenet_dim=16, attention_dim=24, attention_location_n_filters=12, attention_location_kernel_size=9,
               postnet_embedding_dim=32, postnet_kernel_size=3, postnet_n_convolutions=3), n_mels=16))


def _ts(name, dims, B, L, T, kinds, why, mask_padding=True, forced=None):
    chunks = tuple((lo, min(B, lo + 32)) for lo in range(0, B, 32))
    return TrainStepCase(name, dims, B, L, T, mask_padding, forced, chunks, tuple(kinds), why)


_S, _D2 = ((0, 0),), ((2, 2),)
TRAIN_STEP_CASES = [
    _ts("fixture_4x9x10", "small", 4, 9, 10, _S, "the shape of the reference's own fixture, reduced sizes"),
    # chunk edges at reduced sizes: 1, 2, 31, 32 rows in one chunk; 33 = 32 + 1, 64 = 32 + 32, 65 = 32 + 32 + 1
    _ts("small_1x9x6", "small", 1, 9, 6, _S, "one row"),
    _ts("small_2x9x6", "small", 2, 9, 6, _S, "two rows: token lengths 9 and 1, mel lengths 6 and 1"),
    _ts("small_31x9x5", "small", 31, 9, 5, _S, "one row short of a chunk"),
    _ts("small_32x9x5", "small", 32, 9, 5, _S, "a full chunk"),
    _ts("small_33x9x5", "small", 33, 9, 5, _S * 2, "a second chunk of one row: _accumulate, row offsets"),
    _ts("small_64x9x4", "small", 64, 9, 4, _S * 2, "two full chunks"),
    _ts("small_65x9x4", "small", 65, 9, 4, _S * 3, "three chunks, the last of one row"),
    _ts("small_5x9x1", "small", 5, 9, 1, _S, "T = 1: the tape's slot shifts with a single step"),
    _ts("small_5x1x6", "small", 5, 1, 6, _S, "L = 1: one token per row"),
    _ts("small_nomask_4x9x10", "small", 4, 9, 10, _S, "mask_padding = False", mask_padding=False),
    _ts("unusual_6x19x8", "unusual", 6, 19, 8, _S, "layer sizes no fast path is built for"),
    # default layer sizes
    _ts("def_3x24x12", "def", 3, 24, 12, _D2, "default sizes, one small chunk on the resident loop"),
    _ts("def_32x128x20", "def", 32, 128, 20, _D2, "the benchmark's rows and tokens"),
    _ts("def_37x40x8", "def", 37, 40, 8, _D2 * 2, "two chunks of different size (32 + 5) at default sizes"),
    _ts("def_4x129x5", "def", 4, 129, 5, _D2, "first L of the deal for rows above 128 tokens"),
    _ts("def_5x150x6", "def", 5, 150, 6, _D2, "rows above 128 tokens"),
    _ts("def_3x300x5", "def", 3, 300, 5, ((0, 0),), "L past the resident limit: a launch pair per step"),
    _ts("def_32x60x200", "def", 32, 60, 200, _D2, "many addends: 6400 (t, b) rows per weight gradient"),
    _ts("def_resident_off_3x24x12", "def", 3, 24, 12, ((0, 0),), "forced: launch-per-step kernels", forced="resident_off"),
    _ts("def_enc_walk_3x24x12", "def", 3, 24, 12, _D2, "forced: encoder BiLSTM backward as a launch per time step", forced="enc_walk_per_step"),
]
TRAIN_STEP_BY_NAME = {c.name: c for c in TRAIN_STEP_CASES}
TRAIN_STEP_MANY = "def_32x60x200"
# the four consecutive steps of the trajectory tests: (B, L, T) per step, other rows and frames each time
TRAIN_TRAJECTORY = {"small": [(5, 9, 7), (33, 11, 4), (3, 6, 9), (34, 9, 5)], "def": [(3, 24, 6), (33, 20, 4), (2, 30, 8), (5, 16, 5)]}


def train_step_configs(case):
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig

    d = TRAIN_STEP_DIMS[case.dims if isinstance(case, TrainStepCase) else case]
    mc = Tacotron2Config(**d["model"])
    if isinstance(case, TrainStepCase):
        mc.mask_padding = case.mask_padding
    return mc, AudioConfig(filter_length=1024, hop_length=256, n_mels=d["n_mels"], log_func="np.log"), TextConfig(n_tokens=40)


def train_step_mel_lengths(B, T):
    """Mel lengths of a case: spread over 1 .. T, the last row with one frame (B >= 2), row (B - 1) // 2 with all T."""
    ml = [1 + (i * 7 + 3) % T for i in range(B)]
    ml[-1] = 1
    ml[(B - 1) // 2] = T
    return ml
