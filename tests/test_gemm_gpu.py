"""GPU: the dense fp32 GEMM (genvox_amd/csrc/gemm_f32.hip) as what it is - every tile shape of launch_gemm, the two-launch
split, every k tail, split-K and the K-major form - through gvx_train_gemm_nt / gvx_train_gemm_tn, and the implicit-GEMM
convolution edges (row_len, c_halo, two-level row maps) through gvx_postnet_forward.

Two references for every shape.  Exact: operands are integers in [-3, 3], so every partial sum in any order is an integer below
2^24 and the fp32 result must EQUAL the product (taken in float64, where it is exact too): a skipped, doubled or foreign k, row
or column cannot hide in a tolerance.  Rounded: mixed-magnitude operands against float64 within the bound that holds for any
order of an fma chain, (K + 2 + pieces) 2^-24 (|A| |W|^T + |bias|) per element.  The operands' padding columns hold NaN (the k
tail must be selected away, not multiplied by zero), C's padding columns and guard rows hold a sentinel that must survive.
The shapes and the branch each one is there for are in tests/helpers.py; tests/test_host_cpu.py pins them on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from genvox_amd import _lib
from tests.helpers import (GEMM_8W_CASES, GEMM_BRANCH_CASES, GEMM_CASES, GEMM_KMAJOR_CASES, GEMM_KTAIL_CASES, GEMM_SPLITK_CASES,
                           GemmCase, gemm_plan, gemm_scratch_bytes)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SENTINEL = 0x5A5A5A5A   # bit pattern of the untouched parts of C (1.5e16 as a float)
GUARD = 3               # sentinel rows before and after C


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def make_operands(c, kind, seed):
    """a, w, bias of case c: [M, K], [N, K] (row-major form) or [K, M], [K, N] (K-major form; no bias there)."""
    g = _gen(seed)
    sa, sw = ((c.K, c.M), (c.K, c.N)) if c.kmajor else ((c.M, c.K), (c.N, c.K))
    if kind == "exact":
        assert 9 * c.K + 3 < 2 ** 24
        draw = lambda s: torch.randint(-3, 4, s, generator=g, device="cuda").float()
    else:   # magnitudes from 1e-2 to 1e2, element by element
        draw = lambda s: torch.randn(s, generator=g, device="cuda") * 10.0 ** (4.0 * torch.rand(s, generator=g, device="cuda") - 2.0)
    a, w = draw(sa), draw(sw)
    bias = None if c.kmajor else draw((c.N,))
    return a, w, bias


def with_nan_padding(x, pad):
    """x in a buffer whose rows are `pad` floats longer, the padding NaN."""
    if pad == 0:
        return x.contiguous()
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device="cuda")
    buf[:, :x.shape[1]] = x
    return buf


def call_gemm(lib, c, a, w, bias, padded, use_bias=True, expect_rc=0):
    """Runs case c on operands a, w (values only; this puts them into NaN-padded buffers when `padded`), checks C's padding
    columns and guard rows, returns C [M, N].  Leading dimensions of the operands stay multiples of 4 floats (16-byte loads)."""
    ab, wb = with_nan_padding(a, 4 if padded else 0), with_nan_padding(w, 12 if padded else 0)
    ldc = c.N + (5 if padded else 0)
    cbuf = torch.full((c.M + 2 * GUARD, ldc), SENTINEL, dtype=torch.int32, device="cuda")
    cptr = cbuf.data_ptr() + GUARD * ldc * 4
    nbytes = gemm_scratch_bytes(c)
    scratch = None if nbytes is None else torch.empty(nbytes // 4 + 64, device="cuda")
    if scratch is not None:
        scratch.view(torch.int32).fill_(SENTINEL)
    sp = None if scratch is None else scratch.data_ptr()
    if c.kmajor:
        rc = lib.gvx_train_gemm_tn(ab.data_ptr(), ab.shape[1], wb.data_ptr(), wb.shape[1], cptr, ldc, c.M, c.N, c.K, sp, nbytes or 0, _stream())
    else:
        rc = lib.gvx_train_gemm_nt(ab.data_ptr(), ab.shape[1], wb.data_ptr(), wb.shape[1], cptr, ldc, c.M, c.N, c.K,
                                   bias.data_ptr() if (use_bias and bias is not None) else None, sp, nbytes or 0, _stream())
    torch.cuda.synchronize()
    if expect_rc != 0:
        assert rc != 0, (c, rc)
        assert bool((cbuf == SENTINEL).all()), f"{c}: a refused call wrote to C"
        return None
    assert rc == 0, (c, rc, lib.gvx_last_error())
    assert bool((cbuf[:GUARD] == SENTINEL).all()) and bool((cbuf[GUARD + c.M:] == SENTINEL).all()), f"{c}: guard rows of C written"
    assert bool((cbuf[:, c.N:] == SENTINEL).all()), f"{c}: padding columns of C written"
    if scratch is not None:
        assert bool((scratch.view(torch.int32)[nbytes // 4:] == SENTINEL).all()), f"{c}: wrote past scratch_bytes"
    return cbuf[GUARD:GUARD + c.M, :c.N].contiguous().view(torch.float32)


def reference64(c, a, w, bias):
    """(product, bound weight) in float64: A W^T + bias and |A| |W|^T + |bias| (the K-major form: A^T Bm)."""
    a64, w64 = a.double(), w.double()
    if c.kmajor:
        return a64.t() @ w64, a64.abs().t() @ w64.abs()
    b64 = bias.double() if bias is not None else torch.zeros(c.N, dtype=torch.float64, device="cuda")
    return a64 @ w64.t() + b64, a64.abs() @ w64.abs().t() + b64.abs()


def check_exact(lib, c, padded, seed):
    a, w, bias = make_operands(c, "exact", seed)
    got = call_gemm(lib, c, a, w, bias, padded)
    want, _ = reference64(c, a, w, bias)
    assert torch.equal(got.double(), want), f"{c} padded={padded}: {int((got.double() != want).sum())} elements differ from the exact product, " \
                                            f"first at {(got.double() != want).nonzero()[:4].tolist()}"
    return got


def check_rounded(lib, c, padded, seed):
    """-> (C, largest |got - want| / bound)."""
    a, w, bias = make_operands(c, "rounded", seed)
    got = call_gemm(lib, c, a, w, bias, padded)
    want, weight = reference64(c, a, w, bias)
    bound = (c.K + 2 + c.pieces) * U * weight
    ratio = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())
    assert torch.isfinite(got).all() and ratio <= 1.0, f"{c} padded={padded}: error / bound = {ratio:.3f}"
    return got, ratio


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _ids(cases):
    return [f"{'tn' if c.kmajor else 'nt'}-{c.M}x{c.N}x{c.K}-{c.scratch}" for c in cases]


def test_every_listed_branch_is_reached(lib):
    """Through the same query the CPU test pins: each case lands where its line says, and together they reach every tile shape,
    the two-launch split, split-K on both forms and a split cut short by the scratch."""
    seen = set()
    for c in GEMM_CASES:
        rc, tile, rows_big, pieces = gemm_plan(lib, c.M, c.N, c.K, c.kmajor, gemm_scratch_bytes(c))
        assert (rc, tile, rows_big, pieces) == (0, c.tile, c.rows_big, c.pieces), c
        seen.add((c.kmajor, tile, rows_big > 0, pieces > 1))
    for want in [(0, 4111, False, False), (0, 2311, False, False), (0, 4113, False, False), (0, 2211, False, False), (0, 2212, False, False),
                 (0, 4212, False, False), (0, 4212, True, False), (1, 2212, False, False), (1, 2222, False, False),
                 (0, 2211, False, True), (0, 2311, False, True), (0, 4111, False, True), (1, 2212, False, True)]:
        assert want in seen, want


@pytest.mark.parametrize("c", GEMM_BRANCH_CASES + GEMM_KTAIL_CASES + GEMM_KMAJOR_CASES, ids=_ids(GEMM_BRANCH_CASES + GEMM_KTAIL_CASES + GEMM_KMAJOR_CASES))
def test_gemm_exact_and_rounded(lib, c):
    """No split-K: exact on integers and within the fma-chain bound of float64, dense and with NaN-padded leading dimensions;
    the same call twice gives the same bits."""
    seed = c.M * 7 + c.N * 3 + c.K
    for padded in (True, False):
        check_exact(lib, c, padded, seed)
        got, ratio = check_rounded(lib, c, padded, seed + 1)
    again, _ = check_rounded(lib, c, False, seed + 1)
    assert torch.equal(got, again), f"{c}: two runs of the same call differ"
    print(f"gemm {c}: error / bound {ratio:.3f}")


@pytest.mark.parametrize("c", GEMM_SPLITK_CASES, ids=_ids(GEMM_SPLITK_CASES))
def test_gemm_splitk_exact_rounded_and_reproducible(lib, c):
    """Split-K (and the same products with a scratch too small for the split that was wanted, or none): exact on integers - every
    k in exactly one piece, the short last piece included -, the rounded bound, bias added once, run-to-run bit equality."""
    seed = c.M * 5 + c.N + c.K + c.pieces
    for padded in (True, False):
        check_exact(lib, c, padded, seed)
        got, ratio = check_rounded(lib, c, padded, seed + 1)
    again, _ = check_rounded(lib, c, False, seed + 1)
    assert torch.equal(got, again), f"{c}: two runs of the same split-K call differ"
    print(f"split-K {c}: error / bound {ratio:.3f}")


@pytest.mark.parametrize("c", [GemmCase(200, 130, 36, 0, None, 2211, 0, 1), GemmCase(257, 24, 92, 0, None, 4111, 0, 1), GemmCase(65, 33, 44, 0, None, 2311, 0, 1),
                               GemmCase(4229, 96, 36, 0, None, 4113, 0, 1), GemmCase(12803, 512, 36, 0, None, 4212, 0, 1),
                               GemmCase(132, 260, 36, 1, None, 2212, 0, 1), GemmCase(132, 260, 33, 1, None, 2212, 0, 1)])
def test_k_tail_is_selected_away_not_multiplied_by_zero(lib, c):
    """The loads of the k tail are redirected to in-bounds elements (the start of the row; the first row of a K-major operand),
    so NaN in the padding alone cannot tell a select from a multiplication by zero.  An infinity in exactly those elements can:
    the product then holds +-inf where that element meets a non-zero weight and NaN where it meets a zero one - as float64 has
    it - and nothing else; a tail multiplied by zero turns the whole row (column) into NaN."""
    assert gemm_plan(lib, c.M, c.N, c.K, c.kmajor)[1] == c.tile and c.K % 32 != 0
    a, w, bias = make_operands(c, "exact", c.M + c.K)
    if c.kmajor:
        a[0, 5], w[0, 7] = float("inf"), float("-inf")
    else:
        a[5, :4], w[7, :4] = float("inf"), float("-inf")
        a[5, 4:], w[7, 4:] = a[5, 4:].abs(), w[7, 4:].abs()     # (so that no inf - inf arises in the row's own sums)
        w[:, :4], a[:, :4] = w[:, :4].abs(), a[:, :4].abs()
        a[5, :4], w[7, :4] = float("inf"), float("-inf")
    got = call_gemm(lib, c, a, w, bias, True)
    want, _ = reference64(c, a, w, bias)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{c}: {int(torch.isnan(got).sum())} NaN, float64 has {int(torch.isnan(want).sum())}"
    assert torch.equal(torch.nan_to_num(got.double(), nan=0.0), torch.nan_to_num(want, nan=0.0))
    assert int(torch.isinf(got).sum()) > 0 and int(torch.isfinite(got).sum()) >= (c.M - 1) * (c.N - 1)


def test_gemm_refused_shapes_leave_c_untouched(lib):
    """K % 4 != 0, K < 4 (row-major form); M, N or a leading dimension that is no multiple of 4 (K-major form): a non-zero
    status and not one word of C written."""
    for M, N, K in ((8, 8, 6), (8, 8, 2), (8, 8, 3), (130, 40, 33)):
        c = GemmCase(M, N, K, 0, None, 0, 0, 1)
        a, w, bias = make_operands(c, "exact", 1)
        call_gemm(lib, c, a, w, bias, False, expect_rc=-1)
    for M, N, K in ((6, 8, 8), (8, 6, 8), (2, 8, 8), (8, 3, 8), (130, 260, 64)):
        c = GemmCase(M, N, K, 1, None, 0, 0, 1)
        a, w, bias = make_operands(c, "exact", 2)
        call_gemm(lib, c, a, w, bias, False, expect_rc=-1)
    # K-major with good M, N but leading dimensions that are not multiples of 4
    M, N, K = 8, 12, 16
    a, w = torch.ones(K, M + 1, device="cuda"), torch.ones(K, N + 4, device="cuda")
    cbuf = torch.full((M, N), SENTINEL, dtype=torch.int32, device="cuda")
    assert lib.gvx_train_gemm_tn(a.data_ptr(), M + 1, w.data_ptr(), N + 4, cbuf.data_ptr(), N, M, N, K, None, 0, _stream()) != 0
    assert lib.gvx_train_gemm_tn(w.data_ptr(), N + 4, a.data_ptr(), M + 1, cbuf.data_ptr(), M, N, M, K, None, 0, _stream()) != 0
    torch.cuda.synchronize()
    assert bool((cbuf == SENTINEL).all())


def _sub_nt(lib, a, w, bias, rows=None, cols=None):
    """The product of a block of rows of a, or of a block of rows of w (columns of C), as a call of its own."""
    a2 = a if rows is None else a[rows[0]:rows[1]].contiguous()
    w2 = w if cols is None else w[cols[0]:cols[1]].contiguous()
    b2 = bias if cols is None else bias[cols[0]:cols[1]].contiguous()
    c = GemmCase(a2.shape[0], w2.shape[0], a.shape[1], 0, None, 0, 0, 1)
    return c, call_gemm(lib, c, a2, w2, b2, False)


@pytest.mark.parametrize("c", [x for x in GEMM_BRANCH_CASES if x.tile == 4212], ids=_ids([x for x in GEMM_BRANCH_CASES if x.tile == 4212]))
def test_results_do_not_depend_on_the_tile_shape(lib, c):
    """"Every output element sums its K products in the same order": a block of rows of a large product, computed again as a
    product of its own (which dispatches to another tile shape), and a block of its columns, must be the same bits - for blocks
    inside the big-tile launch, across rows_big, and inside the m_begin launch."""
    a, w, bias = make_operands(c, "rounded", c.M + c.K)
    full = call_gemm(lib, c, a, w, bias, False)
    edge = c.rows_big if c.rows_big else (c.M // 256) * 128
    blocks = [(1000, 1200), (edge - 70, edge + 58), (c.M - 133, c.M), (c.M - 7000, c.M), (0, 4100)]
    tiles = set()
    for lo, hi in blocks:
        sub, got = _sub_nt(lib, a, w, bias, rows=(lo, hi))
        tiles.add(gemm_plan(lib, sub.M, sub.N, sub.K)[1])
        assert torch.equal(got, full[lo:hi]), f"{c}: rows {lo}..{hi} differ between tile shapes ({int((got != full[lo:hi]).sum())} elements)"
    for lo, hi in ((0, 24), (c.N // 4, c.N // 4 + 80), (c.N - 97, c.N)):
        sub, got = _sub_nt(lib, a, w, bias, cols=(lo, hi))
        tiles.add(gemm_plan(lib, sub.M, sub.N, sub.K)[1])
        assert torch.equal(got, full[:, lo:hi]), f"{c}: columns {lo}..{hi} differ between tile shapes"
    assert len(tiles - {c.tile}) >= 3, tiles   # the blocks really took other shapes


def test_k_major_form_equals_row_major_form_bit_for_bit(lib):
    """The K-major loaders put the same [row][k] tiles into LDS: gvx_train_gemm_tn on A, Bm gives the bits of gvx_train_gemm_nt
    on their transposed copies, whichever tiles the two calls take."""
    for M, N, rows in ((132, 260, 36), (132, 260, 2560), (1536, 4096, 64), (4, 4, 32)):
        c = GemmCase(M, N, rows, 1, None, 0, 0, 1)
        a, w, _ = make_operands(c, "rounded", M + rows)
        tn = call_gemm(lib, c, a, w, None, True)
        nt = call_gemm(lib, GemmCase(M, N, rows, 0, None, 0, 0, 1), a.t().contiguous(), w.t().contiguous(), None, True)
        assert torch.equal(tn, nt), (M, N, rows)


# ---- GVX_GEMM_8W=0: the four-wave 128 x 128 tile in place of the eight-wave one; read once per process, so one child ------------
CHILD = r"""
import sys
sys.path.insert(0, {repo!r})
import numpy as np, torch
from genvox_amd import _lib
from tests.helpers import GEMM_8W_CASES, gemm_plan
from tests import test_gemm_gpu as t
lib = _lib.load()
out = {{}}
for i, c in enumerate(GEMM_8W_CASES):
    plan = gemm_plan(lib, c.M, c.N, c.K)
    assert plan == (0, 2222, c.rows_big, 1), (c, plan)
    t.check_exact(lib, c, True, 100 + i)
    got, ratio = t.check_rounded(lib, c, True, 200 + i)
    out[f"c{{i}}"] = got.cpu().numpy()
np.savez({path!r}, **out)
print("gemm 4w child ok")
"""


def test_four_wave_switch_gives_the_same_bits(lib, tmp_path):
    """GVX_GEMM_8W=0 is still a supported way to run: the >= 384-tile and two-launch cases in one child process - exact, within
    the rounded bound, and bit for bit what the eight-wave tiles give here."""
    path = str(tmp_path / "four_wave.npz")
    env = {**os.environ, "PYTHONNOUSERSITE": "1", "GVX_GEMM_8W": "0"}
    r = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, path=path)], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gemm 4w child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        for i, c in enumerate(GEMM_8W_CASES):
            assert gemm_plan(lib, c.M, c.N, c.K)[1] == 4212
            got, _ = check_rounded(lib, c, True, 200 + i)
            assert np.array_equal(z[f"c{i}"], got.cpu().numpy()), f"{c}: four-wave and eight-wave tiles differ"


# ---- the implicit-GEMM convolution: halo rows, row_len, two-level row maps - through gvx_postnet_forward ------------------------
def _postnet_model(full):
    from genvox_amd import weights as gw
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
    from genvox_amd.tacotron2 import Tacotron2

    mc, ac, tc = Tacotron2Config(), AudioConfig(filter_length=1024, log_func="np.log"), TextConfig(n_tokens=40)
    if not full:   # reduced layer sizes for the sweep: only the Postnet runs
        mc.postnet_embedding_dim = 64
    sd = gw.generate_state_dict(mc, ac, tc, seed=3)
    model = Tacotron2(mc, ac, tc)
    model.load_state_dict(sd)
    return model.to("cuda:0"), {k: v.double() for k, v in sd.items() if k.startswith("postnet.")}


@pytest.fixture(scope="module")
def small_postnet():
    return _postnet_model(False)


@pytest.fixture(scope="module")
def full_postnet():
    return _postnet_model(True)


def _postnet_ref(sd64, mel, length=None):
    """mel + Postnet(mel) in float64 for ONE row [n_mels, T] at its own length (zeros behind it), and a bound on what fp32
    evaluation may differ by: each layer's fma-chain bound on the folded weights, carried through the next layers' absolute
    weights (tanh is 1-Lipschitz; a few ulp for tanhf and the BatchNorm fold)."""
    import torch.nn.functional as F
    from oracle import tacotron2_ref

    T = mel.shape[1]
    n = T if length is None else length
    x = mel[None, :, :n].double().cpu()
    want = torch.zeros(mel.shape, dtype=torch.float64)
    want[:, :n] = (x + tacotron2_ref.postnet(sd64, x))[0]
    err, cur, i = torch.zeros_like(x), x, 0
    while f"postnet.convolutions.{i}.0.conv.weight" in sd64:
        p = f"postnet.convolutions.{i}"
        w, b = sd64[p + ".0.conv.weight"], sd64[p + ".0.conv.bias"]
        scale = sd64[p + ".1.weight"] / torch.sqrt(sd64[p + ".1.running_var"] + tacotron2_ref.BN_EPS)
        wf, bf = (w * scale[:, None, None]).abs(), ((b - sd64[p + ".1.running_mean"]) * scale + sd64[p + ".1.bias"]).abs()
        K = w.shape[1] * w.shape[2]
        mag = F.conv1d(cur.abs(), wf, bf, padding=(w.shape[2] - 1) // 2)
        err = F.conv1d(err, wf, None, padding=(w.shape[2] - 1) // 2) + (K + 8) * U * mag + 4 * U
        cur = tacotron2_ref._conv_bn(cur, sd64, p)
        last = f"postnet.convolutions.{i + 1}.0.conv.weight" not in sd64
        if not last:
            cur = torch.tanh(cur)
        i += 1
    bound = torch.full(mel.shape, 0.0, dtype=torch.float64)
    bound[:, :n] = (err + 2 * U * (x.abs() + cur.abs()))[0]
    return want, bound


def _mel(B, n_mels, T, seed):
    return torch.randn(B, n_mels, T, generator=_gen(seed), device="cuda")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 127, 128, 129])
def test_postnet_conv_edges(small_postnet, B, T):
    """T below the halo width (launch_zero_halo), T = 2, 3 (one row owns the front and the back halo), tile edges; ragged
    lengths including 1 and T: every row equals, bit for bit, the batch-1 call at its own length, with exact zeros behind it,
    and float64 within the five-layer bound."""
    model, sd64 = small_postnet
    mel = _mel(B, 80, T, 10 * T + B)
    lens = [T, 1, max(1, T // 2 + 1)][:B]
    worst = 0.0
    for lengths in (None, torch.tensor(lens, dtype=torch.int32)):
        out = model.postnet_residual(mel, lengths)
        torch.cuda.synchronize()
        for b in range(B):
            n = T if lengths is None else lens[b]
            alone = model.postnet_residual(mel[b:b + 1, :, :n].contiguous())
            assert torch.equal(out[b, :, :n], alone[0]), (B, T, b, n)
            assert bool((out[b, :, n:] == 0).all()), (B, T, b, n)
            want, bound = _postnet_ref(sd64, mel[b], n)
            ratio = float(((out[b].double().cpu() - want).abs() / bound.clamp_min(1e-300))[:, :n].max())
            worst = max(worst, ratio)
            assert ratio <= 1.0 and float((out[b].double().cpu() - want).abs().max()) <= 1e-3, (B, T, b, n, ratio)
    print(f"postnet B={B} T={T}: error / bound {worst:.3f}")


def test_postnet_full_size_second_launch_starts_inside_a_sequence(full_postnet):
    """B = 32, T = 800 at the model's layer sizes: M = 25 600 rows, 800 tiles, remainder 32 - the <2,2,1,1> launch starts at row
    24 576, frame 576 of sequence 30.  That sequence and the last one against float64, and sequence 30 bit-equal to its batch-1
    run (which takes other tiles)."""
    model, sd64 = full_postnet
    lib = _lib.load()
    assert gemm_plan(lib, 32 * 800, 512, 2560)[1:3] == (4212, 24576) and 24576 == 30 * 800 + 576
    B, T = 32, 800
    mel = _mel(B, 80, T, 77)
    lens = [T - 13 * (b % 7) for b in range(B)]
    lens[30], lens[31] = T, 611
    out = model.postnet_residual(mel, torch.tensor(lens, dtype=torch.int32))
    alone = model.postnet_residual(mel[30:31].contiguous())
    assert torch.equal(out[30], alone[0])
    worst = 0.0
    for b, sl in ((30, slice(560, 601)), (31, slice(0, T))):
        want, bound = _postnet_ref(sd64, mel[b], lens[b])
        got = out[b].double().cpu()
        assert bool((got[:, lens[b]:] == 0).all())
        ratio = float(((got - want).abs() / bound.clamp_min(1e-300))[:, sl][:, :max(0, lens[b] - (sl.start or 0))].max())
        worst = max(worst, ratio)
        assert ratio <= 1.0 and float((got - want).abs()[:, sl].max()) <= 1e-3, (b, ratio)
    print(f"postnet 32 x 800: error / bound {worst:.3f}")


def test_postnet_full_size_single_utterance(full_postnet):
    """B = 1, T = 568: five row tiles, the <2,3,1,1> last layer."""
    model, sd64 = full_postnet
    assert gemm_plan(_lib.load(), 568, 80, 2560)[1] == 2311
    mel = _mel(1, 80, 568, 78)
    out = model.postnet_residual(mel)
    want, bound = _postnet_ref(sd64, mel[0])
    diff = (out[0].double().cpu() - want).abs()
    ratio = float((diff / bound.clamp_min(1e-300)).max())
    assert ratio <= 1.0 and float(diff.max()) <= 1e-3, ratio
    print(f"postnet 1 x 568: error / bound {ratio:.3f}")
