"""GPU: the two backward kernels of the Vocos generator on their own - gvx_dwconv_layernorm_backward (vcb_ln_kernel, vcb_dw_kernel,
vcb_sum_kernel) and gvx_istft_head_backward (vcb_env_kernel, vcb_istft_kernel), csrc/vocos_train.hip - against float64 autograd of the
plain-torch expressions (F.conv1d + F.layer_norm; vocos_ref64.istft's expression as tests/vocos_grad_ref64.py restates it for autograd), element by element.  Inputs carry NaN behind every row's frames (x, dy, d_res, coeffs) and behind its delivered
samples (d_wav); workspaces and outputs start as NaN and the workspaces have exactly their stated sizes.

Tolerance: the project's rule.  The same expression runs in float32 on the CPU; its largest distance from float64, per tensor, is e.  The
device may differ from float64 by at most 8 x max(e, 2^-23 x the tensor's largest magnitude).  Every ratio is printed.

Largest ratios seen on an MI355X: DESIGN.md, "Vocos generator: tape forward and backward"."""
import pytest
import torch
import torch.nn.functional as F

from genvox_amd import _lib
from genvox_amd.vocos import TILE, dwconv_layernorm_backward, istft_head_backward
from tests import vocos_grad_ref64 as GR
from tests import vocos_ref64 as R
from tests.test_vocos_kernels_gpu import _coeffs, _norm_params
from tests.vocos_train_helpers import DEV, NAN, bound_check

pytestmark = pytest.mark.gpu
P = TILE
PIECE = 128   # GVX_VOCOS_GRAD_PIECE
EPS = 1e-6


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _norm_out(B, T, C_, taps):
    """The five results of the filter + LayerNorm backward, all NaN: a frame, a sum or a zero the kernels do not write shows."""
    return [_nan(B, T, C_), _nan(C_), _nan(C_)] + ([_nan(C_, 1, 7), _nan(C_)] if taps else [None, None])


def _norm_ws(B, T, C_, taps):
    need = _lib.load().gvx_dwconv_layernorm_backward_workspace_bytes(B, T, C_, taps)
    assert need > 0 and need % 256 == 0
    return _nan(need // 4).view(torch.uint8)


def _istft_ws(B, T, n_fft, hop):
    need = _lib.load().gvx_istft_head_backward_workspace_bytes(B, T, n_fft, hop)
    assert need > 0 and need % 256 == 0
    return _nan(need // 4).view(torch.uint8)


# ------------------------------------------------------------------ filter + LayerNorm, backward
def _norm_grads(x, dy, d_res, lens, w, b, lw, lb, dtype):
    """Autograd of conv1d + layer_norm, every row alone at its own length -> (dx, d lw, d lb, d w, d b) in ``dtype``."""
    B, T, C_ = x.shape
    leaf = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
    w_, b_, lw_, lb_ = leaf(w), leaf(b), leaf(lw), leaf(lb)
    dx = torch.zeros(B, T, C_, dtype=dtype)
    for i, n in enumerate(lens):
        xi = x[i, :n].to(dtype).clone().requires_grad_(True)
        y = xi
        if w is not None:
            y = F.conv1d(y.t()[None], w_, b_, padding=3, groups=C_)[0].t()
        out = F.layer_norm(y, (C_,), lw_, lb_, EPS)
        (out * dy[i, :n].to(dtype)).sum().backward()
        dx[i, :n] = xi.grad + (d_res[i, :n].to(dtype) if d_res is not None else 0.0)
    g = lambda t: None if t is None else t.grad.detach()
    return dx, g(lw_), g(lb_), g(w_), g(b_)


def _norm_bwd_case(x, dy, d_res, lens, w, b, lw, lb, what):
    B, T, C_ = x.shape
    want = _norm_grads(x, dy, d_res, lens, w, b, lw, lb, torch.float64)
    got32 = _norm_grads(x, dy, d_res, lens, w, b, lw, lb, torch.float32)
    dirty = [None if t is None else t.clone() for t in (x, dy, d_res)]
    for t in dirty:
        if t is not None:
            for i, n in enumerate(lens):
                t[i, n:] = NAN
    f = lambda t: None if t is None else t.float().to(DEV)
    taps = 7 if w is not None else 0
    got = dwconv_layernorm_backward(f(dirty[0]), f(dirty[1]), f(lw), f(w), f(b), d_res=f(dirty[2]), lengths=lens, workspace=_norm_ws(B, T, C_, taps),
                                    out=_norm_out(B, T, C_, taps))
    torch.cuda.synchronize()
    for i, n in enumerate(lens):
        assert not got[0][i, n:].any(), f"{what}: row {i} of dx is not zero behind its {n} frames"
    for name, g, w64, w32 in zip(("dx", "d ln_w", "d ln_b", "d w", "d b"), got, want, got32):
        if w64 is None:
            assert g is None
            continue
        bound_check(g, w64, (w32.double() - w64).abs().max().item(), f"{what}: {name}")
    return got, dirty


def _rand_case(C_, T, lens, seed, with_res):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    x = torch.randn(B, T, C_, generator=g).double()
    dy = torch.randn(B, T, C_, generator=g).double()
    d_res = torch.randn(B, T, C_, generator=g).double() if with_res else None
    return x, dy, d_res


@pytest.mark.parametrize("taps", [7, 0])
@pytest.mark.parametrize("C_", [32, 64, 96, 192, 512])
def test_backward_at_every_tile_edge(C_, taps):
    """Every channels-per-lane instantiation with whole and partly idle chunks (NC = 1: 32, 64; 2: 96; 4: 192; 8: 512); T at 1, 2, the
    filter's reach (6, 7), either side of the tile of P frames and past two tiles; rows of T, 1 and a middle length; with and without the
    residual path's gradient; dx of a ragged row has the bits of that row run alone."""
    w, b, lw, lb = _norm_params(C_, taps, seed=C_ + taps)
    f = lambda t: None if t is None else t.float().to(DEV)
    for T in (1, 2, 6, 7, P - 1, P, P + 1, 2 * P + 3):
        for with_res in (True, False):
            lens = (T, 1, (T + 1) // 2)
            x, dy, d_res = _rand_case(C_, T, lens, 1000 * C_ + T, with_res)
            got, dirty = _norm_bwd_case(x, dy, d_res, lens, w, b, lw, lb, f"C {C_} taps {taps} T {T} d_res {with_res}")
            n = lens[2]
            cut = lambda t: None if t is None else f(t[2:3, :n].contiguous())
            alone = dwconv_layernorm_backward(cut(dirty[0]), cut(dirty[1]), f(lw), f(w), f(b), d_res=cut(dirty[2]), workspace=_norm_ws(1, n, C_, taps),
                                              out=_norm_out(1, n, C_, taps))
            assert not any(torch.isnan(t).any() for t in alone if t is not None)
            assert torch.equal(alone[0][0], got[0][2, :n])


@pytest.mark.parametrize("taps", [7, 0])
@pytest.mark.parametrize("B,T,lens", [(1, PIECE, None), (1, PIECE + 1, None), (1, 2 * PIECE + 3, None), (3, 2 * PIECE + 3, (2 * PIECE + 3, 1, PIECE + 1))])
def test_piece_edges_of_the_parameter_sums(B, T, lens, taps):
    """C = 32.  One piece exactly, one piece and a frame, two pieces and a tail of 3; three rows whose second has two whole pieces behind
    it and whose third has one frame in its second piece and a piece behind it: those write zeros over the workspace's NaN."""
    C_ = 32
    w, b, lw, lb = _norm_params(C_, taps, seed=3)
    lens = lens or (T,) * B
    x, dy, d_res = _rand_case(C_, T, lens, 17 * T + B, True)
    _norm_bwd_case(x, dy, d_res, lens, w, b, lw, lb, f"pieces taps {taps} lengths {lens}")


@pytest.mark.parametrize("taps", [7, 0])
@pytest.mark.parametrize("C_", [64, 512])
def test_an_offset_of_a_thousand(C_, taps):
    """Unit deviations on an offset of 1e3, as the forward's test: xh must keep its digits."""
    T = P + 1
    w, b, lw, lb = _norm_params(C_, taps, seed=77)
    if taps:
        w = w.abs()
    g = torch.Generator().manual_seed(C_)
    x = (1e3 + torch.randn(2, T, C_, generator=g)).double()
    dy = torch.randn(2, T, C_, generator=g).double()
    _norm_bwd_case(x, dy, None, (T, 5), w, b, lw, lb, f"offset 1e3 C {C_} taps {taps}")


@pytest.mark.parametrize("taps", [7, 0])
def test_a_row_of_variance_zero(taps):
    """Every frame constant over the channels and the filter the same for every channel: u is constant, xh is 0 and rstd = eps^-1/2.
    dxh - mean(dxh) is then the whole of du rstd^-1."""
    C_, T = 96, P + 3
    x = (0.75 * (1 + torch.arange(T, dtype=torch.float64) % 5))[None, :, None].expand(2, T, C_).contiguous()
    w = b = None
    if taps:
        w = torch.tensor([0.5, -0.25, 1.0, 2.0, 0.125, -1.0, 0.5], dtype=torch.float64).expand(C_, 1, 7).contiguous()
        b = torch.full((C_,), 0.375, dtype=torch.float64)
    _, _, lw, lb = _norm_params(C_, 0, seed=5)
    g = torch.Generator().manual_seed(2)
    dy = torch.randn(2, T, C_, generator=g).double()
    _norm_bwd_case(x, dy, None, (T, 4), w, b, lw, lb, f"variance 0 taps {taps}")


def test_two_calls_give_the_same_bits():
    C_, T, lens = 192, 2 * PIECE + 3, (2 * PIECE + 3, 5, PIECE + 1)
    w, b, lw, lb = _norm_params(C_, 7, seed=9)
    x, dy, d_res = _rand_case(C_, T, lens, 4, True)
    f = lambda t: t.float().to(DEV)
    run = lambda: dwconv_layernorm_backward(f(x), f(dy), f(lw), f(w), f(b), d_res=f(d_res), lengths=lens, workspace=_norm_ws(3, T, C_, 7),
                                            out=_norm_out(3, T, C_, 7))
    a, c = run(), run()
    assert all(torch.equal(u, v) and not torch.isnan(u).any() for u, v in zip(a, c))


# ------------------------------------------------------------------ the ISTFT head, backward
def _istft_grads(c, G, lens, n_fft, hop, padding, dtype):
    B, T, _ = c.shape
    out = torch.zeros(B, T, n_fft + 2, dtype=dtype)
    for i, n in enumerate(lens):
        ci = c[i:i + 1, :n].to(dtype).clone().requires_grad_(True)
        w = GR.istft(ci, n_fft, hop, padding)   # R.istft with the trim in front of the division
        if w.shape[1]:
            (w * G[i:i + 1, :w.shape[1]].to(dtype)).sum().backward()
            out[i, :n] = ci.grad[0]
    return out


def _istft_bwd_case(c, lens, n_fft, hop, padding, what, seed=0):
    B, T, _ = c.shape
    H = n_fft // 2
    m = c[..., :H + 1]
    assert (m - R.LOG_CLAMP).abs().min().item() >= 1e-4, "the margin around ln 100"
    g = torch.Generator().manual_seed(seed + T)
    G = torch.randn(B, T * hop, generator=g).double()
    want = _istft_grads(c, G, lens, n_fft, hop, padding, torch.float64)
    w32 = _istft_grads(c, G, lens, n_fft, hop, padding, torch.float32)
    dirty, Gd = c.clone(), G.clone()
    cfg = dict(hop_length=hop, padding=padding)
    for i, n in enumerate(lens):
        dirty[i, n:] = NAN
        Gd[i, R.sample_count(cfg, n):] = NAN
    got = istft_head_backward(dirty.float().to(DEV), Gd.float().to(DEV), n_fft, hop, padding, lengths=lens, workspace=_istft_ws(B, T, n_fft, hop),
                              out=_nan(B, T, n_fft + 2))
    torch.cuda.synchronize()
    for i, n in enumerate(lens):
        assert not got[i, n:].any(), f"{what}: row {i} is not zero behind its frames"
    # the two halves have different scales: each against its own
    e = lambda a: (a[0].double() - a[1]).abs().max().item()
    bound_check(got[..., :H + 1], want[..., :H + 1], e((w32[..., :H + 1], want[..., :H + 1])), f"{what}: d m")
    bound_check(got[..., H + 1:], want[..., H + 1:], e((w32[..., H + 1:], want[..., H + 1:])), f"{what}: d p")
    return got, dirty, Gd, want


@pytest.mark.parametrize("padding", ["same", "center"])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_istft_backward_at_every_frame_count_and_hop(n_fft, padding):
    least = 2 if padding == "center" else 1
    for hop in (n_fft // 4, n_fft // 2, n_fft // 8 + 2):
        for T in (1, 2, 3, 4, 5, 9):
            if T < least:
                continue
            c = _coeffs(2, T, n_fft, seed=n_fft + hop + T)
            _istft_bwd_case(c, (T, T), n_fft, hop, padding, f"n_fft {n_fft} hop {hop} {padding} T {T}")


@pytest.mark.parametrize("n_fft,hop,padding", [(512, 128, "same"), (1024, 130, "center"), (1024, 256, "center"), (2048, 1024, "same")])
def test_istft_backward_ragged_rows(n_fft, hop, padding):
    T = 9
    least = 2 if padding == "center" else 1
    lens = (T, least, 5, 3)
    c = _coeffs(4, T, n_fft, seed=n_fft + hop)
    got, dirty, Gd, _ = _istft_bwd_case(c, lens, n_fft, hop, padding, f"ragged n_fft {n_fft} hop {hop} {padding}")
    for i in (1, 2):   # a row of a ragged batch has the bits of that row run alone
        n = lens[i]
        alone = istft_head_backward(dirty[i:i + 1, :n].float().to(DEV).contiguous(), Gd[i:i + 1, :n * hop].float().to(DEV).contiguous(), n_fft, hop, padding,
                                    workspace=_istft_ws(1, n, n_fft, hop), out=_nan(1, n, n_fft + 2))
        assert not torch.isnan(alone).any()
        assert torch.equal(alone[0], got[i, :n])


def test_a_frame_wholly_above_the_clamp():
    """m = ln 100 + 1 in every bin of frame 1: d m is exactly 0 in every bin of it, and d p is still held to the bound."""
    n_fft, hop, T = 1024, 256, 4
    H = n_fft // 2
    c = _coeffs(1, T, n_fft, seed=9)
    c[0, 1, :H + 1] = R.LOG_CLAMP + 1.0
    got, _, _, want = _istft_bwd_case(c, (T,), n_fft, hop, "same", "clamped frame")
    assert not got[0, 1, :H + 1].any() and not want[0, 1, :H + 1].any()
    assert got[0, 1, H + 1:].abs().max().item() > 0.0
