"""GPU: the two Vocos kernels on their own - gvx_dwconv_layernorm (vc_dwconv_ln_kernel) and gvx_istft_head (vc_istft_kernel,
vc_ola_kernel), csrc/vocos.hip - against float64, element by element.

Tolerance: the project's rule.  Every case evaluates the same plain-torch expression in float32 on the CPU and takes its largest
distance from float64, a number that depends on the reference alone; the device may differ from float64 by at most 8 times the larger
of that number and one float32 ulp at the tensor's scale (2^-23 x its largest magnitude).  The ratio is printed.

Largest ratios seen on an MI355X: see README.md, "Vocos"."""
import math

import pytest
import torch
import torch.nn.functional as F

from genvox_amd.vocos import TILE, dwconv_layernorm, istft_head
from tests import vocos_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23
P = TILE
EPS = 1e-6


def _bound_check(got, want, err32, what):
    d = (got.double().cpu() - want).abs().max().item()
    scale = ULP * want.abs().max().item()
    base = max(err32, scale)
    print(f"{what}: device error {d:.3e}, float32 restatement error {err32:.3e}, one ulp at scale {scale:.3e}, ratio {d / base if base else 0.0:.2f}")
    assert d <= FACTOR * base, f"{what}: differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"


# ------------------------------------------------------------------ filter + LayerNorm
def _norm_ref(x, lens, w, b, lw, lb, dtype):
    """Every row alone at its own length: x [B, T, C] float64 (float32-representable) -> [B, T, C] in ``dtype``, zeros behind a row."""
    B, T, C_ = x.shape
    out = torch.zeros(B, T, C_, dtype=dtype)
    cast = lambda t: None if t is None else t.to(dtype)
    for i, n in enumerate(lens):
        y = x[i, :n].to(dtype)
        if w is not None:
            y = F.conv1d(y.t()[None], cast(w), cast(b), padding=3, groups=C_)[0].t()
        out[i, :n] = F.layer_norm(y, (C_,), cast(lw), cast(lb), EPS)
    return out


def _norm_params(C_, taps, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).double()   # float32-representable
    w, b = (r(C_, 1, 7) * 7 ** -0.5, 0.1 * r(C_)) if taps else (None, None)
    return w, b, 1.0 + 0.25 * r(C_), 0.1 * r(C_)


def _norm_case(x, lens, w, b, lw, lb, what):
    B, T, _ = x.shape
    want = _norm_ref(x, lens, w, b, lw, lb, torch.float64)
    err32 = (_norm_ref(x, lens, w, b, lw, lb, torch.float32).double() - want).abs().max().item()
    dirty = x.clone()
    for i, n in enumerate(lens):
        dirty[i, n:] = float("nan")   # never read
    f = lambda t: None if t is None else t.float().to(DEV)
    got = dwconv_layernorm(dirty.float().to(DEV), f(lw), f(lb), f(w), f(b), lengths=lens)
    torch.cuda.synchronize()
    for i, n in enumerate(lens):
        assert not got[i, n:].any(), f"{what}: row {i} is not zero behind its {n} frames"
    _bound_check(got, want, err32, what)
    return got, dirty


@pytest.mark.parametrize("taps", [7, 0])
@pytest.mark.parametrize("C_", [32, 64, 96, 512])
def test_filter_and_layernorm_at_every_tile_edge(C_, taps):
    """T at 1, 2, the filter's reach (6, 7), either side of the tile of P frames and past two tiles; rows of T, 1 and a middle length, with
    NaN behind every row's frames; a ragged row has the bits of that row run alone."""
    w, b, lw, lb = _norm_params(C_, taps, seed=C_ + taps)
    for T in (1, 2, 6, 7, P - 1, P, P + 1, 2 * P + 3):
        g = torch.Generator().manual_seed(1000 * C_ + T)
        x = torch.randn(3, T, C_, generator=g).double()
        lens = (T, 1, (T + 1) // 2)
        got, dirty = _norm_case(x, lens, w, b, lw, lb, f"C {C_} taps {taps} T {T}")
        f = lambda t: None if t is None else t.float().to(DEV)
        n = lens[2]
        alone = dwconv_layernorm(dirty[2:3, :n].float().to(DEV).contiguous(), f(lw), f(lb), f(w), f(b))
        assert torch.equal(alone[0], got[2, :n])


@pytest.mark.parametrize("taps", [7, 0])
@pytest.mark.parametrize("C_", [96, 512])
def test_a_constant_frame_has_variance_zero(C_, taps):
    """Every frame constant over the channels, the filter the same for every channel, all values dyadic: the filter's output is exact and
    constant, the variance is 0 and the result is the LayerNorm's shift."""
    T = P + 3
    x = (0.75 * (1 + torch.arange(T, dtype=torch.float64) % 5))[None, :, None].expand(2, T, C_).contiguous()
    w = b = None
    if taps:
        w = torch.tensor([0.5, -0.25, 1.0, 2.0, 0.125, -1.0, 0.5], dtype=torch.float64).expand(C_, 1, 7).contiguous()
        b = torch.full((C_,), 0.375, dtype=torch.float64)
    _, _, lw, lb = _norm_params(C_, 0, seed=5)
    got, _ = _norm_case(x, (T, 4), w, b, lw, lb, f"constant frames C {C_} taps {taps}")
    assert torch.equal(got[0].cpu(), lb.float().expand(T, C_))


@pytest.mark.parametrize("taps", [7, 0])
@pytest.mark.parametrize("C_", [64, 512])
def test_an_offset_of_a_thousand(C_, taps):
    """Unit deviations on an offset of 1e3: a variance formed as a mean of squares minus a squared mean would lose every digit."""
    T = P + 1
    w, b, lw, lb = _norm_params(C_, taps, seed=77)
    if taps:
        w = w.abs()   # the offset survives the filter
    g = torch.Generator().manual_seed(C_)
    x = (1e3 + torch.randn(2, T, C_, generator=g)).double()
    _norm_case(x, (T, 5), w, b, lw, lb, f"offset 1e3 C {C_} taps {taps}")


# ------------------------------------------------------------------ the ISTFT head
def _istft_ref(c, lens, n_fft, hop, padding, dtype):
    B, T, _ = c.shape
    out = torch.zeros(B, T * hop, dtype=dtype)
    for i, n in enumerate(lens):
        w = R.istft(c[i:i + 1, :n].to(dtype), n_fft, hop, padding)
        out[i, :w.shape[1]] = w[0]
    return out


def _coeffs(B, T, n_fft, seed):
    """Log-magnitudes on both sides of ln 100 and phases over a few turns, float32-representable, with a margin of 1e-4 around ln 100."""
    H = n_fft // 2
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(B, T, n_fft + 2, generator=g)
    c[..., :H + 1] = 2.3 + 3.0 * c[..., :H + 1]
    c[..., H + 1:] = 2.0 * c[..., H + 1:]
    m = c[..., :H + 1]
    near = (m - R.LOG_CLAMP).abs() < 2e-4
    m[near] = R.LOG_CLAMP + torch.where(m[near] < R.LOG_CLAMP, -3e-4, 3e-4)
    return c.double()


def _istft_case(c, lens, n_fft, hop, padding, what):
    B, T, _ = c.shape
    H = n_fft // 2
    m = c[..., :H + 1]
    assert (m - R.LOG_CLAMP).abs().min().item() >= 1e-4, "the margin around ln 100"
    assert (m > R.LOG_CLAMP).any() and (m < R.LOG_CLAMP).any()
    want = _istft_ref(c, lens, n_fft, hop, padding, torch.float64)
    err32 = (_istft_ref(c, lens, n_fft, hop, padding, torch.float32).double() - want).abs().max().item()
    dirty = c.clone()
    for i, n in enumerate(lens):
        dirty[i, n:] = float("nan")
    got = istft_head(dirty.float().to(DEV), n_fft, hop, padding, lengths=lens)
    torch.cuda.synchronize()
    assert got.shape == (B, T * hop)
    cfg = dict(hop_length=hop, padding=padding)
    for i, n in enumerate(lens):
        assert not got[i, R.sample_count(cfg, n):].any(), f"{what}: row {i} is not zero behind its samples"
    _bound_check(got, want, err32, what)
    return got, dirty


@pytest.mark.parametrize("padding", ["same", "center"])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_istft_head_at_every_frame_count_and_hop(n_fft, padding):
    """hop n_fft / 4, n_fft / 2 and one that divides nothing; T at the counts at which a sample gains a frame."""
    least = 2 if padding == "center" else 1
    for hop in (n_fft // 4, n_fft // 2, n_fft // 8 + 2):
        for T in (1, 2, 3, 4, 5, 9):
            if T < least:
                continue
            c = _coeffs(2, T, n_fft, seed=n_fft + hop + T)
            _istft_case(c, (T, T), n_fft, hop, padding, f"n_fft {n_fft} hop {hop} {padding} T {T}")


@pytest.mark.parametrize("n_fft,hop,padding", [(512, 128, "same"), (1024, 130, "center"), (1024, 256, "center"), (2048, 1024, "same")])
def test_istft_head_ragged_rows(n_fft, hop, padding):
    T = 9
    least = 2 if padding == "center" else 1
    lens = (T, least, 5, 3)
    c = _coeffs(4, T, n_fft, seed=n_fft + hop)
    got, dirty = _istft_case(c, lens, n_fft, hop, padding, f"ragged n_fft {n_fft} hop {hop} {padding}")
    for i in (1, 2):   # a row of a ragged batch has the bits of that row run alone
        n = lens[i]
        alone = istft_head(dirty[i:i + 1, :n].float().to(DEV).contiguous(), n_fft, hop, padding)
        assert torch.equal(alone[0, :R.sample_count(dict(hop_length=hop, padding=padding), n)],
                           got[i, :R.sample_count(dict(hop_length=hop, padding=padding), n)])


def test_the_clamp_exactly_one_above_ln_100():
    """m = fl32(ln 100) + 1 in every bin: exp(m) is 271.8, clamped to 100."""
    n_fft, hop, T = 1024, 256, 4
    c = _coeffs(1, T, n_fft, seed=9)
    R_LOG = R.LOG_CLAMP
    assert math.exp(R_LOG + 1.0) > 271.0
    c[0, 1, :n_fft // 2 + 1] = R_LOG + 1.0   # float64: the restatement's value; the device sees its float32 rounding, clamped as well
    got, _ = _istft_case(c, (T,), n_fft, hop, "same", "clamped frame")
    # the frame alone: every bin at magnitude exactly 100
    alone = c[:, 1:2].clone()
    want = R.istft(alone, n_fft, hop, "same")
    want100 = R.istft(torch.cat([torch.full_like(alone[..., :n_fft // 2 + 1], R_LOG), alone[..., n_fft // 2 + 1:]], dim=-1), n_fft, hop, "same")
    assert (want - want100).abs().max().item() < 1e-9 * want.abs().max().item()
