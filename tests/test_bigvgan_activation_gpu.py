"""GPU: BigVGAN's anti-aliased Snake activation on its own (gvx_snake_antialiased, csrc/bigvgan.hip, through
``genvox_amd.bigvgan.antialiased_snake``) against the float64 padded-convolution form of tests/bigvgan_ref64.py, element by element.

Tolerance: the project's rule.  Every case evaluates the SAME restatement in float32 on the CPU and takes its largest distance from
float64; the device may differ from float64 by at most 8 times the larger of that number and one float32 ulp at the tensor's scale
(2^-23 x its largest magnitude).  The device sums the same 6 + 12 products per output in another order and calls another sine.

Behind a row's length the kernel writes exact zeros, and never reads its input.

Largest ratios of device error to that bound's base seen on an MI355X: see README.md, "BigVGAN"."""
import functools

import pytest
import torch

from genvox_amd.bigvgan import ACT_TILE as P
from genvox_amd.bigvgan import antialiased_snake
from tests import bigvgan_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23
LENGTHS = (1, 2, 5, 6, 7, 11, P - 1, P, P + 1, 2 * P + 1)
SCALES = (1e-3, 1.0, 30.0)


@functools.lru_cache(maxsize=None)
def _params(C, activation, logscale):
    g = torch.Generator().manual_seed(1000 * C + 2 * (activation == "snake") + logscale)
    return R.random_snake(C, g, logscale), (R.random_snake(C, g, logscale) if activation == "snakebeta" else None)


@functools.lru_cache(maxsize=None)
def _case(C, n, scale, activation, logscale, B=1):
    """(x float64 [B, C, n], float64 result, the float32 restatement's error): computed once."""
    alpha, beta = _params(C, activation, logscale)
    g = torch.Generator().manual_seed(7 * n + C + B)
    x = scale * torch.randn(B, C, n, generator=g, dtype=torch.float64)
    want = R.activation(x, alpha, beta, activation, logscale)
    low = R.activation(x.float(), alpha.float(), beta.float() if beta is not None else None, activation, logscale)
    return x, want, (low.double() - want).abs().max().item()


def _device(x64, C, activation, logscale, lengths=None, out=None):
    """x float64 [B, C, n] -> the device's result as [B, C, n]."""
    alpha, beta = _params(C, activation, logscale)
    x = x64.transpose(1, 2).contiguous().to(DEV, torch.float32)
    y = antialiased_snake(x, alpha, beta, lengths=lengths, activation=activation, logscale=logscale, out=out)
    torch.cuda.synchronize()
    return y.transpose(1, 2)


@pytest.mark.parametrize("logscale", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("activation", ["snakebeta", "snake"])
@pytest.mark.parametrize("C", [4, 36, 64, 132])
def test_every_length_and_scale_against_float64(C, activation, logscale):
    """Rows shorter than the filter's reach (1 .. 11: both clamps at once), one position short of a tile, a full tile, one over, and
    three tiles; 4 channels (the narrowest block), 36 and 132 (a channel tail), 64 (one full block).  a_c spans 0.3 .. 5, so at scale
    30 the sine's argument reaches a few hundred."""
    worst = 0.0
    for n in LENGTHS:
        for scale in SCALES:
            x, want, err = _case(C, n, scale, activation, logscale)
            got = _device(x, C, activation, logscale)
            assert got.shape == want.shape
            d = (got.double().cpu() - want).abs().max().item()
            base = max(err, ULP * want.abs().max().item())
            worst = max(worst, d / base)
            print(f"C {C} n {n} scale {scale} {activation} log {logscale}: device error {d:.3e}, float32 restatement error {err:.3e}, "
                  f"one ulp at scale {ULP * want.abs().max().item():.3e}, ratio {d / base:.2f}")
            assert d <= FACTOR * base, f"n = {n}, scale {scale}: differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"
    print(f"activation C {C} {activation} log {logscale}: largest ratio {worst:.2f}")


@pytest.mark.parametrize("C", [36, 64])
def test_ragged_rows_equal_their_one_row_runs(C):
    """Rows (P + 1, 1, P, 7) in a batch padded to P + 1: the padding of the input is NaN and the output starts as NaN; every row has
    the bits of its one-row run, and exact zeros behind its length."""
    lens = (P + 1, 1, P, 7)
    n_max = P + 1
    x, want, err = _case(C, n_max, 1.0, "snakebeta", True, B=len(lens))
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, :, n:] = float("nan")
    out = torch.full((len(lens), n_max, C), float("nan"), dtype=torch.float32, device=DEV)
    got = _device(x, C, "snakebeta", True, lengths=lens, out=out)
    alpha, beta = _params(C, "snakebeta", True)
    for b, n in enumerate(lens):
        assert not got[b, :, n:].any(), f"row {b}: not zeros behind its {n} positions"
        alone = _device(x[b:b + 1, :, :n], C, "snakebeta", True)
        assert torch.equal(alone[0], got[b, :, :n]), f"row {b} differs from its one-row run"
        ref = R.activation(x[b:b + 1, :, :n], alpha, beta)[0]
        d = (alone[0].double().cpu() - ref).abs().max().item()
        assert d <= FACTOR * max(err, ULP * ref.abs().max().item())
    again = _device(x, C, "snakebeta", True, lengths=torch.tensor(lens, device=DEV))   # device lengths; a fresh output buffer
    assert torch.equal(again, got)


def test_two_calls_give_the_same_bits():
    x, _, _ = _case(132, 2 * P + 1, 30.0, "snake", False, B=3)
    a, b = _device(x, 132, "snake", False), _device(x, 132, "snake", False)
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_arguments_are_checked_before_the_launch():
    x = torch.zeros(2, 8, 4, device=DEV)
    alpha = torch.zeros(4)
    with pytest.raises(ValueError, match="alpha"):
        antialiased_snake(x, alpha)                      # snakebeta without beta
    with pytest.raises(ValueError, match="lengths"):
        antialiased_snake(x, alpha, alpha, lengths=(8, 9))
    with pytest.raises(ValueError, match="out"):
        antialiased_snake(x, alpha, alpha, out=x)
    with pytest.raises(ValueError, match="float32"):
        antialiased_snake(x.cpu(), alpha, alpha)
    y = antialiased_snake(x, alpha, alpha, lengths=(8, 0))   # a row of no positions is zeros
    assert not y.any()
