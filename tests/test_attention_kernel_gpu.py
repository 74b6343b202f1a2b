"""GPU: the self-attention kernel alone (gvx_self_attention, csrc/fastpitch.hip, through ``fastpitch.self_attention``) against the
float64 restatement of tests/fastpitch_ref64.py (explicit ``softmax(q k^T / sqrt(d)) v``, every row over its own keys).

Tolerance: the 8 x rule of tests/test_vocos_gpu.py.  Every case evaluates the SAME restatement in float32 on the CPU and takes its
largest distance from float64; the device may differ from float64 by at most 8 times the larger of that number and one float32 ulp at
the tensor's scale.  The ratio is printed.  The kernel's tiles are 128 queries and 64 keys: the lengths sit on, one before and one
behind both edges, and 129 and 257 need three and five key tiles.

Largest ratios seen on an MI355X: see README.md, "FastPitch"."""
import pytest
import torch

from genvox_amd.fastpitch import K_TILE, Q_TILE, self_attention
from tests import fastpitch_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23
HEADS = [(1, 64), (2, 64), (1, 32), (4, 32)]
NAN = float("nan")


def _qkv(B, T, H, D, seed, lens=None, gain=1.0):
    """float32-representable values in float64; q and k scaled by ``gain``; NaN behind every row's length."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * H * D, generator=g, dtype=torch.float64)
    qkv[:, :, :2 * H * D] *= gain
    qkv = qkv.float().double()
    if lens is not None:
        for b, n in enumerate(lens):
            qkv[b, n:] = NAN
    return qkv


def _run(qkv, lens, H, D):
    out = torch.full((qkv.shape[0], qkv.shape[1], H * D), NAN, dtype=torch.float32, device=DEV)   # NaN beforehand: every element is written
    got = self_attention(qkv.to(DEV, torch.float32), lens, H, D, out=out)
    torch.cuda.synchronize()
    return got


def _check(qkv, lens, H, D, what):
    want, err = R.attention_pair(qkv, lens, H, D)
    got = _run(qkv, lens, H, D)
    assert not torch.isnan(got).any(), what
    d = (got.double().cpu() - want).abs().max().item()
    base = max(err, ULP * want.abs().max().item())
    print(f"{what}: device error {d:.3e}, float32 restatement error {err:.3e}, one ulp at scale {ULP * want.abs().max().item():.3e}, ratio {d / base:.2f}")
    assert d <= FACTOR * base, f"{what}: differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"
    for b, n in enumerate(lens if lens is not None else []):
        assert not got[b, n:].any(), f"{what}: row {b} is not zeros behind its length"
    return got


def test_the_tiles_are_the_ones_the_shapes_were_chosen_for():
    assert (Q_TILE, K_TILE) == (128, 64)


@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 129, 257])
def test_full_rows(T, H, D):
    B = 3 if T <= 65 else 2
    _check(_qkv(B, T, H, D, seed=T + H), None, H, D, f"{B} x {T}, {H} heads of {D}")


@pytest.mark.parametrize("H,D", HEADS)
@pytest.mark.parametrize("T,lens", [(66, (64, 63, 65)), (130, (128, 127, 129)), (257, (1, 257, 192)), (65, (1, 65, 2))])
def test_ragged_rows_with_nan_behind_them(T, lens, H, D):
    """Lengths on, one before and one behind a key tile's and a query tile's edge, and a row of length 1; qkv is NaN behind every row."""
    _check(_qkv(3, T, H, D, seed=T + D, lens=lens), lens, H, D, f"3 x {T} lengths {lens}, {H} heads of {D}")


@pytest.mark.parametrize("H,D", [(2, 64), (4, 32)])
def test_a_row_has_the_bits_of_the_row_alone_and_of_a_longer_padding(H, D):
    lens = (129, 64, 1, 200)
    T = 200
    qkv = _qkv(4, T, H, D, seed=9, lens=lens)
    got = _run(qkv, lens, H, D)
    padded = torch.full((4, 300, 3 * H * D), NAN, dtype=torch.float64)
    padded[:, :T] = qkv
    got_padded = _run(padded, lens, H, D)
    for b, n in enumerate(lens):
        alone = _run(qkv[b:b + 1, :n], None, H, D)
        assert torch.equal(got[b, :n], alone[0]), f"row {b} of the ragged batch differs from the row alone"
        assert torch.equal(got_padded[b, :n], alone[0]), f"row {b} padded to 300 differs from the row alone"
        assert not got_padded[b, n:].any()


@pytest.mark.parametrize("H,D", [(1, 64), (4, 32)])
def test_scores_of_magnitude_60_stay_finite_and_inside_the_rule(H, D):
    """q and k scaled up: the scores' standard deviation is 20, the largest pass 60 - exp() of one overflows float32 without the
    running maximum - and the largest key moves from tile to tile."""
    lens = (150, 129)
    qkv = _qkv(2, 150, H, D, seed=21, lens=lens, gain=20.0 ** 0.5)
    q, k = qkv[0, :150, :D], qkv[0, :150, H * D:H * D + D]
    assert (q @ k.t() / D ** 0.5).abs().max().item() > 60.0
    got = _check(qkv, lens, H, D, f"scores beyond 60, {H} heads of {D}")
    assert torch.isfinite(got).all()


def test_two_calls_give_the_same_bits():
    lens = (257, 100)
    qkv = _qkv(2, 257, 2, 64, seed=4, lens=lens)
    assert torch.equal(_run(qkv, lens, 2, 64), _run(qkv, lens, 2, 64))


def test_refused_arguments():
    x = torch.zeros(1, 4, 3 * 48, device=DEV)
    with pytest.raises(ValueError):
        self_attention(x, None, 1, 48)
    with pytest.raises(ValueError):
        self_attention(torch.zeros(1, 4, 192, device=DEV), [5], 1, 64)
    with pytest.raises(ValueError):
        self_attention(torch.zeros(1, 4, 192), None, 1, 64)
