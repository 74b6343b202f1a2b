"""GPU: the gated location-variable convolution layer on its own (gvx_lvc_gated, csrc/univnet.hip, through ``univnet.lvc_gated``) against
the float64 restatement of tests/univnet_ref64.py, element by element: both kernels (the matrix-pipe one at C = 32 with 64 and 256
positions per frame, the fmaf one at C = 16 and at 8 positions per frame), with and without the dilated convolution in front.

The predicted kernels differ strongly from frame to frame - frame t's are scaled by (-1)^t (1 + t) - so a tile that used a neighbouring
frame's weights cannot pass, and x, the kernels and the bias are NaN behind every row's length, so a read past a row's end shows.

Tolerance: the project's rule, as tests/test_vocos_kernels_gpu.py: the device may differ from float64 by at most 8 times the larger of the
float32 restatement's own distance from float64 and one float32 ulp at the tensor's scale.  The ratio is printed."""
import pytest
import torch
from torch import nn

from genvox_amd.univnet import lvc_gated
from tests import univnet_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23


def _inputs(C, cum, T, lens, dilation, seed):
    g = torch.Generator().manual_seed(seed)
    B = 1 if lens is None else len(lens)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()   # float32 values: what the device holds
    x = rnd(B, C, T * cum)
    swing = torch.tensor([(-1.0) ** t * (1 + t) for t in range(T)], dtype=torch.float64)
    kernels = rnd(B, C, 2 * C, 3, T) * (3 * C) ** -0.5 * swing
    bias = rnd(B, 2 * C, T) * 0.3
    conv = None
    if dilation:
        conv = nn.Conv1d(C, C, 3, dilation=dilation, padding=dilation).double()
        with torch.no_grad():
            conv.weight.copy_(rnd(C, C, 3) * (3 * C) ** -0.5)
            conv.bias.copy_(rnd(C) * 0.1)
    return x, kernels, bias, conv


def _reference(x, kernels, bias, conv, lens):
    """Row by row at the row's own length -> (float64 [B, C, L] with zeros behind a row, the float32 restatement's distance from it)."""
    import copy

    B, _, L = x.shape
    T = kernels.shape[4]
    cum = L // T
    want, err = torch.zeros_like(x), 0.0
    conv32 = copy.deepcopy(conv).float() if conv is not None else None
    with torch.no_grad():
        for b in range(B):
            t = T if lens is None else lens[b]
            args = (x[b:b + 1, :, :t * cum], kernels[b:b + 1, ..., :t], bias[b:b + 1, :, :t])
            w = R.lvc_gated(*args, conv)
            want[b, :, :t * cum] = w[0]
            got32 = R.lvc_gated(*(a.float() for a in args), conv32)
            err = max(err, (got32.double() - w).abs().max().item())
    return want, err


CASES = [
    # C, cum, T, lens (frames per row; None: one full row), dilation (0: no convolution in front)
    (32, 8, 5, None, 27),            # block 0: the window of the dilated convolution spans 7 frames' positions, the weights change every 8
    (32, 8, 1, None, 1),
    (32, 8, 2, (2, 1), 0),
    (32, 64, 2, None, 1),            # one 128-position tile of the convolution, two frames of 64: two waves per LVC workgroup
    (32, 64, 5, (5, 2, 1, 3), 27),   # row ends at a tile's edge (2 frames = 128), inside one (1, 3, 5 frames)
    (32, 64, 5, None, 0),
    (32, 256, 1, None, 27),
    (32, 256, 2, None, 1),           # two LVC workgroups per frame
    (32, 256, 5, (5, 1, 2), 27),
    (32, 32, 5, (5, 3), 3),          # one wave per frame
    (16, 8, 5, (5, 2), 27),
    (16, 64, 2, None, 1),
    (16, 256, 5, (5, 1), 27),        # four fmaf workgroups per frame
    (16, 256, 1, None, 0),
    (12, 6, 5, (5, 4), 3),           # a channel count and a frame that are no power of two
]


@pytest.mark.parametrize("C,cum,T,lens,dilation", CASES)
def test_lvc_gated_against_float64(C, cum, T, lens, dilation):
    x, kernels, bias, conv = _inputs(C, cum, T, lens, dilation, seed=1000 * C + 10 * cum + T)
    want, err = _reference(x, kernels, bias, conv, lens)
    if lens is not None:
        for b, t in enumerate(lens):
            x[b, :, t * cum:] = float("nan")
            kernels[b, ..., t:] = float("nan")
            bias[b, :, t:] = float("nan")
    dev = lambda t: t.to(DEV, torch.float32)
    got = lvc_gated(dev(x.transpose(1, 2)), dev(kernels), dev(bias), None if conv is None else conv.weight, None if conv is None else conv.bias,
                    dilation=max(dilation, 1), lengths=lens)
    torch.cuda.synchronize()
    assert got.shape == (x.shape[0], T * cum, C)
    got = got.double().cpu().transpose(1, 2)
    scale, worst = want.abs().max().item(), 0.0
    for b in range(x.shape[0]):
        n = (T if lens is None else lens[b]) * cum
        assert not torch.isnan(got[b, :, :n]).any(), f"row {b}: something behind the row's end was read"
        worst = max(worst, (got[b, :, :n] - want[b, :, :n]).abs().max().item())
        assert torch.isnan(got[b, :, n:]).all()   # behind the row: x as it was given
    base = max(err, ULP * scale)
    print(f"C {C} cum {cum} T {T} lens {lens} d {dilation}: device error {worst:.3e}, float32 restatement error {err:.3e}, one ulp at scale {ULP * scale:.3e}, "
          f"ratio {worst / base:.2f}")
    assert worst <= FACTOR * base, f"differs from float64 by {worst:.3e}, above {FACTOR} x {base:.3e}"


@pytest.mark.parametrize("C,cum", [(32, 64), (32, 8), (16, 256)])
def test_ragged_rows_have_the_bits_of_the_rows_alone_and_two_calls_agree(C, cum):
    lens = (5, 1, 2, 4)
    x, kernels, bias, conv = _inputs(C, cum, 5, lens, 9, seed=7)
    for b, t in enumerate(lens):
        x[b, :, t * cum:] = float("nan")
        kernels[b, ..., t:] = float("nan")
        bias[b, :, t:] = float("nan")
    dev = lambda t: t.to(DEV, torch.float32)
    xd, kd, bd = dev(x.transpose(1, 2)).contiguous(), dev(kernels), dev(bias)
    many = lvc_gated(xd, kd, bd, conv.weight, conv.bias, dilation=9, lengths=lens)
    assert torch.equal(many.view(torch.int32), lvc_gated(xd, kd, bd, conv.weight, conv.bias, dilation=9, lengths=lens).view(torch.int32))
    for b, t in enumerate(lens):
        alone = lvc_gated(xd[b:b + 1, :t * cum].contiguous(), kd[b:b + 1, ..., :t].contiguous(), bd[b:b + 1, :, :t].contiguous(), conv.weight, conv.bias,
                          dilation=9)
        assert torch.equal(alone[0], many[b, :t * cum]) and not torch.isnan(alone).any()


@pytest.mark.parametrize("C,cum", [(32, 64), (16, 8)])
def test_in_place_with_a_convolution_has_the_bits_of_the_call_with_an_out_of_its_own_and_is_refused_without_one(C, cum):
    """With a convolution the layer reads y from scratch, so out may be x.  Without one y IS x and a workgroup reads one position of
    its neighbours' either side: in place the result would depend on which workgroup ran first, so the library refuses before a launch."""
    lens = (5, 2, 3)
    x, kernels, bias, conv = _inputs(C, cum, 5, lens, 3, seed=9)
    dev = lambda t: t.to(DEV, torch.float32)
    xd, kd, bd = dev(x.transpose(1, 2)).contiguous(), dev(kernels), dev(bias)
    want = lvc_gated(xd, kd, bd, conv.weight, conv.bias, dilation=3, lengths=lens)
    mine = xd.clone()
    got = lvc_gated(mine, kd, bd, conv.weight, conv.bias, dilation=3, lengths=lens, in_place=True)
    assert got.data_ptr() == mine.data_ptr() and torch.equal(got, want) and not torch.equal(got, xd)
    before = xd.clone()
    with pytest.raises(Exception, match="out must not be x"):
        lvc_gated(xd, kd, bd, lengths=lens, in_place=True)
    torch.cuda.synchronize()
    assert torch.equal(xd, before)   # nothing was launched


def test_refusals_come_before_any_launch():
    x = torch.zeros(1, 16, 32, device=DEV)
    k, b = torch.zeros(1, 32, 64, 3, 2, device=DEV), torch.zeros(1, 64, 2, device=DEV)
    with pytest.raises(ValueError, match="kernels"):
        lvc_gated(x, k[:, :16], b)
    with pytest.raises(ValueError, match="bias"):
        lvc_gated(x, k, b[:, :, :1])
    with pytest.raises(ValueError, match="conv_weight"):
        lvc_gated(x, k, b, torch.zeros(32, 32, 3))
    with pytest.raises(ValueError, match="lengths"):
        lvc_gated(x, k, b, lengths=[3])
    with pytest.raises(Exception, match="dilation"):
        lvc_gated(x, k, b, torch.zeros(32, 32, 3), torch.zeros(32), dilation=37)
    wide = torch.zeros(1, 4, 64, device=DEV)
    with pytest.raises(Exception, match="channel_size"):
        lvc_gated(wide, torch.zeros(1, 64, 128, 3, 2, device=DEV), torch.zeros(1, 128, 2, device=DEV))
