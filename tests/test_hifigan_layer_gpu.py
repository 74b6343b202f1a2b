"""GPU: one layer of the HiFi-GAN / BigVGAN / UnivNet generators on its own (gvx_hifigan_layer, csrc/hifigan_train.hip, through
``hifigan.conv_layer``): the three matrix tiles and the dot-product kernels of csrc/hifigan_kernels.h, forward and data gradient, against
torch's own convolutions in float64 (tests/hifigan_layer_cases.py), element by element.

The table there picks its row lengths from the 128-position tile and from each window's halo, not from a model's frame count; its
channel counts leave K tails inside a 32-channel block and column tails inside every tile; every epilogue is checked on its own.
tests/test_generator_configs_cpu.py asserts what the table holds, kernel by kernel.

Every case: the operand, the residual, the mask and add2 are NaN behind each row's length, so a read past a row's end shows; ``out``
starts as NaN (as finite junk inside the rows where the layer accumulates) and behind a row must come out as exact zeros with
zero_tail and untouched without; every row has the bits of that row run alone; two calls give the same bits.

Tolerance: the project's rule, as tests/test_univnet_kernels_gpu.py: the device may differ from float64 by at most 8 times the larger of
the float32 restatement's own distance from float64 and one float32 ulp at the tensor's scale.  The ratio is printed.

Largest ratios seen on an MI355X: see README.md, "HiFi-GAN"."""
import pytest
import torch

from genvox_amd.hifigan import conv_layer
from tests import hifigan_layer_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _device_inputs(case, t, rows=None):
    """Channels-last float32 device tensors of rows ``rows`` (all: None) with NaN behind every row's length; a single row is cut to
    its own length."""
    B = len(case.rows)
    pick = range(B) if rows is None else rows
    alone = rows is not None and len(rows) == 1
    out = {}
    for name in ("x", "res", "mask", "add2", "out0"):
        if name not in t:
            continue
        mul = case.phases if name == "out0" else 1
        v = t[name].clone()
        for b in range(B):
            v[b, :, case.rows[b] * case.in_mul * mul:] = NAN
        v = v[list(pick)]
        if alone:
            v = v[:, :, :case.rows[rows[0]] * case.in_mul * mul]
        out[name] = v.transpose(1, 2).to(DEV, torch.float32).contiguous()
    return out


def _run(case, t, d, lens):
    out = d["out0"].clone() if "out0" in d else torch.full((d["x"].shape[0], d["x"].shape[1] * case.phases, case.cout), NAN, device=DEV)
    got = conv_layer(d["x"], t["weight"], t.get("bias"), dilation=max(case.dil, 1), stride=case.phases, lengths=lens, in_mul=case.in_mul,
                     act=case.act, slope=case.slope, res=d.get("res"), out=out, accumulate="acc" in case.epi, divide=K.divide_of(case),
                     zero_tail=case.zero_tail, tanh_out=case.tanh, gradient=case.grad, mask=d.get("mask"), add2=d.get("add2"))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return got


@pytest.mark.parametrize("index", range(len(K.CASES)), ids=[K.case_id(c) for c in K.CASES])
def test_layer_against_float64(index):
    case = K.CASES[index]
    t = K.inputs(case, seed=100 + index)
    want, err = K.reference(case, t)
    d = _device_inputs(case, t)
    got = _run(case, t, d, case.rows)
    assert got.shape == (len(case.rows), max(case.rows) * case.in_mul * case.phases, case.cout)
    assert torch.equal(got.view(torch.int32), _run(case, t, d, case.rows).view(torch.int32)), "two calls differ"
    host = got.double().cpu().transpose(1, 2)
    scale, worst = want.abs().max().item(), 0.0
    for b, frames in enumerate(case.rows):
        n = frames * case.in_mul * case.phases
        assert not torch.isnan(host[b, :, :n]).any(), f"row {b}: something behind the row's end was read"
        worst = max(worst, (host[b, :, :n] - want[b, :, :n]).abs().max().item())
        if case.zero_tail:
            assert not host[b, :, n:].any(), f"row {b}: not exact zeros behind the row"   # NaN is truthy
        else:
            assert torch.isnan(host[b, :, n:]).all(), f"row {b}: out was written behind the row"
        alone = _run(case, t, _device_inputs(case, t, [b]), None)
        assert torch.equal(alone[0].view(torch.int32), got[b, :n].view(torch.int32)), f"row {b} differs from that row run alone"
    base = max(err, K.ULP * scale)
    print(f"{K.case_id(case)} [{K.kernel_of(case.cin, case.cout, case.grad)}]: device error {worst:.3e}, float32 restatement error {err:.3e}, "
          f"one ulp at scale {K.ULP * scale:.3e}, ratio {worst / base:.2f}")
    assert worst <= K.FACTOR * base, f"differs from float64 by {worst:.3e}, above {K.FACTOR} x {base:.3e}"


def test_a_row_of_no_frames_is_left_alone_or_zeroed():
    """lens = 0: nothing of the row is read or computed; with zero_tail the whole row is zeros."""
    x = torch.full((2, 130, 36), NAN, device=DEV)
    x[0] = 0.5
    w, b = torch.ones(36, 36, 3) / 108, torch.zeros(36)
    for zero_tail in (False, True):
        out = conv_layer(x, w, b, lengths=(130, 0), zero_tail=zero_tail, out=torch.full((2, 130, 36), NAN, device=DEV))
        torch.cuda.synchronize()
        assert not torch.isnan(out[0]).any()
        assert not out[1].any() if zero_tail else torch.isnan(out[1]).all()


def test_refusals_come_before_any_launch():
    x = torch.zeros(1, 8, 36, device=DEV)
    w, b = torch.zeros(36, 36, 3), torch.zeros(36)
    out = torch.full((1, 8, 36), NAN, device=DEV)
    bad = [
        (dict(dilation=37), "GVX_HIFIGAN_MAX_WINDOW"),                      # (3 - 1) * 37 = 74
        (dict(dilation=0), "dilation"),
        (dict(slope=1.5), "slope"),
        (dict(divide=-1.0), "divide"),
        (dict(tanh_out=True), "tanh_out"),                                  # a matrix tile has no tanh
        (dict(mask=torch.zeros(1, 8, 36, device=DEV)), "mask and add2"),    # forward
        (dict(gradient=True, act=True), "data gradient"),
        (dict(gradient=True, zero_tail=True), "data gradient"),
    ]
    for kw, match in bad:
        with pytest.raises(Exception, match=match):
            conv_layer(x, w, None if kw.get("gradient") else b, out=out, **kw)
    with pytest.raises(Exception, match="bias"):
        conv_layer(x, w, None, out=out)
    with pytest.raises(Exception, match="taps must be odd"):
        conv_layer(x, torch.zeros(36, 36, 4), b, out=out)
    with pytest.raises(Exception, match="residual"):                        # a transposed convolution takes none
        conv_layer(x, torch.zeros(36, 36, 4), b, stride=2, res=torch.zeros(1, 8, 36, device=DEV))
    with pytest.raises(ValueError, match="lengths"):
        conv_layer(x, w, b, lengths=[9], out=out)
    with pytest.raises(ValueError, match="weight"):
        conv_layer(x, torch.zeros(36, 32, 3), b, out=out)
    with pytest.raises(ValueError, match="stride"):
        conv_layer(x, torch.zeros(36, 36, 6), b, stride=3)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()   # nothing was launched
    # 34 input channels with 34 outputs is NOT refused: it runs on the dot-product kernel (a case of the table)
