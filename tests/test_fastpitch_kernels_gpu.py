"""GPU: FastPitch's residual + LayerNorm kernel alone (gvx_add_layer_norm, fp_add_ln_kernel<NC> of csrc/fastpitch.hip, through
``fastpitch.add_layernorm``) against ``torch.nn.functional.layer_norm(x + y)`` in float64, row by row at the row's own length.

Tolerance: the 8 x rule exactly as tests/test_attention_kernel_gpu.py states it.  Every case evaluates the SAME restatement in float32 on
the CPU and takes its largest distance from float64; the device may differ from float64 by at most 8 times the larger of that number and
one float32 ulp at the tensor's scale.  The ratio is printed.

The shapes: the kernel gives a wave a position and a lane the channels ``lane + 64 i``, i < NC in (1, 2, 4, 8), and a workgroup
LN_POSITIONS = 16 positions.  C = 32 is one half-idle chunk, 64, 256 and 512 are whole chunks of NC = 1, 4 and 8, and 96, 160 and 288
end in a half-idle chunk behind one, two and four full ones - where a lane that holds no channel must stay out of the mean and of the
squared deviations.  N sits on, one before and one behind the workgroup's edge, at 1 and 2 (one wave writes both halo rows, two waves one
each) and at 33 (three workgroups).  Then ragged rows with NaN behind them, rows of variance 0, and a mean of 1000 over unit deviations.

Largest ratios seen on an MI355X: see README.md, "FastPitch"."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from genvox_amd import _lib
from genvox_amd.fastpitch import LN_EPS, LN_POSITIONS, MAX_DIM, add_layernorm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23
NAN = float("nan")
CHANNELS = (32, 64, 96, 160, 256, 288, 512)
LENGTHS = (1, 2, 15, 16, 17, 33)


def _ref(x, y, lens, lw, lb, dtype):
    """Every row alone at its own length: x, y [B, N, C] float64 (float32-representable) -> [B, N, C] in ``dtype``, zeros behind a row."""
    B, N, C_ = x.shape
    out = torch.zeros(B, N, C_, dtype=dtype)
    for b, n in enumerate([N] * B if lens is None else lens):
        if n > 0:
            v = x[b, :n].to(dtype)
            if y is not None:
                v = v + y[b, :n].to(dtype)
            out[b, :n] = F.layer_norm(v, (C_,), lw.to(dtype), lb.to(dtype), LN_EPS)
    return out


def _params(C_, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.75 + 0.5 * torch.rand(C_, generator=g)).double(), (0.1 * torch.randn(C_, generator=g)).double()   # float32-representable


def _inputs(B, N, C_, with_y, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, C_, generator=g).double()
    y = (0.5 * torch.randn(B, N, C_, generator=g)).double() if with_y else None
    return x, y


def _run(x, y, lens, lw, lb):
    """Both outputs start as NaN: every element is written.  NaN goes into x and y at and behind a row's length: never read."""
    B, N, C_ = x.shape
    x32, y32 = x.float(), None if y is None else y.float()
    for b, n in enumerate(lens if lens is not None else []):
        x32[b, n:] = NAN
        if y32 is not None:
            y32[b, n:] = NAN
    out = (torch.full((B, N + 2, C_), NAN, dtype=torch.float32, device=DEV), torch.full((B, N, C_), NAN, dtype=torch.float32, device=DEV))
    haloed, plain = add_layernorm(x32.to(DEV), lw.float().to(DEV), lb.float().to(DEV), None if y32 is None else y32.to(DEV), lens, out=out)
    torch.cuda.synchronize()
    return haloed, plain


def _check(x, y, lens, lw, lb, what):
    B, N, C_ = x.shape
    want = _ref(x, y, lens, lw, lb, torch.float64)
    err = (_ref(x, y, lens, lw, lb, torch.float32).double() - want).abs().max().item()
    haloed, plain = _run(x, y, lens, lw, lb)
    assert haloed.shape == (B, N + 2, C_) and plain.shape == (B, N, C_)
    assert not torch.isnan(haloed).any() and not torch.isnan(plain).any(), f"{what}: an element was not written"
    assert (haloed[:, 0] == 0).all() and (haloed[:, N + 1] == 0).all(), f"{what}: a halo row is not exact zeros"
    assert torch.equal(haloed[:, 1:N + 1], plain), f"{what}: the plain output differs from the haloed one's interior"
    d = (plain.double().cpu() - want).abs().max().item()
    scale = ULP * want.abs().max().item()
    base = max(err, scale)
    print(f"{what}: device error {d:.3e}, float32 restatement error {err:.3e}, one ulp at scale {scale:.3e}, ratio {d / base:.2f}")
    assert d <= FACTOR * base, f"{what}: differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"
    for b, n in enumerate(lens if lens is not None else []):
        assert (plain[b, n:] == 0).all(), f"{what}: row {b} is not exact zeros behind its length"
    return haloed, plain


def test_the_constants_are_the_ones_the_shapes_were_chosen_for():
    assert (LN_POSITIONS, MAX_DIM, LN_EPS) == (16, 512, 1e-5)
    assert LN_POSITIONS in LENGTHS and LN_POSITIONS - 1 in LENGTHS and LN_POSITIONS + 1 in LENGTHS and 2 * LN_POSITIONS + 1 in LENGTHS
    assert {(c + 63) // 64 for c in CHANNELS} == {1, 2, 3, 4, 5, 8}   # every NC: 1, 2, 4 (3 and 4 chunks), 8 (5 and 8 chunks)
    assert [c for c in CHANNELS if c % 64] == [32, 96, 160, 288]


@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("C_", CHANNELS)
def test_every_channel_count_at_every_workgroup_edge(C_, N, with_y):
    lw, lb = _params(C_, seed=C_)
    x, y = _inputs(2, N, C_, with_y, seed=1000 * C_ + N)
    _check(x, y, None, lw, lb, f"C {C_} N {N} {'x + y' if with_y else 'x alone'}")


@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("C_", CHANNELS)
def test_ragged_rows_with_nan_behind_them(C_, with_y):
    """Rows of N, 1, N - 1 and 16 positions at N = 33: NaN in x and y at and behind a row's length, exact zeros there in both outputs,
    every row the bits of that row run alone, two calls the same bits."""
    N = 2 * LN_POSITIONS + 1
    lens = (N, 1, N - 1, LN_POSITIONS)
    lw, lb = _params(C_, seed=C_ + 1)
    x, y = _inputs(4, N, C_, with_y, seed=7 * C_)
    haloed, plain = _check(x, y, lens, lw, lb, f"ragged C {C_} {'x + y' if with_y else 'x alone'}")
    again_haloed, again_plain = _run(x, y, lens, lw, lb)
    assert torch.equal(haloed, again_haloed) and torch.equal(plain, again_plain)
    for b, n in enumerate(lens):
        alone_haloed, alone_plain = _run(x[b:b + 1, :n], None if y is None else y[b:b + 1, :n], None, lw, lb)
        assert torch.equal(plain[b, :n], alone_plain[0]), f"row {b} of the ragged batch differs from the row alone"
        assert torch.equal(haloed[b, :n + 1], alone_haloed[0, :n + 1]) and (haloed[b, n + 1:] == 0).all(), f"row {b}, haloed"


@pytest.mark.parametrize("const", [0.75, 0.1])
@pytest.mark.parametrize("C_", [96, 512])
def test_a_constant_row_has_variance_zero(C_, const):
    """x + y constant over the channels: 0.75 sums exactly in float32, fl32(0.1) does not (its sum over C rounds, so the first mean may be
    an ulp off and the second centring pass has to take the rest).  Float64 gives the LayerNorm's shift; the same rule."""
    N = LN_POSITIONS + 3
    lw, lb = _params(C_, seed=5)
    c = torch.tensor(const).float().double()
    x = (c * (1 + torch.arange(N, dtype=torch.float64) % 3))[None, :, None].expand(2, N, C_).contiguous()   # a different constant per position
    x = x.float().double()
    want = _ref(x, None, (N, 4), lw, lb, torch.float64)
    assert torch.equal(want[0], lb.expand(N, C_)) and torch.equal(want[1, :4], lb.expand(4, C_))
    _check(x, None, (N, 4), lw, lb, f"constant {const} C {C_}, x alone")
    half = 0.25 * torch.ones_like(x)
    _check((x - half).float().double(), half, (N, 4), lw, lb, f"constant {const} C {C_}, x + y")   # still one value over a position's channels


@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("C_", [64, 512])
def test_a_mean_of_a_thousand_over_unit_deviations(C_, with_y):
    """A variance formed as a mean of squares minus a squared mean would lose every digit (tests/test_vocos_kernels_gpu.py, the body this
    kernel copies)."""
    N = LN_POSITIONS + 1
    lw, lb = _params(C_, seed=77)
    g = torch.Generator().manual_seed(C_)
    x = (1e3 + torch.randn(2, N, C_, generator=g)).double()
    y = None
    if with_y:
        y = (400.0 + torch.randn(2, N, C_, generator=g)).double()
        x = (x.float() - 400.0).double()
    _check(x, y, (N, 5), lw, lb, f"mean 1e3 C {C_} {'x + y' if with_y else 'x alone'}")


def test_refused_arguments():
    lib = _lib.load()
    B, N, C_ = 2, 5, 64
    x, y = torch.zeros(B, N, C_, device=DEV), torch.zeros(B, N, C_, device=DEV)
    lw, lb = torch.ones(C_, device=DEV), torch.full((C_,), 0.5, device=DEV)   # a launch would write 0.5
    haloed, plain = torch.zeros(B, N + 2, C_, device=DEV), torch.zeros(B, N, C_, device=DEV)
    p = lambda t: t.data_ptr()
    good = dict(x=p(x), y=p(y), lens=None, B=B, N=N, C=C_, ln_w=p(lw), ln_b=p(lb), out=p(haloed), out2=p(plain))

    def refused(reason, **change):
        a = {**good, **change}
        rc = lib.gvx_add_layer_norm(a["x"], a["y"], a["lens"], a["B"], a["N"], a["C"], a["ln_w"], a["ln_b"], a["out"], a["out2"], None)
        assert rc == -1, (change, rc)   # GVX_ERR_INVALID_ARG, before any launch
        assert reason in lib.gvx_last_error().decode(), (change, lib.gvx_last_error().decode())

    for name in ("x", "ln_w", "ln_b", "out"):
        refused("null argument", **{name: None})
    for bad in (0, 16, 48, 80, MAX_DIM + 32, 2 * MAX_DIM, -64):
        refused("multiple of 32", C=bad)
    for bad in (0, -1, 65536):
        refused("B must be", B=bad)
    for bad in (0, -1, (1 << 16) + 1):
        refused("positions of a row", N=bad)
    refused("beyond 2^24", B=65535, N=1 << 16)
    f4 = ctypes.sizeof(ctypes.c_float)
    refused("overlaps an input", out=p(x))
    refused("overlaps an input", out2=p(x))
    refused("overlaps an input", out=p(y))
    refused("overlaps an input", out2=p(y) + f4 * (B * N * C_ - 1))   # its first element is y's last
    refused("overlaps an input", out2=p(lw))
    refused("overlaps an input", out=p(lb) - f4 * (B * (N + 2) * C_ - 1))   # its last element is ln_b's first
    refused("out_haloed and out_plain overlap", out2=p(haloed) + f4 * C_)
    refused("out_haloed and out_plain overlap", out2=p(haloed))
    torch.cuda.synchronize()
    assert not haloed.any() and not plain.any() and not x.any()   # nothing was launched
    # out_plain may be NULL, y may be NULL
    assert lib.gvx_add_layer_norm(p(x), None, None, B, N, C_, p(lw), p(lb), p(haloed), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(haloed[:, 1:N + 1], lb.expand(B, N, C_)) and not haloed[:, 0].any() and not haloed[:, N + 1].any() and not plain.any()

    # the wrapper: float32, on the device, of the right shape
    for bad in (dict(x=x.double()), dict(x=x.cpu()), dict(x=x[0]), dict(x=torch.zeros(B, N, 48, device=DEV), lw=torch.ones(48, device=DEV), lb=torch.ones(48, device=DEV)),
                dict(x=torch.zeros(B, N, MAX_DIM + 32, device=DEV), lw=torch.ones(MAX_DIM + 32, device=DEV), lb=torch.ones(MAX_DIM + 32, device=DEV)),
                dict(x=torch.zeros(B, 0, C_, device=DEV)), dict(y=y[:, :4]), dict(y=y.double()), dict(y=y.cpu()), dict(lw=lw[:32]), dict(lb=lb.double()),
                dict(lw=lw.cpu()), dict(lb=lb.reshape(1, C_)), dict(lens=[N]), dict(lens=[N, N + 1]), dict(lens=[-1, N]),
                dict(out=(plain, plain)), dict(out=(haloed, plain.double())), dict(out=(haloed.cpu(), plain))):
        a = dict(x=x, lw=lw, lb=lb, y=y, lens=None, out=None)
        a.update(bad)
        with pytest.raises(ValueError):
            add_layernorm(a["x"], a["lw"], a["lb"], a["y"], a["lens"], out=a["out"])
    with pytest.raises(_lib.GvxError, match="overlaps an input"):
        add_layernorm(x, lw, lb, y, out=(haloed, x))
