"""The cases of tests/test_hifigan_layer_gpu.py (gvx_hifigan_layer: one layer of the HiFi-GAN, BigVGAN and UnivNet generators on its own),
their inputs and their float64 reference, shared with the CPU test that asserts what the table holds
(tests/test_generator_configs_cpu.py).  It imports nothing from genvox_amd.

The reference is torch's own ``conv1d`` / ``conv_transpose1d`` (kernel 2 r, stride r, padding r / 2) row by row at the row's own length,
in the dtype it is given: float64 for the reference, float32 for the reference's own rounding error, which sets the tolerance.  For a
data gradient it is autograd of ``conv1d(lrelu(m))`` at the cotangent dY, with respect to m.

``kernel_of`` restates the dispatch of hg_launch / hgb_dgrad (csrc/hifigan.hip, csrc/hifigan_train.hip)."""
import collections

import torch
import torch.nn.functional as F

FACTOR = 8.0
ULP = 2.0 ** -23
MASK_MARGIN = 1e-3   # |mask| is above it: the side of a LeakyReLU never hangs on rounding
S01 = float(torch.tensor(0.1, dtype=torch.float32))   # the device's 0.1

FORWARD_KERNELS = ("tile128", "tile64", "tile32", "valu")
WINDOWS = ((3, 1), (3, 36), (5, 2), (7, 5), (9, 9), (11, 5), (7, 12))   # (taps, dilation); 72 = the window limit three times over
PHASES = (2, 6, 10)
EPILOGUES = ("none", "res", "acc", "acc_div3", "res_div1")
GRAD_EPILOGUES = ("none", "mask", "mask_res", "mask_res_add2_div")
SLOPES = (0.0, S01, 1.0)
CHANNELS = ((32, 32), (36, 36), (40, 96), (72, 72), (64, 160), (144, 132), (8, 32), (12, 24), (34, 34), (36, 1))

# rows: frames per row (T is the largest); a row has frames * in_mul positions
Case = collections.namedtuple("Case", "cin cout taps dil phases rows in_mul epi act slope zero_tail tanh grad")


def kernel_of(cin: int, cout: int, grad: bool = False) -> str:
    """The forward has a dot-product kernel of eight lanes per element for Cout == 1; a data gradient runs one lane per element."""
    if cout >= 32 and cin % 4 == 0:
        return "tile128" if cout >= 128 else ("tile64" if cout > 32 else "tile32")
    return "valu8" if cout == 1 and not grad else "valu"


def left_of(case) -> int:
    return (case.taps - 1) * case.dil // 2 if case.phases == 1 else 1


def _fwd(ch, win, rows, epi="none", act=True, slope=S01, in_mul=1, zero_tail=False, tanh=False):
    return Case(ch[0], ch[1], win[0], win[1], 1, tuple(rows), in_mul, epi, act, slope, zero_tail, tanh, False)


def _up(ch, phases, rows, epi="none", act=True, slope=S01, zero_tail=False):
    return Case(ch[0], ch[1], 2, 0, phases, tuple(rows), 1, epi, act, slope, zero_tail, False, False)


def _grad(ch, win, rows, epi, slope=S01):
    return Case(ch[0], ch[1], win[0], win[1], 1, tuple(rows), 1, epi, False, slope, False, False, True)


def _forward_rows(a, b, up):
    """One forward kernel's rows: channels a and b in turns over the seven windows, `up` under the three phase counts."""
    return [
        _fwd(a, (3, 1), (257, 1, 129), "res"),                              # a ragged batch: row 1 ends inside tile 0, row 2 one past tile 0
        _fwd(b, (3, 36), (36, 37), "none", slope=0.0),                      # rows of left and left + 1 positions: the halo is wider than the row
        _fwd(a, (5, 2), (128, 2, 127), "acc", act=False, zero_tail=True),   # at and one short of the tile's edge
        _fwd(b, (7, 5), (129, 1, 65), "acc_div3", slope=1.0),
        _fwd(a, (9, 9), (127, 36, 37), "res_div1"),
        _fwd(b, (11, 5), (128, 1, 64), "res", zero_tail=True),
        _fwd(a, (7, 12), (22, 1, 11), "none", in_mul=6),                    # lens count frames of 6 positions: 132, 6 and 66
        _up(up, 2, (129, 1, 65)),
        _up(up, 6, (128, 2), "acc", slope=0.0),
        _up(up, 10, (127, 1, 64), "acc_div3", act=False, zero_tail=True),
    ]


CASES = (
    _forward_rows((64, 160), (144, 132), (36, 260))     # 128-wide: column tails of 32 and 4; 260 columns are three tiles under every phase
    + _forward_rows((36, 36), (72, 72), (36, 36))       # 64-wide: K tails of 4 and 8, column tails of 4 and 8, one tile under every phase
    + [_fwd((40, 96), (5, 2), (257, 1, 129), "res"), _up((40, 96), 6, (129, 1, 65))]   # two 64-wide tiles, a K tail of 8
    + _forward_rows((32, 32), (8, 32), (32, 32))        # 32-wide; 8 channels: the K block is mostly padding
    + _forward_rows((12, 24), (34, 34), (12, 24))       # dot products; 34 channels although Cout >= 32
    + [_up((34, 34), 6, (129, 1, 65))]
    # the output layer's kernel: eight lanes per element, tanh
    + [_fwd((36, 1), (7, 5), (257, 1, 129), "none", zero_tail=True, tanh=True), _fwd((36, 1), (3, 1), (128, 2, 127), "res", slope=0.0, tanh=True)]
    # data gradients: (cin, cout) = the channels of dY and of dX
    + [
        _grad((64, 160), (3, 1), (257, 1, 129), "mask"),
        _grad((144, 132), (9, 9), (36, 37), "mask_res", slope=0.0),
        _grad((64, 160), (7, 12), (129, 1, 65), "mask_res_add2_div", slope=1.0),
        _grad((144, 132), (5, 2), (128, 2, 127), "none"),
        _grad((36, 36), (3, 36), (129, 1, 65), "mask"),
        _grad((40, 96), (7, 5), (128, 2), "mask_res", slope=1.0),
        _grad((72, 72), (11, 5), (257, 1, 129), "mask_res_add2_div", slope=0.0),
        _grad((36, 36), (9, 9), (37, 36, 127), "none"),
        _grad((32, 32), (5, 2), (257, 1, 129), "mask", slope=0.0),
        _grad((8, 32), (3, 36), (36, 37), "mask_res"),
        _grad((32, 32), (7, 12), (128, 127), "mask_res_add2_div"),
        _grad((8, 32), (11, 5), (129, 1, 65), "none"),
        _grad((12, 24), (3, 1), (257, 1, 129), "mask"),
        _grad((34, 34), (9, 9), (127, 36, 37), "mask_res", slope=0.0),
        _grad((12, 24), (7, 5), (128, 2, 127), "mask_res_add2_div"),
        _grad((34, 34), (3, 36), (129, 1, 65), "none"),
        _grad((36, 1), (7, 12), (129, 1, 65), "mask", slope=1.0),
    ]
)


def case_id(case) -> str:
    kind = "grad" if case.grad else (f"x{case.phases}" if case.phases > 1 else "conv")
    win = "" if case.phases > 1 else f"-k{case.taps}d{case.dil}"
    rows = "_".join(str(r) for r in case.rows) + (f"x{case.in_mul}" if case.in_mul > 1 else "")
    return f"{kind}-{case.cin}to{case.cout}{win}-{rows}-{case.epi}" + ("-tanh" if case.tanh else "")


def divide_of(case) -> float:
    return {"acc_div3": 3.0, "res_div1": 1.0, "mask_res_add2_div": 3.0}.get(case.epi, 0.0)


def inputs(case, seed: int):
    """float64 tensors holding float32 values, channels-first [B, C, positions]: x (the operand; dY of a gradient), weight in PyTorch's
    layout, bias, and what the epilogue takes - res, out0 (what ``out`` holds before an accumulating call), mask, add2."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
    B, L = len(case.rows), max(case.rows) * case.in_mul
    t = dict(x=rnd(B, case.cin, L))
    if case.phases > 1:
        t["weight"] = (rnd(case.cin, case.cout, 2 * case.phases) * (2 * case.cin) ** -0.5).float().double()
    elif case.grad:
        t["weight"] = (rnd(case.cin, case.cout, case.taps) * (case.taps * case.cin) ** -0.5).float().double()   # the forward's [N, C, k]
    else:
        t["weight"] = (rnd(case.cout, case.cin, case.taps) * (case.taps * case.cin) ** -0.5).float().double()
    if not case.grad:
        t["bias"] = (0.1 * rnd(case.cout)).float().double()
    if "res" in case.epi:
        t["res"] = rnd(B, case.cout, L)
    if "acc" in case.epi:
        t["out0"] = rnd(B, case.cout, L * case.phases)
    if "mask" in case.epi:
        m = rnd(B, case.cout, L)
        t["mask"] = (torch.where(m < 0, -1.0, 1.0) * (m.abs() + 2 * MASK_MARGIN)).float().double()
    if "add2" in case.epi:
        t["add2"] = rnd(B, case.cout, L)
    return t


def expression(case, t, b: int):
    """Row b alone at its own length, in the dtype of ``t`` -> [cout, positions * phases]."""
    n, k, d, dt = case.rows[b] * case.in_mul, case.taps, case.dil, t["x"].dtype
    x = t["x"][b:b + 1, :, :n]
    if case.grad:
        m = (t["mask"][b:b + 1, :, :n] if "mask" in t else torch.zeros(1, case.cout, n, dtype=dt)).clone().requires_grad_(True)
        # the forward convolution whose data gradient this is: [C = cout of the layer] -> [N = cin of the layer]
        y = F.conv1d(F.leaky_relu(m, case.slope) if "mask" in t else m, t["weight"], None, dilation=d, padding=(k - 1) * d // 2)
        (y * x).sum().backward()
        v = m.grad
        if "res" in t:
            v = v + t["res"][b:b + 1, :, :n]
        if "add2" in t:
            v = v + t["add2"][b:b + 1, :, :n]
    else:
        a = F.leaky_relu(x, case.slope) if case.act else x
        if case.phases == 1:
            v = F.conv1d(a, t["weight"], t["bias"], dilation=d, padding=(k - 1) * d // 2)
        else:
            v = F.conv_transpose1d(a, t["weight"], t["bias"], stride=case.phases, padding=case.phases // 2)
        if "res" in t:
            v = v + t["res"][b:b + 1, :, :n]
        if "out0" in t:
            v = t["out0"][b:b + 1, :, :n * case.phases] + v
    if divide_of(case) > 0:
        v = v / divide_of(case)
    if case.tanh:
        v = torch.tanh(v)
    return v.detach()[0]


def reference(case, t):
    """-> (float64 [B, cout, L * phases] with zeros behind every row, the largest |float32 restatement - float64| over the rows)."""
    B, L = len(case.rows), max(case.rows) * case.in_mul * case.phases
    want, err = torch.zeros(B, case.cout, L, dtype=torch.float64), 0.0
    t32 = {k: v.float() for k, v in t.items()}
    for b in range(B):
        w = expression(case, t, b)
        want[b, :, :w.shape[1]] = w
        err = max(err, (expression(case, t32, b).double() - w).abs().max().item())
    return want, err
