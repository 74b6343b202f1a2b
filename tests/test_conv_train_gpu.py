"""GPU: the training-mode convolution layer as the operation it is - gvx_conv_bn_act_train_forward / _backward
(genvox_amd/csrc/train_conv.hip) through ctypes, every element of every output against float64 autograd.

The reference here is NOT oracle/train_ref.py: F.conv1d -> F.batch_norm(training=True, momentum 0.1, eps 1e-5) -> none / relu / tanh
-> * keep / (1 - p) in torch float64 on the CPU, gradients by autograd from a given dy.  Every leaf is the fp32 number the kernel
gets, so the only difference is the kernel's arithmetic.  With x_wgrad, dw is conv1d_weight(x_wgrad, dz): the weight gradient's
input is x_wgrad while dz (and with it dx, dbias, dgamma, dbeta) stays that of the layer's own input, as train_conv.hip's backward
states it.  torch refuses one value per channel in training mode, so rows = B T = 1 takes the explicit form the header documents
(xhat = 0, y = act(beta); dx, dw, dbias, dgamma zero, dbeta = du; running_var times 0.9).
relu: a pre-activation within a few u of 0 has no stable gradient.  The elements where the kernel's y and float64 fall on different
sides of the kink are excluded by giving them dy = 0 after the forward call (du is then 0 on either side); they must be fewer
than one in 10^4 of a case's elements (asserted), and their y is held to its bound like every other.

The bounds, u = 2^-24, K = k Cin, n = B T, per channel c: m, std, invstd the batch statistics, X = max |xhat|, G = |gamma| invstd.
  z (pre-BatchNorm, not an output): an fma chain of K products in any order, the bias added to the finished sum in the epilogue:
      E = max_r ((K + 1) u (|x| * |w|) + u |z|).
  xhat: Exh = invstd (E (2 + X) + u |m|) + 2 u X - the element's own E, the mean's, the deviation's (d invstd / invstd <= E / std,
      times |xhat|), and the batch mean rounded once to fp32 (u |m|: what channel means of order 1e3 cost).
  y:  s (|gamma| Exh + 4 u (|gamma| X + |beta|) + 4 u max |a|), s = 1 / (1 - p): per channel, carrying |gamma| invstd; the
      activations are 1-Lipschitz, tanhf is good to a few u of its result.
  running_mean: 0.1 (E + u |m|) + 3 u (0.9 |rm| + 0.1 |m|);  running_var: 0.1 f (2 std E + E^2) + 3 u (0.9 |rv| + 0.1 f var), f = n / (n - 1).
  du (not an output): edu = s |dy| 2 |a| Ea + 3 u |du| per element (tanh' = 1 - a^2 at an a that is Ea off; Ea = y's bound / s), 3 u |du| else.
  dbeta:  sum_r edu + 2 u sum_r |du| (double accumulation, one rounding to fp32).
  dgamma: sum_r (edu |xhat| + |du| Exh) + 3 u sum_r |du| |xhat|.
  dz (not an output) = gamma invstd (du - dbeta / n - xhat dgamma / n) cancels, so it is bounded against the channel's largest terms,
      not per element: edz = G (max edu + e(dbeta) / n + X e(dgamma) / n + Exh |dgamma| / n + (E / std + 10 u) (max |du| + |dbeta| / n + X |dgamma| / n)).
  dbias = sum_r dz is 0 in exact arithmetic.  What the kernel sums are the fp32 dz: each a few u of its three terms off, and xhat's
      common shift (Exh, the rounded mean above all) leaves mean(xhat) dgamma behind:
      |dbias| <= G (8 u (sum_r |du| + |dbeta| + mean_r |xhat| |dgamma|) + Exh |dgamma|).  No absolute floor: a column sum of anything that
      is not dz (du, say: that is dbeta) is of the order of sqrt(n) |du|, a million times that.
  dw: a chain of n addends cut into split-K pieces that are added in order: (n + pieces + 2) u sum_r |dz| |x| + edz sum_r |x| per element,
      both sums in float64 over the very rows the element sums over.  One foreign addend - a k-quad of the K-major loader landing
      on the wrong padded row at a sequence border - is of the order |dz| |x|: thousands of u.
  dx: (k Cout + 2) u sum |dz| |w| + sum edz |w| per element.
Every bound is multiplied by TOL[name].  The derived bounds are worst cases over the order of summation and over the signs of
every rounding, which a chain of hundreds of addends never meets, so the largest error / bound a run meets is collected in
RATIOS (written as JSON when GVX_CONV_REPORT names a file) and TOL holds the tightening where that ratio was below 0.1.
Measured on the derived bounds (worst case of the table): dbeta 0.88 (t_13x5_24to40_k5), running_mean 0.53, running_var 0.46 (r_2x1_8to136_k3),
y 0.30, dbias 0.16, dgamma 0.15, dw 0.077 (all off_3x3_8to136_k5), dx 0.0064 (r_1x127_8to8_k3) - so dw is held to 0.4 and dx to 0.03 of
theirs, the rest to the bound as derived.

Buffers: y, dx, dw and the six vectors lie between sentinel borders and start as finite junk; `saved` and `workspace` have exactly
the sizes the two queries return, a sentinel border around them, and are filled with NaN before the forward and (the workspace) again
before the backward: a halo row, a padding column or a split-K partial tile that is read without having been written shows as NaN.
The shapes and the branch each one is there for are in tests/helpers.py; tests/test_host_cpu.py pins them on the CPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from genvox_amd import _lib
from tests.helpers import CONV_TRAIN_BY_NAME, CONV_TRAIN_CASES, CONV_TRAIN_OPTION_CASES, CONV_TRAIN_REGROUP_CASES

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-5
SENTINEL = 0x5A5A5A5A
GUARD = 64            # words of sentinel in front of and behind every buffer (256 bytes: the payload stays 256-byte aligned)
ACT = {"none": 0, "relu": 1, "tanh": 2}
OUTPUTS = ("y", "running_mean", "running_var", "dx", "dw", "dbias", "dgamma", "dbeta")
TOL = {k: 1.0 for k in OUTPUTS}
TOL["dw"], TOL["dx"] = 0.4, 0.03   # measured 0.077 and 0.0064 of the derived bound (the others 0.15 .. 0.88: left as derived)
RATIOS = {}           # output name -> (largest error / bound, case)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GVX_CONV_REPORT")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({k: {"ratio": v[0], "case": v[1]} for k, v in sorted(RATIOS.items())}, f, indent=1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Out:
    """A device buffer of fp32 words with a sentinel border on both sides; `t` is the payload, pre-filled with finite junk."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)
        self.t.copy_(torch.linspace(-7.0, 9.0, self.n, device="cuda").view(*shape))

    def border_intact(self):
        w = self.buf.view(torch.int32)
        return bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + self.n:] == SENTINEL).all())


class _Scratch:
    """`nbytes` bytes (a multiple of 4) between sentinel borders, not one more: what a size query returned.  fill_nan() before a call."""

    def __init__(self, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        self.nbytes, self.n = nbytes, nbytes // 4
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        assert self.ptr % 256 == 0

    def fill_nan(self):
        self.buf[GUARD:GUARD + self.n] = -1      # 0xFFFFFFFF: a NaN in every word

    def border_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_inputs(case, regroup=False):
    """The fp32 tensors one call gets, on the host.  regroup: the same rows as ONE sequence of B T frames."""
    B, Cin, Cout, T, k = case.B, case.Cin, case.Cout, case.T, case.k
    g = torch.Generator().manual_seed(7000 + sum(map(ord, case.name)))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    x = r(B, Cin, T) * (0.25 + 1.5 * torch.rand(1, Cin, 1, generator=g))
    w = r(Cout, Cin, k) * (1.0 / (Cin * k) ** 0.5) * (0.5 + 1.5 * torch.rand(Cout, 1, 1, generator=g))
    sign = torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0)
    b = 0.1 * r(Cout) + case.offset * sign * (0.5 + torch.rand(Cout, generator=g))
    gamma = (1.0 + 0.2 * r(Cout)) * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0)
    beta = 0.3 * r(Cout)
    dy = r(B, Cout, T)
    keep = None if case.p is None else (torch.rand(B, Cout, T, generator=g) < (0.8 if case.p == 0.0 else 1.0 - case.p)).to(torch.uint8)
    rm, rv = 0.5 * r(Cout) + case.offset * sign, 0.5 + torch.rand(Cout, generator=g)
    xw = x * (torch.rand(B, 1, T, generator=g) < 0.7) + 0.05 * r(B, Cin, T)      # a masked, slightly different input for the weight gradient
    inp = dict(x=x, w=w, b=b, gamma=gamma, beta=beta, dy=dy, keep=keep, rm=rm, rv=rv, xw=xw)
    if regroup:
        flat = lambda t: None if t is None else t.transpose(0, 1).reshape(1, t.shape[1], B * T).contiguous()
        inp.update(x=flat(x), dy=flat(dy), keep=flat(keep), xw=flat(xw))
    return inp


# --------------------------------------------------------------------------------------------------------------- reference
def reference(case, inp, use_xw=False, y_got=None):
    """float64 forward + autograd of one layer, and the bound of every output (module docstring).  Returns (ref, bound, dy): dy is
    inp["dy"] with the elements zeroed where y_got (the kernel's y) took the other side of the relu kink - the dy the kernel must be given."""
    k, act, p = case.k, case.act, case.p
    pad = (k - 1) // 2
    d = lambda t: t.double()
    x, w, b, gamma, beta = (d(inp[n]).requires_grad_() for n in ("x", "w", "b", "gamma", "beta"))
    B, Cin, T = x.shape
    Cout = w.shape[0]
    n, K = B * T, k * Cin
    keep = None if inp["keep"] is None else d(inp["keep"])
    s = 1.0 if keep is None else 1.0 / (1.0 - p)
    z = F.conv1d(x, w, b, padding=pad)
    z.retain_grad()
    rm, rv = d(inp["rm"]).clone(), d(inp["rv"]).clone()
    if n > 1:
        ub = F.batch_norm(z, rm, rv, gamma, beta, training=True, momentum=0.1, eps=EPS)
    else:   # (torch raises "Expected more than 1 value per channel"; include/genvox_amd.h says what the library does)
        ub = beta.view(1, -1, 1) + gamma.view(1, -1, 1) * (z - z)
        rm, rv = 0.9 * rm + 0.1 * z.detach().view(-1), 0.9 * rv
    ub.retain_grad()
    a = {"none": lambda t: t, "relu": torch.relu, "tanh": torch.tanh}[act](ub)
    y = a if keep is None else a * keep * s

    # ---- forward bounds
    zd = z.detach()
    ch = lambda t: t.view(1, -1, 1)
    amax = lambda t: t.abs().amax(dim=(0, 2))
    with torch.no_grad():
        E = amax((K + 1) * U * F.conv1d(x.abs(), w.abs(), None, padding=pad) + U * zd.abs())
        m, var = zd.mean(dim=(0, 2)), zd.var(dim=(0, 2), unbiased=False)
        std, invstd = var.sqrt(), 1.0 / (var + EPS).sqrt()
        xhat = (zd - ch(m)) * ch(invstd)
        X, G = amax(xhat), gamma.abs() * invstd
        Exh = invstd * (E * (2 + X) + U * m.abs()) + 2 * U * X
        Ea = gamma.abs() * Exh + 4 * U * (gamma.abs() * X + beta.abs()) + 4 * U * amax(a)
        f = n / (n - 1.0) if n > 1 else 1.0
        bound = {"y": (s * ch(Ea)).expand_as(y),
                 "running_mean": 0.1 * (E + U * m.abs()) + 3 * U * (0.9 * d(inp["rm"]).abs() + 0.1 * m.abs()),
                 "running_var": 0.1 * f * (2 * std * E + E * E) + 3 * U * (0.9 * d(inp["rv"]).abs() + 0.1 * f * var)}
        dy = d(inp["dy"]).clone()
        if act == "relu" and y_got is not None:
            kink = (ub.detach() > 0) != (y_got > 0)
            if keep is not None:
                kink &= keep > 0
            assert int(kink.sum()) <= 1e-4 * kink.numel(), (case.name, int(kink.sum()), kink.numel())
            dy[kink] = 0.0
    y.backward(dy)
    with torch.no_grad():
        du, dz = ub.grad, z.grad
        xw = d(inp["xw"]) if use_xw else x.detach()
        dw = torch.nn.grad.conv1d_weight(xw, w.shape, dz, padding=pad) if use_xw else w.grad
        ref = {"y": y.detach(), "running_mean": rm, "running_var": rv, "dx": x.grad, "dw": dw, "dbias": b.grad, "dgamma": gamma.grad,
               "dbeta": beta.grad, "du": du, "dz": dz}
        # ---- backward bounds
        rsum = lambda t: t.sum(dim=(0, 2))
        edu = 3 * U * du.abs()
        if act == "tanh":
            edu = edu + s * dy.abs() * (1.0 if keep is None else keep) * 2 * a.detach().abs() * ch(Ea)
        dbeta, dgamma = beta.grad.abs(), gamma.grad.abs()
        e_dbeta = rsum(edu) + 2 * U * rsum(du.abs())
        e_dgamma = rsum(edu * xhat.abs() + du.abs() * ch(Exh)) + 3 * U * rsum(du.abs() * xhat.abs())
        D = amax(du)
        edz = G * (amax(edu) + e_dbeta / n + X * e_dgamma / n + Exh * dgamma / n + (E * invstd + 10 * U) * (D + dbeta / n + X * dgamma / n))
        pieces = case.plan[5] if (B, T) == (case.B, case.T) else 8
        ones = torch.ones(B, 1, T, dtype=torch.float64)
        bound.update({
            "dbeta": e_dbeta, "dgamma": e_dgamma,
            "dbias": G * (8 * U * (rsum(du.abs()) + dbeta + rsum(xhat.abs()) / n * dgamma) + Exh * dgamma),
            "dw": (n + pieces + 2) * U * torch.nn.grad.conv1d_weight(xw.abs(), w.shape, dz.abs(), padding=pad)
                  + edz.view(-1, 1, 1) * torch.nn.grad.conv1d_weight(xw.abs(), (1, Cin, k), ones, padding=pad),
            "dx": (k * Cout + 2) * U * F.conv_transpose1d(dz.abs(), w.abs(), padding=pad)
                  + F.conv_transpose1d(ch(edz).expand(B, Cout, T).contiguous(), w.abs(), padding=pad)})
    return ref, bound, dy.float()


# ------------------------------------------------------------------------------------------------------------------ the call
def run_layer(lib, case, inp, dy, want_dx=True, use_xw=False):
    """One forward and one backward call on sentinel-bordered buffers; returns the outputs on the host (dx None when not asked for).
    dy: a tensor, or a function of the forward's y that returns it."""
    B, Cin, T = inp["x"].shape
    Cout, k = case.Cout, case.k
    dev = lambda t: None if t is None else t.cuda().contiguous()
    p_ = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    x, w, b, gamma, beta, keep = (dev(inp[n]) for n in ("x", "w", "b", "gamma", "beta", "keep"))
    xw = dev(inp["xw"]) if use_xw else None
    sb, wb = lib.gvx_conv_train_saved_bytes(B, Cin, Cout, T, k), lib.gvx_conv_train_workspace_bytes(B, Cin, Cout, T, k)
    saved, ws = _Scratch(sb), _Scratch(wb)
    o = {"y": _Out((B, Cout, T)), "dx": _Out((B, Cin, T)), "dw": _Out((Cout, Cin, k))}
    o.update({name: _Out((Cout,)) for name in ("running_mean", "running_var", "dbias", "dgamma", "dbeta")})
    if case.running:
        o["running_mean"].t.copy_(inp["rm"])
        o["running_var"].t.copy_(inp["rv"])
    junk = {name: o[name].t.clone() for name in o}
    saved.fill_nan()
    ws.fill_nan()
    p = 0.0 if case.p is None else case.p
    rc = lib.gvx_conv_bn_act_train_forward(p_(x), p_(w), p_(b), p_(gamma), p_(beta), p_(o["running_mean"].t) if case.running else None,
                                           p_(o["running_var"].t) if case.running else None, B, Cin, Cout, T, k, ACT[case.act], p_(keep), p,
                                           p_(o["y"].t), saved.ptr, sb, ws.ptr, wb, _stream())
    assert rc == 0, (rc, lib.gvx_last_error())
    torch.cuda.synchronize()
    dyd = dev(dy(o["y"].t.cpu()) if callable(dy) else dy)
    ws.fill_nan()
    rc = lib.gvx_conv_bn_act_train_backward(p_(dyd), saved.ptr, sb, p_(w), p_(gamma), p_(xw), B, Cin, Cout, T, k, ACT[case.act], p_(keep), p,
                                            p_(o["dx"].t) if want_dx else None, p_(o["dw"].t), p_(o["dbias"].t), p_(o["dgamma"].t),
                                            p_(o["dbeta"].t), ws.ptr, wb, _stream())
    assert rc == 0, (rc, lib.gvx_last_error())
    torch.cuda.synchronize()
    assert saved.border_intact() and ws.border_intact(), "a write past the size a query returned"
    for name, buf in o.items():
        assert buf.border_intact(), name
    untouched = [] if case.running else ["running_mean", "running_var"]
    if not want_dx:
        untouched.append("dx")
    for name in untouched:
        assert torch.equal(o[name].t, junk[name]), name + " written although NULL was passed"
    return {name: (None if name in untouched else buf.t.cpu()) for name, buf in o.items()}


def run_both(lib, case, inp, **kw):
    """The kernel's outputs and the float64 reference of the same call: (got, ref, bound, dy)."""
    box = []

    def dy_after_forward(y_got):
        box.append(reference(case, inp, use_xw=kw.get("use_xw", False), y_got=y_got))
        return box[0][2]
    got = run_layer(lib, case, inp, dy_after_forward, **kw)
    return (got,) + box[0]


def far_apart(name, a, b, bound):
    """Some element of a and b differs by more than eight times the bound the kernel is held to."""
    return bool(((a - b).abs() > 8 * TOL[name] * bound).any())


def compare(case, got, ref, bound, names=OUTPUTS, tag=""):
    for name in names:
        if got[name] is None:
            continue
        g = got[name].double()
        assert bool(torch.isfinite(g).all()), (case.name, name, "not finite: something read that was never written")
        err, bd = (g - ref[name]).abs(), TOL[name] * bound[name]
        ratio = float(torch.where(err > 0, err / bd.clamp_min(1e-300), torch.zeros_like(err)).max())
        if ratio > RATIOS.get(name, (0.0, ""))[0]:
            RATIOS[name] = (ratio, case.name + tag)
        if ratio > 1.0:
            i = int(torch.argmax((err / bd.clamp_min(1e-300)).flatten()))
            idx = np.unravel_index(i, tuple(g.shape))
            raise AssertionError("%s%s %s%s: got %.9g, float64 %.9g, error %.3g = %.3g x bound (%d of %d elements above it)" % (
                case.name, tag, name, list(map(int, idx)), float(g.flatten()[i]), float(ref[name].flatten()[i]), float(err.flatten()[i]), ratio,
                int((err > bd).sum()), err.numel()))


# ------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("case", CONV_TRAIN_CASES, ids=lambda c: c.name)
def test_layer_against_float64_autograd(lib, case):
    """Every element of y, the running statistics and the five gradients within its derived bound, all of them finite although every
    byte of `saved` and `workspace` started as NaN, every border intact."""
    inp = make_inputs(case)
    got, ref, bound, _ = run_both(lib, case, inp)
    compare(case, got, ref, bound)
    if case.B * case.T == 1:   # one value per channel (include/genvox_amd.h): zeros are exact zeros, running_var loses a tenth
        for name in ("dx", "dw", "dbias", "dgamma"):
            assert not bool(got[name].any()), name
        if case.running:
            assert torch.equal(got["running_var"], (1.0 - torch.tensor(0.1)) * inp["rv"])


@pytest.mark.parametrize("name", CONV_TRAIN_OPTION_CASES + ["sk_23x89_24to24_k5", "m_1x568_512to80_k5"])
def test_two_identical_calls_are_bit_equal(lib, name):
    """Every sum of the layer has a fixed order (double-precision column sums lane by lane, split-K pieces added in index order)."""
    case = CONV_TRAIN_BY_NAME[name]
    inp = make_inputs(case)
    a, _, _, dy = run_both(lib, case, inp)
    b = run_layer(lib, case, inp, dy)
    for n in OUTPUTS:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("name", CONV_TRAIN_OPTION_CASES)
def test_dx_null_and_x_wgrad(lib, name):
    """dx = NULL changes nothing else, bit for bit.  x_wgrad changes dw alone - to the weight gradient of x_wgrad under the dz of
    the layer's own input, element by element within dw's bound - and leaves every other output bit-equal."""
    case = CONV_TRAIN_BY_NAME[name]
    inp = make_inputs(case)
    base, ref, bound, dy = run_both(lib, case, inp)
    compare(case, base, ref, bound)
    nodx = run_layer(lib, case, inp, dy, want_dx=False)
    assert nodx["dx"] is None
    for n in OUTPUTS:
        if n != "dx":
            assert torch.equal(base[n], nodx[n]), n
    got_w, ref_w, bound_w, dy_w = run_both(lib, case, inp, use_xw=True)
    assert torch.equal(dy, dy_w)
    for n in OUTPUTS:
        if n != "dw":
            assert torch.equal(base[n], got_w[n]), n
            assert torch.equal(ref[n], ref_w[n]), n
    compare(case, got_w, ref_w, bound_w, names=("dw",), tag="+x_wgrad")
    # the two weight gradients are different tensors: a kernel that ignored x_wgrad would be far outside the bound
    assert far_apart("dw", ref_w["dw"], ref["dw"], bound_w["dw"])


@pytest.mark.parametrize("name", CONV_TRAIN_REGROUP_CASES)
def test_sequences_are_not_one_long_sequence(lib, name):
    """Batch statistics tie every row to every other, so rows of the batch are not independent here.  What the row maps' R decides
    is where the halos lie: B sequences of T frames and ONE sequence of B T frames with the same rows differ at every sequence
    border.  Both must match their own float64 reference, and the references differ by far more than the bounds - so a kernel that
    ignored R (one of the two groupings computed as the other) fails one of the two comparisons."""
    case = CONV_TRAIN_BY_NAME[name]
    assert case.B > 1 and case.k > 1
    inp, flat = make_inputs(case), make_inputs(case, regroup=True)
    got, ref, bound, _ = run_both(lib, case, inp)
    got1, ref1, bound1, _ = run_both(lib, case, flat)
    compare(case, got, ref, bound)
    compare(case, got1, ref1, bound1, tag="+one_sequence")
    as_rows = lambda t: t.transpose(0, 1).reshape(1, t.shape[1], -1)
    assert far_apart("y", as_rows(ref["y"]), ref1["y"], bound1["y"]) and far_apart("dw", ref["dw"], ref1["dw"], bound1["dw"])
    assert far_apart("dx", as_rows(ref["dx"]), ref1["dx"], bound1["dx"])
    assert not torch.equal(as_rows(got["y"]), got1["y"]) and not torch.equal(got["dw"], got1["dw"])
