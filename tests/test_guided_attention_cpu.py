"""CPU: the float64 restatement of the guided attention loss (tests/guided_ref64.py) worked by hand, and what of the feature is host
logic - the argument checks of gvx_guided_attention_loss and gvx_train_decoder_bptt_ext, which run before anything touches a GPU,
and the criterion's Python surface.  The kernels themselves: tests/test_guided_attention_gpu.py."""
import ctypes as C
import math

import pytest
import torch

from genvox_amd import _lib
from tests import guided_ref64 as GR
from tests.helpers import BPTT_EVEN, bptt_args_for_plan, train_step_configs


def test_equal_lengths_put_exact_zeros_on_the_diagonal_and_a_diagonal_alignment_costs_nothing():
    T = L = 7
    G, live = GR.guide([L, 5], [T, 5], T, L, 0.4)
    assert bool(live[0].all()) and int(live[1].sum()) == 25
    for b, n in ((0, 7), (1, 5)):
        assert bool((torch.diagonal(G[b])[:n] == 0).all())
        off = G[b, :n, :n][~torch.eye(n, dtype=torch.bool)]
        assert bool((off > 0).all()) and bool((off < 1).all())
    assert bool((G[1, 5:] == 0).all()) and bool((G[1, :, 5:] == 0).all())
    # the same fraction by other integers is the same float64 quotient: T_b = 2 L_b has zeros at t = 2 l
    G2, _ = GR.guide([3], [6], 6, 3, 0.4)
    assert all(float(G2[0, 2 * l, l]) == 0.0 for l in range(3)) and float(G2[0, 1, 0]) > 0
    A = torch.zeros(2, T, L, dtype=torch.float64)
    A[0] = torch.eye(7)
    A[1, :5, :5] = torch.eye(5)
    assert float(GR.guided_attention_loss(A, [L, 5], [T, 5], 0.4)) == 0.0
    # one value by hand: l = 2, t = 0 of a 4 x 4 row, sigma = 0.5 -> 1 - exp(-(2/4)^2 / (2 * 0.25)) = 1 - exp(-0.5)
    G3, _ = GR.guide([4], [4], 4, 4, 0.5)
    assert abs(float(G3[0, 0, 2]) - (1.0 - math.exp(-0.5))) < 1e-15 and float(G3[0, 0, 2]) == float(G3[0, 2, 0])


def test_uniform_alignment_against_a_plain_triple_loop_and_the_cell_count():
    B, T, L, sigma = 3, 6, 5, 0.4
    tl, ml = [5, 3, 1], [6, 1, 4]
    assert GR.n_cells(tl, ml, T, L) == 5 * 6 + 3 * 1 + 1 * 4
    assert GR.n_cells([9, -2], [6, 3], 6, 5) == 5 * 6                     # clamped to [0, L] / [0, T]
    A = torch.zeros(B, T, L, dtype=torch.float64)
    for b in range(B):
        A[b, :, :tl[b]] = 1.0 / tl[b]                                        # what a softmax over equal energies gives
    s, n = 0.0, 0
    for b in range(B):
        for t in range(ml[b]):
            for l in range(tl[b]):
                s += (1.0 - math.exp(-((l / tl[b] - t / ml[b]) ** 2) / (2 * sigma * sigma))) * (1.0 / tl[b])
                n += 1
    got = float(GR.guided_attention_loss(A, tl, ml, sigma))
    assert n == 37 and abs(got - s / n) <= 1e-15 * abs(s / n) * 40
    # L_b = 1: the only cell of every frame is l = 0, G = 1 - exp(-(t / T_b)^2 / (2 sigma^2)); T_b = 1: t = 0 only
    G, _ = GR.guide(tl, ml, T, L, sigma)
    assert float(G[2, 0, 0]) == 0.0 and abs(float(G[2, 2, 0]) - (1 - math.exp(-(0.5 ** 2) / (2 * sigma * sigma)))) < 1e-15
    assert float(G[1, 0, 0]) == 0.0 and abs(float(G[1, 0, 2]) - (1 - math.exp(-((2 / 3) ** 2) / (2 * sigma * sigma)))) < 1e-15


def test_masked_cells_are_skipped_not_multiplied_and_the_gradient_is_alpha_g_over_n():
    B, T, L, sigma, alpha = 3, 6, 5, 0.3, 2.5
    tl, ml = [5, 3, 1], [6, 2, 4]
    gen = torch.Generator().manual_seed(3)
    A = torch.rand(B, T, L, generator=gen, dtype=torch.float64)
    _, live = GR.guide(tl, ml, T, L, sigma)
    want = GR.guided_attention_loss(A, tl, ml, sigma)
    poisoned = A.clone()
    poisoned[~live] = float("nan")
    assert float(GR.guided_attention_loss(poisoned, tl, ml, sigma)) == float(want)
    leaf = A.clone().requires_grad_()
    (alpha * GR.guided_attention_loss(leaf, tl, ml, sigma)).backward()
    dA = GR.alignment_grad(tl, ml, T, L, sigma, alpha)
    assert bool((dA[~live] == 0).all()) and bool((leaf.grad[~live] == 0).all())
    assert float((leaf.grad - dA).abs().max()) <= 1e-16
    # no cell at all: loss 0, gradient 0
    assert float(GR.guided_attention_loss(A, [0, 0, 0], ml, sigma)) == 0.0 and float(GR.alignment_grad([0, 0, 0], ml, T, L, sigma, alpha).abs().max()) == 0.0


def test_guided_attention_loss_entry_point_validates_its_arguments_on_the_host():
    lib = _lib.load()
    fn, P = lib.gvx_guided_attention_loss, 256   # any non-null value: a refused call never dereferences
    need = lib.gvx_guided_attention_loss_scratch_bytes(32, 200, 128)
    assert 0 < need <= 1 << 16
    assert lib.gvx_guided_attention_loss_scratch_bytes(0, 200, 128) == 0 and b"must be >= 1" in lib.gvx_last_error()
    good = dict(align=P, tl=P, ml=P, B=2, T=3, L=4, sigma=0.4, alpha=1.0, out=P, dalign=P, scratch=P, nbytes=need)

    def call(**kw):
        a = {**good, **kw}
        return fn(a["align"], a["tl"], a["ml"], a["B"], a["T"], a["L"], a["sigma"], a["alpha"], a["out"], a["dalign"], a["scratch"], a["nbytes"], None)

    for k in ("align", "tl", "ml", "out"):
        assert call(**{k: None}) == -1 and b"null pointer" in lib.gvx_last_error(), k
    for k in ("B", "T", "L"):
        assert call(**{k: 0}) == -1 and b"must be >= 1" in lib.gvx_last_error(), k
    for bad in (0.0, -0.4, float("nan"), float("inf"), 1e-30):
        assert call(sigma=bad) == -1 and b"sigma" in lib.gvx_last_error(), bad
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(alpha=bad) == -1 and b"alpha" in lib.gvx_last_error(), bad
    assert call(scratch=None) == -5 and b"scratch" in lib.gvx_last_error()
    assert call(nbytes=need - 1) == -5 and b"scratch" in lib.gvx_last_error()
    assert call(scratch=P + 4) == -5 and b"8-byte aligned" in lib.gvx_last_error()


def test_decoder_bptt_ext_entry_point_validates_its_arguments_on_the_host():
    lib = _lib.load()
    fn = lib.gvx_train_decoder_bptt_ext
    assert fn(None, 256, 9, 9, 256, 1 << 30, None) == -1 and b"null argument block" in lib.gvx_last_error()
    B, L, T = 3, 9, 4
    a = bptt_args_for_plan(B, L, T, BPTT_EVEN)
    wsb = lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(a))
    assert wsb > 0
    for ts, bs, what in ((L - 1, T * L, "steps overlap"), (B * L, L - 1, "rows overlap"), (-B * L, L, "negative"), (L, -T * L, "negative")):
        assert fn(C.byref(a), 256, ts, bs, 256, wsb, None) == -1 and b"dw_ext strides" in lib.gvx_last_error(), what
    # good strides of both layouts (time-major, row slice of [B, T, L]): the next check is the workspace's
    for ts, bs in ((B * L, L), (L, T * L)):
        assert fn(C.byref(a), 256, ts, bs, None, wsb, None) == -5 and b"workspace" in lib.gvx_last_error()
        assert fn(C.byref(a), 256, ts, bs, 256, wsb - 1, None) == -5
        assert fn(C.byref(a), 256, ts, bs, 260, wsb, None) == -5 and b"aligned" in lib.gvx_last_error()
    # without a gradient the strides are not looked at; the block's own checks come first either way
    assert fn(C.byref(a), None, -1, -1, None, wsb, None) == -5
    a.B = 33
    assert fn(C.byref(a), 256, B * L, L, 256, wsb, None) == -2 and b"B <= 32" in lib.gvx_last_error()
    a.B, a.w_all = B, None
    assert fn(C.byref(a), 256, B * L, L, 256, wsb, None) == -1 and b"null pointer" in lib.gvx_last_error()
    # T = 1 / B = 1: the stride that separates nothing may be anything >= 0
    one = bptt_args_for_plan(1, L, 1, BPTT_EVEN)
    assert fn(C.byref(one), 256, 0, 0, None, 1 << 30, None) == -5


def test_criterion_surface():
    import genvox_amd
    from genvox_amd.tacotron2 import Tacotron2, Tacotron2GuidedLoss, Tacotron2Loss

    assert genvox_amd.Tacotron2GuidedLoss is Tacotron2GuidedLoss
    mc, ac, tc = train_step_configs("small")
    m = Tacotron2(mc, ac, tc)
    assert m.get_criterion() == {"loss": Tacotron2Loss} and m.get_criterion()["loss"] is Tacotron2Loss
    assert m.get_criterion(guided_attention_alpha=0.0, guided_attention_sigma=0.2)["loss"] is Tacotron2Loss
    crit = m.get_criterion(guided_attention_alpha=2.0)["loss"]
    assert isinstance(crit, Tacotron2GuidedLoss) and crit.alpha == 2.0 and crit.sigma == 0.4
    crit = m.get_criterion(guided_attention_alpha=0.5, guided_attention_sigma=0.2)["loss"]
    assert (crit.alpha, crit.sigma) == (0.5, 0.2)
    d = Tacotron2GuidedLoss()
    assert (d.alpha, d.sigma) == (1.0, 0.4) and Tacotron2GuidedLoss(alpha=0).alpha == 0
    for kw in (dict(alpha=-1.0), dict(alpha=float("nan")), dict(sigma=0.0), dict(sigma=-0.4), dict(sigma=float("inf"))):
        with pytest.raises(ValueError):
            Tacotron2GuidedLoss(**kw)
    with pytest.raises(ValueError):
        m.get_criterion(guided_attention_alpha=-0.5)
    # plain attributes: a schedule may change them, and a bad value is caught at the next call, before anything runs
    d.alpha, d.sigma = 0.25, 0.3
    assert (d.alpha, d.sigma) == (0.25, 0.3)
    d.sigma = 0.0
    with pytest.raises(ValueError):
        d({}, {})
    # nothing of this lands in the model's config (config.yaml stays readable by the reference)
    assert not any("guided" in k for k in vars(mc))
