"""CPU: the restatement of the multi-resolution STFT loss (tests/stft_loss_ref64.py) checked by hand, and every refusal of the plan and
of the module that needs no device."""
import ctypes as C
import math
import os

import pytest
import torch

from genvox_amd import _lib, build
from genvox_amd.losses import DEFAULT_RESOLUTIONS, MultiResolutionSTFTLoss
from tests import stft_loss_ref64 as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_by_hand_on_three_frames():
    """n_fft 512, hop 128, win_length 300 on a row of 300 samples: F = 1 + 300 // 128 = 3 frames, both reflections inside every frame.
    Frames are built sample by sample from the definition's indices and window and transformed with an explicit DFT."""
    n_fft, hop, wl, n = 512, 128, 300, 300
    g = torch.Generator().manual_seed(3)
    xp, xt = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    F = R.frames(n, hop)
    assert F == 3
    # the definition's indices: the left edge mirrors around sample 0, the right edge around sample n - 1, neither repeats its pivot
    assert [R.source_index(p, n_fft, n) for p in (0, 255, 256, 257, 555, 556, 557, 811)] == [256, 1, 0, 1, 299, 298, 297, 43]
    win = [0.0] * n_fft
    for k in range(wl):
        win[(n_fft - wl) // 2 + k] = 0.5 - 0.5 * math.cos(2.0 * math.pi * k / wl)
    assert torch.equal(R.window(n_fft, wl), torch.tensor(win, dtype=torch.float64)) and win[105] == 0.0 and win[106] == 0.0 and win[107] > 0
    kk = torch.arange(n_fft // 2 + 1, dtype=torch.float64)[:, None] * torch.arange(n_fft, dtype=torch.float64)[None, :]
    dft = torch.complex(torch.cos(2 * math.pi * kk / n_fft), -torch.sin(2 * math.pi * kk / n_fft))
    mags = []
    for x in (xp, xt):
        fr = torch.tensor([[win[k] * float(x[R.source_index(t * hop + k, n_fft, n)]) for k in range(n_fft)] for t in range(F)], dtype=torch.float64)
        X = fr.to(torch.complex128) @ dft.T
        got = R.spectrum(x, (n_fft, hop, wl))
        assert got.shape == (F, n_fft // 2 + 1) and float((got - X).abs().max()) < 1e-10
        mags.append(torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=R.EPS)))
    Mp, Mt = mags
    sc = float(((Mt - Mp) ** 2).sum().sqrt() / (Mt ** 2).sum().sqrt())
    mag = float((Mt.log() - Mp.log()).abs().sum() / (F * (n_fft // 2 + 1)))
    out = R.run(xp[None], xt[None], None, ((n_fft, hop, wl),))
    assert abs(float(out["parts"][0, 0, 0]) - sc) < 1e-12 and abs(float(out["parts"][0, 0, 1]) - mag) < 1e-12
    assert abs(float(out["loss"]) - (sc + mag)) < 1e-12
    # the pinned form with the restatement's own signs is the free form, value and gradient
    signs = [[torch.sign(Mt.log() - Mp.log())]]
    pinned = R.run(xp[None], xt[None], None, ((n_fft, hop, wl),), signs=signs)
    assert abs(float(pinned["loss"] - out["loss"])) < 1e-14 and float((pinned["d_pred"] - out["d_pred"]).abs().max()) < 1e-14


def test_per_row_form_is_the_batch_form_on_one_row():
    """On B = 1 the per-row norms and means are Parallel WaveGAN's batch-wide ones: torch.stft of the [1, n] batch, Frobenius norms and
    an L1 mean over the whole batch."""
    g = torch.Generator().manual_seed(4)
    n = 1500
    xp, xt = torch.randn(1, n, generator=g, dtype=torch.float64), torch.randn(1, n, generator=g, dtype=torch.float64)
    total = 0.0
    for n_fft, hop, wl in DEFAULT_RESOLUTIONS:
        w = torch.hann_window(wl, periodic=True, dtype=torch.float64)
        m = []
        for x in (xp, xt):
            X = torch.stft(x, n_fft, hop, wl, w, center=True, pad_mode="reflect", return_complex=True)
            m.append(torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=1e-7)).transpose(2, 1))
        total += float(torch.norm(m[1] - m[0], p="fro") / torch.norm(m[1], p="fro")) + float(torch.nn.functional.l1_loss(m[0].log(), m[1].log()))
    out = R.run(xp, xt, None, DEFAULT_RESOLUTIONS)
    assert abs(float(out["loss"]) - total / 3) < 1e-12
    # and a ragged row is the row cut at its length: the batch of two equals the two rows run alone
    two_p, two_t = torch.randn(2, n, generator=g, dtype=torch.float64), torch.randn(2, n, generator=g, dtype=torch.float64)
    both = R.run(two_p, two_t, [1100, n], DEFAULT_RESOLUTIONS)
    a, b = R.run(two_p[:1, :1100], two_t[:1, :1100], None, DEFAULT_RESOLUTIONS), R.run(two_p[1:], two_t[1:], None, DEFAULT_RESOLUTIONS)
    assert torch.equal(both["parts"][0], a["parts"][0]) and torch.equal(both["parts"][1], b["parts"][0])
    assert bool((both["d_pred"][0, 1100:] == 0).all()) and float((both["d_pred"][0, :1100] * 2 - a["d_pred"][0]).abs().max()) < 1e-12


def test_c_abi_is_declared_built_and_refuses_bad_plans_on_the_host():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    assert "Multi-resolution STFT loss" in header and "PER ROW" in header
    for name in ("gvx_stft_loss_create", "gvx_stft_loss_destroy", "gvx_stft_loss_workspace_bytes", "gvx_stft_loss"):
        assert name in _lib.SIGNATURES
    assert "stft_loss.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "stft_loss.hip"))
    assert os.path.exists(os.path.join(build.CSRC, "fft_lds.h"))
    lib = _lib.load()
    h = C.c_void_p()

    def create(res, w_sc=1.0, w_mag=1.0, eps=1e-7, R_=None):
        table = (_lib.gvx_stft_resolution * max(1, len(res)))(*[_lib.gvx_stft_resolution(*r) for r in res])
        return lib.gvx_stft_loss_create(table, len(res) if R_ is None else R_, w_sc, w_mag, eps, C.byref(h))

    for n_fft in (256, 4096, 1000, 0, -512):
        assert create([(n_fft, 64, 128)]) == -2 and b"n_fft" in lib.gvx_last_error(), n_fft
    for bad in ((512, 0, 512), (512, 513, 512), (512, 128, 1), (512, 128, 513), (2048, -1, 1200)):
        assert create([bad]) == -1, bad
    assert create([(512, 128, 512)] * 9) == -1 and create([(512, 128, 512)], R_=0) == -1
    assert create([(512, 128, 512)], w_sc=-1.0) == -1 and create([(512, 128, 512)], w_mag=float("nan")) == -1
    assert create([(512, 128, 512)], eps=0.0) == -1 and create([(512, 128, 512)], eps=float("inf")) == -1
    assert lib.gvx_stft_loss_create(None, 1, 1.0, 1.0, 1e-7, C.byref(h)) == -1
    assert not h.value
    assert lib.gvx_stft_loss_workspace_bytes(None, 2, 4096) == 0
    assert lib.gvx_stft_loss(None, None, None, None, 1, 4096, None, None, None, None, None, 0, None) == -1
    lib.gvx_stft_loss_destroy(None)


def test_module_refusals_need_no_device():
    assert MultiResolutionSTFTLoss().resolutions == ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240)) == R.DEFAULT_RESOLUTIONS
    assert list(MultiResolutionSTFTLoss().parameters()) == []
    for bad in ([], [(512, 128, 512)] * 9, [(256, 64, 256)], [(512, 0, 512)], [(512, 600, 512)], [(512, 128, 1)], [(512, 128, 600)], [(512, 128)]):
        with pytest.raises(ValueError):
            MultiResolutionSTFTLoss(bad)
    for kw in (dict(w_sc=-1.0), dict(w_mag=float("inf")), dict(eps=0.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            MultiResolutionSTFTLoss(**kw)
    crit = MultiResolutionSTFTLoss()
    x = torch.zeros(2, 2000)
    for pred, target, lens in ((x.double(), x, None), (x, x.double(), None), (x[0], x[0], None), (x, x[:, :1999], None), (x[:, :1024], x[:, :1024], None),
                               (x, x, [2000]), (x, x, [2000, 1024]), (x, x, [2001, 2000]), (x, x, torch.tensor([1500, 1000]))):
        with pytest.raises(ValueError):
            crit(pred, target, lens)
    with pytest.raises(ValueError, match="row 1 has 1024 samples"):
        crit(x, x, [2000, 1024])
    with pytest.raises(RuntimeError, match="MI355X only"):   # well-formed arguments on the CPU: there is no CPU path
        crit(x, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        crit(x, x, [2000, 1025])
    from genvox_amd import metrics
    with pytest.raises(RuntimeError, match="MI355X only"):
        metrics.stft_distance(x, x)
    import genvox_amd
    assert genvox_amd.MultiResolutionSTFTLoss is MultiResolutionSTFTLoss and genvox_amd.stft_distance is metrics.stft_distance
