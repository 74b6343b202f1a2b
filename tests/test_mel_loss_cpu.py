"""CPU: the C ABI of the mel-spectrogram L1 loss as far as it needs no device - declared, bound, built, every create-time refusal, the
workspace arithmetic, the band extraction against a dense product - the restatement (tests/mel_loss_ref64.py) against the published
formula, and the module's refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from genvox_amd import _lib, build
from tests import mel_loss_ref64 as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gvx_mel_loss_create", "gvx_mel_loss_destroy", "gvx_mel_loss_bands", "gvx_mel_loss_workspace_bytes", "gvx_mel_loss")


def test_c_abi_is_declared_bound_and_built():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    assert "Mel-spectrogram L1 loss" in header and "PER ROW" in header
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "mel_loss.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mel_loss.hip"))
    from tests.mel_loss_helpers import G, MAX_MELS, S
    assert G >= 1 and S >= 64 and MAX_MELS == 128


def test_create_refuses_bad_plans_on_the_host():
    lib = _lib.load()
    h = C.c_void_p()
    basis = np.ones((129, 1025), dtype=np.float32)

    def create(n_fft=1024, hop=256, win_length=1024, n_mels=80, clamp=1e-5, mag_eps=1e-9, b=basis):
        return lib.gvx_mel_loss_create(n_fft, hop, win_length, n_mels, None if b is None else b.ctypes.data, clamp, mag_eps, C.byref(h))

    for n_fft in (768, 256, 4096, 0, -512):
        assert create(n_fft=n_fft, hop=64, win_length=128) == -2 and b"n_fft" in lib.gvx_last_error(), n_fft
    assert create(hop=255) == -1 and b"odd" in lib.gvx_last_error()          # n_fft - hop odd
    assert create(n_fft=512, hop=127, win_length=512) == -1
    for kw in (dict(hop=0), dict(hop=1026), dict(hop=-2), dict(win_length=1), dict(win_length=1025), dict(n_mels=0), dict(n_mels=129), dict(n_mels=-1),
               dict(clamp=0.0), dict(clamp=float("inf")), dict(clamp=float("nan")), dict(mag_eps=0.0), dict(mag_eps=-1e-9), dict(mag_eps=float("nan")),
               dict(b=None)):
        assert create(**kw) == -1, kw
    bad = basis.copy()
    bad.reshape(-1)[3 * 513 + 7] = np.nan   # the call reads [80][513]
    assert create(b=bad) == -1 and b"mel_basis[3][7]" in lib.gvx_last_error()
    assert lib.gvx_mel_loss_create(1024, 256, 1024, 80, basis.ctypes.data, 1e-5, 1e-9, None) == -1
    assert not h.value
    lib.gvx_mel_loss_destroy(None)
    assert lib.gvx_mel_loss(None, None, None, None, 1, 4096, None, None, None, None, None, 0, None) == -1
    assert lib.gvx_mel_loss_workspace_bytes(None, 2, 4096) == 0


def test_workspace_bytes_arithmetic():
    """The header's layout, restated below, for every n_fft; 0 for a NULL plan and for B or n_max out of range.  A plan is host work
    until its first call, so this needs no device."""
    from tests.mel_loss_helpers import G, create
    lib = _lib.load()
    for n_fft, hop, n_mels in ((1024, 256, 80), (512, 512, 5), (2048, 512, 128), (1024, 120, 80)):
        rc, h = create(R.Config(n_fft, hop, n_fft, torch.ones(n_mels, n_fft // 2 + 1)))
        assert rc == 0 and h
        for B, n_max in ((3, 1300), (1, hop - 1), (1, hop), (16, 8192), (2, G * hop), (2, G * hop + hop), (65535, 1)):
            got = lib.gvx_mel_loss_workspace_bytes(h, B, n_max)
            assert got == workspace_bytes(n_fft, hop, B, n_max, G) and got % 256 == 0 and got > 0, (n_fft, hop, B, n_max)
        for B, n_max in ((0, 4096), (-1, 4096), (65536, 4096), (2, 0), (2, -5), (2, (1 << 30) + 1)):
            assert lib.gvx_mel_loss_workspace_bytes(h, B, n_max) == 0, (B, n_max)
        lib.gvx_mel_loss_destroy(h)
    assert workspace_bytes(1024, 256, 3, 1300, G) == 256 * ((3 * 5 * 1024 * 4 + 255) // 256) + 256 + 256


def workspace_bytes(n_fft, hop, B, n_max, G):
    """The header's layout: frame gradients [B][n_max / hop][n_fft] fp32, partial sums [B][workgroups] and row sums [B] in float64, each
    rounded up to 256 bytes."""
    r = lambda n: (n + 255) // 256 * 256
    f_max = n_max // hop
    return r(B * f_max * n_fft * 4) + r(B * ((f_max + G - 1) // G) * 8) + r(B * 8)


def _bands(basis):
    lib = _lib.load()
    n_mels, bins = basis.shape
    arrays = [np.full(n, 99, dtype=np.int32) for n in (n_mels, n_mels, bins, bins)]
    assert lib.gvx_mel_loss_bands(basis.ctypes.data, n_mels, bins, *[a.ctypes.data for a in arrays]) == 0
    return arrays


def test_bands_against_a_dense_product():
    """A matrix with a zero row, a zero column inside other rows' bands, a row with two separated runs, single entries at bin 0 and at
    the last bin: the banded products, forward and transposed, equal the dense ones exactly, and the bands are tight."""
    g = torch.Generator().manual_seed(2)
    bins = 257
    basis = np.zeros((6, bins), dtype=np.float32)
    basis[0, 10:40] = torch.rand(30, generator=g).numpy() + 0.1
    basis[1, 30:90] = torch.rand(60, generator=g).numpy() + 0.1
    basis[2, 5:9] = 1.0
    basis[2, 200:203] = 2.0            # two separated runs: the band is 5 .. 202
    # row 3 stays zero
    basis[4, 0] = 1.5
    basis[5, bins - 1] = 0.5
    basis[:, 35] = 0.0                 # a zero column inside the bands of rows 0 and 1
    mel_lo, mel_hi, bin_lo, bin_hi = _bands(basis)
    assert list(mel_lo) == [10, 30, 5, 0, 0, 256] and list(mel_hi) == [39, 89, 202, -1, 0, 256]
    assert (bin_lo[35], bin_hi[35]) == (0, -1) and (bin_lo[0], bin_hi[0]) == (4, 4) and (bin_lo[32], bin_hi[32]) == (0, 1)
    assert (bin_lo[6], bin_hi[6]) == (2, 2) and (bin_lo[100], bin_hi[100]) == (0, -1)   # inside row 2's band, but the column is zero
    s = torch.rand(bins, generator=g, dtype=torch.float64).numpy()
    dm = torch.rand(6, generator=g, dtype=torch.float64).numpy()
    dense, dense_t = basis.astype(np.float64) @ s, basis.astype(np.float64).T @ dm
    for j in range(6):
        band = sum(float(basis[j, k]) * s[k] for k in range(mel_lo[j], mel_hi[j] + 1))
        assert abs(band - dense[j]) <= 1e-12 * max(1.0, abs(dense[j]))
        outside = np.r_[basis[j, :mel_lo[j]], basis[j, mel_hi[j] + 1:]] if mel_hi[j] >= 0 else basis[j]
        assert not outside.any() and (mel_hi[j] < 0 or (basis[j, mel_lo[j]] != 0 and basis[j, mel_hi[j]] != 0))
    for k in range(bins):
        band = sum(float(basis[j, k]) * dm[j] for j in range(bin_lo[k], bin_hi[k] + 1))
        assert abs(band - dense_t[k]) <= 1e-12 * max(1.0, abs(dense_t[k]))
        assert bin_hi[k] < 0 or (basis[bin_lo[k], k] != 0 and basis[bin_hi[k], k] != 0)
    # the published basis: every mel has a band, the work is about 1.1 k products per frame against 41 k dense
    pub = R.slaney(22050, 1024, 80).numpy()
    lo, hi, _, _ = _bands(pub)
    assert (hi >= lo).all() and 500 < int((hi - lo + 1).sum()) < 2000
    assert _lib.load().gvx_mel_loss_bands(None, 6, bins, None, None, None, None) == -1


def _published_mel(y, cfg):
    """HiFi-GAN's mel_spectrogram (meldataset.py) on a [1, n] batch, in the dtype of y."""
    pad = (cfg.n_fft - cfg.hop) // 2
    y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, cfg.n_fft, hop_length=cfg.hop, win_length=cfg.win_length, window=torch.hann_window(cfg.win_length, dtype=y.dtype),
                      center=False, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    return torch.log(torch.clamp(torch.matmul(cfg.basis.to(y.dtype), spec), min=1e-5))


@pytest.mark.parametrize("shape", [(1024, 256, 1024, 80, 1279), (1024, 120, 600, 80, 1201), (512, 512, 301, 5, 1535), (512, 128, 512, 40, 193)])
def test_restatement_is_the_published_formula(shape):
    n_fft, hop, wl, n_mels, n = shape
    cfg = R.Config(n_fft, hop, wl, R.slaney(22050, n_fft, n_mels))
    g = torch.Generator().manual_seed(9)
    xp, xt = 0.3 * torch.randn(1, n, generator=g, dtype=torch.float64), 0.3 * torch.randn(1, n, generator=g, dtype=torch.float64)
    out = R.run(xp, xt, None, cfg)
    F = n // hop
    assert R.frames(n, hop) == F and out["lp"][0].shape == (F, n_mels)
    pub_p, pub_t = _published_mel(xp, cfg)[0].transpose(0, 1), _published_mel(xt, cfg)[0].transpose(0, 1)
    assert pub_p.shape == (F, n_mels)
    assert float((pub_p - out["lp"][0]).abs().max()) < 1e-9 and float((pub_t - out["lt"][0]).abs().max()) < 1e-9
    assert abs(float(torch.nn.functional.l1_loss(pub_p, pub_t)) - float(out["loss"])) < 1e-12
    # the frames by hand: padded position p of frame t is t hop + k, its source through the reflection
    pad = R.pad_of(cfg)
    row = xp[0]
    fr = torch.stack([torch.stack([row[R.source_index(t * hop + k, pad, n)] for k in range(n_fft)]) for t in range(F)])
    assert torch.equal(fr, R.padded(row, cfg).unfold(0, n_fft, hop)[:F])
    assert R.source_index(0, pad, n) == pad and R.source_index(pad, pad, n) == 0
    if pad:   # neither reflection repeats its pivot
        assert R.source_index(pad - 1, pad, n) == 1 and R.source_index(pad + n, pad, n) == n - 2


def test_ragged_rows_of_the_restatement_are_the_rows_run_alone():
    cfg = R.Config(512, 128, 512, R.slaney(22050, 512, 20))
    pred, target = R.noise(1, 2, 900)
    both = R.run(pred, target, [700, 900], cfg)
    a, b = R.run(pred[:1, :700], target[:1, :700], None, cfg), R.run(pred[1:], target[1:], None, cfg)
    assert torch.equal(both["parts"][0], a["parts"][0]) and torch.equal(both["parts"][1], b["parts"][0])
    assert bool((both["d_pred"][0, 700:] == 0).all()) and float((both["d_pred"][0, :700] * 2 - a["d_pred"][0]).abs().max()) < 1e-15
    same = R.run(target, target, [700, 900], cfg)
    assert float(same["loss"]) == 0.0 and bool((same["d_pred"] == 0).all())
    silent = R.run(torch.zeros_like(pred), target, [700, 900], cfg)
    assert bool(torch.isfinite(silent["loss"])) and bool((silent["d_pred"] == 0).all()) and all(bool((m < cfg.clamp).all()) for m in silent["mp"])


def test_module_refusals_need_no_device():
    import genvox_amd
    from genvox_amd import metrics
    from genvox_amd.losses import MelSpectrogramLoss
    crit = MelSpectrogramLoss()
    assert (crit.n_fft, crit.hop_length, crit.win_length, crit.n_mels, crit.clamp, crit.mag_eps) == (1024, 256, 1024, 80, 1e-5, 1e-9)
    assert crit.mel_basis.shape == (80, 513) and np.array_equal(crit.mel_basis, R.slaney(22050, 1024, 80).numpy())
    assert crit.min_samples == 385 and list(crit.parameters()) == []
    assert MelSpectrogramLoss(n_fft=512, hop_length=512, win_length=301, n_mels=5).min_samples == 512
    for kw in (dict(n_fft=768), dict(hop_length=255), dict(hop_length=0), dict(win_length=1), dict(win_length=2048), dict(n_mels=129), dict(n_mels=0),
               dict(clamp=0.0), dict(mag_eps=float("nan")), dict(fmax=20000.0), dict(fmin=-1.0), dict(mel_basis=np.ones((80, 512), dtype=np.float32)),
               dict(mel_basis=np.full((80, 513), np.inf, dtype=np.float32))):
        with pytest.raises(ValueError):
            MelSpectrogramLoss(**kw)
    x = torch.zeros(2, 2000)
    for pred, target, lens in ((x.double(), x, None), (x, x.double(), None), (x[0], x[0], None), (x, x[:, :1999], None), (x[:, :384], x[:, :384], None),
                               (x, x, [2000]), (x, x, [2000, 384]), (x, x, [2001, 2000])):
        with pytest.raises(ValueError):
            crit(pred, target, lens)
    with pytest.raises(ValueError, match="row 1 has 384 samples"):
        crit(x, x, [2000, 384])
    with pytest.raises(RuntimeError, match="MI355X only"):   # well-formed arguments on the CPU: there is no CPU path
        crit(x, x, [2000, 385])
    with pytest.raises(RuntimeError, match="MI355X only"):
        metrics.mel_distance(x, x)
    assert genvox_amd.MelSpectrogramLoss is MelSpectrogramLoss and genvox_amd.mel_distance is metrics.mel_distance
