"""CPU: the C ABI of the vocoder denoiser as far as it needs no device - declared, bound, built, every create-time and call-time
refusal, the workspace arithmetic - the restatement (tests/denoise_ref64.py) held to things worked by hand, and the refusals of
Denoiser and of Synthesizer's ``denoise``."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from genvox_amd import _lib, build
from tests import denoise_ref64 as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gvx_denoise_create", "gvx_denoise_destroy", "gvx_denoise_workspace_bytes", "gvx_denoise")
OK, INVALID, UNSUPPORTED, SHAPE, WORKSPACE = 0, -1, -2, -4, -5


def test_c_abi_is_declared_bound_and_built():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    assert "Vocoder denoiser" in header and "zero only" in header
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "denoise.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "denoise.hip"))
    from tests.denoise_helpers import G, S
    assert f"GVX_DENOISE_FRAMES_PER_WORKGROUP = {G}" in header and f"GVX_DENOISE_GATHER_SAMPLES = {S}" in header


def test_create_refuses_bad_plans_on_the_host():
    from tests.denoise_helpers import create
    lib = _lib.load()
    for n_fft in (768, 256, 4096, 0, -512, 8):
        rc, h = create(n_fft, 1)
        assert rc == UNSUPPORTED and not h and b"n_fft" in lib.gvx_last_error(), n_fft
    for n_fft in (512, 1024, 2048):
        for hop in (0, -1, n_fft // 2 + 1, n_fft):
            rc, h = create(n_fft, hop)
            assert rc == INVALID and not h and b"hop" in lib.gvx_last_error(), (n_fft, hop)
        for hop in (1, 120, n_fft // 4, n_fft // 2):
            rc, h = create(n_fft, hop)
            assert rc == OK and h, (n_fft, hop)
            lib.gvx_denoise_destroy(h)
    assert lib.gvx_denoise_create(1024, 256, None) == INVALID
    lib.gvx_denoise_destroy(None)


def test_call_refusals_come_before_any_launch():
    """Every refusal that needs no device, with pointers that are never followed: a call that launched anything would fault here."""
    from tests.denoise_helpers import create
    lib = _lib.load()
    rc, h = create(1024, 256)
    assert rc == OK
    need = lib.gvx_denoise_workspace_bytes(h, 2, 4096)
    fake, ws = 1 << 20, 1 << 21   # non-null, 256-byte aligned, never dereferenced

    def call(plan=h, wav=fake, lens=None, B=2, n_max=4096, bias=fake, strength=0.5, out=fake, mag=fake, w=ws, wb=need):
        return lib.gvx_denoise(plan, wav, lens, B, n_max, bias, strength, out, mag, w, wb, None)

    assert call(plan=None) == INVALID
    assert call(wav=None) == INVALID
    assert call(out=None, mag=None) == INVALID and b"both null" in lib.gvx_last_error()
    for B in (0, -1, 65536):
        assert call(B=B) == INVALID, B
    for n_max in (0, -4, (1 << 30) + 1):
        assert call(n_max=n_max) == INVALID, n_max
    for s in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert call(strength=s) == INVALID and b"strength" in lib.gvx_last_error(), s
    assert call(bias=None) == INVALID and b"bias" in lib.gvx_last_error()
    for n_max in (1, 511, 512):
        assert call(n_max=n_max, wb=lib.gvx_denoise_workspace_bytes(h, 2, n_max)) == SHAPE and b"513" in lib.gvx_last_error(), n_max
    assert call(w=None) == WORKSPACE and call(w=ws + 128) == WORKSPACE and call(w=ws + 4) == WORKSPACE
    assert call(wb=need - 1) == WORKSPACE and call(wb=0) == WORKSPACE and b"too small" in lib.gvx_last_error()
    lib.gvx_denoise_destroy(h)


def workspace_bytes(n_fft, hop, B, n_max):
    """The header's layout: the windowed inverse frames [B][1 + n_max / hop][n_fft] fp32, rounded up to 256 bytes."""
    return (B * (1 + n_max // hop) * n_fft * 4 + 255) // 256 * 256


def test_workspace_bytes_arithmetic():
    from tests.denoise_helpers import G, create
    lib = _lib.load()
    for n_fft, hop in ((1024, 256), (512, 256), (2048, 512), (1024, 120), (512, 1)):
        rc, h = create(n_fft, hop)
        assert rc == OK and h
        for B, n_max in ((3, 1300), (1, 1), (1, hop), (16, 8192), (2, G * hop), (2, G * hop - 1), (65535, 1), (8, 32768)):
            got = lib.gvx_denoise_workspace_bytes(h, B, n_max)
            assert got == workspace_bytes(n_fft, hop, B, n_max) and got % 256 == 0 and got > 0, (n_fft, hop, B, n_max)
        for B, n_max in ((0, 4096), (-1, 4096), (65536, 4096), (2, 0), (2, -5), (2, (1 << 30) + 1)):
            assert lib.gvx_denoise_workspace_bytes(h, B, n_max) == 0, (B, n_max)
        lib.gvx_denoise_destroy(h)
    assert lib.gvx_denoise_workspace_bytes(None, 2, 4096) == 0
    # the number DESIGN.md gives: 32 rows of 800 frames at 1024 / 256 are 100 MiB
    assert workspace_bytes(1024, 256, 32, 799 * 256) == 32 * 800 * 1024 * 4 == 100 * (1 << 20)


def _dft_denoise(x, n_fft, hop, bias=None, strength=0.0):
    """The definition with an explicit DFT matrix and loops, for tiny sizes: float64 [n] -> out [n]."""
    n, pad = len(x), n_fft // 2
    F = 1 + n // hop
    w = [0.5 - 0.5 * math.cos(2.0 * math.pi * j / n_fft) for j in range(n_fft)]

    def src(p):
        i = p - pad
        i = -i if i < 0 else i
        return 2 * (n - 1) - i if i >= n else i

    num, den = [0.0] * (n + n_fft + hop), [0.0] * (n + n_fft + hop)
    for t in range(F):
        fr = [w[j] * float(x[src(t * hop + j)]) for j in range(n_fft)]
        X = [sum(fr[j] * complex(math.cos(2 * math.pi * k * j / n_fft), -math.sin(2 * math.pi * k * j / n_fft)) for j in range(n_fft))
             for k in range(n_fft // 2 + 1)]
        Y = []
        for k, v in enumerate(X):
            M, a = abs(v), 0.0 if bias is None else strength * float(bias[k])
            Y.append(v if a == 0.0 else (v * max(0.0, M - a) / M if M > 0 else 0.0))
        full = Y + [Y[n_fft - k].conjugate() for k in range(n_fft // 2 + 1, n_fft)]   # the Hermitian half
        full[0], full[n_fft // 2] = complex(full[0].real, 0.0), complex(full[n_fft // 2].real, 0.0)
        for j in range(n_fft):
            z = sum(full[k] * complex(math.cos(2 * math.pi * k * j / n_fft), math.sin(2 * math.pi * k * j / n_fft)) for k in range(n_fft)).real / n_fft
            num[t * hop + j] += w[j] * z
            den[t * hop + j] += w[j] * w[j]
    return torch.tensor([num[i + pad] / den[i + pad] for i in range(n)], dtype=torch.float64)


def test_restatement_at_strength_zero_returns_its_input():
    g = torch.Generator().manual_seed(4)
    for n_fft, hop, n in ((512, 128, 700), (512, 256, 768), (1024, 256, 1500), (1024, 120, 1201), (2048, 512, 2049), (2048, 1024, 3072), (8, 2, 21), (8, 3, 5)):
        x = torch.randn(1, n, generator=g, dtype=torch.float64)
        out = R.run(x, None, n_fft, hop)
        assert float((out["out"] - x).abs().max()) < 1e-12, (n_fft, hop, n)
        assert out["mag"].shape == (1, 1 + n // hop, n_fft // 2 + 1) and R.clamped_fraction(out) == 0.0
    for n_fft, hop, n in ((8, 2, 21), (8, 4, 12), (8, 3, 5)):
        x = torch.randn(n, generator=g, dtype=torch.float64)
        assert float((_dft_denoise(x, n_fft, hop) - x).abs().max()) < 1e-12
        bias = torch.rand(n_fft // 2 + 1, generator=g, dtype=torch.float64).float()
        for strength in (0.0, 0.5, 2.0):
            got = R.run(x[None], None, n_fft, hop, bias, strength)["out"][0]
            assert float((got - _dft_denoise(x, n_fft, hop, bias, float(np.float32(strength)))).abs().max()) < 1e-12, (n_fft, hop, strength)


def test_restatement_with_a_bias_above_every_magnitude_is_exact_zeros():
    x = R.noise(3, 2, 1500)
    for n_fft, hop in ((512, 128), (1024, 120), (1024, 512)):
        free = R.run(x, [1500, 1201], n_fft, hop)
        bias = torch.full((n_fft // 2 + 1,), 2.0 * float(free["mag"].max()))
        for dtype in (torch.float64, torch.float32):
            got = R.run(x, [1500, 1201], n_fft, hop, bias, 1.0, dtype)
            assert bool((got["out"] == 0).all()) and torch.equal(got["mag"], R.run(x, [1500, 1201], n_fft, hop, dtype=dtype)["mag"])
    assert R.clamped_fraction(R.run(x, [1500, 1201], 1024, 512, bias, 1.0)) == 1.0


def test_restatement_keeps_a_tone_on_a_bin_and_loses_the_noise():
    """A pure tone on bin 32 of 512 points, the bias zero on the bins the Hann window spreads it to (31 .. 33) and large elsewhere: the
    tone comes back, the noise added to it goes but for its share in those three bins."""
    n_fft, hop, n = 512, 128, 4096
    t = torch.arange(n, dtype=torch.float64)
    tone = 0.5 * torch.cos(2.0 * torch.pi * 32 * t / n_fft)
    noise = 1e-2 * R.noise(6, 1, n)[0].double()
    bias = torch.full((n_fft // 2 + 1,), 1e3)
    bias[31:34] = 0.0
    got = R.run((tone + noise)[None], None, n_fft, hop, bias, 1.0)["out"][0]
    inner = slice(n_fft, n - n_fft)   # away from the reflections, where the tone stays a tone
    left = (got - tone)[inner]
    assert float(left.abs().max()) < 0.15 * float(noise.abs().max())
    assert float(left.pow(2).mean().sqrt()) < 0.15 * float(noise[inner].pow(2).mean().sqrt())   # 3 of 257 bins of white noise: about 0.11
    assert float((got[inner] - tone[inner]).abs().max()) < 1e-2 * 0.5


def test_ragged_rows_of_the_restatement_are_the_rows_run_alone():
    x = R.noise(1, 2, 900)
    bias = torch.full((257,), 5.0)
    both = R.reference(x, [700, 900], 512, 128, bias, 1.0)
    a, b = R.run(x[:1, :700], None, 512, 128, bias, 1.0), R.run(x[1:], None, 512, 128, bias, 1.0)
    assert torch.equal(both["out"][0, :700], a["out"][0]) and torch.equal(both["out"][1], b["out"][0])
    assert bool((both["out"][0, 700:] == 0).all()) and bool((both["mag"][0, R.frames(700, 128):] == 0).all())
    assert R.tol(0.0, torch.tensor([4.0])) == 8.0 * 2.0 ** -23 * 4.0 and R.tol(1.0, torch.tensor([4.0])) == 8.0 and R.FACTOR == 8
    assert 0.0 < R.clamped_fraction(both) < 1.0 and len(both["err"]["out"]) == 2


def test_module_refusals_need_no_device():
    import genvox_amd
    from genvox_amd.denoiser import Denoiser
    dn = Denoiser(torch.ones(513))
    assert (dn.n_fft, dn.hop_length, dn.strength, dn.min_samples) == (1024, 256, 0.01, 513)
    assert list(dn.parameters()) == [] and set(dn.state_dict()) == {"bias"} and dn.state_dict()["bias"].dtype == torch.float32
    assert Denoiser(np.ones(257), n_fft=512, hop_length=256).min_samples == 257
    for kw in (dict(n_fft=768), dict(n_fft=256), dict(hop_length=0), dict(hop_length=513), dict(strength=-0.1), dict(strength=float("nan")),
               dict(strength=True), dict(strength="0.1"), dict(bias=torch.ones(512)), dict(bias=torch.ones(1, 513)), dict(bias=-torch.ones(513)),
               dict(bias=torch.full((513,), float("inf")))):
        with pytest.raises(ValueError):
            Denoiser(**{"bias": torch.ones(513), **kw})
    x = torch.zeros(2, 2000)
    for wav, lens, kw in ((x.double(), None, {}), (x[0], None, {}), (x[:, :512], None, {}), (x, [2000], {}), (x, [2000, 512], {}), (x, [2001, 2000], {}),
                          (x, None, dict(strength=-1.0)), (x, None, dict(strength=False)), (x, None, dict(strength=float("inf")))):
        with pytest.raises(ValueError):
            dn(wav, lens, **kw)
    with pytest.raises(ValueError, match="row 1 has 512 samples"):
        dn(x, [2000, 512])
    with pytest.raises(ValueError):
        dn.magnitudes(x[:, :512])
    with pytest.raises(RuntimeError, match="MI355X only"):   # well-formed arguments on the CPU: there is no CPU path
        dn(x, [2000, 513])
    with pytest.raises(RuntimeError, match="MI355X only"):
        dn.magnitudes(x)
    with pytest.raises(ValueError, match="reduce"):
        Denoiser.from_vocoder(None, reduce="median")
    with pytest.raises(ValueError, match="frames"):
        Denoiser.from_vocoder(None, frames=0)
    assert genvox_amd.Denoiser is Denoiser
    import copy
    twin = copy.deepcopy(dn)   # a copy makes its own plan
    assert twin._handle is None and torch.equal(twin.bias, dn.bias)
    other = Denoiser(torch.zeros(513))
    other.load_state_dict(dn.state_dict())
    assert torch.equal(other.bias, dn.bias)


def test_synthesizer_validates_denoise_without_a_device():
    import inspect

    from genvox_amd.synthesizer import Synthesizer, _check_denoise
    assert _check_denoise(0.0, False) == 0.0 and _check_denoise(0, True) == 0.0 and _check_denoise(0.25, True) == 0.25
    assert _check_denoise(np.float32(0.5), True) == 0.5
    for bad in (-0.1, float("nan"), float("inf"), True, False, "0.1", None, [0.1]):
        for has in (True, False):
            with pytest.raises(ValueError, match="denoise must be"):
                _check_denoise(bad, has)
    with pytest.raises(ValueError, match="Griffin-Lim has no bias"):
        _check_denoise(0.01, False)
    for fn in (Synthesizer.tts, Synthesizer.tts_batch):
        assert inspect.signature(fn).parameters["denoise"].default == 0.0
