"""The vocoder denoiser of include/genvox_amd.h ("Vocoder denoiser") restated with torch.stft and an explicit overlap-add, row by row
on the row cut at its own length, in float64 and as a float32 twin on the CPU.  Written from the definition in the header, never
from the kernels.  The gain max(0, M - a) / M is continuous in X, so no decision needs pinning to the device."""
import numpy as np
import torch

FACTOR = 8.0
ULP = 2.0 ** -23


def frames(n, hop):
    return 1 + n // hop


def window(n_fft, dtype=torch.float64):
    """The periodic Hann of n_fft points, computed in double."""
    k = torch.arange(n_fft, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * torch.pi * k / n_fft)).to(dtype)


def spectrum(x, n_fft, hop):
    """[F, bins] complex spectrum of the 1-D row x (already cut at its length)."""
    w = window(n_fft, x.dtype)
    return torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect", return_complex=True).transpose(0, 1)


def magnitude(X):
    return torch.sqrt(X.real * X.real + X.imag * X.imag)


def gain(X, bias, strength):
    """Y = X max(0, M - a) / M where M > 0, 0 where M == 0; a = strength * bias (no bias: X itself).  At a == 0 that is X."""
    if bias is None:
        return X
    M = magnitude(X)
    a = torch.tensor(float(np.float32(strength)), dtype=M.dtype) * bias.to(M.dtype)[None, :]   # the strength as the C ABI receives it
    live = M > 0
    g = torch.where(live, torch.clamp(M - a, min=0.0) / torch.where(live, M, torch.ones_like(M)), torch.zeros_like(M))
    return X * g


def overlap_add(Y, n, n_fft, hop):
    """The inverse half: z_t = irfft(Y_t) * w, then out[i] = sum_t z_t[p - t hop] / sum_t w^2[p - t hop] at p = i + n_fft / 2 over the
    frames that cover p, added in ascending frame order."""
    F = Y.shape[0]
    w = window(n_fft, Y.real.dtype)
    z = torch.fft.irfft(Y, n=n_fft, dim=1) * w[None, :]
    num = torch.zeros((F - 1) * hop + n_fft, dtype=z.dtype)
    den = torch.zeros_like(num)
    for t in range(F):
        num[t * hop:t * hop + n_fft] += z[t]
        den[t * hop:t * hop + n_fft] += w * w
    pad = n_fft // 2
    return num[pad:pad + n] / den[pad:pad + n]


def row(x, n_fft, hop, bias=None, strength=0.0):
    """(out [n], M [F, bins], Y) of one row cut at its length, in x's dtype."""
    X = spectrum(x, n_fft, hop)
    Y = gain(X, bias if strength > 0 else None, strength)
    return overlap_add(Y, x.shape[0], n_fft, hop), magnitude(X), Y


def run(wav, lengths, n_fft, hop, bias=None, strength=0.0, dtype=torch.float64):
    """The definition on a batch: dict(out [B, n_max], mag [B, 1 + n_max // hop, bins], clamped [b] -> bool [F, bins]), zeros behind a
    row's samples and frames."""
    B, n_max = wav.shape
    lengths = [n_max] * B if lengths is None else list(lengths)
    out = torch.zeros(B, n_max, dtype=dtype)
    mag = torch.zeros(B, frames(n_max, hop), n_fft // 2 + 1, dtype=dtype)
    clamped = []
    for b, n in enumerate(lengths):
        o, M, Y = row(wav[b, :n].to(dtype), n_fft, hop, bias, strength)
        out[b, :n], mag[b, :M.shape[0]] = o, M
        clamped.append((magnitude(Y) == 0) & (M > 0))
    return dict(out=out, mag=mag, clamped=clamped)


def tol(err, ref):
    """What the device may differ from float64 by: FACTOR x max(the float32 twin's error, one ulp of the tensor's scale)."""
    return FACTOR * max(err, ULP * float(ref.abs().max()))


def reference(wav, lengths, n_fft, hop, bias=None, strength=0.0):
    """float64 run + the float32 twin's largest error of out and of mag, per row: err = dict(out=[B floats], mag=[B floats])."""
    r64 = run(wav, lengths, n_fft, hop, bias, strength, torch.float64)
    r32 = run(wav, lengths, n_fft, hop, bias, strength, torch.float32)
    B = wav.shape[0]
    r64["err"] = {k: [float((r32[k][b].double() - r64[k][b]).abs().max()) for b in range(B)] for k in ("out", "mag")}
    return r64


def clamped_fraction(ref):
    """The share of the bins with M > 0 or not, over all rows' frames, that the gain sets to 0."""
    total = sum(c.numel() for c in ref["clamped"])
    return sum(int(c.sum()) for c in ref["clamped"]) / total


def ratios(dev_out, dev_mag, ref):
    """Largest |device - float64| per tensor as a fraction of its bound, rows taken one by one: (out ratio, mag ratio).  A row whose
    bound is 0 (a silent row) must match exactly and counts as 0."""
    worst = {"out": 0.0, "mag": 0.0}
    for k, dev in (("out", dev_out), ("mag", dev_mag)):
        if dev is None:
            continue
        for b in range(dev.shape[0]):
            diff = float((dev[b].double() - ref[k][b]).abs().max())
            bound = tol(ref["err"][k][b], ref[k][b])
            if bound == 0.0:
                assert diff == 0.0, f"{k} row {b}: a silent row must be exact zeros, off by {diff}"
                continue
            worst[k] = max(worst[k], diff / bound)
    return worst["out"], worst["mag"]


def noise(seed, B, n_max):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n_max, generator=g, dtype=torch.float64).float()


def tone_noise(seed, B, n_max, scale=1.0):
    """Per row 0.5 sin(2 pi f n + phi) + 1e-2 noise, another tone per row; float32, times ``scale`` (a power of two: exact)."""
    x = noise(seed, B, n_max).double() * 1e-2
    n = torch.arange(n_max, dtype=torch.float64)
    for b in range(B):
        x[b] += 0.5 * torch.sin(2.0 * torch.pi * 0.0631 * (1.0 + 0.37 * b) * n + 0.3)
    return x.float() * scale


def tone_case(n_fft, hop, lengths, n_max, scale=1.0, seeds=range(1, 9)):
    """(seed, wav, bias, reference at strength 1) of tone + 1e-2 noise: the bias is flat at the median float64 magnitude of the signal's
    own bins, so that about half of them are clamped; the first seed of 1..8 at which between 25 % and 75 % are."""
    for seed in seeds:
        wav = tone_noise(seed, len(lengths), n_max, scale)
        free = run(wav, lengths, n_fft, hop)
        level = torch.cat([free["mag"][b, :frames(n, hop)].flatten() for b, n in enumerate(lengths)]).median()
        bias = torch.full((n_fft // 2 + 1,), float(level), dtype=torch.float64).float()
        ref = reference(wav, lengths, n_fft, hop, bias, 1.0)
        if 0.25 <= clamped_fraction(ref) <= 0.75:
            return seed, wav, bias, ref
    raise AssertionError("no seed of 1..8 clamps between 25 % and 75 % of the bins")
