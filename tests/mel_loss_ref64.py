"""The mel-spectrogram L1 loss of include/genvox_amd.h ("Mel-spectrogram L1 loss") restated with torch on the CPU, row by row on the
row cut at its own length: an explicit reflect pad through the definition's source indices, torch.stft(center=False), the basis
product, the clamp, the logarithm, per-row means, and d_pred by autograd - in float64 and as a float32 twin of the same code, whose
distance from float64 is the error e per tensor.  Written from the definition in the header, never from the kernels."""
import collections

import torch

FACTOR = 8.0
ULP = 2.0 ** -23
CLAMP = 1e-5
MAG_EPS = 1e-9
MARGIN = 1e-4   # of |l_t - l_p| and of |m / clamp - 1|: the two decisions a cell takes

Config = collections.namedtuple("Config", "n_fft hop win_length basis clamp mag_eps", defaults=(CLAMP, MAG_EPS))   # basis: float32 [n_mels, bins]


def slaney(sampling_rate, n_fft, n_mels, fmin=0.0, fmax=None):
    from genvox_amd.audio import get_mel_filter
    return torch.from_numpy(get_mel_filter(sampling_rate, n_fft, n_mels, fmin, sampling_rate / 2.0 if fmax is None else fmax).copy())


def pad_of(cfg):
    return (cfg.n_fft - cfg.hop) // 2


def n_min(cfg):
    return max(cfg.hop, pad_of(cfg) + 1)


def frames(n, hop):
    return n // hop


def window(n_fft, win_length, dtype=torch.float64):
    """The periodic Hann of win_length, centred in n_fft at offset (n_fft - win_length) // 2, computed in double."""
    w = torch.zeros(n_fft, dtype=torch.float64)
    k = torch.arange(win_length, dtype=torch.float64)
    off = (n_fft - win_length) // 2
    w[off:off + win_length] = 0.5 - 0.5 * torch.cos(2.0 * torch.pi * k / win_length)
    return w.to(dtype)


def source_index(p, pad, n):
    """Source sample of padded position p of a row of n samples."""
    i = p - pad
    if i < 0:
        return -i
    return 2 * (n - 1) - i if i >= n else i


def padded(x, cfg):
    """The 1-D row x (already cut at its length) reflect-padded by pad on both sides, through the definition's indices."""
    n, pad = x.shape[0], pad_of(cfg)
    assert n >= n_min(cfg)
    return x[torch.tensor([source_index(p, pad, n) for p in range(n + 2 * pad)])]


def mel(x, cfg):
    """(m, l): [F, n_mels] mel magnitudes before the clamp and their clamped logarithms, of the 1-D row x."""
    w = window(cfg.n_fft, cfg.win_length, x.dtype)
    X = torch.stft(padded(x, cfg), cfg.n_fft, hop_length=cfg.hop, win_length=cfg.n_fft, window=w, center=False, return_complex=True).transpose(0, 1)
    S = torch.sqrt(X.real * X.real + X.imag * X.imag + cfg.mag_eps)
    m = S @ cfg.basis.to(x.dtype).transpose(0, 1)
    return m, torch.log(torch.clamp(m, min=cfg.clamp))


def run(pred, target, lengths, cfg, dtype=torch.float64, want_grad=True):
    """The definition on a batch: dict(loss, parts [B], d_pred [B, n_max] or None, lp / lt / mp / mt as per-row lists of [F, n_mels])."""
    B, n_max = pred.shape
    lengths = [n_max] * B if lengths is None else list(lengths)
    p = pred.to(dtype).clone().requires_grad_(want_grad)
    t = target.to(dtype)
    total = torch.zeros((), dtype=dtype)
    parts = torch.zeros(B, dtype=dtype)
    out = dict(lp=[], lt=[], mp=[], mt=[])
    for b in range(B):
        mp, lp = mel(p[b, :lengths[b]], cfg)
        mt, lt = mel(t[b, :lengths[b]], cfg)
        assert lp.shape == (frames(lengths[b], cfg.hop), cfg.basis.shape[0])
        part = (lt - lp).abs().mean()
        total = total + part
        parts[b] = part.detach()
        for k, v in zip(("lp", "lt", "mp", "mt"), (lp, lt, mp, mt)):
            out[k].append(v.detach())
    loss = total / B
    d_pred = None
    if want_grad:
        loss.backward()
        d_pred = p.grad.detach()
    out.update(loss=loss.detach(), parts=parts, d_pred=d_pred)
    return out


def tol(err, ref):
    """What the device may differ from float64 by: FACTOR x max(the float32 twin's error, one ulp of the tensor's scale)."""
    return FACTOR * max(err, ULP * float(ref.abs().max()))


def reference(pred, target, lengths, cfg):
    """float64 run + the float32 twin's largest error per tensor: loss, parts, lp, lt, d_pred."""
    r64 = run(pred, target, lengths, cfg, torch.float64)
    r32 = run(pred, target, lengths, cfg, torch.float32)
    err = {k: float((r32[k].double() - r64[k]).abs().max()) for k in ("loss", "parts", "d_pred")}
    for k in ("lp", "lt"):
        err[k] = max(float((a.double() - b).abs().max()) for a, b in zip(r32[k], r64[k]))
    r64["err"] = err
    return r64


def margins(ref, cfg):
    """(smallest |l_t - l_p| over the cells that are not clamped on both sides, smallest |m / clamp - 1| over both signals,
    fraction of cells clamped on either side) of a float64 run."""
    d_min, c_min, clamped, cells = float("inf"), float("inf"), 0, 0
    for lp, lt, mp, mt in zip(ref["lp"], ref["lt"], ref["mp"], ref["mt"]):
        both = (mp < cfg.clamp) & (mt < cfg.clamp)
        d = (lt - lp).abs()[~both]
        if d.numel():
            d_min = min(d_min, float(d.min()))
        for m in (mp, mt):
            c_min = min(c_min, float((m / cfg.clamp - 1.0).abs().min()))
        clamped += int(((mp < cfg.clamp) | (mt < cfg.clamp)).sum())
        cells += mp.numel()
    return d_min, c_min, clamped / cells


def decided(ref, cfg):
    """Both margins hold, and 8 e(l) is below them: a device inside its bound decides every sign and every clamp as float64 does."""
    d_min, c_min, _ = margins(ref, cfg)
    return d_min >= MARGIN and c_min >= MARGIN and FACTOR * max(ref["err"]["lp"], ref["err"]["lt"]) < MARGIN


def seeded_case(build, lengths, cfg, seeds=range(1, 9)):
    """(seed, pred, target, reference) at the first seed of 1..8 whose float64 reference keeps both margins; build(seed) -> float32
    (pred, target)."""
    for seed in seeds:
        pred, target = build(seed)
        ref = reference(pred, target, lengths, cfg)
        if decided(ref, cfg):
            return seed, pred, target, ref
    raise AssertionError("no seed of 1..8 keeps |l_t - l_p| and |m / clamp - 1| at 1e-4 or more")


def noise(seed, B, n_max, scale=0.3):
    """N(0, scale^2) noise drawn in float64 and rounded once."""
    g = torch.Generator().manual_seed(seed)
    return ((scale * torch.randn(B, n_max, generator=g, dtype=torch.float64)).float(),
            (scale * torch.randn(B, n_max, generator=g, dtype=torch.float64)).float())
