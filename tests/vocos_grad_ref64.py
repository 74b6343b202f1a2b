"""Float64 autograd of tests/vocos_ref64.py's Generator for the Vocos backward tests: every row alone at its own length, a cotangent
drawn from a seed, and per gradient tensor the float32 restatement's own distance from float64 (the base of the tests' bound).  The tape
tensors - the embedding's output, x in front of every block and behind the last, every block's pre-GELU p, the head product - come back
with it, in the device's order.  Nothing here touches the library.

The clamp min(exp(m), 100) has a kink at m = ln 100, and torch.clip hands the gradient to m where exp(m) <= 100.  Two modes:
    tie-free   no float64 log-magnitude inside a row lies within FACTOR x max(e, ulp) of ln 100, e being the float32 restatement's error
               of the head product and ulp 2^-23 x its largest magnitude: plain autograd is the reference (``tie_free_case`` takes the
               first mel seed of 1..8 for which that holds);
    pinned     ``masks`` (bool [B, T, H + 1], the device's own exp(m) <= 100 read off its tape) replaces the clip's decision, after the
               caller has asserted that every decision that differs from float64's is such a near-tie."""
import copy

import torch
import torch.nn.functional as F

from tests import vocos_ref64 as R

FACTOR = 8.0
ULP = 2.0 ** -23


def cotangent(cfg, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T * cfg["hop_length"], generator=g, dtype=torch.float64)


def istft(coeffs, n_fft, hop, padding, keep=None):
    """R.istft's expression, for autograd: the trim comes BEFORE the division by the envelope.  The envelope is 0 at position 0 (the
    periodic Hann window starts at 0 and only frame 0 reaches there), a position both paddings trim away; R.istft divides first, which
    is the same forward value and 0 x inf = NaN in frame 0's gradient.  ``keep`` (bool, like the log-magnitudes): the clip's decision
    handed in - where the magnitude is exp(m); None: torch.clip's own."""
    B, T, _ = coeffs.shape
    H = n_fft // 2
    m, p = coeffs[..., :H + 1], coeffs[..., H + 1:]
    mag = torch.clip(torch.exp(m), max=100.0) if keep is None else torch.where(keep, torch.exp(m), torch.full_like(m, 100.0))
    S = torch.complex(mag * torch.cos(p), mag * torch.sin(p))
    win = torch.hann_window(n_fft, periodic=True, dtype=coeffs.dtype, device=coeffs.device)
    frames = torch.fft.irfft(S, n_fft, dim=-1, norm="backward") * win
    size = (T - 1) * hop + n_fft
    fold = lambda cols: F.fold(cols, output_size=(1, size), kernel_size=(1, n_fft), stride=(1, hop))[:, 0, 0, :]
    y = fold(frames.transpose(1, 2))
    env = fold((win * win).expand(1, T, -1).transpose(1, 2))[0]
    pad = n_fft // 2 if padding == "center" else (n_fft - hop) // 2
    return y[:, pad:size - pad] / env[pad:size - pad]


def forward(gen, mel, keep=None):
    """One row group at full length -> (wav, tape [B, T, C] each: e, x0, (p_i, x_{i+1}) per block, the head product)."""
    bb, cfg = gen.backbone, gen.cfg
    e = bb.embed(mel).transpose(1, 2)
    x = bb.norm(e)
    tape = [e, x]
    for blk in bb.convnext:
        u = blk.dwconv(x.transpose(1, 2)).transpose(1, 2)
        p = blk.pwconv1(blk.norm(u))
        x = x + blk.gamma * blk.pwconv2(F.gelu(p))
        tape += [p, x]
    c = gen.head.out(bb.final_layer_norm(x))
    tape.append(c)
    return istft(c, cfg["n_fft"], cfg["hop_length"], cfg["padding"], keep), tape


def _run(gen, mel, lens, G, masks):
    """Every row alone: parameter gradients summed over the rows, d_mel and the tape assembled with zeros behind a row."""
    cfg = gen.cfg
    B, _, T = mel.shape
    lens = [T] * B if lens is None else list(lens)
    gen.zero_grad(set_to_none=True)
    d_mel = torch.zeros_like(mel)
    wav = torch.zeros(B, T * cfg["hop_length"], dtype=mel.dtype)
    tape = None
    for b, t in enumerate(lens):
        row = mel[b:b + 1, :, :t].clone().requires_grad_(True)
        w, tp = forward(gen, row, None if masks is None else masks[b:b + 1, :t])
        n = w.shape[1]
        if n:
            (w * G[b:b + 1, :n].to(w.dtype)).sum().backward()
            d_mel[b, :, :t] = row.grad[0]
        wav[b, :n] = w[0].detach()
        if tape is None:
            tape = [torch.zeros(B, T, s.shape[2], dtype=mel.dtype) for s in tp]
        for dst, s in zip(tape, tp):
            dst[b, :t] = s[0].detach()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in gen.named_parameters()}
    return wav, tape, grads, d_mel


def reference(gen, mel, lens, G, masks=None):
    """-> dict: wav, tape, grads (by state-dict name), mel (d_mel) in float64, and tape_err / grad_err / mel_err: the float32
    restatement's largest distance from each.  ``mel`` must be float32-representable and finite inside the rows."""
    clean = mel.clone()
    if lens is not None:
        for b, t in enumerate(lens):
            clean[b, :, t:] = 0.0
    wav, tape, grads, d_mel = _run(gen, clean, lens, G, masks)
    g32 = copy.deepcopy(gen).float()
    g32.cfg = gen.cfg
    wav32, tape32, grads32, d_mel32 = _run(g32, clean.float(), lens, G, masks)
    dist = lambda a, b: (a.double() - b).abs().max().item() if b.numel() else 0.0
    return dict(wav=wav, tape=tape, grads=grads, mel=d_mel, wav_err=dist(wav32, wav), tape_err=[dist(a, b) for a, b in zip(tape32, tape)],
                grad_err={k: dist(grads32[k], grads[k]) for k in grads}, mel_err=dist(d_mel32, d_mel))


def clamp_margin(ref):
    c = ref["tape"][-1]
    return FACTOR * max(ref["tape_err"][-1], ULP * c.abs().max().item())


def near_ties(ref, lens, cfg):
    """Log-magnitudes inside the rows within the margin of ln 100."""
    H = cfg["n_fft"] // 2
    m = ref["tape"][-1][..., :H + 1]
    near = (m - R.LOG_CLAMP).abs() <= clamp_margin(ref)
    if lens is not None:
        for b, t in enumerate(lens):
            near[b, t:] = False
    return int(near.sum())


def clamped_share(ref, lens, cfg):
    H = cfg["n_fft"] // 2
    m = ref["tape"][-1][..., :H + 1]
    rows = [m[b, :t] for b, t in enumerate(lens if lens is not None else [m.shape[1]] * m.shape[0])]
    flat = torch.cat([r.reshape(-1) for r in rows])
    return (flat > R.LOG_CLAMP).double().mean().item()


def tie_free_case(gen, cfg, B, T, lens, G_seed):
    """-> (mel seed, mel, G, reference) for the first mel seed of 1..8 without a near-tie; AssertionError if there is none."""
    G = cotangent(cfg, B, T, G_seed)
    for seed in range(1, 9):
        mel = R.random_mel(cfg, B, T, seed).float().double()
        ref = reference(gen, mel, lens, G)
        if near_ties(ref, lens, cfg) == 0:
            return seed, mel, G, ref
    raise AssertionError(f"no mel seed in 1..8 is tie-free for {B} x {T} {lens}")


def masks_from_coeffs(coeffs32, cfg):
    """The device's decisions from its own head product (float32 tensor on the CPU): where ITS expf(m) <= 100.  expf in float32 on the
    host rounds as the device's does to within an ulp; a decision that close to the kink is a near-tie in any case, which the caller
    asserts."""
    H = cfg["n_fft"] // 2
    return torch.exp(coeffs32[..., :H + 1].float()) <= 100.0


def unfold_gamma(dw2f, db2f, gamma, w2, b2):
    """The device's unfold, restated: gradients w.r.t. gamma (.) W2 and gamma (.) b2 -> (dW2, db2, d gamma)."""
    return gamma[:, None] * dw2f, gamma * db2f, (dw2f * w2).sum(1) + db2f * b2
