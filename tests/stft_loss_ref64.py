"""The multi-resolution STFT loss of include/genvox_amd.h ("Multi-resolution STFT loss") restated with torch.stft, row by row on the
row cut at its own length, in float64 and as a float32 twin on the CPU, with autograd for the gradient.  Written from the definition
in the header, never from the kernels.

`signs` (per row and resolution a [F, bins] tensor of -1 / 0 / +1) replaces |log M_t - log M_p| by signs * (log M_t - log M_p): the
pinned form, whose gradient follows the given sign decisions instead of the restatement's own."""
import torch

FACTOR = 8.0
ULP = 2.0 ** -23
DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
EPS = 1e-7


def frames(n, hop):
    return 1 + n // hop


def window(n_fft, win_length, dtype=torch.float64):
    """The periodic Hann of win_length, centred in n_fft at offset (n_fft - win_length) // 2, computed in double."""
    w = torch.zeros(n_fft, dtype=torch.float64)
    k = torch.arange(win_length, dtype=torch.float64)
    off = (n_fft - win_length) // 2
    w[off:off + win_length] = 0.5 - 0.5 * torch.cos(2.0 * torch.pi * k / win_length)
    return w.to(dtype)


def source_index(p, n_fft, n):
    """Source sample of padded position p of a row of n samples."""
    i = p - n_fft // 2
    if i < 0:
        return -i
    return 2 * (n - 1) - i if i >= n else i


def spectrum(x, res):
    """[F, bins] complex spectrum of the 1-D row x (already cut at its length)."""
    n_fft, hop, win_length = res
    w = window(n_fft, win_length, x.dtype)
    return torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect", return_complex=True).transpose(0, 1)


def magnitude(X, eps=EPS):
    return torch.sqrt(torch.clamp(X.real * X.real + X.imag * X.imag, min=eps))


def row_terms(xp, xt, res, eps=EPS, sign=None):
    """(sc, mag, M_p, M_t, X_p, X_t) of one row and one resolution."""
    Xp, Xt = spectrum(xp, res), spectrum(xt, res)
    Mp, Mt = magnitude(Xp, eps), magnitude(Xt, eps)
    sc = torch.linalg.norm(Mt - Mp) / torch.linalg.norm(Mt)
    u = torch.log(Mt) - torch.log(Mp)
    mag = (u.abs() if sign is None else sign.to(u.dtype) * u).mean()
    return sc, mag, Mp, Mt, Xp, Xt


def run(pred, target, lengths, resolutions, w_sc=1.0, w_mag=1.0, eps=EPS, dtype=torch.float64, signs=None, want_grad=True):
    """The definition on a batch: dict(loss, parts [B, R, 2], d_pred [B, n_max] or None, Mp / Mt / Xp / Xt as [b][r] lists)."""
    B, n_max = pred.shape
    lengths = [n_max] * B if lengths is None else list(lengths)
    p = pred.to(dtype).clone().requires_grad_(want_grad)
    t = target.to(dtype)
    R = len(resolutions)
    total = torch.zeros((), dtype=dtype)
    parts = torch.zeros(B, R, 2, dtype=dtype)
    out = dict(Mp=[], Mt=[], Xp=[], Xt=[])
    for b in range(B):
        rows = dict(Mp=[], Mt=[], Xp=[], Xt=[])
        for r, res in enumerate(resolutions):
            sc, mag, Mp, Mt, Xp, Xt = row_terms(p[b, :lengths[b]], t[b, :lengths[b]], res, eps, None if signs is None else signs[b][r])
            total = total + w_sc * sc + w_mag * mag
            parts[b, r, 0], parts[b, r, 1] = sc.detach(), mag.detach()
            for k, v in zip(("Mp", "Mt", "Xp", "Xt"), (Mp, Mt, Xp, Xt)):
                rows[k].append(v.detach())
        for k in rows:
            out[k].append(rows[k])
    loss = total / (B * R)
    d_pred = None
    if want_grad:
        loss.backward()
        d_pred = p.grad.detach()
    out.update(loss=loss.detach(), parts=parts, d_pred=d_pred)
    return out


def tol(err, ref):
    """What the device may differ from float64 by: FACTOR x max(the float32 twin's error, one ulp of the tensor's scale)."""
    return FACTOR * max(err, ULP * float(ref.abs().max()))


def reference(pred, target, lengths, resolutions, w_sc=1.0, w_mag=1.0, eps=EPS, signs=None):
    """float64 run + the float32 twin's largest error per tensor (loss, parts, each resolution's magnitudes over all rows, d_pred) and,
    per row / resolution / frame, the twin's largest complex error |X32 - X64| of pred and of target (E_f of the near-tie rule)."""
    r64 = run(pred, target, lengths, resolutions, w_sc, w_mag, eps, torch.float64, signs)
    r32 = run(pred, target, lengths, resolutions, w_sc, w_mag, eps, torch.float32, signs)
    B, R = len(r64["Mp"]), len(resolutions)
    err = dict(loss=float((r32["loss"].double() - r64["loss"]).abs()), parts=float((r32["parts"].double() - r64["parts"]).abs().max()),
               d_pred=float((r32["d_pred"].double() - r64["d_pred"]).abs().max()))
    for k in ("Mp", "Mt"):
        err[k] = [max(float((r32[k][b][r].double() - r64[k][b][r]).abs().max()) for b in range(B)) for r in range(R)]
    r64["err"] = err
    r64["frame_err"] = {k: [[(r32[k][b][r].to(torch.complex128) - r64[k][b][r]).abs().amax(dim=1) for r in range(R)] for b in range(B)]
                        for k in ("Xp", "Xt")}
    return r64


def eps_clear(ref, eps=EPS):
    """No float64 power of either signal lies within [eps / 2, 2 eps]: the clamp decides the same way in any precision."""
    for k in ("Xp", "Xt"):
        for rows in ref[k]:
            for X in rows:
                P = X.real * X.real + X.imag * X.imag
                if bool(((P >= eps / 2) & (P <= 2 * eps)).any()):
                    return False
    return True


def noise_case(B, n_max, lengths, resolutions, seeds=range(1, 9), eps=EPS):
    """(seed, pred, target, free reference) of unit-variance noise: the first seed of 1..8 whose powers stay clear of the clamp."""
    for seed in seeds:
        g = torch.Generator().manual_seed(seed)
        pred = torch.randn(B, n_max, generator=g, dtype=torch.float64).float()
        target = torch.randn(B, n_max, generator=g, dtype=torch.float64).float()
        ref = reference(pred, target, lengths, resolutions, eps=eps)
        if eps_clear(ref, eps):
            return seed, pred, target, ref
    raise AssertionError("no seed of 1..8 keeps every power clear of [eps / 2, 2 eps]")


def sign_flips_are_near_ties(ref, signs_dev):
    """Every device sign that differs from float64's sits on a true near-tie: |dlog64| <= FACTOR (E_f(pred) / M_p + E_f(target) / M_t).
    Returns (flips, near-ties under that bound)."""
    flips = ties = 0
    for b, rows in enumerate(signs_dev):
        for r, s in enumerate(rows):
            Mp, Mt = ref["Mp"][b][r], ref["Mt"][b][r]
            u = torch.log(Mt) - torch.log(Mp)
            bound = FACTOR * (ref["frame_err"]["Xp"][b][r][:, None] / Mp + ref["frame_err"]["Xt"][b][r][:, None] / Mt)
            differ = torch.sign(u) != s.to(u.dtype)
            assert bool((u.abs()[differ] <= bound[differ]).all()), f"row {b} resolution {r}: a sign differs from float64 away from a tie"
            flips += int(differ.sum())
            ties += int((u.abs() <= bound).sum())
    return flips, ties
