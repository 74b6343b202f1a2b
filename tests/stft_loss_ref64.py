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
    """float64 run + the float32 twin's largest error per tensor (loss, parts, each resolution's magnitudes over all rows, d_pred; parts and
    d_pred per row too) and,
    per row / resolution / frame, the twin's largest complex error |X32 - X64| of pred and of target (E_f of the near-tie rule)."""
    r64 = run(pred, target, lengths, resolutions, w_sc, w_mag, eps, torch.float64, signs)
    r32 = run(pred, target, lengths, resolutions, w_sc, w_mag, eps, torch.float32, signs)
    B, R = len(r64["Mp"]), len(resolutions)
    err = dict(loss=float((r32["loss"].double() - r64["loss"]).abs()), parts=float((r32["parts"].double() - r64["parts"]).abs().max()),
               d_pred=float((r32["d_pred"].double() - r64["d_pred"]).abs().max()))
    # row by row as well: where the rows' scales lie far apart (a silent target beside a live one) the row's own error is the tighter bound
    err["parts_rows"] = [float((r32["parts"][b].double() - r64["parts"][b]).abs().max()) for b in range(B)]
    err["d_pred_rows"] = [float((r32["d_pred"][b].double() - r64["d_pred"][b]).abs().max()) for b in range(B)]
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


# ---- signals that are not noise: silence, tones, scale, rows equal to their target.  Every builder is deterministic in its seed and
# returns float32 (pred, target, lengths); the noise is drawn in float64 and rounded once, as noise_case has it.

def _noise(seed, B, n_max):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n_max, generator=g, dtype=torch.float64), torch.randn(B, n_max, generator=g, dtype=torch.float64)


def gated_case(seed, n_max, lengths, pred_silent, target_silent, hush=0.0):
    """Unit noise in which the stretches (row, start, stop) - stop None: to the end of the buffer - are exact zeros, or, with ``hush``,
    the noise times that factor: at 2^-20 every power of a frame inside a stretch lies far below eps / 2 without being 0, so the
    clamp's derivative multiplies a spectrum that is not 0 - a clamp that passed gradient would show, as it cannot on zeros.  With every
    boundary on a multiple of every hop a frame's window covers either zeros alone (every power is exactly 0: the frame is silent)
    or at least half a hop of noise, far above eps - except in a frame that the reflection makes symmetric (frame 0 of every row), whose
    spectrum is real up to a phase and may cross 0; the seed rule of signal_case looks after those."""
    pred, target = _noise(seed, len(lengths), n_max)
    for x, spans in ((pred, pred_silent), (target, target_silent)):
        for b, lo, hi in spans:
            x[b, lo:hi] *= hush
    return pred.float(), target.float(), list(lengths)


def tone_case(seed, n_max, lengths, dc=()):
    """Per row a sin(2 pi f n + phi) + 1e-2 noise, pred and target slightly apart in a, f and phi; dc[b] is added to both signals of
    row b.  No bin is near the clamp and a frame's powers span about 60 dB."""
    B = len(lengths)
    pred, target = _noise(seed, B, n_max)
    n = torch.arange(n_max, dtype=torch.float64)
    for b in range(B):
        spread = 1.0 + 0.37 * b   # another tone per row
        pred[b] = 0.5 * torch.sin(2.0 * torch.pi * 0.0631 * spread * n + 0.3) + 1e-2 * pred[b]
        target[b] = 0.45 * torch.sin(2.0 * torch.pi * 0.0637 * spread * n + 0.4) + 1e-2 * target[b]
        if b < len(dc):
            pred[b] += dc[b]
            target[b] += dc[b]
    return pred.float(), target.float(), list(lengths)


def scaled_case(seed, n_max, lengths, exponent):
    """Unit noise times 2^exponent: the float32 inputs of two exponents are exact scalings of each other."""
    pred, target = _noise(seed, len(lengths), n_max)
    return pred.float() * 2.0 ** exponent, target.float() * 2.0 ** exponent, list(lengths)


def mixed_equal_case(seed, n_max, lengths):
    """Three rows of unit noise: row 0 has pred == target bit for bit, row 1 on the first half of its own length, row 2 nowhere."""
    assert len(lengths) == 3
    pred, target = _noise(seed, 3, n_max)
    pred, target = pred.float(), target.float()
    pred[0] = target[0]
    pred[1, :lengths[1] // 2] = target[1, :lengths[1] // 2]
    return pred, target, list(lengths)


def clamp_takes_whole_frames(ref, eps=EPS):
    """eps_clear and more: a frame's float64 powers lie below eps either all or not at all.  A bin is clamped exactly where its frame
    reads a gated stretch alone, so the tone, scaled and mixed cases clamp nothing and the gated ones whole frames."""
    for k in ("Xp", "Xt"):
        for rows in clamped(ref, k, eps):
            for m in rows:
                if bool((m.any(dim=1) & ~m.all(dim=1)).any()):
                    return False
    return eps_clear(ref, eps)


_R512, _R1024, _R2048 = ((512, 128, 512),), ((1024, 120, 600),), ((2048, 240, 1200),)
# name: (resolutions, builder, its arguments after the seed).  Every supported n_fft once as a single resolution with all four frame
# kinds (both live, only pred silent, only target silent, both silent) and the default resolutions together once; the gated stretches
# start and stop on common multiples of the hops (1200 for the defaults).
SIGNAL_CASES = {
    # row 0: a silent stretch of pred inside the row, target silent from 640 on and so across the right reflection; row 1 (1153 of 1280
    # samples): pred silent from sample 0, so the left reflection is silent, target silent throughout
    "gated_r512": (_R512, gated_case, (1280, (1280, 1153), ((0, 384, 1152), (1, 0, 512)), ((0, 640, None), (1, 0, None)))),
    "hushed_r512": (_R512, gated_case, (1280, (1280, 1153), ((0, 384, 1152), (1, 0, 512)), ((0, 640, None), (1, 0, None)), 2.0 ** -20)),
    "gated_r1024": (_R1024, gated_case, (2400, (2400,), ((0, 600, 1920),), ((0, 1200, None),))),
    "gated_r2048": (_R2048, gated_case, (6000, (6000,), ((0, 1200, 4800),), ((0, 2400, None),))),
    # at 4800 samples the 2048-point resolution has no frame in which both signals are silent: its 1199 non-zero taps lie within 599
    # samples of a multiple of 240, and 2400 .. 3600 holds them only around 3000, half a hop off; gated_r2048 has that kind
    "gated_default": (DEFAULT_RESOLUTIONS, gated_case, (4800, (4800,), ((0, 1200, 3600),), ((0, 2400, None),))),
    # frame 0 of every row is symmetric about sample 0 under the reflection, so its spectrum is real up to the frame's phase and its
    # powers come near 0 far more often than a complex bin's: the tone cases stay small so that a seed of 1..8 clears the clamp
    "tone_r512": (_R512, tone_case, (700, (700, 650), (0.0, 0.25))),
    "tone_r1024": (_R1024, tone_case, (1500, (1500,))),
    "unit_r2048": (((2048, 512, 2048),), scaled_case, (2100, (2049, 1500), 0)),
    "loud_r2048": (((2048, 512, 2048),), scaled_case, (2100, (2049, 1500), 15)),
    "quiet_r2048": (((2048, 512, 2048),), scaled_case, (2100, (2049, 1500), -6)),
    "mixed_equal_r512": (((512, 50, 240),), mixed_equal_case, (640, (640, 600, 515))),
}
# cases that take their seed together: the scaled ones are compared with each other
SEED_GROUPS = (("unit_r2048", "loud_r2048", "quiet_r2048"),)
_signal_cache = {}


def _build_signal(name, seed):
    res, builder, args = SIGNAL_CASES[name]
    pred, target, lengths = builder(seed, *args)
    return dict(name=name, seed=seed, res=res, pred=pred, target=target, lengths=lengths, n_max=pred.shape[1],
                ref=reference(pred, target, lengths, res))


def signal_case(name, seeds=range(1, 9)):
    """The case of that name at the first seed of 1..8 whose powers - and those of every case of its seed group - are clear of the
    clamp: dict(name, seed, res, pred, target, lengths, n_max, ref = the free reference).  Computed once, never changed."""
    if name not in _signal_cache:
        group = next((g for g in SEED_GROUPS if name in g), (name,))
        for seed in seeds:
            built = [_build_signal(n, seed) for n in group]
            if all(clamp_takes_whole_frames(c["ref"]) for c in built):
                _signal_cache.update({c["name"]: c for c in built})
                break
        else:
            raise AssertionError(f"{name}: no seed of 1..8 keeps the powers clear of [eps / 2, 2 eps] and the clamp to whole frames")
    return _signal_cache[name]


def clamped(ref, key, eps=EPS):
    """[b][r] -> bool [F, bins]: the float64 powers of that signal ("Xp" or "Xt") below eps."""
    return [[(X.real * X.real + X.imag * X.imag) < eps for X in rows] for rows in ref[key]]


def silent_frames(ref, key):
    """[b][r] -> bool [F]: frames whose float64 spectrum is exactly zero at every bin."""
    return [[((X.real == 0) & (X.imag == 0)).all(dim=1) for X in rows] for rows in ref[key]]


def clamped_frames(ref, key, eps=EPS):
    """[b][r] -> bool [F]: frames whose float64 powers all lie below eps (silent, or hushed far below it)."""
    return [[m.all(dim=1) for m in rows] for rows in clamped(ref, key, eps)]


def live_support(ref, lengths, resolutions, n_max):
    """bool [B, n_max]: the samples of pred that some frame with an unclamped bin reads - itself or through a reflection - under a
    non-zero window tap.  Everywhere else the clamp passes no gradient: d_pred is exactly 0."""
    B = len(ref["Xp"])
    out = torch.zeros(B, n_max, dtype=torch.bool)
    cl = clamped(ref, "Xp")
    for b in range(B):
        for r, (n_fft, hop, win_length) in enumerate(resolutions):
            taps = torch.nonzero(window(n_fft, win_length) != 0).flatten().tolist()
            for t in torch.nonzero(~cl[b][r].all(dim=1)).flatten().tolist():
                out[b, [source_index(t * hop + k, n_fft, lengths[b]) for k in taps]] = True
    return out


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
