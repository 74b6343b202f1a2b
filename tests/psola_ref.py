"""The pitch control of include/genvox_amd.h (gvx_psola_plan, gvx_psola_synth) restated in numpy, written from the definitions
there.  The plan is integers and comparisons and has one answer; the overlap-add takes a dtype: float64 is the reference the
kernel is held to, float32 the same operations at the kernel's precision.

Besides y, ``synth`` returns per output sample what the rounding bound needs: the number of grains summed, the sum of w |x|, the
sum of |x| over those grains, D and Num (``y_bound``)."""
import math

import numpy as np

EPS32 = 2.0 ** -24
OK, EMPTY, BAD_RATIO = 0, 1, 2
RATIO_MIN, RATIO_MAX = 0.5, 2.0
TILE = 256


def tiled_period(P: int, n: int) -> np.ndarray:
    """One harmonic-rich period of P samples, tiled: five cosines in phase, so every period has one clear peak, at its first sample."""
    t = np.arange(P)
    one = sum(a * np.cos(2 * np.pi * h * t / P) for h, a in enumerate((1.0, 0.5, 0.3, 0.2, 0.1), start=1))
    return (0.4 * np.tile(one, -(-n // P))[:n]).astype(np.float32)


def frames_of(n: int, hop: int) -> int:
    return 0 if n <= 0 else -(-n // hop)


def max_marks(N: int, p_min: int) -> int:
    return 0 if N < 1 or p_min < 1 else N // ((3 * p_min + 3) // 4) + 1


def max_grains(N: int, p_min: int) -> int:
    return 0 if N < 1 or p_min < 1 else N // max(1, (p_min + 1) // 2) + 1


class Grid:
    """The frame grid of one row and what the lag contour says at a sample."""

    def __init__(self, n, lag, hop, first_centre, lag_min, lag_max, unvoiced_period):
        self.n, self.lag, self.hop, self.first_centre = n, lag, hop, first_centre
        self.lag_min, self.lag_max, self.U, self.Fb = lag_min, lag_max, unvoiced_period, frames_of(n, hop)

    def frame_of(self, t: int) -> int:
        return min(max((t - self.first_centre + self.hop // 2) // self.hop, 0), self.Fb - 1)   # // floors

    def voiced_at(self, t: int) -> bool:
        return int(self.lag[self.frame_of(t)]) >= 1

    def period_at(self, t: int) -> int:
        return min(max(int(self.lag[self.frame_of(t)]), self.lag_min), self.lag_max) if self.voiced_at(t) else self.U


def plan_row(x, n, lag, ratio, *, hop, first_centre, lag_min, lag_max, unvoiced_period):
    """One row: (marks, periods, voiced, syn_pos, syn_src, status) as Python lists of ints (voiced: bools)."""
    if n == 0:
        return [], [], [], [], [], EMPTY
    g = Grid(n, lag, hop, first_centre, lag_min, lag_max, unvoiced_period)
    marks, periods, voiced = [], [], []
    while True:
        prev = marks[-1] if marks else -1
        c = prev + periods[-1] if marks else 0
        if c >= n:
            break
        m = c
        if g.voiced_at(c):
            r = (min(g.period_at(c), periods[-1]) if marks else g.period_at(0)) // 4
            best = -math.inf
            for i in range(max(c - r, prev + 1), min(c + r, n - 1) + 1):
                if x[i] > best:
                    best, m = x[i], i
        marks.append(m)
        periods.append(g.period_at(m))
        voiced.append(g.voiced_at(m))
    assert len(marks) <= max_marks(n, min(lag_min, unvoiced_period))
    with np.errstate(invalid="ignore"):
        q = np.asarray(ratio[:g.Fb], np.float32)
        if not np.all((q >= RATIO_MIN) & (q <= RATIO_MAX)):
            return marks, periods, voiced, [], [], BAD_RATIO
    pos, src = [marks[0]], [0]
    while True:
        s, a = pos[-1], src[-1]
        qj = float(np.float32(ratio[g.frame_of(s)])) if voiced[a] else 1.0
        step = max(1, int(math.floor(float(periods[a]) / qj + 0.5)))
        s2 = s + step
        if s2 >= n:
            break
        while a + 1 < len(marks) and abs(marks[a + 1] - s2) < abs(marks[a] - s2):
            a += 1
        pos.append(s2)
        src.append(a)
    assert len(pos) <= max_grains(n, min(lag_min, unvoiced_period))
    return marks, periods, voiced, pos, src, OK


def synth_row(x, n, marks, periods, pos, src, status, dtype=np.float64):
    """One row's overlap-add.  Returns a dict of arrays over [len(x)]: y, grains (summed into the sample), wabs (sum of w |x|), xabs
    (sum of |x| over those grains), D, Num, inside (between the first and the last synthesis mark)."""
    N = len(x)
    out = {"y": np.zeros(N, dtype), "grains": np.zeros(N, np.int64), "wabs": np.zeros(N, dtype), "xabs": np.zeros(N, dtype),
           "D": np.zeros(N, dtype), "Num": np.zeros(N, dtype), "inside": np.zeros(N, bool)}
    if n == 0:
        return out
    xr = np.asarray(x[:n]).astype(dtype)
    if status != OK or not pos:
        out["y"][:n] = xr
        return out
    num, den = np.zeros(n, dtype), np.zeros(n, dtype)
    one, two, three = dtype(1), dtype(2), dtype(3)
    for s, a in zip(pos, src):   # j ascending: every sample receives its grains in that order
        p, m = periods[a], marks[a]
        t = np.arange(max(s - p + 1, 0), min(s + p - 1, n - 1) + 1)
        u = t - s
        v = (one - (np.abs(u).astype(dtype) / dtype(p)).astype(dtype)).astype(dtype)
        w = ((v * v).astype(dtype) * (three - (two * v).astype(dtype)).astype(dtype)).astype(dtype)
        at = m + u
        ok = (at >= 0) & (at < n)
        xv = np.zeros(len(t), dtype)
        xv[ok] = xr[at[ok]]
        if dtype == np.float32:   # fmaf(w, xv, num): the product exact in double (24 x 24 bits), the sum rounded to float32 - one rounding up to double rounding
            num[t] = (w.astype(np.float64) * xv.astype(np.float64) + num[t].astype(np.float64)).astype(np.float32)
        else:
            num[t] = num[t] + w * xv
        den[t] = (den[t] + w).astype(dtype)
        out["grains"][t] += 1
        out["wabs"][t] += w * np.abs(xv)
        out["xabs"][t] += np.abs(xv)
    t = np.arange(n)
    inside = (t >= pos[0]) & (t <= pos[-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        y_in = (num / np.maximum(den, dtype(0.5))).astype(dtype)
        y_div = (num / den).astype(dtype)
    if dtype == np.float32:
        y_keep = ((one - den).astype(np.float32).astype(np.float64) * xr.astype(np.float64) + num.astype(np.float64)).astype(np.float32)
    else:
        y_keep = (one - den) * xr + num
    out["y"][:n] = np.where(inside, y_in, np.where(den >= one, y_div, y_keep))
    out["D"][:n], out["Num"][:n], out["inside"][:n] = den, num, inside
    return out


def y_bound(ref: dict, x, n: int) -> np.ndarray:
    """|y32 - y64| <= this, per sample, for the fp32 arithmetic of the header in the header's order; eps = 2^-24, everything below
    evaluated on the float64 restatement ``ref`` = synth_row(..., dtype=float64).  G = grains summed into the sample.

      w    a = |u| / p rounds once (a <= 1: at most eps absolute); v = 1 - a rounds once more (v <= 1): v is off by at most 2 eps
           ABSOLUTE - not relative: 1 - a cancels.  S(v) = v^2 (3 - 2 v) has |S'| = 6 v (1 - v) <= 3/2, so the error of v moves w
           by at most 3 eps; v * v, 3 - 2 v (2 v is exact) and their product round once each, on a w <= 1: 3 eps more.  With 1 eps
           for the second-order terms: |w32 - w| <= 7 eps, absolute.
      Num  the sum over G grains of w x by fused multiply-adds, one rounding each: the wrong weights contribute at most
           7 eps * sum |x|, the G roundings (the first rounds a product alone, then G - 1 additions of products) at most
           G eps * sum w |x| at first order; (G + 1) covers the second order.  E_N = 7 eps xabs + (G + 1) eps wabs.
      D    the same with x = 1: E_D = 7 eps G + (G + 1) eps D.
      y    = Num / Q with Q = max(D, 1/2) inside, Q = D >= 1 outside (max does not stretch an error): the quotient of two wrong
           numbers, rounded once: (E_N + |y| E_D) / (Q - E_D) + eps |y|.  Outside with D < 1, y = fmaf(1 - D, x[t], Num):
           1 - D carries E_D and one rounding, the fused correction one more: E_N + (E_D + eps) |x[t]| + eps |y|.
      D ~ 1  outside, a D within E_D of 1 may take the other form in fp32; the two forms differ by |1 - D| |Num / D - x[t]|
           <= E_D (|Num| + |x[t]|) / (1 - E_D) there, which is added.
    One expression covers every case: (E_N + (|y| + |x[t]|) (E_D + eps)) / (Q - E_D) + 2 eps |y|, with Q = 1 where D < 1 outside,
    plus the last term where it applies."""
    N = len(ref["y"])
    G = ref["grains"].astype(np.float64)
    D, Num, y = ref["D"].astype(np.float64), ref["Num"].astype(np.float64), np.abs(ref["y"].astype(np.float64))
    xt = np.zeros(N)
    xt[:n] = np.abs(np.asarray(x[:n], np.float64))
    E_N = 7 * EPS32 * ref["xabs"] + (G + 1) * EPS32 * ref["wabs"]
    E_D = 7 * EPS32 * G + (G + 1) * EPS32 * D
    Q = np.where(ref["inside"], np.maximum(D, 0.5), np.where(D >= 1, D, 1.0))
    bound = (E_N + (y + xt) * (E_D + EPS32)) / (Q - E_D) + 2 * EPS32 * y
    flip = ~ref["inside"] & (np.abs(D - 1) <= E_D)
    bound = bound + np.where(flip, E_D * (np.abs(Num) + xt) / (1 - E_D), 0.0)
    bound[n:] = 0.0
    return bound


def psola(wav, lengths, lag, ratio, *, hop, first_centre=0, lag_min, lag_max, unvoiced_period, dtype=np.float64):
    """wav [B, N] (anything at and behind lengths[b], NaN included), lag int [B, F], ratio [B, F].  Returns a dict: per row lists
    ``marks``, ``periods`` (signed: -p for an unvoiced mark, as the plan stores them), ``syn_pos``, ``syn_src``; arrays ``status``
    [B], ``n_marks`` [B], ``n_grains`` [B], ``y`` [B, N] in dtype; and ``rows``: synth_row's dict per row."""
    wav = np.asarray(wav)
    B, N = wav.shape
    lengths = [N] * B if lengths is None else [min(max(int(n), 0), N) for n in lengths]
    out = {"marks": [], "periods": [], "syn_pos": [], "syn_src": [], "rows": [], "status": np.zeros(B, np.int32),
           "n_marks": np.zeros(B, np.int32), "n_grains": np.zeros(B, np.int32), "y": np.zeros((B, N), dtype)}
    for b in range(B):
        n = lengths[b]
        marks, periods, voiced, pos, src, status = plan_row(wav[b], n, lag[b], ratio[b], hop=hop, first_centre=first_centre, lag_min=lag_min,
                                                            lag_max=lag_max, unvoiced_period=unvoiced_period)
        row = synth_row(wav[b], n, marks, periods, pos, src, status, dtype)
        out["marks"].append(marks)
        out["periods"].append([p if v else -p for p, v in zip(periods, voiced)])
        out["syn_pos"].append(pos)
        out["syn_src"].append(src)
        out["rows"].append(row)
        out["status"][b], out["n_marks"][b], out["n_grains"][b] = status, len(marks), len(pos)
        out["y"][b] = row["y"]
    return out
