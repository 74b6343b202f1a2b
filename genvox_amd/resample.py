"""Host side of the GPU resampler (csrc/resample.hip): rate ratios, the Kaiser-windowed sinc prototype, its polyphase table and
the grouping of a mixed batch of recordings.  Everything here is float64 NumPy and needs no GPU.

Definition of the resampler (the kernels, ``tests/resample_ref64.py`` and the header's comment restate it): a row of ``n`` samples
is zero outside its bounds; with ``h`` the prototype of ``resample_filter(up, down)``, centred on index 0,

    y[m] = sum_j x[j] * h[m * down - j * up],      0 <= m < resampled_length(n, up, down),

so output 0 sits on input 0 (no delay).  The filter is this project's own choice; the library takes any table of the same layout.
"""
from __future__ import annotations

from math import gcd
from typing import Dict, List, Sequence, Tuple

import numpy as np

# Chosen once against the two bars the tests measure on the prototype's FFT, for every pair of RATES: pass band
# (0 .. 0.85 x the lower Nyquist) ripple <= 0.01 dB, everything from 1.05 x the lower Nyquist up attenuated by >= 96 dB.
ZERO_CROSSINGS = 32   # of the sinc, per side
ROLLOFF = 0.95        # cut-off as a fraction of the lower Nyquist: the middle of the 0.85 .. 1.05 transition band
KAISER_BETA = 10.0    # Kaiser's estimate for 96 dB is 9.6; 10 leaves ~4 dB of margin
MAX_UP = 2048         # largest reduced interpolation factor the kernels take (GVX_RESAMPLE_MAX_UP)
MAX_DOWN = 2048       # largest reduced decimation factor (GVX_RESAMPLE_MAX_DOWN)
MAX_TAPS = 1024       # largest taps_per_phase
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000)


def resample_ratio(src: int, dst: int) -> Tuple[int, int]:
    """(up, down) of src -> dst, reduced by their gcd: dst / src = up / down."""
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError(f"sampling rates must be positive, got {src} -> {dst}")
    g = gcd(src, dst)
    return dst // g, src // g


def resampled_length(n: int, up: int, down: int) -> int:
    """Samples a row of n becomes: ceil(n * up / down)."""
    return -((-int(n) * int(up)) // int(down))


def check_ratio(up: int, down: int) -> None:
    if up < 1 or down < 1:
        raise ValueError(f"up = {up} and down = {down} must be positive")
    if up > MAX_UP or down > MAX_DOWN:
        raise ValueError(f"a rate pair that reduces to up = {up}, down = {down} is outside what the resampler takes "
                         f"(up <= {MAX_UP}, down <= {MAX_DOWN})")


def resample_filter(up: int, down: int, zero_crossings: int = ZERO_CROSSINGS, rolloff: float = ROLLOFF,
                    beta: float = KAISER_BETA) -> np.ndarray:
    """The float64 prototype low-pass at the rate ``src * up = dst * down``: 2 * half + 1 taps, centre at index ``half``.

    A sinc whose cut-off is ``rolloff`` x the lower of the two Nyquist frequencies, ``zero_crossings`` of it on each side, under a
    Kaiser window; scaled so that every polyphase branch has unit gain on average (a constant signal keeps its level)."""
    check_ratio(up, down)
    cutoff = rolloff / max(up, down)                 # in units of the high rate's Nyquist frequency
    half = int(np.ceil(zero_crossings / cutoff))
    t = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(cutoff * t) * np.kaiser(2 * half + 1, beta)
    return h * (up / h.sum())


def taps_per_phase(n_taps: int, up: int) -> int:
    """K of the polyphase table: ceil(n_taps / up) rounded up to a multiple of 4."""
    k = -(-int(n_taps) // int(up))
    return (k + 3) & ~3


def polyphase_table(h: np.ndarray, up: int, dtype=np.float32) -> np.ndarray:
    """``[up][K]`` table of the prototype ``h`` (odd length, centre in the middle) in the order the kernel reads: for output m with
    ``q, p = divmod(m * down, up)``, tap k of row p multiplies input sample ``q - (K / 2 - 1) + k``, which makes
    ``table[p][k] = h_centred[p + (K / 2 - 1 - k) * up]`` (0 outside the prototype)."""
    h = np.asarray(h, dtype=np.float64)
    if h.ndim != 1 or h.shape[0] % 2 != 1:
        raise ValueError("the prototype is a 1-D array of odd length (its centre tap in the middle)")
    half = h.shape[0] // 2
    K = taps_per_phase(h.shape[0], up)
    if K > MAX_TAPS:
        raise ValueError(f"{K} taps per phase are more than the resampler takes ({MAX_TAPS})")
    idx = np.arange(up)[:, None] + (K // 2 - 1 - np.arange(K))[None, :] * up     # centred prototype index
    inside = np.abs(idx) <= half
    table = np.where(inside, h[np.clip(idx + half, 0, 2 * half)], 0.0)
    return np.ascontiguousarray(table, dtype=dtype)


def prototype_from_table(table: np.ndarray, n_taps: int) -> np.ndarray:
    """Inverse of ``polyphase_table``: the table re-interleaved into the prototype of ``n_taps`` taps."""
    up, K = table.shape
    half = n_taps // 2
    t = np.arange(-half, half + 1)
    p = t % up
    k = K // 2 - 1 - (t - p) // up
    return table[p, k]


def plan_groups(keys: Sequence[Tuple]) -> List[Tuple[Tuple, List[int]]]:
    """Recordings described by hashable keys - ``(rate, channels, sample kind)`` - to the resampler's calls: one
    ``(key, indices)`` per distinct key, in order of first appearance, indices ascending.  ``scatter_groups`` undoes it."""
    groups: Dict[Tuple, List[int]] = {}
    for i, k in enumerate(keys):
        groups.setdefault(tuple(k), []).append(i)
    return list(groups.items())


def scatter_groups(groups: Sequence[Tuple[Tuple, List[int]]], per_group: Sequence[Sequence]) -> list:
    """Per-group result lists back into input order."""
    n = sum(len(idx) for _, idx in groups)
    out = [None] * n
    for (_, idx), vals in zip(groups, per_group):
        if len(vals) != len(idx):
            raise ValueError(f"a group of {len(idx)} recordings came back with {len(vals)} results")
        for i, v in zip(idx, vals):
            out[i] = v
    return out
