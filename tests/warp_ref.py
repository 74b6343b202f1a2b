"""Restatements of gvx_duration_scale and gvx_mel_time_warp (include/genvox_amd.h) in numpy, for the tests of the device kernels.

The plan is written with Python integers and Python floats (IEEE double: one rounding per multiply, divide and add, `round` to
nearest with halves to even - what llrint does) exactly as the header states it.  The map is exact integers; frac takes the same two
roundings as the kernel (the double quotient, then its conversion to fp32).  The interpolation is float64.
"""
import math

import numpy as np

OK, EMPTY, BAD, CUT = 0, 1, 2, 3            # GVX_WARP_*
RATE_MIN, RATE_MAX = 0.125, 8.0             # GVX_RATE_MIN / GVX_RATE_MAX
MAX_FRAMES, MAX_TOKENS = 32768, 4096        # GVX_MAS_MAX_FRAMES / GVX_MAS_MAX_TOKENS
TILE = 64                                   # GVX_WARP_TILE_FRAMES


def _len(lens, b, full):
    return full if lens is None else max(0, min(int(lens[b]), full))


def plan_row(d, speed, rates=None):
    """One row inside its tokens: (status, d' list, S' list, T').  `speed` and `rates` are taken through fp32, as the call takes them."""
    Lb = len(d)
    if Lb == 0:
        return EMPTY, [], [], 0
    sp = float(np.float32(speed))
    q = []
    for l in range(Lb):
        e = sp * (1.0 if rates is None else float(np.float32(rates[l])))
        if int(d[l]) < 0 or not (RATE_MIN <= e <= RATE_MAX):      # a NaN fails the comparison
            return BAD, [0] * Lb, [-1] * Lb, 0
        q.append(float(int(d[l])) / e)
    E, S, starts = 0.0, 0, []
    for l in range(Lb):
        E = E + q[l]
        c = round(E)                                               # Python's round: half to even, exact integer
        starts.append(S)
        S = max(S + (1 if int(d[l]) > 0 else 0), c)
    if S == 0:
        return EMPTY, [0] * Lb, [-1] * Lb, 0
    if S > MAX_FRAMES:
        return BAD, [0] * Lb, [-1] * Lb, 0
    ends = starts[1:] + [S]
    return OK, [b - a for a, b in zip(starts, ends)], starts, S


def duration_scale(durations, token_lengths=None, speed=1.0, rates=None):
    """durations int [B, L] -> dict of durations, starts (int32 [B, L]), out_lengths, status (int32 [B])."""
    durations = np.asarray(durations)
    B, L = durations.shape
    out = {"durations": np.zeros((B, L), np.int32), "starts": np.full((B, L), -1, np.int32),
           "out_lengths": np.zeros(B, np.int32), "status": np.zeros(B, np.int32)}
    for b in range(B):
        Lb = _len(token_lengths, b, L)
        st, dp, sp, Tp = plan_row(durations[b, :Lb].tolist(), speed, None if rates is None else np.asarray(rates)[b, :Lb])
        out["status"][b], out["out_lengths"][b] = st, Tp
        out["durations"][b, :Lb], out["starts"][b, :Lb] = dp, sp
    return out


def frame_map(d, dp, u):
    """Output frame u of a row with source counts d and target counts dp (Python ints, inside the row, consistent): (i0, frac as
    np.float32), clamped as the header says."""
    S = Sp = 0
    for l in range(len(d)):
        if Sp <= u < Sp + dp[l]:
            break
        S, Sp = S + d[l], Sp + dp[l]
    else:
        raise ValueError(f"frame {u} lies behind the row")
    j = u - Sp
    n = (2 * j + 1) * d[l] - dp[l]
    den = 2 * dp[l]
    i0 = S + n // den                               # Python's // and % are floor and its remainder
    rem = n % den
    frac = np.float32(float(rem) / float(den))
    Tb = sum(d)
    if i0 < 0:
        i0, frac = 0, np.float32(0.0)
    if i0 >= Tb - 1:
        i0, frac = Tb - 1, np.float32(0.0)
    return i0, frac


def warp_status(d, dp, T, T_out):
    """Status of one row inside its tokens, and the number of frames computed."""
    d, dp = [int(v) for v in d], [int(v) for v in dp]
    if any(v < 0 for v in d) or any(v < 0 for v in dp) or any((a > 0) != (b > 0) for a, b in zip(d, dp)) or sum(d) > T:
        return BAD, 0
    if len(d) == 0 or sum(dp) == 0:
        return EMPTY, 0
    if sum(dp) > T_out:
        return CUT, T_out
    return OK, sum(dp)


def mel_time_warp(mel, durations, target_durations, token_lengths=None, T_out=None):
    """mel [B, M, T] -> dict of mel float64 [B, M, T_out], src_frame int32 [B, T_out], src_frac fp32 [B, T_out], status int32 [B].
    The interpolation is x0 + frac * (x1 - x0) in float64 with the fp32 frac; x1 is not looked at where frac == 0."""
    mel = np.asarray(mel)
    durations, target_durations = np.asarray(durations), np.asarray(target_durations)
    B, M, T = mel.shape
    L = durations.shape[1]
    out = {"mel": np.zeros((B, M, T_out), np.float64), "src_frame": np.full((B, T_out), -1, np.int32),
           "src_frac": np.zeros((B, T_out), np.float32), "status": np.zeros(B, np.int32)}
    for b in range(B):
        Lb = _len(token_lengths, b, L)
        d, dp = durations[b, :Lb].tolist(), target_durations[b, :Lb].tolist()
        st, n = warp_status(d, dp, T, T_out)
        out["status"][b] = st
        for u in range(n):
            i0, frac = frame_map(d, dp, u)
            out["src_frame"][b, u], out["src_frac"][b, u] = i0, frac
            x0 = mel[b, :, i0].astype(np.float64)
            out["mel"][b, :, u] = x0 if frac == 0 else x0 + float(frac) * (mel[b, :, i0 + 1].astype(np.float64) - x0)
    return out


def interp_bound(x0, x1, frac):
    """The derived bound on |device - float64| of fmaf(frac, x1 - x0, x0) with the device's own fp32 frac: the subtraction rounds once
    (half an fp32 ulp of |x1 - x0|, scaled by frac <= 1 - taken as 1) and the fused multiply-add rounds once (half an ulp of the
    result; the ulp is taken at |float64 value| + the first term, which is where the unrounded result can lie, so that a value next
    to a power of two is given the binade it may round in).  Exactly 0 where frac == 0: the kernel returns x0 itself."""
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    want = x0 + np.asarray(frac, np.float64) * (x1 - x0)
    half_ulp = lambda v: 0.5 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    first = half_ulp(x1 - x0)
    return np.where(np.asarray(frac) == 0, 0.0, first + half_ulp(np.abs(want) + first))
