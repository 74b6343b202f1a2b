"""Restatements of gvx_monotonic_align (include/genvox_amd.h) in numpy, for the tests of the device kernel.

(a) align_f32: the recurrence in np.float32 from a GIVEN score table.  fp32 addition is correctly rounded on both sides, max is
    exact and the library is built with -ffp-contract=off, so this reproduces the device bit for bit: path, durations, starts,
    status and the bits of the score.
(b) align_f64: scores log(max(a, floor)) and the recurrence in float64 - what the numbers mean, free of the device's roundings.

Both stay on a tie, read the path back from (T_b - 1, L_b - 1) and treat a cell no path from (0, 0) reaches (l > t) as -inf.
brute_force enumerates every monotone path of a small table.
"""
import itertools

import numpy as np

OK, EMPTY, INFEASIBLE = 0, 1, 2


def _clamp(v, hi):
    return max(0, min(int(v), hi))


def align_row(s, dtype):
    """s [T_b, L_b] scores of one row -> (path [T_b], durations [L_b], starts [L_b], score, status), arithmetic in `dtype`."""
    Tb, Lb = s.shape
    if Tb == 0 or Lb == 0:
        return None, None, None, np.nan, EMPTY
    if Tb < Lb:
        return None, None, None, np.nan, INFEASIBLE
    s = s.astype(dtype)
    ninf = dtype(-np.inf)
    q = np.full(Lb, ninf, dtype)
    q[0] = s[0, 0]
    advance = np.zeros((Tb, Lb), bool)
    for t in range(1, Tb):
        hi = min(t, Lb - 1)                                   # cells l <= t are reachable
        stay = q[:hi + 1].copy()
        if hi == t:
            stay[t] = ninf                                    # (t - 1, t) is not reachable
        up = np.concatenate([[ninf], q[:hi]]).astype(dtype)
        adv = up > stay                                       # a tie stays
        advance[t, :hi + 1] = adv
        q = q.copy()
        q[:hi + 1] = s[t, :hi + 1] + np.where(adv, up, stay)  # one correctly rounded add per cell
    path = np.empty(Tb, np.int32)
    starts = np.zeros(Lb, np.int32)
    l = Lb - 1
    for t in range(Tb - 1, -1, -1):
        path[t] = l
        if advance[t, l]:
            starts[l] = t
            l -= 1
    assert l == 0
    durations = np.diff(np.concatenate([starts, [Tb]])).astype(np.int32)
    return path, durations, starts, q[Lb - 1], OK


def _batch(tables, mel_lengths, token_lengths, dtype):
    B, T, L = tables.shape
    out = {"path": np.full((B, T), -1, np.int32), "durations": np.zeros((B, L), np.int32), "starts": np.full((B, L), -1, np.int32),
           "score": np.full(B, np.nan, dtype), "status": np.zeros(B, np.int32)}
    for b in range(B):
        Tb = T if mel_lengths is None else _clamp(mel_lengths[b], T)
        Lb = L if token_lengths is None else _clamp(token_lengths[b], L)
        path, dur, st, score, status = align_row(tables[b, :Tb, :Lb], dtype)
        out["status"][b] = status
        if status == OK:
            out["path"][b, :Tb], out["durations"][b, :Lb], out["starts"][b, :Lb], out["score"][b] = path, dur, st, score
    return out


def align_f32(scores, mel_lengths=None, token_lengths=None):
    """(a): scores fp32 [B, T, L] (the device's scores_out; what lies behind a row's lengths is not looked at)."""
    return _batch(np.asarray(scores, np.float32), mel_lengths, token_lengths, np.float32)


def scores_f64(alignments, floor):
    a = np.asarray(alignments, np.float64)
    return np.log(np.where(a > floor, a, np.float64(floor)))   # fmaxf passes over a NaN: NaN > floor is false


def align_f64(alignments, floor, mel_lengths=None, token_lengths=None):
    """(b): alignments [B, T, L] (fp32 values, taken exactly) and the floor as the device sees it (np.float32(floor))."""
    floor = np.float64(np.float32(floor))
    a = np.asarray(alignments)
    B, T, L = a.shape
    s = np.zeros((B, T, L), np.float64)
    for b in range(B):   # row by row, inside the lengths only: poison behind them never reaches a log
        Tb = T if mel_lengths is None else _clamp(mel_lengths[b], T)
        Lb = L if token_lengths is None else _clamp(token_lengths[b], L)
        s[b, :Tb, :Lb] = scores_f64(a[b, :Tb, :Lb], floor)
    return _batch(s, mel_lengths, token_lengths, np.float64)


def brute_force(s):
    """Every monotone path of s [T, L] (T >= L): (best sum in s's dtype, added frame by frame in path order; the set of best paths)."""
    T, L = s.shape
    best, arg = None, []
    for ups in itertools.combinations(range(1, T), L - 1):   # the frames at which the path advances
        path = np.zeros(T, np.int32)
        for t in ups:
            path[t:] += 1
        total = s[0, 0]
        for t in range(1, T):
            total = total + s[t, path[t]]
        if best is None or total > best:
            best, arg = total, [path]
        elif total == best:
            arg.append(path)
    return best, arg
