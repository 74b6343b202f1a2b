"""The evaluation metrics of include/genvox_amd.h (alignment statistics, projection, DTW distance) in float64 NumPy, cell by cell and
without cleverness: what the GPU tests hold the kernels to."""
import math

import numpy as np


def _clamp(v, hi):
    return max(0, min(int(v), hi))


def alignment_stats(a, mel_lengths=None, token_lengths=None):
    """a [B, T, L] (any float dtype; the values are compared, never combined, except in focus) -> dict of arrays."""
    a = np.asarray(a)
    B, T, L = a.shape
    out = {"positions": np.full((B, T), -1, np.int32), "durations": np.zeros((B, L), np.int32), "peaks": np.zeros((B, T), np.float64),
           "focus": np.full(B, np.nan), "monotonic": np.zeros(B, np.int32), "max_jump": np.zeros(B, np.int32),
           "covered": np.zeros(B, np.int32), "first_pos": np.zeros(B, np.int32), "last_pos": np.zeros(B, np.int32),
           "monotonic_fraction": np.zeros(B), "coverage": np.full(B, np.nan)}
    for b in range(B):
        Tb = T if mel_lengths is None else _clamp(mel_lengths[b], T)
        Lb = L if token_lengths is None else _clamp(token_lengths[b], L)
        if Lb > 0:
            out["coverage"][b] = 0.0
        if Tb == 0 or Lb == 0:
            continue
        pos = np.zeros(Tb, np.int64)
        peak = np.zeros(Tb, np.float64)
        for t in range(Tb):
            best, where = None, 0
            for l in range(Lb):
                v = float(a[b, t, l])
                if math.isnan(v):
                    continue
                if best is None or v > best:   # strictly greater: a tie stays with the lowest index
                    best, where = v, l
            pos[t] = where
            peak[t] = math.nan if best is None else best
        out["positions"][b, :Tb] = pos
        out["peaks"][b, :Tb] = peak
        for t in range(Tb):
            out["durations"][b, pos[t]] += 1
        out["focus"][b] = peak.sum() / Tb
        steps = pos[1:] - pos[:-1]
        out["monotonic"][b] = int((steps >= 0).sum())
        out["max_jump"][b] = int(np.abs(steps).max()) if Tb > 1 else 0
        out["covered"][b] = int((out["durations"][b, :Lb] > 0).sum())
        out["first_pos"][b], out["last_pos"][b] = pos[0], pos[-1]
        out["monotonic_fraction"][b] = out["monotonic"][b] / max(Tb - 1, 1)
        out["coverage"][b] = out["covered"][b] / Lb
    return out


def dct_rows(M, K):
    """Rows 1 .. K of the orthonormal DCT-II of size M."""
    P = np.zeros((K, M))
    for k in range(K):
        for m in range(M):
            P[k, m] = math.sqrt(2.0 / M) * math.cos(math.pi * (k + 1) * (2 * m + 1) / (2.0 * M))
    return P


def project(mel, P):
    """mel [B, M, T], P [K, M] -> c [B, T, K] = sum_m P[k, m] mel[b, m, t]."""
    return np.einsum("km,bmt->btk", np.asarray(P, np.float64), np.asarray(mel, np.float64))


def dtw_accumulated(cp, cg):
    """One row: cp [Tp, K], cg [Tg, K] -> A [Tp, Tg] of the symmetric step pattern."""
    cp, cg = np.asarray(cp, np.float64), np.asarray(cg, np.float64)
    Tp, Tg = cp.shape[0], cg.shape[0]
    d = np.stack([np.sqrt(((cp[i][None, :] - cg) ** 2).sum(-1)) for i in range(Tp)])
    A = np.zeros((Tp, Tg))
    for i in range(Tp):
        for j in range(Tg):
            if i == 0 and j == 0:
                A[i, j] = 2.0 * d[0, 0]
            elif j == 0:
                A[i, j] = A[i - 1, 0] + d[i, 0]
            elif i == 0:
                A[i, j] = A[0, j - 1] + d[0, j]
            else:
                A[i, j] = min(A[i - 1, j] + d[i, j], A[i, j - 1] + d[i, j], A[i - 1, j - 1] + 2.0 * d[i, j])
    return A


def dtw_distance_row(cp, cg):
    cp, cg = np.asarray(cp, np.float64), np.asarray(cg, np.float64)
    Tp, Tg = cp.shape[0], cg.shape[0]
    if Tp == 0 or Tg == 0:
        return math.nan
    return dtw_accumulated(cp, cg)[-1, -1] / (Tp + Tg)


def dtw_distance(cp, cg, pred_lengths=None, target_lengths=None):
    """cp [B, Tp, K], cg [B, Tg, K] -> dist [B], every row at its own (clamped) lengths."""
    B, Tp, Tg = cp.shape[0], cp.shape[1], cg.shape[1]
    out = np.zeros(B)
    for b in range(B):
        p = Tp if pred_lengths is None else _clamp(pred_lengths[b], Tp)
        g = Tg if target_lengths is None else _clamp(target_lengths[b], Tg)
        out[b] = dtw_distance_row(cp[b, :p], cg[b, :g])
    return out


def mcd_db(dist, log10_mels):
    return (10.0 / math.log(10.0)) * math.sqrt(2.0) * (math.log(10.0) if log10_mels else 1.0) * np.asarray(dist, np.float64)
