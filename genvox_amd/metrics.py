"""Evaluation by synthesis on the device: statistics of an attention alignment, the DTW mel-cepstral distance between a
free-running mel and its target, the monotonic alignment search that turns an alignment into frames per token, and the speaking
rate control built on those frame counts - the plan and the token-wise time warp of a mel (C ABI: gvx_alignment_stats,
gvx_mel_project, gvx_dtw_distance, gvx_monotonic_align, gvx_duration_scale, gvx_mel_time_warp; definitions in include/genvox_amd.h,
restatements in tests/metrics_ref64.py, tests/mas_ref.py and tests/warp_ref.py), the pitch tracker and the comparison of two contours
(gvx_pitch_yin, gvx_f0_compare; tests/pitch_ref64.py) and the pitch control built on the tracker's contour - the plan and the
overlap-add of a TD-PSOLA pitch shift (gvx_psola_plan, gvx_psola_synth; tests/psola_ref.py), and the multi-resolution STFT distance
between two waveforms (gvx_stft_loss, forward only; tests/stft_loss_ref64.py).

Every function takes and returns device tensors and enqueues on the current stream; none of them synchronises with the host
(stft_distance with device-side sample lengths does: the call reads them back to refuse a row that is too short).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

ROW_INT_NAMES = ("monotonic", "max_jump", "covered", "first_pos", "last_pos")   # GVX_ALIGN_* of include/genvox_amd.h, in order


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _need_gpu(t: torch.Tensor, what: str) -> torch.device:
    if t.device.type != "cuda":
        raise RuntimeError(f"genvox_amd.metrics: {what} must be a GPU tensor (there is no CPU path)")
    return t.device


def _lengths(lens: Optional[torch.Tensor], B: int, dev) -> Optional[torch.Tensor]:
    if lens is None:
        return None
    lens = lens.to(device=dev, dtype=torch.int32).contiguous()
    if lens.shape != (B,):
        raise ValueError(f"lengths of shape {tuple(lens.shape)} for a batch of {B} rows")
    return lens


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def alignment_stats(alignments: torch.Tensor, mel_lengths: Optional[torch.Tensor] = None,
                    token_lengths: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Per-row statistics of attention alignments [B, T, L] (what ``Tacotron2.inference`` / ``forward`` return), each row at
    its own ``mel_lengths[b]`` frames and ``token_lengths[b]`` tokens (None: all of them).

    Returns ``positions`` int32 [B, T] (the token each frame attends most, lowest index on a tie, -1 behind the row's frames),
    ``durations`` int32 [B, L] (frames per token), ``peaks`` fp32 [B, T], and per row: ``focus`` (mean peak weight),
    ``monotonic``, ``max_jump``, ``covered``, ``first_pos``, ``last_pos`` (int32), ``monotonic_fraction`` =
    monotonic / max(T_b - 1, 1) and ``coverage`` = covered / L_b (fp32; NaN for a row without tokens)."""
    dev = _need_gpu(alignments, "alignments")
    a = alignments.to(dtype=torch.float32).contiguous()
    if a.dim() != 3:
        raise ValueError(f"alignments must be [B, T, L], got {tuple(a.shape)}")
    B, T, L = a.shape
    ml, tl = _lengths(mel_lengths, B, dev), _lengths(token_lengths, B, dev)
    positions = torch.empty(B, T, dtype=torch.int32, device=dev)
    durations = torch.empty(B, L, dtype=torch.int32, device=dev)
    peaks = torch.empty(B, T, dtype=torch.float32, device=dev)
    ints = torch.empty(B, len(ROW_INT_NAMES), dtype=torch.int32, device=dev)
    focus = torch.empty(B, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().gvx_alignment_stats(a.data_ptr(), _ptr(ml), _ptr(tl), B, T, L, positions.data_ptr(), durations.data_ptr(),
                                               peaks.data_ptr(), ints.data_ptr(), focus.data_ptr(), _stream(dev)))
    out = {"positions": positions, "durations": durations, "peaks": peaks, "focus": focus}
    for i, name in enumerate(ROW_INT_NAMES):
        out[name] = ints[:, i]
    Tb = (ml.clamp(0, T) if ml is not None else torch.full((B,), T, dtype=torch.int32, device=dev)).to(torch.float32)
    Lb = (tl.clamp(0, L) if tl is not None else torch.full((B,), L, dtype=torch.int32, device=dev)).to(torch.float32)
    out["monotonic_fraction"] = out["monotonic"].to(torch.float32) / (Tb - 1).clamp(min=1)
    out["coverage"] = out["covered"].to(torch.float32) / Lb
    return out


MAS_STATUS_NAMES = ("ok", "empty", "infeasible")   # GVX_MAS_* of include/genvox_amd.h, in order

_mas_ws: Dict[str, torch.Tensor] = {}   # device -> the search's workspace, grown to the largest call seen


def _mas_workspace(need: int, dev) -> Optional[torch.Tensor]:
    if need == 0:
        return None
    ws = _mas_ws.get(str(dev))
    if ws is None or ws.numel() < need:
        ws = _mas_ws[str(dev)] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def monotonic_align(alignments: torch.Tensor, mel_lengths: Optional[torch.Tensor] = None, token_lengths: Optional[torch.Tensor] = None,
                    floor: float = 1e-8, want_scores: bool = False) -> Dict[str, torch.Tensor]:
    """Monotonic alignment search over alignments [B, T, L], each row at its own ``mel_lengths[b]`` frames and ``token_lengths[b]``
    tokens (None: all of them): the best path that starts on the first token, ends on the last and stays or advances by one token
    per frame, under the score log(max(a, floor)) (gvx_monotonic_align of include/genvox_amd.h; a tie stays).

    Returns ``path`` int32 [B, T] (the token of every frame, -1 behind the row's frames), ``durations`` int32 [B, L] (frames per
    token: >= 1 inside the row, summing to its frames, 0 behind its tokens), ``starts`` int32 [B, L] (first frame of every token,
    -1 behind), ``score`` fp32 [B] and ``status`` int32 [B] (index into ``MAS_STATUS_NAMES``: a row without frames or tokens is
    "empty", one with fewer frames than tokens "infeasible"; both have path -1, durations 0, starts -1, score NaN).  With
    ``want_scores`` also ``scores`` fp32 [B, T, L], the score table the search ran on (defined inside each row's lengths only).
    One launch; the workspace of long rows is kept and grown by size."""
    dev = _need_gpu(alignments, "alignments")
    a = alignments.to(dtype=torch.float32).contiguous()
    if a.dim() != 3:
        raise ValueError(f"alignments must be [B, T, L], got {tuple(a.shape)}")
    B, T, L = a.shape
    ml, tl = _lengths(mel_lengths, B, dev), _lengths(token_lengths, B, dev)
    lib = _lib.load()
    out = {"path": torch.empty(B, T, dtype=torch.int32, device=dev), "durations": torch.empty(B, L, dtype=torch.int32, device=dev),
           "starts": torch.empty(B, L, dtype=torch.int32, device=dev), "score": torch.empty(B, dtype=torch.float32, device=dev),
           "status": torch.empty(B, dtype=torch.int32, device=dev)}
    scores = torch.empty(B, T, L, dtype=torch.float32, device=dev) if want_scores else None
    ws = _mas_workspace(lib.gvx_monotonic_align_workspace_bytes(B, T, L), dev)
    _lib.check(lib.gvx_monotonic_align(a.data_ptr(), _ptr(ml), _ptr(tl), B, T, L, float(floor), out["path"].data_ptr(),
                                       out["durations"].data_ptr(), out["starts"].data_ptr(), out["score"].data_ptr(),
                                       out["status"].data_ptr(), _ptr(scores), _ptr(ws), 0 if ws is None else ws.numel(), _stream(dev)))
    if want_scores:
        out["scores"] = scores
    return out


WARP_STATUS_NAMES = ("ok", "empty", "bad", "cut")   # GVX_WARP_* of include/genvox_amd.h, in order


def _token_table(t: torch.Tensor, what: str, dev, dtype) -> torch.Tensor:
    t = t.to(device=dev, dtype=dtype).contiguous()
    if t.dim() != 2:
        raise ValueError(f"{what} must be [B, L], got {tuple(t.shape)}")
    return t


def scale_durations(durations: torch.Tensor, token_lengths: Optional[torch.Tensor] = None, speed: float = 1.0,
                    rates: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The plan of a change of speaking rate: durations int32 [B, L] (frames per token, as ``monotonic_align`` gives them) ->
    frames per token when token l is spoken ``speed * rates[b, l]`` times as fast (``rates`` fp32 [B, L]; None: all 1), each row at
    its own ``token_lengths[b]`` tokens (gvx_duration_scale of include/genvox_amd.h: the rounding error is carried from token to
    token, a spoken token keeps at least one frame).

    Returns ``durations`` int32 [B, L] (0 behind the row's tokens), ``starts`` int32 [B, L] (-1 behind), ``out_lengths`` int32 [B]
    (the row's new frame count) and ``status`` int32 [B] (index into ``WARP_STATUS_NAMES``: "empty" for a row without tokens or
    frames, "bad" for a negative duration, a ``speed * rate`` outside [0.125, 8] or not finite, or more than 32768 frames; both
    have durations 0, starts -1 and length 0).  One launch, no workspace."""
    dev = _need_gpu(durations, "durations")
    d = _token_table(durations, "durations", dev, torch.int32)
    B, L = d.shape
    tl = _lengths(token_lengths, B, dev)
    r = None
    if rates is not None:
        r = _token_table(rates, "rates", dev, torch.float32)
        if r.shape != d.shape:
            raise ValueError(f"rates of shape {tuple(r.shape)} for durations of shape {tuple(d.shape)}")
    out = {"durations": torch.empty(B, L, dtype=torch.int32, device=dev), "starts": torch.empty(B, L, dtype=torch.int32, device=dev),
           "out_lengths": torch.empty(B, dtype=torch.int32, device=dev), "status": torch.empty(B, dtype=torch.int32, device=dev)}
    _lib.check(_lib.load().gvx_duration_scale(d.data_ptr(), _ptr(tl), _ptr(r), B, L, float(speed), out["durations"].data_ptr(),
                                              out["starts"].data_ptr(), out["out_lengths"].data_ptr(), out["status"].data_ptr(), _stream(dev)))
    return out


def time_warp(mel: torch.Tensor, durations: torch.Tensor, target_durations: torch.Tensor, token_lengths: Optional[torch.Tensor] = None,
              T_out: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Token-wise time warp of mel fp32 [B, M, T]: token l of row b, ``durations[b, l]`` frames of the input, becomes
    ``target_durations[b, l]`` frames of the output, frame centres mapped linearly inside the token and the mel interpolated
    linearly between the two source frames (gvx_mel_time_warp of include/genvox_amd.h; equal tables return the input bits).

    ``T_out``: frames of the output; None reads the rows' new lengths once (the one host synchronisation of this function) and
    takes their maximum.  Returns ``mel`` fp32 [B, M, T_out] (zeros behind a row's new length), ``src_frame`` int32 [B, T_out] and
    ``src_frac`` fp32 [B, T_out] (the map: out[u] = x[src_frame[u]] + src_frac[u] * (x[src_frame[u] + 1] - x[src_frame[u]]); -1 and
    0 behind) and ``status`` int32 [B] (index into ``WARP_STATUS_NAMES``: "cut" for a row longer than ``T_out``, "bad" for tables
    that contradict each other or the mel; a "bad" or "empty" row comes out all zero).  One launch, no workspace."""
    dev = _need_gpu(mel, "mel")
    x = mel.to(dtype=torch.float32).contiguous()
    if x.dim() != 3:
        raise ValueError(f"mel must be [B, M, T], got {tuple(x.shape)}")
    B, M, T = x.shape
    d = _token_table(durations, "durations", dev, torch.int32)
    dp = _token_table(target_durations, "target_durations", dev, torch.int32)
    if d.shape != dp.shape or d.shape[0] != B:
        raise ValueError(f"durations {tuple(d.shape)} and target_durations {tuple(dp.shape)} for a batch of {B} rows")
    L = d.shape[1]
    tl = _lengths(token_lengths, B, dev)
    if T_out is None:
        inside = dp if tl is None else dp * (torch.arange(L, device=dev)[None, :] < tl[:, None])
        T_out = max(1, int(inside.to(torch.int64).sum(dim=1).max().item()))
    T_out = int(T_out)
    out = {"mel": torch.empty(B, M, T_out, dtype=torch.float32, device=dev), "src_frame": torch.empty(B, T_out, dtype=torch.int32, device=dev),
           "src_frac": torch.empty(B, T_out, dtype=torch.float32, device=dev), "status": torch.empty(B, dtype=torch.int32, device=dev)}
    _lib.check(_lib.load().gvx_mel_time_warp(x.data_ptr(), d.data_ptr(), dp.data_ptr(), _ptr(tl), B, M, T, L, T_out, out["mel"].data_ptr(),
                                             out["src_frame"].data_ptr(), out["src_frac"].data_ptr(), out["status"].data_ptr(), _stream(dev)))
    return out


F0_ROW_INT_NAMES = ("frames", "voiced_both", "voiced_one", "gross")   # GVX_F0_* of include/genvox_amd.h, in order


def pitch_params(sampling_rate: int, hop_length: int, fmin: float = 60.0, fmax: float = 500.0, window: int = 1024, threshold: float = 0.15,
                 first_centre: int = 0) -> "_lib.gvx_pitch_params":
    """The parameter block of ``pitch_track`` (host arithmetic, no GPU needed): ``lag_min = floor(sampling_rate / fmax)`` and
    ``lag_max = ceil(sampling_rate / fmin)`` - 44 and 368 at 22050 Hz with the defaults.  Whatever gvx_pitch_yin would refuse raises
    ValueError here, by name."""
    for name, v in (("sampling_rate", sampling_rate), ("hop_length", hop_length), ("window", window), ("first_centre", first_centre)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, not {v!r}")
    if sampling_rate < 1 or hop_length < 1:
        raise ValueError(f"sampling_rate = {sampling_rate} and hop_length = {hop_length} must be >= 1")
    if not (math.isfinite(fmin) and math.isfinite(fmax) and 0 < fmin < fmax):
        raise ValueError(f"0 < fmin < fmax is required, not fmin = {fmin!r}, fmax = {fmax!r}")
    lag_min, lag_max = int(math.floor(sampling_rate / fmax)), int(math.ceil(sampling_rate / fmin))
    if not 1 <= lag_min < lag_max <= 1024:
        raise ValueError(f"fmin = {fmin} and fmax = {fmax} at {sampling_rate} Hz are the lags {lag_min} .. {lag_max}: outside 1 <= lag_min < lag_max <= 1024")
    if not 32 <= window <= 2048:
        raise ValueError(f"window = {window} is outside [32, 2048]")
    if not 0.0 < threshold <= 1.0:
        raise ValueError(f"threshold = {threshold!r} is outside (0, 1]")
    if not -2 ** 31 <= first_centre < 2 ** 31:
        raise ValueError(f"first_centre = {first_centre} is not a 32-bit integer")
    return _lib.gvx_pitch_params(int(sampling_rate), int(hop_length), int(window), lag_min, lag_max, float(threshold), int(first_centre))


def pitch_frames(n_samples: int, hop_length: int) -> int:
    """Frames of a row of ``n_samples`` samples: ceil(n_samples / hop_length) (gvx_pitch_frames; host arithmetic)."""
    return int(_lib.load().gvx_pitch_frames(int(n_samples), int(hop_length)))


def pitch_track(wav: torch.Tensor, sample_lengths: Optional[torch.Tensor] = None, *, sampling_rate: int, hop_length: int,
                fmin: float = 60.0, fmax: float = 500.0, window: int = 1024, threshold: float = 0.15, first_centre: int = 0,
                want_table: bool = False) -> Dict[str, torch.Tensor]:
    """YIN F0 contours of waveforms [B, N] (float32, or float64, which is converted), each row at its own ``sample_lengths[b]``
    samples (None: all N): one decision per ``hop_length`` samples, frame f centred on sample ``first_centre + f * hop_length``
    (gvx_pitch_yin of include/genvox_amd.h: difference function over ``window`` terms, cumulative-mean normalisation, the first lag
    between ``sampling_rate / fmax`` and ``sampling_rate / fmin`` under ``threshold`` walked down to its local minimum, parabolic
    refinement; no smoothing).  ``first_centre`` puts the frames on another grid: ``-AudioProcessor.TRIM`` tracks a Griffin-Lim
    waveform on the frames of the mel it came from.

    Returns ``f0`` fp32 [B, F] (Hz; 0 = unvoiced and behind a row's frames), ``lag`` int32 [B, F] (-1 there), ``aperiodicity`` fp32
    [B, F] (the normalised difference at the lag, or its minimum over the search range for an unvoiced frame; 1 behind the row) and
    ``frames`` int32 [B] (ceil(samples / hop_length) per row); with ``want_table`` also ``cmnd`` fp32 [B, F, lag_max + 1], the table
    the decisions ran on (NaN behind a row's frames).  One launch, no workspace."""
    params = pitch_params(sampling_rate, hop_length, fmin, fmax, window, threshold, first_centre)
    dev = _need_gpu(wav, "wav")
    if wav.dim() != 2 or wav.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"wav must be float32 or float64 [B, N], got {wav.dtype} {tuple(wav.shape)}")
    x = wav.to(dtype=torch.float32).contiguous()
    B, N = x.shape
    sl = _lengths(sample_lengths, B, dev)
    lib = _lib.load()
    F = lib.gvx_pitch_frames(N, params.hop)
    out = {"f0": torch.empty(B, F, dtype=torch.float32, device=dev), "lag": torch.empty(B, F, dtype=torch.int32, device=dev),
           "aperiodicity": torch.empty(B, F, dtype=torch.float32, device=dev)}
    # the kernel writes the table of frames f < F_b only: what lies behind a row's frames is NaN, not whatever the allocator held
    table = torch.full((B, F, params.lag_max + 1), float("nan"), dtype=torch.float32, device=dev) if want_table else None
    _lib.check(lib.gvx_pitch_yin(x.data_ptr(), _ptr(sl), B, N, params, out["f0"].data_ptr(), out["lag"].data_ptr(),
                                 out["aperiodicity"].data_ptr(), _ptr(table), _stream(dev)))
    n = sl.clamp(0, N) if sl is not None else torch.full((B,), N, dtype=torch.int32, device=dev)
    out["frames"] = torch.div(n + (params.hop - 1), params.hop, rounding_mode="floor").to(torch.int32)
    if want_table:
        out["cmnd"] = table
    return out


def f0_compare(f0_a: torch.Tensor, f0_b: torch.Tensor, frames_a: Optional[torch.Tensor] = None,
               frames_b: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Two F0 contours [B, F] on the same frame grid (Hz, 0 = unvoiced, as ``pitch_track`` gives them), each row over the smaller of
    its two frame counts (None: all F): gvx_f0_compare of include/genvox_amd.h.

    Returns per row ``frames``, ``voiced_both``, ``voiced_one`` (voiced in exactly one contour), ``gross`` (voiced in both and more
    than 20 % apart) as int32 [B], and fp32 [B]: ``vde`` = voiced_one / frames, ``gpe`` = gross / voiced_both, ``rmse_cents`` = the
    root mean square of 1200 log2(a / b) over the frames voiced in both and not gross - NaN where a denominator is 0.  One launch."""
    dev = _need_gpu(f0_a, "f0_a")
    a, b = f0_a.to(dtype=torch.float32).contiguous(), f0_b.to(device=dev, dtype=torch.float32).contiguous()
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"contours {tuple(a.shape)} and {tuple(b.shape)} must both be [B, F]")
    B, F = a.shape
    na, nb = _lengths(frames_a, B, dev), _lengths(frames_b, B, dev)
    ints = torch.empty(B, len(F0_ROW_INT_NAMES), dtype=torch.int32, device=dev)
    out = {k: torch.empty(B, dtype=torch.float32, device=dev) for k in ("vde", "gpe", "rmse_cents")}
    _lib.check(_lib.load().gvx_f0_compare(a.data_ptr(), b.data_ptr(), _ptr(na), _ptr(nb), B, F, ints.data_ptr(), out["vde"].data_ptr(),
                                          out["gpe"].data_ptr(), out["rmse_cents"].data_ptr(), _stream(dev)))
    for i, name in enumerate(F0_ROW_INT_NAMES):
        out[name] = ints[:, i]
    return out


PSOLA_STATUS_NAMES = ("ok", "empty", "bad_ratio")   # GVX_PSOLA_* of include/genvox_amd.h, in order
PSOLA_RATIO_MIN, PSOLA_RATIO_MAX = 0.5, 2.0         # GVX_PSOLA_RATIO_MIN / GVX_PSOLA_RATIO_MAX


def psola_params(sampling_rate: int, hop_length: int, first_centre: int = 0, unvoiced_period: Optional[int] = None, fmin: float = 60.0,
                 fmax: float = 500.0) -> "_lib.gvx_psola_params":
    """The parameter block of ``psola_plan`` and ``pitch_shift`` (host arithmetic, no GPU needed): the frame grid and the lag range
    of ``pitch_params`` with the same arguments, and ``unvoiced_period`` - the spacing of marks where there is no pitch; None:
    ``sampling_rate // 100``, 10 ms.  Whatever the calls would refuse raises ValueError here."""
    p = pitch_params(sampling_rate, hop_length, fmin, fmax, first_centre=first_centre)
    U = sampling_rate // 100 if unvoiced_period is None else unvoiced_period
    if isinstance(U, bool) or not isinstance(U, (int, np.integer)) or not 1 <= U <= 1024:
        raise ValueError(f"unvoiced_period = {U!r} is not an integer in [1, 1024]")
    return _lib.gvx_psola_params(p.hop, p.first_centre, p.lag_min, p.lag_max, int(U))


def _psola_inputs(wav, sample_lengths, what: str):
    dev = _need_gpu(wav, what)
    if wav.dim() != 2 or wav.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what} must be float32 or float64 [B, N], got {wav.dtype} {tuple(wav.shape)}")
    x = wav.to(dtype=torch.float32).contiguous()
    return dev, x, _lengths(sample_lengths, x.shape[0], dev)


def psola_plan(wav: torch.Tensor, sample_lengths: Optional[torch.Tensor], lag: torch.Tensor, ratio: torch.Tensor, *, sampling_rate: int,
               hop_length: int, first_centre: int = 0, unvoiced_period: Optional[int] = None, fmin: float = 60.0,
               fmax: float = 500.0) -> Dict[str, torch.Tensor]:
    """The plan of a pitch shift of waveforms [B, N], each row at its own ``sample_lengths[b]`` samples (None: all N): the pitch
    marks of the input from its ``lag`` contour (int32 [B, F], what ``pitch_track`` returns for the same ``sampling_rate``,
    ``hop_length``, ``first_centre``, ``fmin`` and ``fmax``) and the places of the output's grains for ``ratio`` fp32 [B, F], the
    factor on the pitch per frame (gvx_psola_plan of include/genvox_amd.h; unvoiced frames are marked every ``unvoiced_period``
    samples and never repitched).

    Returns ``marks`` int32 [B, K], ``periods`` int32 [B, K] (negative: an unvoiced mark), ``syn_pos`` and ``syn_src`` int32 [B, J]
    (where grain j goes and which mark it copies), ``n_marks`` and ``n_grains`` int32 [B] - nothing behind them is written - and
    ``status`` int32 [B] (index into ``PSOLA_STATUS_NAMES``: "empty" for a row without samples, "bad_ratio" for a ratio inside the
    row's frames that is NaN or outside [0.5, 2]: such a row has marks and no grains).  One launch, no workspace."""
    params = psola_params(sampling_rate, hop_length, first_centre, unvoiced_period, fmin, fmax)
    dev, x, sl = _psola_inputs(wav, sample_lengths, "wav")
    B, N = x.shape
    lib = _lib.load()
    F = lib.gvx_pitch_frames(N, params.hop)
    lg = lag.to(device=dev, dtype=torch.int32).contiguous()
    rt = ratio.to(device=dev, dtype=torch.float32).contiguous()
    if lg.shape != (B, F) or rt.shape != (B, F):
        raise ValueError(f"lag {tuple(lg.shape)} and ratio {tuple(rt.shape)} must both be [{B}, {F}]: one value per frame of {hop_length} samples")
    p_min = min(params.lag_min, params.unvoiced_period)
    K, J = max(1, lib.gvx_psola_max_marks(N, p_min)), max(1, lib.gvx_psola_max_grains(N, p_min))
    out = {"marks": torch.empty(B, K, dtype=torch.int32, device=dev), "periods": torch.empty(B, K, dtype=torch.int32, device=dev),
           "syn_pos": torch.empty(B, J, dtype=torch.int32, device=dev), "syn_src": torch.empty(B, J, dtype=torch.int32, device=dev),
           "status": torch.empty(B, dtype=torch.int32, device=dev)}
    counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
    _lib.check(lib.gvx_psola_plan(x.data_ptr(), _ptr(sl), lg.data_ptr(), rt.data_ptr(), B, N, params, out["marks"].data_ptr(),
                                  out["periods"].data_ptr(), out["syn_pos"].data_ptr(), out["syn_src"].data_ptr(), counts.data_ptr(),
                                  out["status"].data_ptr(), _stream(dev)))
    out["counts"], out["n_marks"], out["n_grains"] = counts, counts[:, 0], counts[:, 1]
    return out


def pitch_shift(wav: torch.Tensor, sample_lengths: Optional[torch.Tensor], lag: torch.Tensor, ratio: torch.Tensor, *, sampling_rate: int,
                hop_length: int, first_centre: int = 0, unvoiced_period: Optional[int] = None, fmin: float = 60.0,
                fmax: float = 500.0) -> Dict[str, torch.Tensor]:
    """Waveforms [B, N] with their pitch multiplied by ``ratio`` fp32 [B, F], frame by frame, and their durations unchanged:
    ``psola_plan`` with the same arguments and the overlap-add of gvx_psola_synth (grains of two periods under a polynomial
    window, copied from the input's pitch marks to the output's; what lies before the first and behind the last mark is kept).

    Returns ``wav`` fp32 [B, N] (zeros behind a row's samples; a "bad_ratio" row is the input), ``status``, ``n_marks`` and
    ``n_grains`` int32 [B] as ``psola_plan`` gives them.  Two launches, no workspace, no synchronisation with the host."""
    plan = psola_plan(wav, sample_lengths, lag, ratio, sampling_rate=sampling_rate, hop_length=hop_length, first_centre=first_centre,
                      unvoiced_period=unvoiced_period, fmin=fmin, fmax=fmax)
    params = psola_params(sampling_rate, hop_length, first_centre, unvoiced_period, fmin, fmax)
    dev, x, sl = _psola_inputs(wav, sample_lengths, "wav")
    B, N = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.load().gvx_psola_synth(x.data_ptr(), _ptr(sl), plan["marks"].data_ptr(), plan["periods"].data_ptr(), plan["syn_pos"].data_ptr(),
                                           plan["syn_src"].data_ptr(), plan["counts"].data_ptr(), plan["status"].data_ptr(), B, N, params,
                                           y.data_ptr(), _stream(dev)))
    return {"wav": y, "status": plan["status"], "n_marks": plan["n_marks"], "n_grains": plan["n_grains"]}


def dct_rows(n_mels: int, n_cepstra: int) -> np.ndarray:
    """Rows 1 .. n_cepstra of the orthonormal DCT-II of size n_mels, float64 [n_cepstra, n_mels]:
    P[k][m] = sqrt(2 / M) cos(pi (k + 1) (2 m + 1) / (2 M)) - the mel cepstra without the energy term."""
    if not 1 <= n_cepstra <= n_mels - 1:
        raise ValueError(f"n_cepstra = {n_cepstra} is outside [1, n_mels - 1 = {n_mels - 1}]")
    k = np.arange(1, n_cepstra + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (2.0 * m + 1.0) / (2.0 * n_mels))


_dct_cache: Dict[Tuple[int, int, str], torch.Tensor] = {}


def _dct_on(dev, n_mels: int, n_cepstra: int) -> torch.Tensor:
    key = (n_mels, n_cepstra, str(dev))
    if key not in _dct_cache:
        _dct_cache[key] = torch.from_numpy(dct_rows(n_mels, n_cepstra).astype(np.float32)).to(dev)
    return _dct_cache[key]


def project(mel: torch.Tensor, P: torch.Tensor) -> torch.Tensor:
    """c[b, t, k] = sum_m P[k, m] * mel[b, m, t]: [B, M, T] -> [B, T, K] for any fp32 projection P [K, M], K <= M."""
    dev = _need_gpu(mel, "mel")
    mel = mel.to(dtype=torch.float32).contiguous()
    P = P.to(device=dev, dtype=torch.float32).contiguous()
    if mel.dim() != 3 or P.dim() != 2 or P.shape[1] != mel.shape[1]:
        raise ValueError(f"mel {tuple(mel.shape)} must be [B, M, T] and P {tuple(P.shape)} [K, M]")
    B, M, T = mel.shape
    out = torch.empty(B, T, P.shape[0], dtype=torch.float32, device=dev)
    _lib.check(_lib.load().gvx_mel_project(mel.data_ptr(), B, M, T, P.data_ptr(), P.shape[0], out.data_ptr(), _stream(dev)))
    return out


def mel_cepstra(mel: torch.Tensor, n_cepstra: int = 13) -> torch.Tensor:
    """Mel cepstra 1 .. n_cepstra of every frame of mel [B, n_mels, T] (log-mels, as the model produces them): fp32 [B, T, n_cepstra]."""
    return project(mel, _dct_on(_need_gpu(mel, "mel"), mel.shape[1], n_cepstra))


def dtw_distance(cp: torch.Tensor, cg: torch.Tensor, pred_lengths: Optional[torch.Tensor] = None,
                 target_lengths: Optional[torch.Tensor] = None, return_accumulated: bool = False):
    """The warp alone, on features cp [B, Tp, K] and cg [B, Tg, K]: fp32 [B] (NaN for a row without frames on either side); with
    ``return_accumulated`` also the accumulated-cost table [B, Tp, Tg] (defined inside each row's Tp_b x Tg_b rectangle only)."""
    dev = _need_gpu(cp, "cp")
    cp, cg = cp.to(dtype=torch.float32).contiguous(), cg.to(device=dev, dtype=torch.float32).contiguous()
    if cp.dim() != 3 or cg.dim() != 3 or cp.shape[0] != cg.shape[0] or cp.shape[2] != cg.shape[2]:
        raise ValueError(f"features {tuple(cp.shape)} and {tuple(cg.shape)} must be [B, Tp, K] and [B, Tg, K]")
    B, Tp, K = cp.shape
    Tg = cg.shape[1]
    pl, tl = _lengths(pred_lengths, B, dev), _lengths(target_lengths, B, dev)
    lib = _lib.load()
    dist = torch.empty(B, dtype=torch.float32, device=dev)
    acc = torch.empty(B, Tp, Tg, dtype=torch.float32, device=dev) if return_accumulated else None
    ws = torch.empty(lib.gvx_dtw_workspace_bytes(B, Tp, Tg, K), dtype=torch.uint8, device=dev)
    _lib.check(lib.gvx_dtw_distance(cp.data_ptr(), cg.data_ptr(), _ptr(pl), _ptr(tl), B, Tp, Tg, K, dist.data_ptr(), _ptr(acc),
                                    _ptr(ws), ws.numel(), _stream(dev)))
    return (dist, acc) if return_accumulated else dist


def dtw_mel_distance(mel_pred: torch.Tensor, mel_target: torch.Tensor, pred_lengths: Optional[torch.Tensor] = None,
                     target_lengths: Optional[torch.Tensor] = None, n_cepstra: int = 13, return_accumulated: bool = False):
    """DTW distance between the mel cepstra of mel_pred [B, M, Tp] and mel_target [B, M, Tg], each row at its own lengths:
    accumulated cost of the best symmetric warp over (Tp_b + Tg_b), in the mels' own log units (``mcd_db`` turns it into dB)."""
    return dtw_distance(mel_cepstra(mel_pred, n_cepstra), mel_cepstra(mel_target, n_cepstra), pred_lengths, target_lengths,
                        return_accumulated)


def mcd_db(dist: torch.Tensor, audio_config) -> torch.Tensor:
    """Mel-cepstral distortion in dB of a ``dtw_mel_distance``: (10 / ln 10) * sqrt(2) * s * dist, s = ln 10 for log10-mels
    (AudioConfig.log_func "np.log10") and 1 for natural-log mels."""
    s = math.log(10.0) if audio_config.log_func == "np.log10" else 1.0
    return dist * (10.0 / math.log(10.0) * math.sqrt(2.0) * s)


_stft_criteria: Dict[tuple, object] = {}


def stft_distance(wav_a: torch.Tensor, wav_b: torch.Tensor, sample_lengths=None, resolutions=None) -> Dict[str, torch.Tensor]:
    """Multi-resolution STFT distance of wav_a [B, n_max] from the reference wav_b, per row at its own length: {"spectral_convergence":
    [B], "log_magnitude": [B]}, each the mean over the resolutions (default: losses.DEFAULT_RESOLUTIONS) of the parts of
    losses.MultiResolutionSTFTLoss - ||M_b - M_a||_F / ||M_b||_F and mean |log M_b - log M_a|.  Forward only."""
    from .losses import DEFAULT_RESOLUTIONS, MultiResolutionSTFTLoss, check_resolutions

    res = check_resolutions(DEFAULT_RESOLUTIONS if resolutions is None else resolutions)
    crit = _stft_criteria.get(res)
    if crit is None:
        crit = _stft_criteria[res] = MultiResolutionSTFTLoss(res)
    with torch.no_grad():
        crit(wav_a, wav_b, sample_lengths)
    parts = crit.last_parts.mean(dim=1)
    return {"spectral_convergence": parts[:, 0], "log_magnitude": parts[:, 1]}


_mel_criteria: Dict[tuple, "torch.nn.Module"] = {}


def mel_distance(wav_a: torch.Tensor, wav_b: torch.Tensor, sample_lengths=None, **mel_args) -> torch.Tensor:
    """Log-mel L1 distance of wav_a [B, n_max] from the reference wav_b, per row at its own length: [B], the parts of
    losses.MelSpectrogramLoss(**mel_args) (default: HiFi-GAN's 22.05 kHz, 1024 / 256 / 1024, 80 mels up to Nyquist).  Forward only."""
    from .losses import MelSpectrogramLoss

    basis = mel_args.get("mel_basis")
    key = None if basis is not None else tuple(sorted(mel_args.items()))
    crit = _mel_criteria.get(key) if key is not None else None
    if crit is None:
        crit = MelSpectrogramLoss(**mel_args)
        if key is not None:
            _mel_criteria[key] = crit
    with torch.no_grad():
        crit(wav_a, wav_b, sample_lengths)
    return crit.last_parts
