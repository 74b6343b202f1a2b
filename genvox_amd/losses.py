"""Training losses for the neural vocoder, on the device.

MultiResolutionSTFTLoss is the non-adversarial objective a waveform generator is trained on - spectral convergence plus log-magnitude
L1 over several STFT resolutions - as one call of gvx_stft_loss (definition in include/genvox_amd.h, restatement in
tests/stft_loss_ref64.py) that returns the value and, when pred asks for it, the gradient:

    criterion = MultiResolutionSTFTLoss()
    loss = criterion(vocoder.vocode_with_grad(mel, mel_lengths), recording, sample_lengths)
    loss.backward()

The norms and means are per row (a row's numbers never depend on the rows beside it), not over the batch as Parallel WaveGAN has them.

MelSpectrogramLoss is HiFi-GAN's spectral term - the L1 distance between the log-mel spectrograms of the two waveforms, the published
mel_spectrogram + F.l1_loss - as one call of gvx_mel_loss (restatement in tests/mel_loss_ref64.py), with the same per-row mean:

    trainer = HiFiGANTrainer(generator, discriminators, aux_loss=MelSpectrogramLoss())   # aux_weight = 45 is this term's published weight
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

DEFAULT_RESOLUTIONS: Tuple[Tuple[int, int, int], ...] = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))   # Parallel WaveGAN's
SUPPORTED_N_FFT = (512, 1024, 2048)
MAX_RESOLUTIONS = 8


def check_resolutions(resolutions: Sequence[Sequence[int]]) -> Tuple[Tuple[int, int, int], ...]:
    res = tuple(tuple(int(v) for v in r) for r in resolutions)
    if not 1 <= len(res) <= MAX_RESOLUTIONS:
        raise ValueError(f"{len(res)} resolutions: 1 .. {MAX_RESOLUTIONS} are supported")
    for r in res:
        if len(r) != 3:
            raise ValueError(f"a resolution is (n_fft, hop, win_length), got {r}")
        n_fft, hop, win_length = r
        if n_fft not in SUPPORTED_N_FFT:
            raise ValueError(f"n_fft = {n_fft}: supported are {SUPPORTED_N_FFT}")
        if not 1 <= hop <= n_fft or not 2 <= win_length <= n_fft:
            raise ValueError(f"resolution {r}: 1 <= hop <= n_fft and 2 <= win_length <= n_fft are required")
    return res


class _STFTLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, lens_dev, module, want_grad):
        loss, parts, d_pred = module._call(pred, target, lens_dev, want_grad)
        module.last_parts = parts
        ctx.d_pred, ctx.name = d_pred, type(module).__name__
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        if ctx.d_pred is None:
            raise RuntimeError(f"{ctx.name}: no gradient was kept for this call")
        return grad_output * ctx.d_pred, None, None, None, None


class _WaveformLoss(torch.nn.Module):
    """What the two waveform losses share: the plan's ownership, the checks before anything is launched, and forward through
    _STFTLossFunction.  A subclass sets ``min_samples`` and ``_min_rule`` (how that number comes about, for the message), names the
    C ABI's destroy function in ``_destroy`` and gives ``_call(pred, target, lens_dev, want_grad) -> (loss, parts, d_pred)``."""

    _destroy = ""
    _min_rule = ""

    def __init__(self):
        super().__init__()
        self.last_parts: Optional[torch.Tensor] = None
        self._handle = None
        self._workspace: Optional[torch.Tensor] = None

    def __del__(self):
        try:
            if self._handle is not None:
                getattr(_lib.load(), self._destroy)(self._handle)
        except Exception:
            pass

    def __getstate__(self):   # a copy makes its own plan: the handle is destroyed once, by its owner
        state = dict(self.__dict__)
        state.update(_handle=None, _workspace=None, last_parts=None)
        return state

    # ---- checks, all before anything is launched
    def _require_gpu(self, pred: torch.Tensor) -> torch.device:
        if pred.device.type != "cuda":
            raise RuntimeError(f"genvox_amd.{type(self).__name__} runs on an MI355X only: pass tensors on 'cuda:0'. There is no CPU fallback.")
        return pred.device

    def _check(self, pred, target, sample_lengths):
        if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise ValueError("pred and target must be tensors")
        if pred.dim() != 2 or pred.shape != target.shape:
            raise ValueError(f"pred and target must both be [B, n_max], got {tuple(pred.shape)} and {tuple(target.shape)}")
        if pred.dtype != torch.float32 or target.dtype != torch.float32:
            raise ValueError(f"pred and target must be float32, got {pred.dtype} and {target.dtype}")
        B, n_max = pred.shape
        if B < 1 or n_max < self.min_samples:
            raise ValueError(f"a row needs at least {self._min_rule.format(self.min_samples)}, got [B, n_max] = [{B}, {n_max}]")
        host = None
        on_device = isinstance(sample_lengths, torch.Tensor) and sample_lengths.device.type == "cuda"
        if sample_lengths is not None and not on_device:   # lengths the host has: refused here, with the row named
            host = [int(v) for v in (sample_lengths.tolist() if isinstance(sample_lengths, torch.Tensor) else sample_lengths)]
            if len(host) != B:
                raise ValueError(f"{len(host)} sample lengths for a batch of {B} rows")
            for b, n in enumerate(host):
                if not self.min_samples <= n <= n_max:
                    raise ValueError(f"row {b} has {n} samples: outside [{self.min_samples}, n_max = {n_max}]")
        elif on_device and sample_lengths.shape != (B,):
            raise ValueError(f"sample lengths of shape {tuple(sample_lengths.shape)} for a batch of {B} rows")
        dev = self._require_gpu(pred)
        if target.device != dev:
            raise ValueError(f"pred is on {dev}, target on {target.device}")
        if sample_lengths is None:
            return dev, None
        if host is not None:
            return dev, torch.tensor(host, dtype=torch.int32, device=dev)
        return dev, sample_lengths.to(device=dev, dtype=torch.int32).contiguous()   # checked by the call itself (GvxError naming the row)

    def forward(self, pred: torch.Tensor, target: torch.Tensor, sample_lengths=None) -> torch.Tensor:
        _, lens_dev = self._check(pred, target, sample_lengths)
        want_grad = pred.requires_grad and torch.is_grad_enabled()
        return _STFTLossFunction.apply(pred, target, lens_dev, self, want_grad)


class MultiResolutionSTFTLoss(_WaveformLoss):
    """loss = mean over rows and resolutions of (w_sc * spectral convergence + w_mag * log-magnitude L1).  No parameters.

    forward(pred, target, sample_lengths=None): float32 [B, n_max] device tensors; returns a 0-d float32 device tensor.  `last_parts`
    holds [B, R, 2] = (spectral convergence, log magnitude) of the last call.  target gets no gradient."""

    _destroy = "gvx_stft_loss_destroy"
    _min_rule = "n_fft / 2 + 1 = {} samples for the reflection"

    def __init__(self, resolutions: Sequence[Sequence[int]] = DEFAULT_RESOLUTIONS, w_sc: float = 1.0, w_mag: float = 1.0, eps: float = 1e-7):
        super().__init__()
        self.resolutions = check_resolutions(resolutions)
        if not (w_sc >= 0.0 and w_mag >= 0.0) or w_sc == float("inf") or w_mag == float("inf"):
            raise ValueError("w_sc and w_mag must be finite and >= 0")
        if not 0.0 < eps < float("inf"):
            raise ValueError("eps must be finite and > 0")
        self.w_sc, self.w_mag, self.eps = float(w_sc), float(w_mag), float(eps)
        self.min_samples = max(r[0] for r in self.resolutions) // 2 + 1

    # ---- the call
    def _plan(self):
        if self._handle is None:
            table = (_lib.gvx_stft_resolution * len(self.resolutions))(*[_lib.gvx_stft_resolution(*r) for r in self.resolutions])
            h = C.c_void_p()
            _lib.check(_lib.load().gvx_stft_loss_create(table, len(self.resolutions), self.w_sc, self.w_mag, self.eps, C.byref(h)))
            self._handle = h.value
        return self._handle

    def _call(self, pred, target, lens_dev, want_grad):
        lib = _lib.load()
        dev = pred.device
        B, n_max = pred.shape
        with torch.cuda.device(dev):
            plan = self._plan()
            need = lib.gvx_stft_loss_workspace_bytes(plan, B, n_max)
            if need == 0:
                _lib.check(-1)
            if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            pred, target = pred.detach().contiguous(), target.detach().contiguous()
            loss = torch.empty((), dtype=torch.float32, device=dev)
            parts = torch.empty(B, len(self.resolutions), 2, dtype=torch.float32, device=dev)
            d_pred = torch.empty_like(pred) if want_grad else None
            _lib.check(lib.gvx_stft_loss(plan, pred.data_ptr(), target.data_ptr(), None if lens_dev is None else lens_dev.data_ptr(), B, n_max,
                                         loss.data_ptr(), parts.data_ptr(), None if d_pred is None else d_pred.data_ptr(), None,
                                         self._workspace.data_ptr(), self._workspace.numel(), torch.cuda.current_stream(dev).cuda_stream))
        return loss, parts, d_pred


MAX_MELS = 128   # GVX_MEL_LOSS_MAX_MELS


class MelSpectrogramLoss(_WaveformLoss):
    """loss = mean over rows of the row's mean |log mel(target) - log mel(pred)| over its own n_b // hop_length frames and n_mels bands:
    HiFi-GAN's mel_spectrogram (reflect padding by (n_fft - hop_length) / 2, center=False, sqrt(re^2 + im^2 + mag_eps), the mel basis,
    log(max(., clamp))) and F.l1_loss, per row.  No parameters.  Without ``mel_basis`` ([n_mels, n_fft / 2 + 1]) the basis is
    audio.get_mel_filter's Slaney filterbank from ``fmin`` to ``fmax`` (None: Nyquist, the published ``fmax_for_loss: null``).

    forward(pred, target, sample_lengths=None): float32 [B, n_max] device tensors; returns a 0-d float32 device tensor.  `last_parts`
    holds [B], the rows' means of the last call.  target gets no gradient."""

    _destroy = "gvx_mel_loss_destroy"
    _min_rule = "max(hop_length, (n_fft - hop_length) / 2 + 1) = {} samples"

    def __init__(self, sampling_rate: int = 22050, n_fft: int = 1024, hop_length: int = 256, win_length: int = 1024, n_mels: int = 80,
                 fmin: float = 0.0, fmax: Optional[float] = None, clamp: float = 1e-5, mag_eps: float = 1e-9, mel_basis=None):
        super().__init__()
        n_fft, hop_length, win_length, n_mels = int(n_fft), int(hop_length), int(win_length), int(n_mels)
        if n_fft not in SUPPORTED_N_FFT:
            raise ValueError(f"n_fft = {n_fft}: supported are {SUPPORTED_N_FFT}")
        if not 1 <= hop_length <= n_fft or (n_fft - hop_length) % 2:
            raise ValueError(f"hop_length = {hop_length}: 1 <= hop_length <= n_fft = {n_fft} with n_fft - hop_length even is required")
        if not 2 <= win_length <= n_fft:
            raise ValueError(f"win_length = {win_length}: 2 <= win_length <= n_fft = {n_fft} is required")
        if not 1 <= n_mels <= MAX_MELS:
            raise ValueError(f"n_mels = {n_mels}: 1 .. {MAX_MELS} are supported")
        if not 0.0 < clamp < float("inf") or not 0.0 < mag_eps < float("inf"):
            raise ValueError("clamp and mag_eps must be finite and > 0")
        if mel_basis is None:
            from .audio import get_mel_filter
            top = sampling_rate / 2.0 if fmax is None else float(fmax)
            if not 0.0 <= fmin < top <= sampling_rate / 2.0:
                raise ValueError(f"0 <= fmin < fmax <= sampling_rate / 2 is required, got fmin = {fmin}, fmax = {top}")
            basis = get_mel_filter(int(sampling_rate), n_fft, n_mels, float(fmin), top)
        else:
            basis = mel_basis.detach().cpu().numpy() if isinstance(mel_basis, torch.Tensor) else np.asarray(mel_basis)
        basis = np.ascontiguousarray(basis, dtype=np.float32)
        if basis.shape != (n_mels, n_fft // 2 + 1) or not np.isfinite(basis).all():
            raise ValueError(f"mel_basis must be a finite [n_mels, n_fft / 2 + 1] = [{n_mels}, {n_fft // 2 + 1}] matrix, got {basis.shape}")
        self.sampling_rate, self.n_fft, self.hop_length, self.win_length, self.n_mels = int(sampling_rate), n_fft, hop_length, win_length, n_mels
        self.clamp, self.mag_eps = float(clamp), float(mag_eps)
        self.mel_basis = basis
        self.pad = (n_fft - hop_length) // 2
        self.min_samples = max(hop_length, self.pad + 1)

    def _plan(self):
        if self._handle is None:
            h = C.c_void_p()
            _lib.check(_lib.load().gvx_mel_loss_create(self.n_fft, self.hop_length, self.win_length, self.n_mels, self.mel_basis.ctypes.data,
                                                       self.clamp, self.mag_eps, C.byref(h)))
            self._handle = h.value
        return self._handle

    def _call(self, pred, target, lens_dev, want_grad):
        lib = _lib.load()
        dev = pred.device
        B, n_max = pred.shape
        with torch.cuda.device(dev):
            plan = self._plan()
            need = lib.gvx_mel_loss_workspace_bytes(plan, B, n_max)
            if need == 0:
                _lib.check(-1)
            if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            pred, target = pred.detach().contiguous(), target.detach().contiguous()
            loss = torch.empty((), dtype=torch.float32, device=dev)
            parts = torch.empty(B, dtype=torch.float32, device=dev)
            d_pred = torch.empty_like(pred) if want_grad else None
            _lib.check(lib.gvx_mel_loss(plan, pred.data_ptr(), target.data_ptr(), None if lens_dev is None else lens_dev.data_ptr(), B, n_max,
                                        loss.data_ptr(), parts.data_ptr(), None if d_pred is None else d_pred.data_ptr(), None,
                                        self._workspace.data_ptr(), self._workspace.numel(), torch.cuda.current_stream(dev).cuda_stream))
        return loss, parts, d_pred


# ---- the adversarial losses of the MelGAN step: small elementwise reductions over the discriminator's maps, in plain torch
def _row_mean(values: torch.Tensor, lengths) -> torch.Tensor:
    """values [B, C, L] -> the mean over rows of each row's mean over its own C x L_b elements (``lengths`` None: all L)."""
    B, Cn, L = values.shape
    if lengths is None:
        return values.mean(dim=(1, 2)).mean()
    lens = torch.as_tensor(lengths, device=values.device).to(torch.int64).reshape(B)
    inside = (torch.arange(L, device=values.device)[None, :] < lens[:, None])[:, None, :]
    return (torch.where(inside, values, torch.zeros((), dtype=values.dtype, device=values.device)).sum(dim=(1, 2)) / (Cn * lens).to(values.dtype)).mean()


def _lengths_of(map_lengths, k: int, i: int):
    return None if map_lengths is None else map_lengths[k][i]


class MelGANDiscriminatorLoss(torch.nn.Module):
    """Hinge loss of the discriminator: the sum over the scales of mean(relu(1 - D(real))) + mean(relu(1 + D(fake))) on the scores (the
    last map of every scale).  ``map_lengths[k][i]`` ([B] per map, ``MelGANDiscriminator.map_lengths``) makes every mean a mean per row
    over the row's own positions, then over rows - the rule of MultiResolutionSTFTLoss - so ragged rows never see each other's padding."""

    def forward(self, real, fake, map_lengths=None) -> torch.Tensor:
        loss = 0.0
        for k, (r, f) in enumerate(zip(real, fake)):
            lens = _lengths_of(map_lengths, k, len(r) - 1)
            loss = loss + _row_mean(torch.relu(1.0 - r[-1]), lens) + _row_mean(torch.relu(1.0 + f[-1]), lens)
        return loss


class MelGANGeneratorLoss(torch.nn.Module):
    """The generator's side: adversarial = the sum over the scales of -mean(D(fake)) on the scores; feature matching = ``feat_match``
    times the L1 distance between the fake and the (detached) real features over every non-score map, each map weighted
    4 / (n_layers + 1) / n_scales as in the published implementation (n_layers + 1 = the maps of a scale without its last feature map
    and its score).  Means as in MelGANDiscriminatorLoss.  ``last_terms`` holds (adversarial, feature matching) of the last call."""

    def __init__(self, feat_match: float = 10.0) -> None:
        super().__init__()
        self.feat_match = float(feat_match)
        self.last_terms = None

    def forward(self, real, fake, map_lengths=None) -> torch.Tensor:
        n_scales = len(fake)
        adv, fm = 0.0, 0.0
        for k, (r, f) in enumerate(zip(real, fake)):
            adv = adv - _row_mean(f[-1], _lengths_of(map_lengths, k, len(f) - 1))
            weight = 4.0 / (len(f) - 2) / n_scales   # len(f) = n_layers + 3 maps
            for i in range(len(f) - 1):
                fm = fm + weight * _row_mean((f[i] - r[i].detach()).abs(), _lengths_of(map_lengths, k, i))
        fm = self.feat_match * fm
        self.last_terms = (adv, fm)
        return adv + fm


# ---- the least-squares losses of the HiFi-GAN step (Kong et al. 2020), over any number of discriminators
def _row_mean_any(values: torch.Tensor, lengths) -> torch.Tensor:
    """values [B, C, L] or [B, C, H, p] -> the mean over rows of each row's mean over its own elements: C x L_b, or C x H_b x p
    (``lengths`` [B]: L_b or H_b; None: the whole map, the published mean).  A 4-D map is masked along dim 2 and its dim 3 taken whole:
    ``HiFiGANPeriodDiscriminator``'s [B, C, H, p] with the row's heights, ``MultiResolutionDiscriminator``'s [B, C, W, F] with its
    frames."""
    if values.dim() == 3:
        return _row_mean(values, lengths)
    if values.dim() != 4:
        raise ValueError(f"a discriminator map is [B, C, L] or [B, C, H, p], got {tuple(values.shape)}")
    B, Cn, H, P = values.shape
    if lengths is None:
        return values.mean(dim=(1, 2, 3)).mean()
    lens = torch.as_tensor(lengths, device=values.device).to(torch.int64).reshape(B)
    inside = (torch.arange(H, device=values.device)[None, :] < lens[:, None])[:, None, :, None]
    kept = torch.where(inside, values, torch.zeros((), dtype=values.dtype, device=values.device))
    return (kept.sum(dim=(1, 2, 3)) / (Cn * P * lens).to(values.dtype)).mean()


def _as_outputs(maps, map_lengths):
    """One discriminator's output ([sub-discriminator][map] tensors) or a list of such -> the list form, with its lengths."""
    if len(maps) and len(maps[0]) and isinstance(maps[0][0], torch.Tensor):
        return [maps], [map_lengths]
    return list(maps), ([None] * len(maps) if map_lengths is None else list(map_lengths))


class HiFiGANDiscriminatorLoss(torch.nn.Module):
    """The published least-squares discriminator loss: the sum over all sub-discriminators (periods, scales) of
    mean((1 - D(real))^2) + mean(D(fake)^2) on the scores (the last map of each).  ``real`` / ``fake``: the output of one discriminator
    ([sub-discriminator][map]) or a list of such outputs - ``HiFiGANPeriodDiscriminator``'s 4-D maps and ``MelGANDiscriminator``'s 3-D
    maps alike; ``map_lengths`` the matching ``map_lengths(sample_lengths)`` (or list of them): every mean is then a mean per row over
    the row's own elements, then over rows; for rows of equal length that is the published mean."""

    def forward(self, real, fake, map_lengths=None) -> torch.Tensor:
        real, lens = _as_outputs(real, map_lengths)
        fake, _ = _as_outputs(fake, map_lengths)
        loss = 0.0
        for d, (rs, fs) in enumerate(zip(real, fake)):
            for k, (r, f) in enumerate(zip(rs, fs)):
                ln = _lengths_of(lens[d], k, len(r) - 1)
                loss = loss + _row_mean_any((1.0 - r[-1]) ** 2, ln) + _row_mean_any(f[-1] ** 2, ln)
        return loss


class HiFiGANGeneratorLoss(torch.nn.Module):
    """The generator's side as published: adversarial = the sum over all sub-discriminators of mean((1 - D(fake))^2) on the scores;
    feature matching = ``feat_match`` times the sum over ALL maps - the score's included, as published - of mean|real - fake|, the real
    maps detached.  Inputs and means as in HiFiGANDiscriminatorLoss.  ``last_terms`` holds (adversarial, feature matching) of the
    last call."""

    def __init__(self, feat_match: float = 2.0) -> None:
        super().__init__()
        self.feat_match = float(feat_match)
        self.last_terms = None

    def forward(self, real, fake, map_lengths=None) -> torch.Tensor:
        real, lens = _as_outputs(real, map_lengths)
        fake, _ = _as_outputs(fake, map_lengths)
        adv, fm = 0.0, 0.0
        for d, (rs, fs) in enumerate(zip(real, fake)):
            for k, (r, f) in enumerate(zip(rs, fs)):
                adv = adv + _row_mean_any((1.0 - f[-1]) ** 2, _lengths_of(lens[d], k, len(f) - 1))
                for i in range(len(f)):
                    fm = fm + _row_mean_any((f[i] - r[i].detach()).abs(), _lengths_of(lens[d], k, i))
        fm = self.feat_match * fm
        self.last_terms = (adv, fm)
        return adv + fm
