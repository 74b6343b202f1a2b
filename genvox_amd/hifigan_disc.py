"""HiFi-GAN multi-period discriminator on the MI355X (include/genvox_amd.h, "HiFi-GAN period discriminators"; kernels in
csrc/hifigan_disc.hip).

The module holds plain weights in PyTorch's ``Conv2d`` layout [out, in, k, 1] under the published names
(``discriminators.<j>.convs.<i>.weight / .bias``, ``discriminators.<j>.conv_post.*``); the kernels read a packed blob that is rebuilt on
the device whenever the parameters change.  ``forward`` is one autograd node whose backward is one call of gvx_hifigan_mpd_backward.
There is no CPU or eager path.  No trained discriminator checkpoint ships with the project; ``load_state_dict`` reads the published
checkpoints (weight-normalised, and the ``{"mpd": ...}`` file itself) as well."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from .configs import BaseConfig, HiFiGANPeriodDiscriminatorConfig
from .melgan import _Layer, fold_weight_norm


def dims_from_config(dc: HiFiGANPeriodDiscriminatorConfig) -> _lib.gvx_hifigan_mpd_dims:
    periods, channels = (C.c_int32 * 8)(), (C.c_int32 * 8)()
    for i, p in enumerate(dc.periods):
        periods[i] = p
    for i, c in enumerate(dc.channels):
        channels[i] = c
    return _lib.gvx_hifigan_mpd_dims(len(dc.periods), periods, len(dc.channels), channels, dc.kernel_size, dc.stride, float(dc.leaky_slope))


def feature_heights(config: HiFiGANPeriodDiscriminatorConfig, n: int) -> List[List[int]]:
    """Per period, the height of each of the len(channels) + 1 maps of a row of ``n`` samples (host arithmetic)."""
    out = []
    for p in config.periods:
        h, hs = -(-n // p), []
        for _cin, _cout, _k, stride, _pad in config.layer_shapes():
            if stride > 1:
                h = (h - 1) // stride + 1 if h > 0 else 0
            hs.append(h)
        out.append(hs)
    return out


def map_published_keys(state_dict) -> Dict[str, torch.Tensor]:
    """The published checkpoint file ``{"mpd": ..., "msd": ...}`` -> its ``mpd`` part; this project's own checkpoint form
    (``{"model_statedict": ...}``) -> its inner dict; anything else passes through."""
    if "mpd" in state_dict and isinstance(state_dict["mpd"], dict):
        return dict(state_dict["mpd"])
    if "model_statedict" in state_dict and isinstance(state_dict["model_statedict"], dict):
        return dict(state_dict["model_statedict"])
    return dict(state_dict)


class _Period(nn.Module):
    def __init__(self, config: HiFiGANPeriodDiscriminatorConfig) -> None:
        super().__init__()
        shapes = config.layer_shapes()
        self.convs = nn.ModuleList([_Layer((cout, cin, k, 1), cout, cin * k) for cin, cout, k, _s, _p in shapes[:-1]])
        cin, cout, k, _s, _p = shapes[-1]
        self.conv_post = _Layer((cout, cin, k, 1), cout, cin * k)


class _PeriodFunction(torch.autograd.Function):
    """gvx_hifigan_mpd_forward / gvx_hifigan_mpd_backward as one autograd node.  The inputs after ``lens_dev`` are the parameters in
    ``named_parameters()`` order; they go through ``save_for_backward``, so an in-place change between forward and backward raises
    torch's own version error.  The features buffer is the tape, and the node keeps it; the returned maps are views of it and go
    through ``save_for_backward`` as well."""

    @staticmethod
    def forward(ctx, model, wav, lens_dev, *params):
        features, maps = model._run_forward(wav, lens_dev)
        ctx.model, ctx.lens_dev, ctx.features, ctx.packed_key = model, lens_dev, features, model._packed_key
        ctx.n_params = len(params)
        ctx.save_for_backward(wav, *params, *maps)
        return tuple(maps)

    @staticmethod
    def backward(ctx, *d_maps):
        wav, *rest = ctx.saved_tensors   # raises if a parameter - or a returned map, which is the tape - was changed in place
        params = rest[:ctx.n_params]
        model = ctx.model
        if model._packed_key != ctx.packed_key:
            raise RuntimeError("the discriminator's weights were packed again between this forward and its backward")
        lib, dims, dev = _lib.load(), model.dims(), wav.device
        B, n_max = wav.shape
        want_params = any(ctx.needs_input_grad[3:])
        d_wav = torch.empty_like(wav) if ctx.needs_input_grad[1] else None
        if not want_params and d_wav is None:
            return (None, None, None) + (None,) * len(params)
        d_features = torch.empty_like(ctx.features)
        for view, g in zip(model._views(d_features, B, n_max), d_maps):
            if g is None:
                view.zero_()
            else:
                view.copy_(g)
        grads, table = [], None
        if want_params:
            names = [k for k, _ in model.named_parameters()]
            grads = [torch.empty_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for p in params]
            table = (_lib.gvx_weight_desc * len(grads))()
            for i, (k, g) in enumerate(zip(names, grads)):
                table[i] = _lib.gvx_weight_desc(k.encode(), g.data_ptr(), g.numel())
        need = lib.gvx_hifigan_mpd_workspace_bytes(C.byref(dims), B, n_max, 1)
        if model._train_workspace is None or model._train_workspace.numel() < need or model._train_workspace.device != dev:
            model._train_workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        ws = model._train_workspace
        _lib.check(lib.gvx_hifigan_mpd_backward(model._handle, wav.data_ptr(), ctx.lens_dev.data_ptr() if ctx.lens_dev is not None else None, B, n_max,
                                                ctx.features.data_ptr(), d_features.data_ptr(), table, len(grads),
                                                d_wav.data_ptr() if d_wav is not None else None, ws.data_ptr(), ws.numel(), model._stream()))
        return (None, d_wav, None, *(grads if want_params else [None] * len(params)))


class HiFiGANPeriodDiscriminator(nn.Module):
    model_name = "hifigan_period_discriminator"

    def __init__(self, model_config: Optional[HiFiGANPeriodDiscriminatorConfig] = None) -> None:
        super().__init__()
        self.model_config = model_config if model_config is not None else HiFiGANPeriodDiscriminatorConfig()
        self.discriminators = nn.ModuleList([_Period(self.model_config) for _ in self.model_config.periods])
        self._handle: Optional[int] = None
        self._blob: Optional[torch.Tensor] = None
        self._packed_key = None
        self._workspace: Optional[torch.Tensor] = None
        self._train_workspace: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ C-ABI plumbing
    def __del__(self):
        try:
            if self._handle is not None:
                _lib.load().gvx_hifigan_mpd_destroy(self._handle)
        except Exception:
            pass

    def dims(self) -> _lib.gvx_hifigan_mpd_dims:
        return dims_from_config(self.model_config)

    @property
    def min_samples(self) -> int:
        return self.model_config.min_samples

    @property
    def maps_per_period(self) -> int:
        return len(self.model_config.channels) + 1

    def _device(self) -> torch.device:
        return self.discriminators[0].conv_post.weight.device

    def _require_gpu(self) -> torch.device:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("genvox_amd.HiFiGANPeriodDiscriminator runs on an MI355X only: move the model with .to('cuda:0'). There is no CPU fallback.")
        return dev

    def _stream(self) -> int:
        return torch.cuda.current_stream(self._device()).cuda_stream

    def _weights_key(self):
        return (str(self._device()),) + tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _ensure_packed(self) -> int:
        dev = self._require_gpu()
        lib, dims = _lib.load(), self.dims()
        if self._handle is None:
            h = C.c_void_p()
            _lib.check(lib.gvx_hifigan_mpd_create(C.byref(dims), C.byref(h)))
            self._handle = h.value
        key = self._weights_key()
        if self._packed_key != key:
            srcs = {k: v.detach().to(device=dev, dtype=torch.float32).contiguous() for k, v in self.state_dict().items()}
            table = (_lib.gvx_weight_desc * len(srcs))()
            for i, (k, v) in enumerate(srcs.items()):
                table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
            blob = torch.empty(lib.gvx_hifigan_mpd_blob_floats(C.byref(dims)), dtype=torch.float32, device=dev)
            _lib.check(lib.gvx_hifigan_mpd_pack_weights_device(C.byref(dims), table, len(srcs), blob.data_ptr(), self._stream()))
            _lib.check(lib.gvx_hifigan_mpd_bind(self._handle, blob.data_ptr()))
            self._blob, self._packed_key = blob, key
        return self._handle

    # ------------------------------------------------------------------ host arithmetic
    def feature_heights(self, n: int) -> List[List[int]]:
        """Per period, the height of each of the maps of a row of ``n`` samples (host arithmetic)."""
        return feature_heights(self.model_config, n)

    def map_lengths(self, sample_lengths) -> List[List[List[int]]]:
        """[period][map] -> the height of that map in every row, for the losses' per-row means (host arithmetic)."""
        host = [int(v) for v in (sample_lengths.tolist() if isinstance(sample_lengths, torch.Tensor) else sample_lengths)]
        per_row = [self.feature_heights(n) for n in host]
        return [[[row[j][i] for row in per_row] for i in range(self.maps_per_period)] for j in range(len(self.model_config.periods))]

    def layout(self, B: int, n_max: int):
        """gvx_hifigan_mpd_layout: per period a list of (byte offset, channels, height, period, (stride_b, stride_c, stride_h, stride_p))."""
        dims = self.dims()
        per, count = self.maps_per_period, len(self.model_config.periods) * self.maps_per_period
        entries = (_lib.gvx_hifigan_mpd_entry * count)()
        got = _lib.load().gvx_hifigan_mpd_layout(C.byref(dims), B, n_max, entries, count)
        if got != count:
            raise ValueError(f"no layout for B = {B}, n_max = {n_max}: a row needs {self.min_samples} samples or more")
        flat = [(e.byte_offset, e.channels, e.height, e.period, (e.stride_b, e.stride_c, e.stride_h, e.stride_p)) for e in entries]
        return [flat[j * per:(j + 1) * per] for j in range(len(self.model_config.periods))]

    def _views(self, features: torch.Tensor, B: int, n_max: int) -> List[torch.Tensor]:
        """The maps of a features buffer (uint8) as float32 [B, C, H, p] views of its channels-last storage, period after period."""
        out = []
        for period in self.layout(B, n_max):
            for off, c, h, p, strides in period:
                flat = features[off:off + 4 * B * c * h * p].view(torch.float32)
                out.append(flat.as_strided((B, c, h, p), strides))
        return out

    # ------------------------------------------------------------------ the call
    def _check_call(self, wav: torch.Tensor, sample_lengths):
        dev = self._require_gpu()
        if not isinstance(wav, torch.Tensor) or wav.dim() != 2:
            raise ValueError(f"wav must be [B, n_max], got {tuple(wav.shape) if isinstance(wav, torch.Tensor) else type(wav)}")
        if wav.device != dev or wav.dtype != torch.float32:
            raise ValueError(f"wav must be float32 on {dev}, got {wav.dtype} on {wav.device}")
        B, n_max = wav.shape
        if B < 1 or n_max < self.min_samples:
            raise ValueError(f"a batch of {B} rows and {n_max} samples: every row needs at least {self.min_samples} samples (the largest period's reflection)")
        lens_dev = None
        if sample_lengths is not None:
            host = [int(v) for v in (sample_lengths.tolist() if isinstance(sample_lengths, torch.Tensor) else sample_lengths)]
            if len(host) != B:
                raise ValueError(f"{len(host)} lengths for {B} rows")
            for b, n in enumerate(host):
                if not self.min_samples <= n <= n_max:
                    raise ValueError(f"row {b}: {n} samples are outside [{self.min_samples}, {n_max}] (the largest period's reflection)")
            lens_dev = (sample_lengths if isinstance(sample_lengths, torch.Tensor) else torch.tensor(host)).to(dev, torch.int32).contiguous()
        return lens_dev

    def _run_forward(self, wav: torch.Tensor, lens_dev, workspace: Optional[torch.Tensor] = None):
        h = self._ensure_packed()
        lib, dims, dev = _lib.load(), self.dims(), wav.device
        B, n_max = wav.shape
        features = torch.empty(lib.gvx_hifigan_mpd_features_bytes(C.byref(dims), B, n_max), dtype=torch.uint8, device=dev)
        if workspace is None:
            need = lib.gvx_hifigan_mpd_workspace_bytes(C.byref(dims), B, n_max, 0)
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = self._workspace
        _lib.check(lib.gvx_hifigan_mpd_forward(h, wav.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, B, n_max, features.data_ptr(),
                                               features.numel(), workspace.data_ptr(), workspace.numel(), self._stream()))
        return features, self._views(features, B, n_max)

    def forward(self, wav: torch.Tensor, sample_lengths=None) -> List[List[torch.Tensor]]:
        """wav float32 [B, n_max] on the device -> per period the list of its len(channels) + 1 maps [B, C, H, p]: the post-activation
        features, then the score.  The shape is the contract; the strides are those of the kernels' channels-last storage.
        ``sample_lengths`` ([B], host or device): every row at its own length - bit for bit that row run alone - and exact zeros behind
        its own heights (``feature_heights``); the padded samples may hold anything.  A row below ``min_samples`` raises ValueError
        before anything is launched.  With gradients enabled and something that requires one, ``backward()`` through any of the maps
        fills ``.grad`` of the parameters that require it, and of ``wav`` if it does, in one call of the device's backward - ``d_wav``
        alone when no parameter requires a gradient; under ``torch.no_grad()`` it is the plain forward with the same bits.  The returned
        maps are views of the buffer the backward reads as its tape: changing one in place before ``backward()`` raises torch's version
        error (clone it first)."""
        lens_dev = self._check_call(wav, sample_lengths)
        wav = wav.contiguous()
        per = self.maps_per_period
        if not torch.is_grad_enabled() or not (wav.requires_grad or any(p.requires_grad for p in self.parameters())):
            _, maps = self._run_forward(wav, lens_dev)
        else:
            for k, p in self.named_parameters():
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError(f"{k}: training needs contiguous float32 parameters")
            maps = list(_PeriodFunction.apply(self, wav, lens_dev, *self.parameters()))
        return [maps[j * per:(j + 1) * per] for j in range(len(self.model_config.periods))]

    # ------------------------------------------------------------------ checkpoints and configs
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(fold_weight_norm(map_published_keys(state_dict)), strict=strict, assign=assign)
        self._packed_key = None
        return out

    def get_checkpoint_statedicts(self, optimizer: Optional[Dict] = None) -> Dict:
        return {"model_statedict": self.state_dict()}

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        self.load_state_dict(statedicts["model_statedict"])

    @staticmethod
    def load_from_config(config_path: str) -> "HiFiGANPeriodDiscriminator":
        configs = BaseConfig.load_configs_from_file(path=config_path, config_map={"discriminator_config": HiFiGANPeriodDiscriminatorConfig})
        return HiFiGANPeriodDiscriminator(configs.get("discriminator_config"))
