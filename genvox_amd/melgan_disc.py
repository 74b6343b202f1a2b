"""MelGAN multi-scale discriminator on the MI355X (include/genvox_amd.h, "MelGAN discriminators"; kernels in csrc/melgan_disc.hip).

The module holds plain weights in PyTorch's ``Conv1d`` layout [out, in / groups, k] under the names the C ABI's packer reads
(``scales.<k>.layers.<i>.weight / .bias``); the kernels read a packed blob that is rebuilt on the device whenever the parameters change.
``forward`` is one autograd node whose backward is one call of gvx_melgan_disc_backward.  There is no CPU or eager path.  No trained
discriminator checkpoint ships with the project; ``load_state_dict`` reads the published implementation's key names as well."""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from .configs import BaseConfig, MelGANDiscriminatorConfig
from .melgan import _Layer, fold_weight_norm


def dims_from_config(dc: MelGANDiscriminatorConfig) -> _lib.gvx_melgan_disc_dims:
    return _lib.gvx_melgan_disc_dims(dc.n_scales, dc.base_channels, dc.n_layers, dc.downsampling_factor, dc.max_channels, float(dc.leaky_slope))


# the published checkpoints: model.discriminator_<k>.model.layer_<i>.<j>.<what>, layer 0's convolution behind its ReflectionPad1d
_PUBLISHED = re.compile(r"^(?:model\.)?discriminator_(\d+)\.model\.layer_(\d+)\.(\d+)\.(.+)$")


def map_published_keys(state_dict) -> Dict[str, torch.Tensor]:
    """Keys of the published implementation -> this module's (``scales.<k>.layers.<i>.<what>``); other keys pass through.  Layer 0's
    convolution sits at index 1 of its ``Sequential`` (behind the reflection padding), every other layer's at index 0."""
    out = {}
    for key, val in state_dict.items():
        m = _PUBLISHED.match(key)
        if m:
            k, i, j, what = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
            if j != (1 if i == 0 else 0):
                raise KeyError(f"{key}: layer {i}'s convolution is expected at index {1 if i == 0 else 0} of its Sequential")
            key = f"scales.{k}.layers.{i}.{what}"
        out[key] = val
    return out


class _Scale(nn.Module):
    def __init__(self, config: MelGANDiscriminatorConfig) -> None:
        super().__init__()
        self.layers = nn.ModuleList([_Layer((cout, cin // g, k), cout, (cin // g) * k) for cin, cout, k, _s, _p, g in config.layer_shapes()])


class _DiscriminatorFunction(torch.autograd.Function):
    """gvx_melgan_disc_forward / gvx_melgan_disc_backward as one autograd node.  The inputs after ``lens_dev`` are the parameters in
    ``named_parameters()`` order; they go through ``save_for_backward``, so an in-place change between forward and backward raises
    torch's own version error.  The features buffer is the tape, and the node keeps it; the returned maps are views of it and go through
    ``save_for_backward`` as well."""

    @staticmethod
    def forward(ctx, model, wav, lens_dev, *params):
        features, maps = model._run_forward(wav, lens_dev)
        ctx.model, ctx.lens_dev, ctx.features, ctx.packed_key = model, lens_dev, features, model._packed_key
        ctx.n_params = len(params)
        ctx.save_for_backward(wav, *params, *maps)   # the maps are the tape: one changed in place raises as a parameter does
        return tuple(maps)

    @staticmethod
    def backward(ctx, *d_maps):
        wav, *rest = ctx.saved_tensors   # raises if a parameter - or a returned map, which is the tape - was changed in place since the forward
        params = rest[:ctx.n_params]
        model = ctx.model
        if model._packed_key != ctx.packed_key:
            raise RuntimeError("the discriminator's weights were packed again between this forward and its backward")
        lib, dims, dev = _lib.load(), model.dims(), wav.device
        B, n_max = wav.shape
        d_features = torch.empty_like(ctx.features)
        for view, g in zip(model._views(d_features, B, n_max), d_maps):
            if g is None:
                view.zero_()
            else:
                view.copy_(g)
        want_params = any(ctx.needs_input_grad[3:])
        grads, table = [], None
        if want_params:
            names = [k for k, _ in model.named_parameters()]
            grads = [torch.empty_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for p in params]
            table = (_lib.gvx_weight_desc * len(grads))()
            for i, (k, g) in enumerate(zip(names, grads)):
                table[i] = _lib.gvx_weight_desc(k.encode(), g.data_ptr(), g.numel())
        d_wav = torch.empty_like(wav) if ctx.needs_input_grad[1] else None
        if not want_params and d_wav is None:
            return (None, None, None) + (None,) * len(params)
        need = lib.gvx_melgan_disc_workspace_bytes(C.byref(dims), B, n_max, 1)
        if model._train_workspace is None or model._train_workspace.numel() < need or model._train_workspace.device != dev:
            model._train_workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        ws = model._train_workspace
        _lib.check(lib.gvx_melgan_disc_backward(model._handle, wav.data_ptr(), ctx.lens_dev.data_ptr() if ctx.lens_dev is not None else None, B, n_max,
                                                ctx.features.data_ptr(), d_features.data_ptr(), table, len(grads),
                                                d_wav.data_ptr() if d_wav is not None else None, ws.data_ptr(), ws.numel(), model._stream()))
        return (None, d_wav, None, *(grads if want_params else [None] * len(params)))


class MelGANDiscriminator(nn.Module):
    model_name = "melgan_discriminator"

    def __init__(self, model_config: Optional[MelGANDiscriminatorConfig] = None) -> None:
        super().__init__()
        self.model_config = model_config if model_config is not None else MelGANDiscriminatorConfig()
        self.scales = nn.ModuleList([_Scale(self.model_config) for _ in range(self.model_config.n_scales)])
        self._handle: Optional[int] = None
        self._blob: Optional[torch.Tensor] = None
        self._packed_key = None
        self._workspace: Optional[torch.Tensor] = None
        self._train_workspace: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ C-ABI plumbing
    def __del__(self):
        try:
            if self._handle is not None:
                _lib.load().gvx_melgan_disc_destroy(self._handle)
        except Exception:
            pass

    def dims(self) -> _lib.gvx_melgan_disc_dims:
        return dims_from_config(self.model_config)

    @property
    def min_samples(self) -> int:
        return self.model_config.min_samples

    def _device(self) -> torch.device:
        return self.scales[0].layers[0].weight.device

    def _require_gpu(self) -> torch.device:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("genvox_amd.MelGANDiscriminator runs on an MI355X only: move the model with .to('cuda:0'). There is no CPU fallback.")
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
            _lib.check(lib.gvx_melgan_disc_create(C.byref(dims), C.byref(h)))
            self._handle = h.value
        key = self._weights_key()
        if self._packed_key != key:
            srcs = {k: v.detach().to(device=dev, dtype=torch.float32).contiguous() for k, v in self.state_dict().items()}
            table = (_lib.gvx_weight_desc * len(srcs))()
            for i, (k, v) in enumerate(srcs.items()):
                table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
            blob = torch.empty(lib.gvx_melgan_disc_blob_floats(C.byref(dims)), dtype=torch.float32, device=dev)
            _lib.check(lib.gvx_melgan_disc_pack_weights_device(C.byref(dims), table, len(srcs), blob.data_ptr(), self._stream()))
            _lib.check(lib.gvx_melgan_disc_bind(self._handle, blob.data_ptr()))
            self._blob, self._packed_key = blob, key
        return self._handle

    # ------------------------------------------------------------------ host arithmetic
    def feature_lengths(self, n: int) -> List[List[int]]:
        """Per scale, the length of each of the n_layers + 3 maps of a row of ``n`` samples (host arithmetic)."""
        mc = self.model_config
        out = []
        for k in range(mc.n_scales):
            length, lens = n >> k, []
            for _cin, _cout, _k, stride, _p, _g in mc.layer_shapes():
                if stride > 1:
                    length = (length - 1) // stride + 1 if length > 0 else 0
                lens.append(length)
            out.append(lens)
        return out

    def map_lengths(self, sample_lengths) -> List[List[List[int]]]:
        """[scale][map] -> the length of that map in every row, for the losses' per-row means (host arithmetic)."""
        host = [int(v) for v in (sample_lengths.tolist() if isinstance(sample_lengths, torch.Tensor) else sample_lengths)]
        per_row = [self.feature_lengths(n) for n in host]
        return [[[row[k][i] for row in per_row] for i in range(len(per_row[0][k]))] for k in range(self.model_config.n_scales)]

    def layout(self, B: int, n_max: int):
        """gvx_melgan_disc_layout: per scale a list of (byte offset, channels, positions) inside the features buffer."""
        mc, dims = self.model_config, self.dims()
        count = mc.n_scales * (mc.n_layers + 3)
        entries = (_lib.gvx_melgan_disc_entry * count)()
        got = _lib.load().gvx_melgan_disc_layout(C.byref(dims), B, n_max, entries, count)
        if got != count:
            raise ValueError(f"no layout for B = {B}, n_max = {n_max}: a row needs {self.min_samples} samples or more")
        flat = [(e.byte_offset, e.channels, e.positions) for e in entries]
        return [flat[k * (mc.n_layers + 3):(k + 1) * (mc.n_layers + 3)] for k in range(mc.n_scales)]

    def _views(self, features: torch.Tensor, B: int, n_max: int) -> List[torch.Tensor]:
        """The maps of a features buffer (uint8) as float32 [B, C, L] views, scale after scale."""
        return [features[off:off + 4 * B * c * n].view(torch.float32).view(B, c, n) for scale in self.layout(B, n_max) for off, c, n in scale]

    # ------------------------------------------------------------------ the call
    def _check_call(self, wav: torch.Tensor, sample_lengths):
        dev = self._require_gpu()
        if not isinstance(wav, torch.Tensor) or wav.dim() != 2:
            raise ValueError(f"wav must be [B, n_max], got {tuple(wav.shape) if isinstance(wav, torch.Tensor) else type(wav)}")
        if wav.device != dev or wav.dtype != torch.float32:
            raise ValueError(f"wav must be float32 on {dev}, got {wav.dtype} on {wav.device}")
        B, n_max = wav.shape
        if B < 1 or n_max < self.min_samples:
            raise ValueError(f"a batch of {B} rows and {n_max} samples: every row needs at least {self.min_samples} samples (the last scale reflects 7)")
        lens_dev = None
        if sample_lengths is not None:
            host = [int(v) for v in (sample_lengths.tolist() if isinstance(sample_lengths, torch.Tensor) else sample_lengths)]
            if len(host) != B:
                raise ValueError(f"{len(host)} lengths for {B} rows")
            for b, n in enumerate(host):
                if not self.min_samples <= n <= n_max:
                    raise ValueError(f"row {b}: {n} samples are outside [{self.min_samples}, {n_max}] (the last scale reflects 7 samples)")
            lens_dev = (sample_lengths if isinstance(sample_lengths, torch.Tensor) else torch.tensor(host)).to(dev, torch.int32).contiguous()
        return lens_dev

    def _run_forward(self, wav: torch.Tensor, lens_dev, workspace: Optional[torch.Tensor] = None):
        h = self._ensure_packed()
        lib, dims, dev = _lib.load(), self.dims(), wav.device
        B, n_max = wav.shape
        features = torch.empty(lib.gvx_melgan_disc_features_bytes(C.byref(dims), B, n_max), dtype=torch.uint8, device=dev)
        if workspace is None:
            need = lib.gvx_melgan_disc_workspace_bytes(C.byref(dims), B, n_max, 0)
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = self._workspace
        _lib.check(lib.gvx_melgan_disc_forward(h, wav.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, B, n_max, features.data_ptr(),
                                               features.numel(), workspace.data_ptr(), workspace.numel(), self._stream()))
        return features, self._views(features, B, n_max)

    def forward(self, wav: torch.Tensor, sample_lengths=None) -> List[List[torch.Tensor]]:
        """wav float32 [B, n_max] on the device -> per scale the list of its n_layers + 3 maps [B, C, L]: the post-activation features,
        then the score.  ``sample_lengths`` ([B], host or device): every row at its own length - bit for bit that row run alone - and
        exact zeros behind its own lengths (``feature_lengths``); the padded samples may hold anything.  A row below ``min_samples``
        raises ValueError before anything is launched.  With gradients enabled and something that requires one, ``backward()`` through
        any of the maps fills ``.grad`` of the parameters that require it, and of ``wav`` if it does, in one call of the device's
        backward; under ``torch.no_grad()`` it is the plain forward with the same bits.  The returned maps are views of the buffer the
        backward reads as its tape: changing one in place before ``backward()`` raises torch's version error (clone it first)."""
        lens_dev = self._check_call(wav, sample_lengths)
        wav = wav.contiguous()
        per = self.model_config.n_layers + 3
        if not torch.is_grad_enabled() or not (wav.requires_grad or any(p.requires_grad for p in self.parameters())):
            _, maps = self._run_forward(wav, lens_dev)
        else:
            for k, p in self.named_parameters():
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError(f"{k}: training needs contiguous float32 parameters")
            maps = list(_DiscriminatorFunction.apply(self, wav, lens_dev, *self.parameters()))
        return [maps[k * per:(k + 1) * per] for k in range(self.model_config.n_scales)]

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
    def load_from_config(config_path: str) -> "MelGANDiscriminator":
        configs = BaseConfig.load_configs_from_file(path=config_path, config_map={"discriminator_config": MelGANDiscriminatorConfig})
        return MelGANDiscriminator(configs.get("discriminator_config"))
