"""Configuration objects for the MI355X Tacotron2 forward path.

Host-side mirror of the three config sections the reference reads when it builds a
model for inference (reference: configs/__init__.py:16-59 BaseConfig file I/O,
:61-82 TextConfig, :92-167 AudioConfig, configs/models.py:4-86 Tacotron2Config).
Only the attribute names, defaults, accepted ranges and the on-disk layout
(one mapping per section: ``model_config``, ``audio_config``, ``text_config``)
are kept; the implementation is table driven and has no dependency on the
reference's ``utils`` package (the reference's configs import a YouTube
downloader through it).
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, Mapping, Optional, Tuple

import yaml

_Range = Tuple[Optional[float], Optional[float]]


def check_argument(name: str, value, min_val=None, max_val=None) -> None:
    """Range assert with the reference's error behaviour (configs/__init__.py:7-13):
    an AssertionError naming the offending field."""
    if min_val is not None and max_val is not None:
        assert min_val <= value <= max_val, (
            f"The value '{name}' ({value}) is not in the required range ({min_val} -> {max_val}).")
    elif min_val is not None:
        assert value >= min_val, f"The value '{name}' ({value}) is below min_val ({min_val})."
    elif max_val is not None:
        assert value <= max_val, f"The value '{name}' ({value}) is above max_val ({max_val})."


class BaseConfig:
    """Field-table driven config. Subclasses declare ``_FIELDS = {name: (default, (lo, hi))}``."""

    _FIELDS: Dict[str, Tuple[Any, Optional[_Range]]] = {}

    def __init__(self, **kwargs):
        unknown = set(kwargs) - set(self._FIELDS)
        if unknown:
            raise TypeError(f"{type(self).__name__}() got unexpected argument(s): {sorted(unknown)}")
        for name, (default, _rng) in self._FIELDS.items():
            setattr(self, name, kwargs.get(name, default))
        self._normalise()
        for name, (_default, rng) in self._FIELDS.items():
            if rng is not None:
                lo, hi = self._resolve_range(name, rng)
                check_argument(name, getattr(self, name), min_val=lo, max_val=hi)

    def _normalise(self) -> None:
        pass

    def _resolve_range(self, name: str, rng: _Range) -> _Range:
        return rng

    # ---- presentation -------------------------------------------------
    def __str__(self) -> str:
        items = list(vars(self).items())
        lines = [type(self).__name__]
        for i, (k, v) in enumerate(items):
            lines.append(("└── " if i == len(items) - 1 else "├── ") + k.ljust(35) + f"({v})")
        return "\n".join(lines)

    def __repr__(self) -> str:
        return f"{type(self).__name__}()"

    def to_dict(self) -> Dict[str, Any]:
        return {k: v for k, v in vars(self).items() if not isinstance(v, BaseConfig)}

    # ---- file I/O (same section layout as the reference's exp/config.yaml) ----
    @staticmethod
    def write_configs_to_file(path: str, configs: Mapping[str, Optional["BaseConfig"]]) -> None:
        ext = os.path.splitext(path)[1][1:]
        assert ext in ("json", "yaml"), f"given config extension ({ext}) is invalid"
        blob = {name: cfg.to_dict() for name, cfg in configs.items() if cfg is not None}
        with open(path, "w") as f:
            if ext == "json":
                json.dump(blob, f, indent=4)
            else:
                yaml.dump(blob, f, sort_keys=False, allow_unicode=True)

    @staticmethod
    def load_configs_from_file(path: str, config_map: Mapping[str, type]) -> Dict[str, "BaseConfig"]:
        ext = os.path.splitext(path)[1][1:]
        assert ext in ("json", "yaml"), f"given config extension ({ext}) is invalid"
        with open(path, "r") as f:
            blob = json.load(f) if ext == "json" else yaml.load(f, Loader=yaml.SafeLoader)
        return {name: config_map[name](**section) for name, section in blob.items() if name in config_map}


class TextConfig(BaseConfig):
    """reference: configs/__init__.py:61-82. ``n_tokens`` sizes the embedding table."""

    _FIELDS = {
        "language": ("english", None),
        "cleaners": (None, None),
        "use_g2p": (False, None),
        "token_map": (None, None),
        "n_tokens": (None, None),
    }

    def _normalise(self) -> None:
        self.language = self.language.lower()


class AudioConfig(BaseConfig):
    """reference: configs/__init__.py:92-167 (same names, defaults and ranges)."""

    _FIELDS = {
        "sampling_rate": (22050, (16000, 44100)),
        "trim_silence": (True, None),
        "trim_dbfs": (-50.0, (-100, 0)),
        "min_wav_duration": (0.5, (0.1, None)),
        "max_wav_duration": (10, ("min_wav_duration", None)),
        "normalize": (True, None),
        "filter_length": (512, (256, 2048)),
        "hop_length": (256, (128, "filter_length")),
        "n_mels": (80, (12, 128)),
        "mel_fmin": (0.0, (0, 8000)),
        "mel_fmax": (8000.0, (8000, 22050)),
        "log_func": ("np.log10", None),
        "ref_level_db": (1.0, (1, None)),
    }

    def _resolve_range(self, name, rng):
        return tuple(getattr(self, b) if isinstance(b, str) else b for b in rng)


class Tacotron2Config(BaseConfig):
    """reference: configs/models.py:4-86 (same names, defaults and ranges)."""

    _FIELDS = {
        "symbols_embedding_dim": (512, (1, None)),
        "encoder_kernel_size": (5, (1, None)),
        "encoder_n_convolutions": (3, (1, None)),
        "encoder_embedding_dim": (512, (1, None)),
        "decoder_rnn_dim": (1024, (1, None)),
        "prenet_dim": (256, (1, None)),
        "max_decoder_steps": (1000, (1, 10000)),
        "gate_threshold": (0.5, (0, 1)),
        "p_attention_dropout": (0.1, (0, None)),
        "p_decoder_dropout": (0.1, (0, None)),
        "attention_rnn_dim": (1024, (1, None)),
        "attention_dim": (128, (1, None)),
        "attention_location_n_filters": (32, (1, None)),
        "attention_location_kernel_size": (31, (1, None)),
        "postnet_embedding_dim": (512, (1, None)),
        "postnet_kernel_size": (5, (1, None)),
        "postnet_n_convolutions": (5, (1, None)),
        "mask_padding": (True, None),
        "learning_rate": (1e-3, (1e-5, None)),
        "weight_decay": (1e-6, (0, None)),
        "grad_clip_thresh": (1.0, (0, None)),
        "beta1": (0.9, (0, 1)),
        "beta2": (0.999, (0, 1)),
    }


class FastPitchConfig(BaseConfig):
    """The FastPitch acoustic model (Lancucki 2021; include/genvox_amd.h, "FastPitch acoustic model").  The reference ships no such
    model; the defaults are the published NVIDIA model's (``enc_*`` its ``in_fft_*`` arguments, ``dec_*`` its ``out_fft_*``, one
    ``d_model`` for both stacks - the published ``symbols_embedding_dim``; ``predictor_*`` serve the duration, pitch and energy
    predictors alike, each a stack of k = 3 convolutions).  ``min_token_frames`` (0 as published) is the least frame count the length
    regulator gives a token; ``max_decoder_steps`` cuts a row's frames; ``max_tokens`` bounds a row's tokens (with ``max_decoder_steps``
    it sizes the position table).  The ranges are what the kernels take: anything else is refused here, by name."""

    MAX_DIM = 512          # GVX_FASTPITCH_MAX_DIM: the LayerNorm kernel's limit
    MAX_INNER = 8192       # GVX_FASTPITCH_MAX_INNER
    MAX_LAYERS = 32        # GVX_FASTPITCH_MAX_LAYERS
    MAX_HEADS = 16         # GVX_FASTPITCH_MAX_HEADS
    MAX_TOKENS = 4096      # GVX_FASTPITCH_MAX_TOKENS
    MAX_POSITIONS = 1 << 16   # GVX_FASTPITCH_MAX_POSITIONS

    _FIELDS = {
        "d_model": (384, None),
        "enc_n_layers": (6, None), "enc_n_head": (1, None), "enc_d_head": (64, None), "enc_d_inner": (1536, None), "enc_kernel_size": (3, None),
        "dec_n_layers": (6, None), "dec_n_head": (1, None), "dec_d_head": (64, None), "dec_d_inner": (1536, None), "dec_kernel_size": (3, None),
        "predictor_filter_size": (256, None),
        "predictor_n_layers": (2, None),
        "energy_conditioning": (True, None),
        "max_duration": (75, None),
        "min_token_frames": (0, None),
        "max_decoder_steps": (2000, None),
        "max_tokens": (512, None),
        "pre_lnorm": (False, None),
        "n_speakers": (1, None),
    }

    def _normalise(self) -> None:
        ints = [k for k in self._FIELDS if k not in ("energy_conditioning", "pre_lnorm")]
        for name in ints:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer, not {v!r}")
        if self.pre_lnorm:
            raise ValueError("pre_lnorm = True is not supported: the kernels run the published default, LayerNorm behind the residual")
        if self.n_speakers != 1:
            raise ValueError(f"n_speakers = {self.n_speakers}: only the single-speaker model is supported")
        self.energy_conditioning = bool(self.energy_conditioning)
        for name in ("d_model", "predictor_filter_size"):
            v = getattr(self, name)
            if v % 32 or not 32 <= v <= self.MAX_DIM:
                raise ValueError(f"{name} = {v} must be a multiple of 32 in [32, {self.MAX_DIM}], the LayerNorm kernel's limit")
        for s in ("enc", "dec"):
            v = getattr(self, f"{s}_d_inner")
            if v % 32 or not 32 <= v <= self.MAX_INNER:
                raise ValueError(f"{s}_d_inner = {v} must be a multiple of 32 in [32, {self.MAX_INNER}]")
            if getattr(self, f"{s}_d_head") not in (32, 64):
                raise ValueError(f"{s}_d_head = {getattr(self, f'{s}_d_head')} must be 32 or 64, the head sizes the attention kernel has")
            if getattr(self, f"{s}_kernel_size") not in (1, 3):
                raise ValueError(f"{s}_kernel_size = {getattr(self, f'{s}_kernel_size')} must be 1 or 3")
            if not 1 <= getattr(self, f"{s}_n_layers") <= self.MAX_LAYERS:
                raise ValueError(f"{s}_n_layers = {getattr(self, f'{s}_n_layers')} is outside [1, {self.MAX_LAYERS}]")
            if not 1 <= getattr(self, f"{s}_n_head") <= self.MAX_HEADS:
                raise ValueError(f"{s}_n_head = {getattr(self, f'{s}_n_head')} is outside [1, {self.MAX_HEADS}]")
        for name, lo, hi in (("predictor_n_layers", 1, 8), ("max_duration", 1, self.MAX_POSITIONS), ("min_token_frames", 0, self.max_duration),
                             ("max_decoder_steps", 1, self.MAX_POSITIONS), ("max_tokens", 1, self.MAX_TOKENS)):
            if not lo <= getattr(self, name) <= hi:
                raise ValueError(f"{name} = {getattr(self, name)} is outside [{lo}, {hi}]")


class MelGANConfig(BaseConfig):
    """reference: configs/models.py:89-121 (the eight training fields: same names, defaults and ranges), followed by the generator's
    own shape, which the reference's config does not carry (it ships no vocoder model): a yaml written from the reference's
    ``MelGANConfig`` loads with these at their defaults.  ``upsample_ratios`` must multiply to the audio config's ``hop_length``
    (``check_hop``: the config alone does not know it)."""

    _FIELDS = {
        "train_repeat_discriminator": (1, (1, None)),
        "max_frames": (200, (100, None)),
        "feat_match": (10.0, (1, None)),
        "learning_rate": (1e-4, (1e-5, None)),
        "weight_decay": (0, (0, None)),
        "grad_clip_thresh": (1.0, (0, None)),
        "beta1": (0.5, (0, 1)),
        "beta2": (0.9, (0, 1)),
        "base_channels": (512, None),
        "upsample_ratios": ((8, 8, 2, 2), None),
        "n_residual_layers": (3, None),
        "dilation_base": (3, None),
        "leaky_slope": (0.2, None),
    }

    def _normalise(self) -> None:
        try:
            self.upsample_ratios = [int(r) for r in self.upsample_ratios]   # a list: what a yaml file holds
        except (TypeError, ValueError):
            raise ValueError(f"upsample_ratios must be a sequence of integers, not {self.upsample_ratios!r}") from None
        ints = {"base_channels": self.base_channels, "n_residual_layers": self.n_residual_layers, "dilation_base": self.dilation_base}
        for name, v in ints.items():
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an integer >= 1, not {v!r}")
        if not 1 <= len(self.upsample_ratios) <= 8:
            raise ValueError(f"upsample_ratios must name 1 to 8 stages, not {len(self.upsample_ratios)}")
        for r in self.upsample_ratios:
            if r < 2 or r % 2:
                raise ValueError(f"every upsampling ratio must be even and >= 2 (kernel 2r, stride r, padding r/2), not {r}")
        if self.base_channels % (1 << len(self.upsample_ratios)):
            raise ValueError(f"base_channels = {self.base_channels} is not divisible by 2^{len(self.upsample_ratios)}: every stage halves the channels")
        if self.n_residual_layers > 8:
            raise ValueError(f"n_residual_layers = {self.n_residual_layers} is above 8")
        if self.dilation_base ** (self.n_residual_layers - 1) >= 4 * self.upsample_ratios[0]:
            raise ValueError(f"the largest dilation {self.dilation_base ** (self.n_residual_layers - 1)} must be below 4 * {self.upsample_ratios[0]}, "
                             f"the shortest row of the first stage")
        if not 0.0 <= float(self.leaky_slope) <= 1.0:
            raise ValueError(f"leaky_slope = {self.leaky_slope} is outside [0, 1]")

    @property
    def hop(self) -> int:
        hop = 1
        for r in self.upsample_ratios:
            hop *= r
        return hop

    def check_hop(self, hop_length: int) -> None:
        if self.hop != int(hop_length):
            raise ValueError(f"upsample_ratios {tuple(self.upsample_ratios)} multiply to {self.hop}, the audio config's hop_length is {hop_length}")


class MelGANDiscriminatorConfig(BaseConfig):
    """The multi-scale discriminator a MelGAN generator is trained against (include/genvox_amd.h, "MelGAN discriminators").  The
    reference ships no such model or config; the defaults are the published architecture's (Kumar et al. 2019)."""

    _FIELDS = {
        "n_scales": (3, None),
        "base_channels": (16, None),
        "n_layers": (4, None),
        "downsampling_factor": (4, None),
        "max_channels": (1024, None),
        "leaky_slope": (0.2, None),
    }

    def _normalise(self) -> None:
        for name in ("n_scales", "base_channels", "n_layers", "downsampling_factor", "max_channels"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer, not {v!r}")
        if not 1 <= self.n_scales <= 4:
            raise ValueError(f"n_scales = {self.n_scales} is outside [1, 4]")
        if self.base_channels < 4 or self.base_channels % 4:
            raise ValueError(f"base_channels = {self.base_channels} must be a positive multiple of 4 (grouped layers take 4 input channels per group)")
        if not 1 <= self.n_layers <= 6:
            raise ValueError(f"n_layers = {self.n_layers} is outside [1, 6]")
        if not 1 <= self.downsampling_factor <= 8:
            raise ValueError(f"downsampling_factor = {self.downsampling_factor} is outside [1, 8]")
        if not 4 <= self.max_channels <= 65536:
            raise ValueError(f"max_channels = {self.max_channels} is outside [4, 65536]")
        if not 0.0 <= float(self.leaky_slope) <= 1.0:
            raise ValueError(f"leaky_slope = {self.leaky_slope} is outside [0, 1]")
        for i, (cin, cout, _k, _stride, _pad, groups) in enumerate(self.layer_shapes()):
            if cin % groups or cout % groups or (groups > 1 and cin != 4 * groups):
                raise ValueError(f"layer {i}: {cin} -> {cout} channels cannot be split into {groups} groups of 4 input channels")

    def layer_shapes(self):
        """The n_layers + 3 convolutions of one scale as (c_in, c_out, taps, stride, padding, groups)."""
        s, c = self.downsampling_factor, self.base_channels
        shapes = [(1, c, 15, 1, 7, 1)]
        for _ in range(self.n_layers):
            cn = min(c * s, self.max_channels)
            shapes.append((c, cn, 10 * s + 1, s, 5 * s, max(c // 4, 1)))
            c = cn
        c2 = min(2 * c, self.max_channels)
        shapes += [(c, c2, 5, 1, 2, 1), (c2, 1, 3, 1, 1, 1)]
        return shapes

    @property
    def min_samples(self) -> int:
        """The shortest row: the last scale still reflects 7 samples."""
        return 8 << (self.n_scales - 1)

    def parameter_count(self) -> int:
        return self.n_scales * sum(cout * (cin // g) * k + cout for cin, cout, k, _s, _p, g in self.layer_shapes())


class HiFiGANConfig(BaseConfig):
    """The HiFi-GAN generator (Kong et al. 2020; include/genvox_amd.h, "HiFi-GAN generator").  The reference ships no such model; the
    fields carry the names of the published implementation's ``config.json`` and the defaults of its V1 generator, followed by the
    two LeakyReLU slopes, which that implementation keeps in its code.  ``upsample_rates`` must multiply to the audio config's
    ``hop_length`` (``check_hop``: the config alone does not know it)."""

    MAX_WINDOW = 72   # GVX_HIFIGAN_MAX_WINDOW: the largest (kernel size - 1) * dilation, V3's k = 7 at d = 12

    _FIELDS = {
        "upsample_initial_channel": (512, None),
        "upsample_rates": ((8, 8, 2, 2), None),
        "upsample_kernel_sizes": ((16, 16, 4, 4), None),
        "resblock": ("1", None),
        "resblock_kernel_sizes": ((3, 7, 11), None),
        "resblock_dilation_sizes": (((1, 3, 5), (1, 3, 5), (1, 3, 5)), None),
        "leaky_slope": (0.1, None),
        "post_leaky_slope": (0.01, None),
    }

    def _normalise(self) -> None:
        try:   # lists: what a yaml or json file holds
            self.upsample_rates = [int(r) for r in self.upsample_rates]
            self.upsample_kernel_sizes = [int(k) for k in self.upsample_kernel_sizes]
            self.resblock_kernel_sizes = [int(k) for k in self.resblock_kernel_sizes]
            self.resblock_dilation_sizes = [[int(d) for d in ds] for ds in self.resblock_dilation_sizes]
        except (TypeError, ValueError):
            raise ValueError("upsample_rates, upsample_kernel_sizes and resblock_kernel_sizes must be sequences of integers and "
                             "resblock_dilation_sizes a sequence of such sequences") from None
        self.resblock = str(self.resblock)
        c0 = self.upsample_initial_channel
        if isinstance(c0, bool) or not isinstance(c0, int) or c0 < 1:
            raise ValueError(f"upsample_initial_channel must be an integer >= 1, not {c0!r}")
        if self.resblock not in ("1", "2"):
            raise ValueError(f"resblock must be '1' or '2', not {self.resblock!r}")
        n = len(self.upsample_rates)
        if not 1 <= n <= 8:
            raise ValueError(f"upsample_rates must name 1 to 8 stages, not {n}")
        if len(self.upsample_kernel_sizes) != n:
            raise ValueError(f"{len(self.upsample_kernel_sizes)} upsample_kernel_sizes for {n} upsample_rates")
        for r, k in zip(self.upsample_rates, self.upsample_kernel_sizes):
            if r < 2 or r % 2:
                raise ValueError(f"every upsampling rate must be even and >= 2, not {r}")
            if k != 2 * r:
                raise ValueError(f"upsample_kernel_sizes[i] must be 2 * upsample_rates[i] (kernel 2r, stride r, padding r/2: the only form "
                                 f"supported, which covers the published V1, V2 and V3), not kernel {k} at rate {r}")
        if self.hop > 4096:
            raise ValueError(f"upsample_rates multiply to {self.hop}, above 4096")
        if c0 % (1 << n) or (c0 >> n) < 4 or (c0 >> n) % 4:
            raise ValueError(f"upsample_initial_channel = {c0}: every stage halves the channels, and every stage's channel count must be a "
                             f"multiple of 4 and at least 4")
        if not 1 <= len(self.resblock_kernel_sizes) <= 4:
            raise ValueError(f"there must be 1 to 4 resblock_kernel_sizes, not {len(self.resblock_kernel_sizes)}")
        if len(self.resblock_dilation_sizes) != len(self.resblock_kernel_sizes):
            raise ValueError(f"{len(self.resblock_dilation_sizes)} resblock_dilation_sizes for {len(self.resblock_kernel_sizes)} resblock_kernel_sizes")
        n_dil = 3 if self.resblock == "1" else 2
        for k, ds in zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes):
            if k < 3 or k > 11 or k % 2 == 0:
                raise ValueError(f"every resblock kernel size must be odd and in [3, 11], not {k}")
            if len(ds) != n_dil:
                raise ValueError(f"resblock '{self.resblock}' has {n_dil} dilations per block, not {len(ds)}")
            for d in ds:
                if d < 1:
                    raise ValueError(f"every dilation must be >= 1, not {d}")
                if (k - 1) * d > self.MAX_WINDOW:
                    raise ValueError(f"(kernel size - 1) * dilation = {(k - 1) * d} (k = {k}, d = {d}) is above the window cap of {self.MAX_WINDOW}")
        for name in ("leaky_slope", "post_leaky_slope"):
            if not 0.0 <= float(getattr(self, name)) <= 1.0:
                raise ValueError(f"{name} = {getattr(self, name)} is outside [0, 1]")

    @property
    def hop(self) -> int:
        hop = 1
        for r in self.upsample_rates:
            hop *= r
        return hop

    def check_hop(self, hop_length: int) -> None:
        if self.hop != int(hop_length):
            raise ValueError(f"upsample_rates {tuple(self.upsample_rates)} multiply to {self.hop}, the audio config's hop_length is {hop_length}")

    @classmethod
    def from_published(cls, config: Mapping[str, Any]) -> "HiFiGANConfig":
        """The generator's part of a published ``config.json`` (as a dict); that file's training and audio keys are ignored."""
        return cls(**{k: config[k] for k in cls._FIELDS if k in config})


class BigVGANConfig(HiFiGANConfig):
    """The BigVGAN generator (Lee et al. 2023; include/genvox_amd.h, "BigVGAN generator").  The reference ships no such model; the
    fields carry the names of the published implementation's ``config.json`` and the defaults of ``bigvgan_base_22khz_80band``.  The
    structure is HiFi-GAN's generator's and is held to ``HiFiGANConfig``'s ranges by that class's own checks; ``upsample_rates`` must
    multiply to the audio config's ``hop_length`` (``check_hop``)."""

    _STRUCTURE = ("upsample_initial_channel", "upsample_rates", "upsample_kernel_sizes", "resblock", "resblock_kernel_sizes",
                  "resblock_dilation_sizes")
    _FIELDS = {
        **{k: HiFiGANConfig._FIELDS[k] for k in _STRUCTURE},
        "activation": ("snakebeta", None),
        "snake_logscale": (True, None),
        "use_tanh_at_final": (True, None),
        "use_bias_at_final": (True, None),
    }

    def _normalise(self) -> None:
        net = HiFiGANConfig(**{k: getattr(self, k) for k in self._STRUCTURE})   # its checks, its normal forms
        for k in self._STRUCTURE:
            setattr(self, k, getattr(net, k))
        if self.activation not in ("snake", "snakebeta"):
            raise ValueError(f"activation must be 'snake' or 'snakebeta', not {self.activation!r}")
        for name in ("snake_logscale", "use_tanh_at_final", "use_bias_at_final"):
            if not isinstance(getattr(self, name), bool):
                raise ValueError(f"{name} must be true or false, not {getattr(self, name)!r}")


class VocosConfig(BaseConfig):
    """The Vocos generator, mel variant (Siuzdak 2023; include/genvox_amd.h, "Vocos generator").  The reference ships no such model; the
    fields carry the names of the published ``config.yaml`` and the defaults of ``charactr/vocos-mel-24khz``.  ``input_channels`` is the
    audio config's ``n_mels``; the window is the periodic Hann of ``n_fft`` points; ``hop_length`` must be the audio config's
    (``check_hop``).  The ranges are what the kernels take."""

    N_FFTS = (512, 1024, 2048)   # the sizes the in-LDS FFT has
    MAX_DIM = 512                # GVX_VOCOS_MAX_DIM
    MAX_INTERMEDIATE = 8192      # GVX_VOCOS_MAX_INTERMEDIATE
    MAX_LAYERS = 64              # GVX_VOCOS_MAX_LAYERS

    _FIELDS = {
        "dim": (512, None),
        "intermediate_dim": (1536, None),
        "num_layers": (8, None),
        "n_fft": (1024, None),
        "hop_length": (256, None),
        "padding": ("center", None),
        "layer_scale_init_value": (None, None),
    }

    def _normalise(self) -> None:
        for name in ("dim", "intermediate_dim", "num_layers", "n_fft", "hop_length"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer, not {v!r}")
        if self.n_fft not in self.N_FFTS:
            raise ValueError(f"n_fft = {self.n_fft} is not one of {self.N_FFTS}, the sizes the FFT kernels have")
        if not self.n_fft // 8 <= self.hop_length <= self.n_fft // 2:
            raise ValueError(f"hop_length = {self.hop_length} is outside [n_fft / 8, n_fft / 2] = [{self.n_fft // 8}, {self.n_fft // 2}]")
        if (self.n_fft - self.hop_length) % 2:
            raise ValueError(f"hop_length = {self.hop_length}: n_fft - hop_length must be even, the trim of either end is half of it")
        for name, most in (("dim", self.MAX_DIM), ("intermediate_dim", self.MAX_INTERMEDIATE)):
            v = getattr(self, name)
            if v % 32 or not 32 <= v <= most:
                raise ValueError(f"{name} = {v} must be a multiple of 32 in [32, {most}]")
        if not 1 <= self.num_layers <= self.MAX_LAYERS:
            raise ValueError(f"num_layers = {self.num_layers} is outside [1, {self.MAX_LAYERS}]")
        if self.padding not in ("center", "same"):
            raise ValueError(f"padding must be 'center' or 'same', not {self.padding!r}")
        if self.layer_scale_init_value is not None:
            self.layer_scale_init_value = float(self.layer_scale_init_value)

    @property
    def hop(self) -> int:
        return self.hop_length

    @property
    def layer_scale(self) -> float:
        return 1.0 / self.num_layers if self.layer_scale_init_value is None else self.layer_scale_init_value

    def check_hop(self, hop_length: int) -> None:
        if self.hop_length != int(hop_length):
            raise ValueError(f"hop_length = {self.hop_length}, the audio config's hop_length is {hop_length}")


class UnivNetConfig(BaseConfig):
    """The UnivNet generator (Jang et al. 2021; include/genvox_amd.h, "UnivNet generator").  The reference ships no such model; the
    fields carry the names of the ``gen:`` block of the published ``config.yaml`` and the defaults of the c32 model (``channel_size``
    16 is the published c16).  The LVC kernel size is 3.  ``strides`` must multiply to the audio config's ``hop_length``
    (``check_hop``).  ``tail_pad_frames`` frames of ``tail_pad_value`` (log 1e-5) are what the published inference appends behind an
    utterance and cuts off again.  The ranges are what the kernels take."""

    MAX_BLOCKS = 4         # GVX_UNIVNET_MAX_BLOCKS
    MAX_DILATIONS = 8      # GVX_UNIVNET_MAX_DILATIONS
    MAX_DILATION = 36      # GVX_UNIVNET_MAX_DILATION: HiFi-GAN's window cap of 72 at kernel size 3
    MAX_HIDDEN = 256       # GVX_UNIVNET_MAX_HIDDEN
    MIN_FRAMES = 4         # GVX_UNIVNET_MIN_FRAMES: the reflection by 3

    _FIELDS = {
        "noise_dim": (64, None),
        "channel_size": (32, None),
        "dilations": ((1, 3, 9, 27), None),
        "strides": ((8, 8, 4), None),
        "lReLU_slope": (0.2, None),
        "kpnet_conv_size": (3, None),
        "kpnet_hidden_channels": (64, None),
        "tail_pad_frames": (10, None),
        "tail_pad_value": (-11.5129, None),
    }

    def _normalise(self) -> None:
        try:
            self.dilations = [int(d) for d in self.dilations]
            self.strides = [int(s) for s in self.strides]
        except (TypeError, ValueError):
            raise ValueError("dilations and strides must be sequences of integers") from None
        for name in ("noise_dim", "channel_size", "kpnet_conv_size", "kpnet_hidden_channels", "tail_pad_frames"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer, not {v!r}")
        if not 1 <= self.noise_dim <= 1024:
            raise ValueError(f"noise_dim = {self.noise_dim} is outside [1, 1024]")
        if self.channel_size % 4 or not 4 <= self.channel_size <= 32:
            raise ValueError(f"channel_size = {self.channel_size} must be a multiple of 4 in [4, 32]")
        if not 1 <= len(self.dilations) <= self.MAX_DILATIONS:
            raise ValueError(f"there must be 1 to {self.MAX_DILATIONS} dilations, not {len(self.dilations)}")
        for d in self.dilations:
            if not 1 <= d <= self.MAX_DILATION:
                raise ValueError(f"every dilation must be in [1, {self.MAX_DILATION}], not {d}")
        if not 1 <= len(self.strides) <= self.MAX_BLOCKS:
            raise ValueError(f"strides must name 1 to {self.MAX_BLOCKS} blocks, not {len(self.strides)}")
        for s in self.strides:
            if s % 2:
                raise ValueError(f"every stride must be even, not {s}: the transposed convolution runs as kernel 2 s, stride s, padding s / 2 "
                                 f"in two-tap phases, and an odd stride's output_padding form is not built")
            if not 2 <= s <= 64:
                raise ValueError(f"every stride must be in [2, 64], not {s}")
        if self.hop > 4096:
            raise ValueError(f"strides multiply to {self.hop}, above 4096")
        if self.kpnet_hidden_channels % 32 or not 32 <= self.kpnet_hidden_channels <= self.MAX_HIDDEN:
            raise ValueError(f"kpnet_hidden_channels = {self.kpnet_hidden_channels} must be a multiple of 32 in [32, {self.MAX_HIDDEN}]")
        if self.kpnet_conv_size != 3:
            raise ValueError(f"kpnet_conv_size must be 3, not {self.kpnet_conv_size}")
        self.lReLU_slope = float(self.lReLU_slope)
        if not 0.0 <= self.lReLU_slope <= 1.0:
            raise ValueError(f"lReLU_slope = {self.lReLU_slope} is outside [0, 1]")
        if not 0 <= self.tail_pad_frames <= 1024:
            raise ValueError(f"tail_pad_frames = {self.tail_pad_frames} is outside [0, 1024]")
        self.tail_pad_value = float(self.tail_pad_value)

    @property
    def hop(self) -> int:
        hop = 1
        for s in self.strides:
            hop *= s
        return hop

    def check_hop(self, hop_length: int) -> None:
        if self.hop != int(hop_length):
            raise ValueError(f"strides {tuple(self.strides)} multiply to {self.hop}, the audio config's hop_length is {hop_length}")


class HiFiGANPeriodDiscriminatorConfig(BaseConfig):
    """HiFi-GAN's multi-period discriminator (Kong et al. 2020; include/genvox_amd.h, "HiFi-GAN period discriminators").  The defaults
    are the published ``MultiPeriodDiscriminator``; the ranges are what the kernels take."""

    MAX_PERIODS = 8      # GVX_HIFIGAN_MPD_MAX_PERIODS
    MAX_LAYERS = 8       # GVX_HIFIGAN_MPD_MAX_LAYERS
    MAX_PERIOD = 64      # GVX_HIFIGAN_MPD_MAX_PERIOD
    MFMA_MULT = 32       # GVX_HIFIGAN_MPD_MFMA_MULT

    _FIELDS = {
        "periods": ((2, 3, 5, 7, 11), None),
        "channels": ((32, 128, 512, 1024, 1024), None),
        "kernel_size": (5, None),
        "stride": (3, None),
        "leaky_slope": (0.1, None),
    }

    def _normalise(self) -> None:
        try:
            self.periods = [int(p) for p in self.periods]
            self.channels = [int(c) for c in self.channels]
        except (TypeError, ValueError):
            raise ValueError("periods and channels must be sequences of integers") from None
        for name in ("kernel_size", "stride"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an integer, not {v!r}")
        if not 1 <= len(self.periods) <= self.MAX_PERIODS:
            raise ValueError(f"periods must name 1 to {self.MAX_PERIODS} periods, not {len(self.periods)}")
        for p in self.periods:
            if not 1 <= p <= self.MAX_PERIOD:
                raise ValueError(f"periods: {p} is outside [1, {self.MAX_PERIOD}]")
        if not 2 <= len(self.channels) <= self.MAX_LAYERS:
            raise ValueError(f"channels must name 2 to {self.MAX_LAYERS} layers, not {len(self.channels)}")
        for c in self.channels:
            if not 1 <= c <= 4096:
                raise ValueError(f"channels: {c} is outside [1, 4096]")
            if c > 64 and c % self.MFMA_MULT:
                raise ValueError(f"channels: {c} is above 64 and no multiple of {self.MFMA_MULT}, the matrix kernels' k-tile")
        if not 1 <= self.kernel_size <= 15 or self.kernel_size % 2 == 0:
            raise ValueError(f"kernel_size = {self.kernel_size} must be odd and in [1, 15]")
        if not 1 <= self.stride <= 8:
            raise ValueError(f"stride = {self.stride} is outside [1, 8]")
        if not 0.0 <= float(self.leaky_slope) <= 1.0:
            raise ValueError(f"leaky_slope = {self.leaky_slope} is outside [0, 1]")

    def layer_shapes(self):
        """The convolutions of one period, the score last, as (c_in, c_out, taps, stride, padding) along the height."""
        shapes, cin = [], 1
        for i, c in enumerate(self.channels):
            shapes.append((cin, c, self.kernel_size, 1 if i == len(self.channels) - 1 else self.stride, self.kernel_size // 2))
            cin = c
        shapes.append((cin, 1, 3, 1, 1))
        return shapes

    @property
    def min_samples(self) -> int:
        """The shortest row: the reflection of the largest period p needs at most p - 1 samples behind the first."""
        return max(self.periods)

    def parameter_count(self) -> int:
        return len(self.periods) * sum(cout * cin * k + cout for cin, cout, k, _s, _p in self.layer_shapes())


class HiFiGANScaleDiscriminatorConfig(BaseConfig):
    """HiFi-GAN's multi-scale discriminator (Kong et al. 2020; include/genvox_amd.h, "HiFi-GAN scale discriminators").  The defaults
    are the published ``MultiScaleDiscriminator``: three scales, the first under spectral norm (``spectral_norm_scales``), the others
    under weight norm, which is folded on load; the ranges are what the kernels take."""

    MAX_SCALES = 4       # GVX_HIFIGAN_MSD_MAX_SCALES
    MAX_LAYERS = 8       # GVX_HIFIGAN_MSD_MAX_LAYERS
    MAX_KERNEL = 41      # GVX_HIFIGAN_MSD_MAX_KERNEL

    _FIELDS = {
        "n_scales": (3, None),
        "channels": ((128, 128, 256, 512, 1024, 1024, 1024), None),
        "kernel_sizes": ((15, 41, 41, 41, 41, 41, 5), None),
        "strides": ((1, 2, 2, 4, 4, 1, 1), None),
        "groups": ((1, 4, 16, 16, 16, 16, 1), None),
        "spectral_norm_scales": ((0,), None),
        "leaky_slope": (0.1, None),
    }

    def _normalise(self) -> None:
        try:
            for name in ("channels", "kernel_sizes", "strides", "groups", "spectral_norm_scales"):
                setattr(self, name, [int(v) for v in getattr(self, name)])
        except (TypeError, ValueError):
            raise ValueError("channels, kernel_sizes, strides, groups and spectral_norm_scales must be sequences of integers") from None
        if isinstance(self.n_scales, bool) or not isinstance(self.n_scales, int):
            raise ValueError(f"n_scales must be an integer, not {self.n_scales!r}")
        if not 1 <= self.n_scales <= self.MAX_SCALES:
            raise ValueError(f"n_scales = {self.n_scales} is outside [1, {self.MAX_SCALES}]")
        if not 2 <= len(self.channels) <= self.MAX_LAYERS:
            raise ValueError(f"channels must name 2 to {self.MAX_LAYERS} layers, not {len(self.channels)}")
        for name in ("kernel_sizes", "strides", "groups"):
            if len(getattr(self, name)) != len(self.channels):
                raise ValueError(f"{name} names {len(getattr(self, name))} layers, channels {len(self.channels)}")
        cin = 1
        for c, k, s, g in zip(self.channels, self.kernel_sizes, self.strides, self.groups):
            if not 1 <= c <= 4096:
                raise ValueError(f"channels: {c} is outside [1, 4096]")
            if not 1 <= k <= self.MAX_KERNEL or k % 2 == 0:
                raise ValueError(f"kernel_sizes: {k} must be odd and in [1, {self.MAX_KERNEL}]")
            if not 1 <= s <= 8:
                raise ValueError(f"strides: {s} is outside [1, 8]")
            if g < 1 or cin % g or c % g:
                raise ValueError(f"groups: {g} must be at least 1 and divide both channel counts of its layer ({cin} -> {c})")
            cin = c
        for s in self.spectral_norm_scales:
            if not 0 <= s < self.n_scales:
                raise ValueError(f"spectral_norm_scales: {s} names no scale of {self.n_scales}")
        if len(set(self.spectral_norm_scales)) != len(self.spectral_norm_scales):
            raise ValueError("spectral_norm_scales names a scale twice")
        if not 0.0 <= float(self.leaky_slope) <= 1.0:
            raise ValueError(f"leaky_slope = {self.leaky_slope} is outside [0, 1]")

    def layer_shapes(self):
        """The convolutions of one scale, the score last, as (c_in, c_out, taps, stride, padding, groups)."""
        shapes, cin = [], 1
        for c, k, s, g in zip(self.channels, self.kernel_sizes, self.strides, self.groups):
            shapes.append((cin, c, k, s, k // 2, g))
            cin = c
        shapes.append((cin, 1, 3, 1, 1, 1))
        return shapes

    @property
    def min_samples(self) -> int:
        """The shortest row: there is no reflection, 1 sample is enough."""
        return 1

    def parameter_count(self) -> int:
        return self.n_scales * sum(cout * (cin // g) * k + cout for cin, cout, k, _s, _p, g in self.layer_shapes())


class MultiResolutionDiscriminatorConfig(BaseConfig):
    """UnivNet's multi-resolution spectrogram discriminator (Jang et al. 2021; include/genvox_amd.h, "Multi-resolution spectrogram
    discriminator").  The defaults are the ones the published BigVGAN recipe trains with; the ranges are what the kernels take.
    ``window`` is ``"rectangular"`` - what ``torch.stft`` uses when it is given no window, as the published code does - or ``"hann"``
    (periodic); either has ``win`` samples and is zero-padded to ``n_fft``, centred."""

    MAX_RESOLUTIONS = 8     # GVX_MRD_MAX_RESOLUTIONS
    N_FFTS = (512, 1024, 2048)
    WINDOWS = ("rectangular", "hann")   # GVX_MRD_WINDOW_*
    MAPS = 6                # GVX_MRD_MAPS

    _FIELDS = {
        "resolutions": (((1024, 120, 600), (2048, 240, 1200), (512, 50, 240)), None),
        "channels": (32, None),
        "leaky_slope": (0.1, None),
        "window": ("rectangular", None),
    }

    def _normalise(self) -> None:
        try:
            self.resolutions = [tuple(int(v) for v in r) for r in self.resolutions]
        except (TypeError, ValueError):
            raise ValueError("resolutions must be a sequence of (n_fft, hop, win) integer triples") from None
        if not 1 <= len(self.resolutions) <= self.MAX_RESOLUTIONS:
            raise ValueError(f"resolutions must name 1 to {self.MAX_RESOLUTIONS} resolutions, not {len(self.resolutions)}")
        for r in self.resolutions:
            if len(r) != 3:
                raise ValueError(f"resolutions: {r} is no (n_fft, hop, win) triple")
            n_fft, hop, win = r
            if n_fft not in self.N_FFTS:
                raise ValueError(f"resolutions: n_fft = {n_fft} is none of {self.N_FFTS}")
            if not 1 <= hop <= win <= n_fft:
                raise ValueError(f"resolutions: {r} does not satisfy 1 <= hop <= win <= n_fft")
        if isinstance(self.channels, bool) or not isinstance(self.channels, int):
            raise ValueError(f"channels must be an integer, not {self.channels!r}")
        if not 32 <= self.channels <= 128 or self.channels % 32:
            raise ValueError(f"channels = {self.channels} must be a multiple of 32 in [32, 128]")
        if not 0.0 <= float(self.leaky_slope) <= 1.0:
            raise ValueError(f"leaky_slope = {self.leaky_slope} is outside [0, 1]")
        if self.window not in self.WINDOWS:
            raise ValueError(f"window = {self.window!r} is none of {self.WINDOWS}")

    def layer_shapes(self):
        """The convolutions of one resolution, the score last, as (c_in, c_out, (taps in frequency, taps in time), stride in time)."""
        C = self.channels
        return [(1, C, (3, 9), 1), (C, C, (3, 9), 2), (C, C, (3, 9), 2), (C, C, (3, 9), 2), (C, C, (3, 3), 1), (C, 1, (3, 3), 1)]

    @property
    def min_samples(self) -> int:
        """The shortest row: a reflection by (n_fft - hop) // 2 samples needs one sample more."""
        return max((n_fft - hop) // 2 + 1 for n_fft, hop, _win in self.resolutions)

    def parameter_count(self) -> int:
        return len(self.resolutions) * sum(cout * cin * kf * kt + cout for cin, cout, (kf, kt), _s in self.layer_shapes())


class HiFiGANTrainingConfig(BaseConfig):
    """The training keys of a published HiFi-GAN ``config.json`` under their names and with their defaults; ``feat_match`` and
    ``aux_weight`` are the weights that implementation keeps in its training script (2 on the feature-matching term, 45 on the
    spectral term).  ``grad_clip_thresh`` <= 0 switches clipping off, as published."""

    _FIELDS = {
        "learning_rate": (2e-4, (0.0, None)),
        "adam_b1": (0.8, (0.0, 1.0)),
        "adam_b2": (0.99, (0.0, 1.0)),
        "lr_decay": (0.999, (0.0, 1.0)),
        "weight_decay": (0.01, (0.0, None)),
        "feat_match": (2.0, (0.0, None)),
        "aux_weight": (45.0, (0.0, None)),
        "grad_clip_thresh": (0.0, None),
    }

    @classmethod
    def from_published(cls, config: Mapping[str, Any]) -> "HiFiGANTrainingConfig":
        return cls(**{k: config[k] for k in cls._FIELDS if k in config})
