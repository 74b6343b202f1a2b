"""The Vocos generator (mel variant) restated in plain torch from include/genvox_amd.h, "Vocos generator": the oracle of
tests/test_vocos_*.py.  It runs in float64 (the reference) and in float32 (the reference's own rounding error, the base of the
tests' bound, and tools/bench_extra.py's "torch" column).  Nothing here touches the library."""
import math

import torch
import torch.nn.functional as F
from torch import nn

LN_EPS = 1e-6
LOG_CLAMP = math.log(100.0)

NARROW = dict(n_mels=20, dim=32, intermediate_dim=64, num_layers=1, n_fft=512, hop_length=128, padding="same")
MID = dict(n_mels=80, dim=64, intermediate_dim=192, num_layers=2, n_fft=512, hop_length=256, padding="center")
ODD = dict(n_mels=37, dim=96, intermediate_dim=160, num_layers=2, n_fft=1024, hop_length=130, padding="same")
DEFAULT = dict(n_mels=100, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256, padding="center")


def model_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k != "n_mels"}


def sample_count(cfg, frames: int) -> int:
    return frames * cfg["hop_length"] if cfg["padding"] == "same" else max(frames - 1, 0) * cfg["hop_length"]


class Block(nn.Module):
    def __init__(self, dim, inter, scale):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.pwconv1 = nn.Linear(dim, inter)
        self.pwconv2 = nn.Linear(inter, dim)
        self.gamma = nn.Parameter(scale * torch.ones(dim))

    def forward(self, x):   # [B, C, T]
        r = x
        x = self.dwconv(x).transpose(1, 2)
        x = self.pwconv2(F.gelu(self.pwconv1(self.norm(x))))
        return r + (self.gamma * x).transpose(1, 2)


class Backbone(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        dim = cfg["dim"]
        self.embed = nn.Conv1d(cfg["n_mels"], dim, 7, padding=3)
        self.norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.convnext = nn.ModuleList([Block(dim, cfg["intermediate_dim"], 1.0 / cfg["num_layers"]) for _ in range(cfg["num_layers"])])
        self.final_layer_norm = nn.LayerNorm(dim, eps=LN_EPS)


class Head(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.out = nn.Linear(cfg["dim"], cfg["n_fft"] + 2)


def istft(coeffs, n_fft, hop, padding):
    """coeffs [B, T, n_fft + 2] -> wav [B, samples]: exp, the clamp, the phase, irfft, the window, overlap-add by F.fold over the
    overlap-added squared window, the trim."""
    B, T, _ = coeffs.shape
    H = n_fft // 2
    m, p = coeffs[..., :H + 1], coeffs[..., H + 1:]
    mag = torch.clip(torch.exp(m), max=100.0)
    S = torch.complex(mag * torch.cos(p), mag * torch.sin(p))
    win = torch.hann_window(n_fft, periodic=True, dtype=coeffs.dtype, device=coeffs.device)
    frames = torch.fft.irfft(S, n_fft, dim=-1, norm="backward") * win          # [B, T, N]
    size = (T - 1) * hop + n_fft
    fold = lambda cols: F.fold(cols, output_size=(1, size), kernel_size=(1, n_fft), stride=(1, hop))[:, 0, 0, :]
    y = fold(frames.transpose(1, 2))
    env = fold((win * win).expand(1, T, -1).transpose(1, 2))
    pad = n_fft // 2 if padding == "center" else (n_fft - hop) // 2
    return (y / env)[:, pad:size - pad]


def envelope(n_fft, hop, frames, padding):
    """The overlap-added squared window under the delivered samples of a row of ``frames`` frames, float64."""
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    size = (frames - 1) * hop + n_fft
    env = F.fold((win * win).expand(1, frames, -1).transpose(1, 2), output_size=(1, size), kernel_size=(1, n_fft), stride=(1, hop))[0, 0, 0]
    pad = n_fft // 2 if padding == "center" else (n_fft - hop) // 2
    return env[pad:size - pad]


class Generator(nn.Module):
    """Random weights: N(0, 1 / fan_in) products, biases and LayerNorm shifts of 0.1, LayerNorm scales and gamma around their published
    starts, and ``head.out`` scaled so that the log-magnitudes span both sides of ln 100."""

    def __init__(self, cfg, seed=0):
        super().__init__()
        self.cfg = cfg
        self.backbone, self.head = Backbone(cfg), Head(cfg)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith("gamma"):
                    p.copy_((0.5 + torch.rand(p.shape, generator=g, dtype=torch.float64)) / cfg["num_layers"])
                elif "norm" in name and name.endswith("weight"):
                    p.copy_(0.75 + 0.5 * torch.rand(p.shape, generator=g, dtype=torch.float64))
                elif name.endswith("bias"):
                    p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
                else:
                    fan_in = p[0].numel()
                    p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * fan_in ** -0.5)
            H = cfg["n_fft"] // 2
            self.head.out.weight[:H + 1] *= 3.0     # m ~ N(2.3, 3): about as many bins above ln 100 = 4.6 as far below it
            self.head.out.bias[:H + 1] += 2.3
            self.head.out.weight[H + 1:] *= 2.0     # phases over a few turns
        self.double()

    def forward(self, mel):
        """mel [B, n_mels, T] -> (wav [B, samples], stages [B, T, C] channels-last: x after embed + norm, after every block, after the
        final norm, then the head product)."""
        bb = self.backbone
        x = bb.norm(bb.embed(mel).transpose(1, 2)).transpose(1, 2)
        stages = [x.transpose(1, 2)]
        for blk in bb.convnext:
            x = blk(x)
            stages.append(x.transpose(1, 2))
        y = bb.final_layer_norm(x.transpose(1, 2))
        stages.append(y)
        c = self.head.out(y)
        stages.append(c)
        return istft(c, self.cfg["n_fft"], self.cfg["hop_length"], self.cfg["padding"]), stages


def random_mel(cfg, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, cfg["n_mels"], T, generator=g, dtype=torch.float64) * 1.5 - 3.0


def _ragged(module, mel, lens):
    """Every row alone at its own length, assembled into [B, T * hop] and [B, T, C] with zeros behind a row."""
    cfg = module.cfg
    B, _, T = mel.shape
    lens = [T] * B if lens is None else lens
    wav = torch.zeros(B, T * cfg["hop_length"], dtype=mel.dtype)
    stages = None
    for b, t in enumerate(lens):
        w, st = module(mel[b:b + 1, :, :t])
        wav[b, :w.shape[1]] = w[0]
        if stages is None:
            stages = [torch.zeros(B, T, s.shape[2], dtype=mel.dtype) for s in st]
        for dst, s in zip(stages, st):
            dst[b, :t] = s[0]
    return wav, stages


def reference_pair(ref, mel, lens=None):
    """-> ((wav, stages) in float64, the float32 restatement's largest distance from it per tensor: wav first, then every stage)."""
    import copy

    with torch.no_grad():
        want = _ragged(ref, mel, lens)
        ref32 = copy.deepcopy(ref).float()
        ref32.cfg = ref.cfg
        mel32 = torch.nan_to_num(mel, nan=0.0).float() if lens is None else mel.float()
        got = _ragged(ref32, mel32, lens)
    errs = [(got[0].double() - want[0]).abs().max().item()] + [(g.double() - w).abs().max().item() for g, w in zip(got[1], want[1])]
    return want, errs
