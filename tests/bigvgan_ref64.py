"""The BigVGAN generator of include/genvox_amd.h ("BigVGAN generator") restated with torch's own operators, for the tests of the device
kernels.  Written from the definition alone: it imports nothing from genvox_amd.  The anti-aliased activation is the padded form -
replicate padding, ``conv_transpose1d`` / ``conv1d`` with the Kaiser-sinc filter from ``torch.kaiser_window`` - not the index form the
kernel implements.  Every function computes in the dtype of the state dict it is given: float64 for the reference, float32 for the
reference's own rounding error, which sets the tests' tolerance.  The filter is always computed in float64 and then cast."""
import functools
import math

import torch
import torch.nn.functional as F
from torch import nn

from tests import hifigan_ref64 as H


def _cfg(base, **over):
    cfg = {k: v for k, v in base.items() if k not in ("slope", "post_slope")}
    cfg.update(activation="snakebeta", logscale=True, tanh=True, bias=True)
    cfg.update(over)
    return cfg


BASE = _cfg(H.V1)                                                        # bigvgan_base_22khz_80band
LARGE = _cfg(H.V1, c0=1536, rates=(4, 4, 2, 2, 2, 2))                    # bigvgan_22khz_80band
MID, NARROW, TWO = _cfg(H.MID), _cfg(H.NARROW), _cfg(H.TWO)              # tests/hifigan_ref64.py's three small nets
MID_CLAMP = _cfg(H.MID, tanh=False)
NARROW_NOBIAS = _cfg(H.NARROW, bias=False)
TWO_SNAKE = _cfg(H.TWO, activation="snake", logscale=False)
ODD_BETA = _cfg(H.ODD)                                                   # tests/hifigan_ref64.py's three that no published shape reaches
FOUR_SNAKE = _cfg(H.FOUR, activation="snake", logscale=False)
ONE_CLAMP = _cfg(H.ONE, tanh=False, bias=False)
NEVER_RUN = ("ODD_BETA", "FOUR_SNAKE", "ONE_CLAMP")

hop = H.hop


def kaiser_sinc_filter() -> torch.Tensor:
    """f, float64 [12]."""
    a_k = 2.285 * (6 - 1) * math.pi * (4 * 0.3) + 7.95
    assert a_k > 50
    w = torch.kaiser_window(12, periodic=False, beta=0.1102 * (a_k - 8.7), dtype=torch.float64)
    t = torch.arange(12, dtype=torch.float64) - 6 + 0.5
    f = 2 * 0.25 * w * torch.sinc(2 * 0.25 * t)
    return f / f.sum()


@functools.lru_cache(maxsize=None)
def _kernel(C: int, dtype, device):
    """f as the grouped convolutions' weight [C, 1, 12], rounded from float64 once per dtype and device."""
    return kaiser_sinc_filter().to(device=device, dtype=dtype).view(1, 1, 12).expand(C, 1, 12).contiguous()


def upsample2(x):
    """[B, C, n] -> [B, C, 2 n]: replicate pad 4, transposed convolution of stride 2, times 2, 13 cropped from each end."""
    C = x.shape[1]
    return 2 * F.conv_transpose1d(F.pad(x, (4, 4), mode="replicate"), _kernel(C, x.dtype, x.device), stride=2, groups=C)[..., 13:-13]


def downsample2(z):
    """[B, C, 2 n] -> [B, C, n]: replicate pad 5 left and 6 right, convolution of stride 2."""
    C = z.shape[1]
    return F.conv1d(F.pad(z, (5, 6), mode="replicate"), _kernel(C, z.dtype, z.device), stride=2, groups=C)


def snake(u, alpha, beta, activation: str, logscale: bool):
    a = alpha.exp() if logscale else alpha
    if activation == "snakebeta":
        b = beta.exp() if logscale else beta
    else:
        b = a
    return u + (1.0 / (b + 1e-9))[None, :, None] * torch.sin(a[None, :, None] * u) ** 2


def activation(x, alpha, beta, activation: str = "snakebeta", logscale: bool = True):
    """A: x [B, C, n], alpha / beta [C] in x's dtype -> [B, C, n]."""
    return downsample2(snake(upsample2(x), alpha, beta, activation, logscale))


def random_snake(C: int, generator, logscale: bool) -> torch.Tensor:
    """alpha (or beta) [C] float64 with a_c = exp(alpha) or alpha log-uniform over 0.3 .. 5."""
    a = torch.exp(math.log(0.3) + (math.log(5.0) - math.log(0.3)) * torch.rand(C, generator=generator, dtype=torch.float64))
    return a.log() if logscale else a


class Generator(nn.Module):
    """The network as a torch module with plain (folded) weights under the published names, float64."""

    def __init__(self, cfg, seed: int):
        super().__init__()
        self.cfg = cfg
        g = torch.Generator().manual_seed(seed)
        beta = cfg["activation"] == "snakebeta"

        def act(c):
            m = nn.Module()
            m.act = nn.Module()
            m.act.alpha = nn.Parameter(random_snake(c, g, cfg["logscale"]))
            if beta:
                m.act.beta = nn.Parameter(random_snake(c, g, cfg["logscale"]))
            return m

        def init(conv, fan_in):
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, dtype=torch.float64) * fan_in ** -0.5)
                if conv.bias is not None:
                    conv.bias.copy_(0.1 * torch.randn(conv.bias.shape, generator=g, dtype=torch.float64))
            return conv

        c = cfg["c0"]
        self.conv_pre = init(nn.Conv1d(cfg["n_mels"], c, 7, padding=3, dtype=torch.float64), 7 * cfg["n_mels"])
        self.ups, self.resblocks = nn.ModuleList(), nn.ModuleList()
        for r in cfg["rates"]:
            self.ups.append(nn.ModuleList([init(nn.ConvTranspose1d(c, c // 2, 2 * r, stride=r, padding=r // 2, dtype=torch.float64), 2 * c)]))
            c //= 2
            for k, ds in zip(cfg["kernels"], cfg["dilations"]):
                blk = nn.Module()
                if cfg["resblock"] == "1":
                    blk.convs1 = nn.ModuleList([init(nn.Conv1d(c, c, k, dilation=d, padding=(k - 1) * d // 2, dtype=torch.float64), k * c) for d in ds])
                    blk.convs2 = nn.ModuleList([init(nn.Conv1d(c, c, k, padding=(k - 1) // 2, dtype=torch.float64), k * c) for _ in ds])
                    blk.activations = nn.ModuleList([act(c) for _ in range(2 * len(ds))])
                else:
                    blk.convs = nn.ModuleList([init(nn.Conv1d(c, c, k, dilation=d, padding=(k - 1) * d // 2, dtype=torch.float64), k * c) for d in ds])
                    blk.activations = nn.ModuleList([act(c) for _ in ds])
                self.resblocks.append(blk)
        self.activation_post = act(c)
        self.conv_post = init(nn.Conv1d(c, 1, 7, padding=3, bias=cfg["bias"], dtype=torch.float64), 7 * c)

    def _a(self, m, x):
        return activation(x, m.act.alpha, getattr(m.act, "beta", None), self.cfg["activation"], self.cfg["logscale"])

    def _block(self, blk, x):
        if self.cfg["resblock"] == "1":
            for m, (c1, c2) in enumerate(zip(blk.convs1, blk.convs2)):
                xt = c1(self._a(blk.activations[2 * m], x))
                xt = c2(self._a(blk.activations[2 * m + 1], xt))
                x = xt + x
        else:
            for m, c in enumerate(blk.convs):
                x = c(self._a(blk.activations[m], x)) + x
        return x

    def forward(self, mel):
        """mel [B, n_mels, T] -> (wav [B, T * hop], [x after every stage's average, [B, C_i, len_i]])."""
        x = self.conv_pre(mel)
        n_k = len(self.cfg["kernels"])
        stages = []
        for i, up in enumerate(self.ups):
            x = up[0](x)
            xs = None
            for j in range(n_k):
                y = self._block(self.resblocks[i * n_k + j], x)
                xs = y if xs is None else xs + y
            x = xs / n_k
            stages.append(x)
        x = self.conv_post(self._a(self.activation_post, x))
        wav = torch.tanh(x) if self.cfg["tanh"] else torch.clamp(x, -1.0, 1.0)
        return wav[:, 0], stages


def random_mel(cfg, B: int, T: int, seed: int) -> torch.Tensor:
    return H.random_mel(cfg, B, T, seed)


def generator_ragged(net, mel, lengths):
    """Every row alone at its own length, zero-filled to the batch's shapes.  Frames at and behind a row's length are never touched."""
    cfg = net.cfg
    B, _, T = mel.shape
    wav, stages, mul, c = torch.zeros(B, T * hop(cfg), dtype=mel.dtype), [], 1, cfg["c0"]
    for r in cfg["rates"]:
        mul, c = mul * r, c // 2
        stages.append(torch.zeros(B, c, T * mul, dtype=mel.dtype))
    for b, t in enumerate(lengths):
        w, st = net(mel[b:b + 1, :, :t])
        wav[b, :w.shape[1]] = w[0]
        for full, one in zip(stages, st):
            full[b, :, :one.shape[2]] = one[0]
    return wav, stages


@torch.no_grad()
def reference_pair(net, mel, lengths):
    """(float64 outputs, per tensor the largest |float32 restatement - float64|): wav first, then the stages.  The second depends on
    the reference alone; the tests derive the device's bound from it, tensor by tensor."""
    import copy

    run = (lambda n, m: n(m)) if lengths is None else (lambda n, m: generator_ragged(n, m, lengths))
    w64, s64 = run(net, mel)
    w32, s32 = run(copy.deepcopy(net).float(), mel.float())
    errs = [(w32.double() - w64).abs().max().item()] + [(a.double() - b).abs().max().item() for a, b in zip(s32, s64)]
    return (w64, s64), errs
