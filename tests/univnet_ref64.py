"""The UnivNet generator restated in plain torch from include/genvox_amd.h, "UnivNet generator": the oracle of tests/test_univnet_*.py.
It runs in float64 (the reference) and in float32 (the reference's own rounding error, the base of the tests' bound, and
tools/bench_extra.py's "torch" column).  Nothing published is at hand, so the location-variable convolution is written twice - the
unfold + einsum form the model runs, and a triple loop over the definition - and tests/test_univnet_cpu.py holds the two equal.  Nothing
here touches the library."""
import torch
import torch.nn.functional as F
from torch import nn

NARROW = dict(n_mels=8, noise_dim=4, kpnet_hidden_channels=32, channel_size=32, dilations=(1, 3), strides=(2, 2))
MID = dict(n_mels=20, noise_dim=16, kpnet_hidden_channels=64, channel_size=32, dilations=(1, 3, 9, 27), strides=(8, 4))
ODD = dict(n_mels=10, noise_dim=6, kpnet_hidden_channels=32, channel_size=12, dilations=(1, 2), strides=(6, 2))
C16 = dict(n_mels=100, noise_dim=64, kpnet_hidden_channels=64, channel_size=16, dilations=(1, 3, 9, 27), strides=(8, 8, 4))
DEFAULT = dict(n_mels=100, noise_dim=64, kpnet_hidden_channels=64, channel_size=32, dilations=(1, 3, 9, 27), strides=(8, 8, 4))
SLOPE = 0.2


def model_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k != "n_mels"}


def hop_of(cfg) -> int:
    hop = 1
    for s in cfg["strides"]:
        hop *= s
    return hop


def lvc_einsum(y, kernels, bias):
    """y [B, C, T * cum], kernels [B, C in, 2C out, 3, T], bias [B, 2C, T] -> o [B, 2C, T * cum]: every frame's own k = 3 convolution over
    that frame's positions, with a zero outside the row."""
    B, C, L = y.shape
    T = kernels.shape[4]
    cum = L // T
    win = F.pad(y, (1, 1)).unfold(2, cum + 2, cum).unfold(3, 3, 1)          # [B, C, T, cum, 3]
    o = torch.einsum("bitpk,bijkt->bjtp", win, kernels) + bias[:, :, :, None]
    return o.reshape(B, -1, L)


def lvc_loops(y, kernels, bias):
    """The definition, term by term:  o[b, j, t cum + p] = bias[b, j, t] + sum_{i, k} kernels[b, i, j, k, t] * y[b, i, t cum + p + k - 1]."""
    B, C, L = y.shape
    T = kernels.shape[4]
    cum = L // T
    o = torch.zeros(B, kernels.shape[2], L, dtype=y.dtype)
    for b in range(B):
        for t in range(T):
            for p in range(cum):
                q = t * cum + p
                acc = bias[b, :, t].clone()
                for k in range(3):
                    if 0 <= q + k - 1 < L:
                        acc = acc + kernels[b, :, :, k, t].t() @ y[b, :, q + k - 1]
                o[b, :, q] = acc
    return o


def gate(x, o):
    C = x.shape[1]
    return x + torch.sigmoid(o[:, :C]) * torch.tanh(o[:, C:])


def lvc_gated(x, kernels, bias, conv=None, slope=SLOPE):
    """One layer as gvx_lvc_gated states it, channels-first: x [B, C, L] -> x + sigmoid * tanh of the LVC of lrelu(conv(lrelu(x))), or of
    lrelu(x) without a convolution."""
    y = F.leaky_relu(conv(F.leaky_relu(x, slope)) if conv is not None else x, slope)
    return gate(x, lvc_einsum(y, kernels, bias))


class KernelPredictor(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        h, c, n = cfg["kpnet_hidden_channels"], cfg["channel_size"], len(cfg["dilations"])
        self.c, self.n = c, n
        self.input_conv = nn.Sequential(nn.Conv1d(cfg["n_mels"], h, 5, padding=2), nn.LeakyReLU(SLOPE))
        self.residual_convs = nn.ModuleList([nn.Sequential(nn.Dropout(0.0), nn.Conv1d(h, h, 3, padding=1), nn.LeakyReLU(SLOPE),
                                                           nn.Conv1d(h, h, 3, padding=1), nn.LeakyReLU(SLOPE)) for _ in range(3)])
        self.kernel_conv = nn.Conv1d(h, c * 2 * c * 3 * n, 3, padding=1)
        self.bias_conv = nn.Conv1d(h, 2 * c * n, 3, padding=1)

    def forward(self, mel):
        B, _, T = mel.shape
        c = self.input_conv(mel)
        for r in self.residual_convs:
            c = c + r(c)
        return self.kernel_conv(c).view(B, self.n, self.c, 2 * self.c, 3, T), self.bias_conv(c).view(B, self.n, 2 * self.c, T)


class LVCBlock(nn.Module):
    def __init__(self, cfg, stride):
        super().__init__()
        c = cfg["channel_size"]
        self.convt_pre = nn.Sequential(nn.LeakyReLU(SLOPE), nn.ConvTranspose1d(c, c, 2 * stride, stride=stride, padding=stride // 2))
        self.conv_blocks = nn.ModuleList([nn.Sequential(nn.LeakyReLU(SLOPE), nn.Conv1d(c, c, 3, dilation=d, padding=d), nn.LeakyReLU(SLOPE))
                                          for d in cfg["dilations"]])
        self.kernel_predictor = KernelPredictor(cfg)

    def forward(self, x, mel):
        x = self.convt_pre(x)
        kernels, bias = self.kernel_predictor(mel)
        for m, conv in enumerate(self.conv_blocks):
            x = gate(x, lvc_einsum(conv(x), kernels[:, m], bias[:, m]))
        return x


class Generator(nn.Module):
    """Random weights: N(0, 1 / fan_in) products and biases of 0.1; ``kernel_conv`` by a further 1 / sqrt(3 C), so that the predicted
    kernels keep the LVC's output at the scale of its input and the gates are not all saturated."""

    def __init__(self, cfg, seed=0):
        super().__init__()
        self.cfg = cfg
        c = cfg["channel_size"]
        self.conv_pre = nn.Conv1d(cfg["noise_dim"], c, 7, padding=3, padding_mode="reflect")
        self.res_stack = nn.ModuleList([LVCBlock(cfg, s) for s in cfg["strides"]])
        self.conv_post = nn.Sequential(nn.LeakyReLU(SLOPE), nn.Conv1d(c, 1, 7, padding=3, padding_mode="reflect"), nn.Tanh())
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith("bias"):
                    p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
                else:
                    fan_in = p[0].numel() if "convt_pre" not in name else 2 * p.shape[0]
                    if "kernel_conv" in name:
                        fan_in *= 3 * c
                    p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * fan_in ** -0.5)
        self.double()

    def forward(self, mel, noise):
        """mel [B, n_mels, T], noise [B, noise_dim, T] -> (wav [B, T * hop], stages channels-last: x after conv_pre [B, T, C], after every
        block [B, T cum_i, C], and the output layer before its tanh [B, T hop, 1])."""
        x = self.conv_pre(noise)
        stages = [x.transpose(1, 2)]
        for blk in self.res_stack:
            x = blk(x, mel)
            stages.append(x.transpose(1, 2))
        pre = self.conv_post[1](self.conv_post[0](x))
        stages.append(pre.transpose(1, 2))
        return torch.tanh(pre)[:, 0], stages


def random_mel(cfg, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, cfg["n_mels"], T, generator=g, dtype=torch.float64) * 1.5 - 3.0


def random_noise(cfg, B, T, seed):
    g = torch.Generator().manual_seed(seed + 7919)
    return torch.randn(B, cfg["noise_dim"], T, generator=g, dtype=torch.float64)


def _ragged(module, mel, noise, lens):
    """Every row alone at its own length, assembled into [B, T * hop] and [B, T * cum, C] with zeros behind a row."""
    B, _, T = mel.shape
    lens = [T] * B if lens is None else lens
    wav, stages = None, None
    for b, t in enumerate(lens):
        w, st = module(mel[b:b + 1, :, :t], noise[b:b + 1, :, :t])
        if wav is None:
            wav = torch.zeros(B, T * (w.shape[1] // t), dtype=mel.dtype)
            stages = [torch.zeros(B, T * (s.shape[1] // t), s.shape[2], dtype=mel.dtype) for s in st]
        wav[b, :w.shape[1]] = w[0]
        for dst, s in zip(stages, st):
            dst[b, :s.shape[1]] = s[0]
    return wav, stages


def reference_pair(ref, mel, noise, lens=None):
    """-> ((wav, stages) in float64, the float32 restatement's largest distance from it per tensor: wav first, then every stage)."""
    import copy

    with torch.no_grad():
        want = _ragged(ref, mel, noise, lens)
        ref32 = copy.deepcopy(ref).float()
        ref32.cfg = ref.cfg
        got = _ragged(ref32, mel.float(), noise.float(), lens)
    errs = [(got[0].double() - want[0]).abs().max().item()] + [(g.double() - w).abs().max().item() for g, w in zip(got[1], want[1])]
    return want, errs
