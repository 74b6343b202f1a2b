"""The HiFi-GAN generator of include/genvox_amd.h ("HiFi-GAN generator") restated with torch's own convolutions, for the tests of the
device kernels.  Written from the definition alone: it imports nothing from genvox_amd.  Every function computes in the dtype of the
state dict it is given - float64 for the reference, float32 for the reference's own rounding error, which sets the tests' tolerance."""
import torch
import torch.nn.functional as F

_D135 = ((1, 3, 5), (1, 3, 5), (1, 3, 5))
_D2 = ((1, 2), (2, 6), (3, 12))
V1 = dict(n_mels=80, c0=512, rates=(8, 8, 2, 2), resblock="1", kernels=(3, 7, 11), dilations=_D135, slope=0.1, post_slope=0.01)
V2 = dict(n_mels=80, c0=128, rates=(8, 8, 2, 2), resblock="1", kernels=(3, 7, 11), dilations=_D135, slope=0.1, post_slope=0.01)
V3 = dict(n_mels=80, c0=256, rates=(8, 8, 4), resblock="2", kernels=(3, 5, 7), dilations=_D2, slope=0.1, post_slope=0.01)
MID = dict(n_mels=20, c0=256, rates=(4, 2), resblock="1", kernels=(3, 7, 11), dilations=_D135, slope=0.1, post_slope=0.01)     # 128 and 64 channels: the matrix kernel everywhere
NARROW = dict(n_mels=12, c0=48, rates=(4, 2), resblock="1", kernels=(3, 7, 11), dilations=_D135, slope=0.1, post_slope=0.01)   # 24 and 12 channels: N tails, conv_pre's K tail, dot products
TWO = dict(n_mels=12, c0=64, rates=(4, 4), resblock="2", kernels=(3, 5, 7), dilations=_D2, slope=0.1, post_slope=0.01)         # 32 and 16 channels; the widest window, 72

# What no published shape reaches (tests/test_generator_configs_cpu.py asserts the path of every layer):
# ODD   37 mels padded to 40; conv_pre's 144 columns on the 128-wide tile with a 16-column tail; 6 phases on the 64-wide tile (72 columns, a
#       tail of 8) and 2 more on it (36, a tail of 4); K tails of 16 (144), 8 (40, 72) and 4 (36) in a 32-channel block; two blocks per stage;
#       the window limit 72 by k = 9, d = 9; an even dilation in resblock "1"
# ONE   5 mels padded to 8; one stage of 10 phases on the 32-wide tile; one block (no accumulate, a division by 1); left = 36; ReLU
#       (slope 0) inside and the identity (slope 1) in front of conv_post
# FOUR  the dot-product kernel throughout (16 and 8 channels; conv_pre's 32 columns on the 32-wide tile), four blocks per stage
ODD = dict(n_mels=37, c0=144, rates=(6, 2), resblock="1", kernels=(5, 9), dilations=((1, 2, 4), (1, 7, 9)), slope=0.2, post_slope=0.05)
ONE = dict(n_mels=5, c0=64, rates=(10,), resblock="2", kernels=(3,), dilations=((1, 36),), slope=0.0, post_slope=1.0)
FOUR = dict(n_mels=12, c0=32, rates=(2, 2), resblock="1", kernels=(3, 5, 7, 9), dilations=((1, 1, 1), (1, 2, 3), (2, 4, 6), (1, 5, 8)),
            slope=0.1, post_slope=0.01)
NEVER_RUN = ("ODD", "ONE", "FOUR")


def hop(cfg) -> int:
    out = 1
    for r in cfg["rates"]:
        out *= r
    return out


def conv_names(cfg, block: int, m: int):
    """The names of dilation m's convolutions in residual block `block`, in the order they run."""
    if cfg["resblock"] == "1":
        return [f"resblocks.{block}.convs1.{m}", f"resblocks.{block}.convs2.{m}"]
    return [f"resblocks.{block}.convs.{m}"]


def random_state(cfg, seed: int):
    """Weights N(0, 1 / fan_in) with fan_in = taps x C_in (2 C_in for the transposed layers: two taps reach an output), biases
    0.1 N(0, 1), float64, in PyTorch's layouts under the published names."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def layer(name, shape, fan_in, n_out):
        sd[name + ".weight"] = torch.randn(*shape, generator=g, dtype=torch.float64) * fan_in ** -0.5
        sd[name + ".bias"] = 0.1 * torch.randn(n_out, generator=g, dtype=torch.float64)

    c = cfg["c0"]
    layer("conv_pre", (c, cfg["n_mels"], 7), 7 * cfg["n_mels"], c)
    n_k = len(cfg["kernels"])
    for i, r in enumerate(cfg["rates"]):
        layer(f"ups.{i}", (c, c // 2, 2 * r), 2 * c, c // 2)   # ConvTranspose1d [in, out, k]
        c //= 2
        for j, (k, ds) in enumerate(zip(cfg["kernels"], cfg["dilations"])):
            for m in range(len(ds)):
                for name in conv_names(cfg, i * n_k + j, m):
                    layer(name, (c, c, k), k * c, c)
    layer("conv_post", (1, c, 7), 7 * c, 1)
    return sd


def random_mel(cfg, B: int, T: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return 0.5 * torch.randn(B, cfg["n_mels"], T, generator=g, dtype=torch.float64) - 0.5


def resblock(sd, x, cfg, block: int, k: int, dilations):
    s = cfg["slope"]
    for m, d in enumerate(dilations):
        names = conv_names(cfg, block, m)
        y = F.conv1d(F.leaky_relu(x, s), sd[names[0] + ".weight"], sd[names[0] + ".bias"], dilation=d, padding=(k - 1) * d // 2)
        if len(names) == 2:
            y = F.conv1d(F.leaky_relu(y, s), sd[names[1] + ".weight"], sd[names[1] + ".bias"], padding=(k - 1) // 2)
        x = x + y
    return x


def generator(sd, mel, cfg):
    """mel [B, n_mels, T] -> (wav [B, T * hop], [x after every stage's average, [B, C_i, len_i]])."""
    x = F.conv1d(mel, sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3)
    n_k = len(cfg["kernels"])
    stages = []
    for i, r in enumerate(cfg["rates"]):
        x = F.conv_transpose1d(F.leaky_relu(x, cfg["slope"]), sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=r, padding=r // 2)
        xs = None
        for j, (k, ds) in enumerate(zip(cfg["kernels"], cfg["dilations"])):
            y = resblock(sd, x, cfg, i * n_k + j, k, ds)
            xs = y if xs is None else xs + y
        x = xs / n_k
        stages.append(x)
    wav = torch.tanh(F.conv1d(F.leaky_relu(x, cfg["post_slope"]), sd["conv_post.weight"], sd["conv_post.bias"], padding=3))
    return wav[:, 0], stages


def generator_ragged(sd, mel, lengths, cfg):
    """Every row alone at its own length, zero-filled to the batch's shapes.  Frames at and behind a row's length are never touched."""
    B, _, T = mel.shape
    wav, stages, mul, c = torch.zeros(B, T * hop(cfg), dtype=mel.dtype), [], 1, cfg["c0"]
    for r in cfg["rates"]:
        mul, c = mul * r, c // 2
        stages.append(torch.zeros(B, c, T * mul, dtype=mel.dtype))
    for b, t in enumerate(lengths):
        w, st = generator(sd, mel[b:b + 1, :, :t], cfg)
        wav[b, :w.shape[1]] = w[0]
        for full, one in zip(stages, st):
            full[b, :, :one.shape[2]] = one[0]
    return wav, stages


def reference_pair(sd, mel, lengths, cfg):
    """(float64 outputs, per tensor the largest |float32 restatement - float64|): wav first, then the stages.  The second depends on
    the reference alone; the tests derive the device's bound from it, tensor by tensor."""
    run = (lambda s, m: generator(s, m, cfg)) if lengths is None else (lambda s, m: generator_ragged(s, m, lengths, cfg))
    w64, s64 = run(sd, mel)
    w32, s32 = run({k: v.float() for k, v in sd.items()}, mel.float())
    errs = [(w32.double() - w64).abs().max().item()] + [(a.double() - b).abs().max().item() for a, b in zip(s32, s64)]
    return (w64, s64), errs
