"""HiFi-GAN's multi-period discriminator of include/genvox_amd.h ("HiFi-GAN period discriminators") restated with torch's own
convolutions, for the tests of the device's forward and backward.  It imports nothing from genvox_amd.  Everything is computed in the
dtype asked for; every row is run alone at its own length.

Gradients come from autograd of ``loss = sum over the maps of sum(map * G_map)`` for cotangents G supplied from outside.  Every
``lrelu(x)`` can be *pinned*: replaced by ``x * m`` with ``m`` in {1, slope} supplied from outside, one mask per non-score map, so that
float64 and the device differentiate the same piecewise-linear function (tests/melgan_disc_ref64.py has the reasoning).

Bounds: per tensor, FACTOR = 8 times max(the largest |float32 restatement - float64|, one ulp of the tensor's largest value).

The three configs, and which kernel of csrc/hifigan_disc.hip each layer reaches (a layer runs on the matrix instruction when both of
its channel counts are multiples of 32; the weight gradient works on 64 x 64 tiles of one tap):
  TINY     periods (2, 3), channels (4, 8, 8, 8, 8): every layer in VALU code with one lane per output (pd_valu_kernel<1>,
           pd_wgrad_valu_kernel), the score included (8 input channels).
  MIXED    periods (2, 3, 5), channels (8, 32, 64, 160, 64); the matrix kernels' N tile is 128 channels wide where 128 or more are
           produced and 64 below:
             layer 0  1 -> 8     VALU, the reflection and the reshape;        layer 1  8 -> 32   VALU (8 is no multiple of 32)
             layer 2  32 -> 64   matrix kernels, one k block, one full 64-wide N tile; its data gradient produces 32 channels: half
                                 a 64-wide tile
             layer 3  64 -> 160  matrix kernels, two k blocks, wide N tiles of 128 + 32 (a partly filled second tile); its data
                                 gradient 64-wide, five k blocks
             layer 4  160 -> 64  matrix kernels at stride 1 (every tap in every phase), five k blocks, 64-wide; its data gradient
                                 produces 160 channels: wide tiles of 128 + 32
             score    64 -> 1    VALU with the channels dealt over a wave (pd_valu_kernel<64>); its data gradient pd_valu_kernel<1>
  DEFAULT  the published shape: 32 -> 128 -> 512 -> 1024 -> 1024 on the matrix kernels, the first layer and the score in VALU code."""
import torch
import torch.nn.functional as F

FACTOR = 8.0
ULP = 2.0 ** -23

TINY = dict(periods=(2, 3), channels=(4, 8, 8, 8, 8), kernel_size=5, stride=3, slope=0.1)
MIXED = dict(periods=(2, 3, 5), channels=(8, 32, 64, 160, 64), kernel_size=5, stride=3, slope=0.1)
DEFAULT = dict(periods=(2, 3, 5, 7, 11), channels=(32, 128, 512, 1024, 1024), kernel_size=5, stride=3, slope=0.1)


def layer_shapes(cfg):
    """(c_in, c_out, taps, stride, padding) along the height, the score last."""
    shapes, cin = [], 1
    for i, c in enumerate(cfg["channels"]):
        shapes.append((cin, c, cfg["kernel_size"], 1 if i == len(cfg["channels"]) - 1 else cfg["stride"], cfg["kernel_size"] // 2))
        cin = c
    return shapes + [(cin, 1, 3, 1, 1)]


def min_samples(cfg):
    return max(cfg["periods"])


def layer_name(j, i, cfg):
    return f"discriminators.{j}.conv_post" if i == len(cfg["channels"]) else f"discriminators.{j}.convs.{i}"


def map_heights(cfg, n):
    """[period][map] -> height, for a row of n samples."""
    out = []
    for p in cfg["periods"]:
        h, hs = -(-n // p), []
        for _ci, _co, _k, stride, _p in layer_shapes(cfg):
            if stride > 1:
                h = (h - 1) // stride + 1
            hs.append(h)
        out.append(hs)
    return out


def random_state(cfg, seed, gain=1.0):
    """N(0, gain^2 / fan_in) weights [out, in, k, 1] and N(0, 0.1^2) biases, float64."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for j in range(len(cfg["periods"])):
        for i, (ci, co, kk, _s, _p) in enumerate(layer_shapes(cfg)):
            sd[layer_name(j, i, cfg) + ".weight"] = torch.randn(co, ci, kk, 1, generator=g, dtype=torch.float64) * gain * (ci * kk) ** -0.5
            sd[layer_name(j, i, cfg) + ".bias"] = torch.randn(co, generator=g, dtype=torch.float64) * 0.1
    return sd


def random_wav(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g, dtype=torch.float64) * 0.5


def to_grid(x, p):
    """[B, n] -> [B, 1, H, p]: reflection to the next multiple of p, as the published DiscriminatorP pads."""
    n = x.shape[1]
    if n % p:
        x = F.pad(x[:, None, :], (0, p - n % p), mode="reflect")[:, 0, :]
    return x.reshape(x.shape[0], 1, -1, p)


def discriminator(sd, wav, cfg, masks=None):
    """wav [B, n] -> [period][map] tensors [B, C, H, p]: post-activation features, then the score.  ``masks``: None, or [period][map]
    tensors (the score's entry unused) that replace lrelu(x) by x * masks[j][i]."""
    out, shapes = [], layer_shapes(cfg)
    for j, p in enumerate(cfg["periods"]):
        maps, h = [], to_grid(wav, p)
        for i, (_ci, _co, _k, stride, pad) in enumerate(shapes):
            h = F.conv2d(h, sd[layer_name(j, i, cfg) + ".weight"], sd[layer_name(j, i, cfg) + ".bias"], stride=(stride, 1), padding=(pad, 0))
            if i < len(shapes) - 1:
                h = F.leaky_relu(h, cfg["slope"]) if masks is None else h * masks[j][i]
            maps.append(h)
        out.append(maps)
    return out


def run(sd, wav, lengths, cfg, G=None, masks=None, dtype=torch.float64):
    """Forward (and, with cotangents G [period][map] of full [B, C, H_max, p] shape, backward) in ``dtype``, every row alone at its
    own length.  -> (maps zero-filled behind the heights, {name: gradient} with "wav" among the names; None without G)."""
    sd = {k: v.to(dtype).clone().requires_grad_(G is not None) for k, v in sd.items()}
    B, n = wav.shape
    lengths = [n] * B if lengths is None else list(lengths)
    full, shapes = map_heights(cfg, n), layer_shapes(cfg)
    maps_all = [[torch.zeros(B, shapes[i][1], full[j][i], p, dtype=dtype) for i in range(len(shapes))] for j, p in enumerate(cfg["periods"])]
    d_wav = torch.zeros(B, n, dtype=dtype)
    for b, nb in enumerate(lengths):
        x = wav[b:b + 1, :nb].to(dtype).clone().requires_grad_(G is not None)
        own = map_heights(cfg, nb)
        mk = None if masks is None else [[m[b:b + 1, :, :own[j][i]].to(dtype) for i, m in enumerate(ms)] for j, ms in enumerate(masks)]
        maps = discriminator(sd, x, cfg, mk)
        loss = 0.0
        for j, ms in enumerate(maps):
            for i, m in enumerate(ms):
                assert m.shape[2] == own[j][i], (j, i, m.shape, own[j][i])
                maps_all[j][i][b:b + 1, :, :m.shape[2]] = m.detach()
                if G is not None and G[j][i] is not None:
                    loss = loss + (m * G[j][i][b:b + 1, :, :m.shape[2]].to(dtype)).sum()
        if G is not None:
            loss.backward()
            d_wav[b, :nb] = x.grad[0]
    if G is None:
        return maps_all, None
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
    grads["wav"] = d_wav
    return maps_all, grads


def tol_of(a32, a64):
    err = (a32.double() - a64).abs().max().item() if a64.numel() else 0.0
    return err, FACTOR * max(err, ULP * (a64.abs().max().item() if a64.numel() else 0.0))


def reference(sd, wav, lengths, cfg, G=None, masks=None):
    """-> dict(maps, grads: float64;  map_err, map_tol: [period][map] the float32 restatement's error and the bound of every map;
    grad_err, grad_tol: the same per gradient tensor)."""
    m64, g64 = run(sd, wav, lengths, cfg, G, masks, torch.float64)
    sd32 = {k: v.float() for k, v in sd.items()}
    m32, g32 = run(sd32, wav.float(), lengths, cfg, None if G is None else [[None if g is None else g.float() for g in gs] for gs in G],
                   None if masks is None else [[m.float() for m in ms] for ms in masks], torch.float32)
    pairs = [[tol_of(a, b) for a, b in zip(r32, r64)] for r32, r64 in zip(m32, m64)]
    ref = dict(maps=m64, map_err=[[p[0] for p in ps] for ps in pairs], map_tol=[[p[1] for p in ps] for ps in pairs], grads=g64)
    if G is not None:
        both = {k: tol_of(g32[k], g64[k]) for k in g64}
        ref["grad_err"] = {k: v[0] for k, v in both.items()}
        ref["grad_tol"] = {k: v[1] for k, v in both.items()}
    return ref


def masks_from_maps(maps, slope):
    """maps [period][map] (any dtype) -> the masks that pin every LeakyReLU to the side ``y > 0`` decides."""
    one, low = torch.tensor(1.0, dtype=torch.float64), torch.tensor(slope, dtype=torch.float64)
    return [[torch.where(m.cpu() > 0, one, low) for m in ms] for ms in maps]


def random_cotangents(cfg, B, n, seed, only=None):
    """[period][map] float64 cotangents of the full shapes; ``only``: a set of (period index, map) that get one, the others are None."""
    g = torch.Generator().manual_seed(seed)
    full, shapes = map_heights(cfg, n), layer_shapes(cfg)
    out = []
    for j, p in enumerate(cfg["periods"]):
        row = []
        for i in range(len(shapes)):
            t = torch.randn(B, shapes[i][1], full[j][i], p, generator=g, dtype=torch.float64)
            row.append(t if only is None or (j, i) in only else None)
        out.append(row)
    return out
