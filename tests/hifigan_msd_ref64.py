"""HiFi-GAN's multi-scale discriminator of include/genvox_amd.h ("HiFi-GAN scale discriminators") restated with torch's own grouped
convolutions and average pooling, for the tests of the device's forward and backward.  It imports nothing from genvox_amd.
Everything is computed in the dtype asked for; every row is run alone at its own length.

Gradients come from autograd of ``loss = sum over the maps of sum(map * G_map)`` for cotangents G supplied from outside.  Every
``lrelu(x)`` can be *pinned*: replaced by ``x * m`` with ``m`` in {1, slope} supplied from outside, one mask per non-score map, so that
float64 and the device differentiate the same piecewise-linear function (tests/melgan_disc_ref64.py has the reasoning).

Bounds: per tensor, FACTOR = 8 times max(the largest |float32 restatement - float64|, one ulp of the tensor's largest value).

The three configs, and which kernel of csrc/hifigan_msd.hip each layer reaches (a layer runs on the matrix instruction when its
per-group input channels are a multiple of 8 and its per-group output channels a multiple of 16: v_mfma_f32_32x32x2_f32 where both are
multiples of 32, v_mfma_f32_16x16x4_f32 otherwise):
  TINY     2 scales, 1 -> 4 -> 8 -> 8 -> 8, k 15, 41, 41, 5, strides 1, 2, 4, 1, groups 1, 2, 2, 1: every layer in VALU code with one
           lane per output (sd_valu_kernel<1>, sd_wgrad_valu_kernel), the score included (8 input channels).
  MIXED    2 scales, every matrix form of the published shape at a quarter of its group count (the grouped layers have k = 41):
             layer 0  1 -> 32     k 15             VALU
             layer 1  32 -> 32    g 1  s 2  32 x 32 per group: 32x32x2, one 32-wide N tile
             layer 2  32 -> 64    g 4  s 2  8 x 16: 16x16x4; its data gradient produces 8 channels, half a 16-wide tile
             layer 3  64 -> 128   g 4  s 4  16 x 32: 16x16x4, two N tiles; data gradient one
             layer 4  128 -> 256  g 4  s 4  32 x 64: 32x32x2, a 64-wide N tile; data gradient 32-wide
             layer 5  256 -> 256  g 4  s 1  64 x 64: 32x32x2, 64-wide both ways
             layer 6  256 -> 256  k 5  dense: 32x32x2, four channel blocks of 64 through the LDS window, four N tiles
             score    256 -> 1    VALU with the channels dealt over a wave (sd_valu_kernel<64>); its data gradient sd_valu_kernel<1>
  DEFAULT  the published shape: layers 1 to 6 on the matrix kernels, the first layer and the score in VALU code."""
import torch
import torch.nn.functional as F

FACTOR = 8.0
ULP = 2.0 ** -23
SPECTRAL_EPS = 1e-12

TINY = dict(n_scales=2, channels=(4, 8, 8, 8), kernel_sizes=(15, 41, 41, 5), strides=(1, 2, 4, 1), groups=(1, 2, 2, 1), slope=0.1)
MIXED = dict(n_scales=2, channels=(32, 32, 64, 128, 256, 256, 256), kernel_sizes=(15, 41, 41, 41, 41, 41, 5), strides=(1, 2, 2, 4, 4, 1, 1),
             groups=(1, 1, 4, 4, 4, 4, 1), slope=0.1)
DEFAULT = dict(n_scales=3, channels=(128, 128, 256, 512, 1024, 1024, 1024), kernel_sizes=(15, 41, 41, 41, 41, 41, 5),
               strides=(1, 2, 2, 4, 4, 1, 1), groups=(1, 4, 16, 16, 16, 16, 1), slope=0.1)


def layer_shapes(cfg):
    """(c_in, c_out, taps, stride, padding, groups), the score last."""
    shapes, cin = [], 1
    for c, k, s, g in zip(cfg["channels"], cfg["kernel_sizes"], cfg["strides"], cfg["groups"]):
        shapes.append((cin, c, k, s, k // 2, g))
        cin = c
    return shapes + [(cin, 1, 3, 1, 1, 1)]


def layer_name(s, i, cfg):
    return f"discriminators.{s}.conv_post" if i == len(cfg["channels"]) else f"discriminators.{s}.convs.{i}"


def scale_samples(cfg, n):
    """samples of a row of n at every scale: n' = n / 2 + 1"""
    out = []
    for _ in range(cfg["n_scales"]):
        out.append(n)
        n = n // 2 + 1
    return out


def map_lengths(cfg, n):
    """[scale][map] -> length, for a row of n samples."""
    out = []
    for ns in scale_samples(cfg, n):
        length, ls = ns, []
        for _ci, _co, _k, stride, _p, _g in layer_shapes(cfg):
            length = (length - 1) // stride + 1
            ls.append(length)
        out.append(ls)
    return out


def random_state(cfg, seed, gain=1.0):
    """N(0, gain^2 / fan_in) weights [out, in / groups, k] and N(0, 0.1^2) biases, float64."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for s in range(cfg["n_scales"]):
        for i, (ci, co, kk, _s, _p, gr) in enumerate(layer_shapes(cfg)):
            sd[layer_name(s, i, cfg) + ".weight"] = torch.randn(co, ci // gr, kk, generator=g, dtype=torch.float64) * gain * (ci // gr * kk) ** -0.5
            sd[layer_name(s, i, cfg) + ".bias"] = torch.randn(co, generator=g, dtype=torch.float64) * 0.1
    return sd


def random_wav(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g, dtype=torch.float64) * 0.5


def spectral_weight(weight_orig, u, v, training):
    """``torch.nn.utils.spectral_norm`` restated: in training one power iteration v = normalize(W^T u), u = normalize(W v) outside the
    graph, then sigma = u . (W v) with u and v as constants -> (weight_orig / sigma, u, v)."""
    w = weight_orig.reshape(weight_orig.shape[0], -1)
    if training:
        with torch.no_grad():
            v = F.normalize(torch.mv(w.t(), u), dim=0, eps=SPECTRAL_EPS)
            u = F.normalize(torch.mv(w, v), dim=0, eps=SPECTRAL_EPS)
    return weight_orig / torch.dot(u, torch.mv(w, v)), u, v


def discriminator(sd, wav, cfg, masks=None):
    """wav [B, n] -> [scale][map] tensors [B, C, L]: post-activation features, then the score.  ``masks``: None, or [scale][map]
    tensors (the score's entry unused) that replace lrelu(x) by x * masks[s][i]."""
    out, shapes = [], layer_shapes(cfg)
    x = wav[:, None, :]
    for s in range(cfg["n_scales"]):
        maps, h = [], x
        for i, (_ci, _co, _k, stride, pad, groups) in enumerate(shapes):
            h = F.conv1d(h, sd[layer_name(s, i, cfg) + ".weight"], sd[layer_name(s, i, cfg) + ".bias"], stride=stride, padding=pad, groups=groups)
            if i < len(shapes) - 1:
                h = F.leaky_relu(h, cfg["slope"]) if masks is None else h * masks[s][i]
            maps.append(h)
        out.append(maps)
        x = F.avg_pool1d(x, 4, 2, 2)
    return out


def run(sd, wav, lengths, cfg, G=None, masks=None, dtype=torch.float64):
    """Forward (and, with cotangents G [scale][map] of full [B, C, L_max] shape, backward) in ``dtype``, every row alone at its own
    length.  -> (maps zero-filled behind the lengths, {name: gradient} with "wav" among the names; None without G)."""
    sd = {k: v.to(dtype).clone().requires_grad_(G is not None) for k, v in sd.items()}
    B, n = wav.shape
    lengths = [n] * B if lengths is None else list(lengths)
    full, shapes = map_lengths(cfg, n), layer_shapes(cfg)
    maps_all = [[torch.zeros(B, shapes[i][1], full[s][i], dtype=dtype) for i in range(len(shapes))] for s in range(cfg["n_scales"])]
    d_wav = torch.zeros(B, n, dtype=dtype)
    for b, nb in enumerate(lengths):
        x = wav[b:b + 1, :nb].to(dtype).clone().requires_grad_(G is not None)
        own = map_lengths(cfg, nb)
        mk = None if masks is None else [[m[b:b + 1, :, :own[s][i]].to(dtype) for i, m in enumerate(ms)] for s, ms in enumerate(masks)]
        maps = discriminator(sd, x, cfg, mk)
        loss = 0.0
        for s, ms in enumerate(maps):
            for i, m in enumerate(ms):
                assert m.shape[2] == own[s][i], (s, i, m.shape, own[s][i])
                maps_all[s][i][b:b + 1, :, :m.shape[2]] = m.detach()
                if G is not None and G[s][i] is not None:
                    loss = loss + (m * G[s][i][b:b + 1, :, :m.shape[2]].to(dtype)).sum()
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
    """-> dict(maps, grads: float64;  map_err, map_tol: [scale][map] the float32 restatement's error and the bound of every map;
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
    """maps [scale][map] (any dtype) -> the masks that pin every LeakyReLU to the side ``y > 0`` decides."""
    one, low = torch.tensor(1.0, dtype=torch.float64), torch.tensor(slope, dtype=torch.float64)
    return [[torch.where(m.cpu() > 0, one, low) for m in ms] for ms in maps]


def random_cotangents(cfg, B, n, seed, only=None):
    """[scale][map] float64 cotangents of the full shapes; ``only``: a set of (scale, map) that get one, the others are None."""
    g = torch.Generator().manual_seed(seed)
    full, shapes = map_lengths(cfg, n), layer_shapes(cfg)
    out = []
    for s in range(cfg["n_scales"]):
        row = []
        for i in range(len(shapes)):
            t = torch.randn(B, shapes[i][1], full[s][i], generator=g, dtype=torch.float64)
            row.append(t if only is None or (s, i) in only else None)
        out.append(row)
    return out
