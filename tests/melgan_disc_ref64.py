"""The MelGAN multi-scale discriminator of include/genvox_amd.h ("MelGAN discriminators") restated with torch's own convolutions, for
the tests of the device's forward and backward.  It imports nothing from genvox_amd.  Everything is computed in the dtype asked for;
every row is run alone at its own length.

Gradients come from autograd of ``loss = sum over the maps of sum(map * G_map)`` for cotangents G supplied from outside.  Every
``lrelu(x)`` can be *pinned*: replaced by ``x * m`` with ``m`` in {1, slope} supplied from outside, one mask per non-score map.  A
pre-activation within rounding of 0 flips a LeakyReLU and changes a gradient by a finite amount; pinned to the device's own decisions
(which it reads off its maps: a LeakyReLU output is positive exactly where its pre-activation is), float64 and the device
differentiate the same piecewise-linear function.

Bounds, as tests/melgan_grad_ref64.py derives them: per tensor, FACTOR = 8 times max(the largest |float32 restatement - float64|, one
ulp of the tensor's largest value)."""
import torch
import torch.nn.functional as F

FACTOR = 8.0
ULP = 2.0 ** -23

TINY = dict(n_scales=2, base_channels=4, n_layers=2, s=2, max_channels=8, slope=0.2)      # groups = 1 in layer 1, the cap bites in layer 2
MIXED = dict(n_scales=3, base_channels=8, n_layers=3, s=4, max_channels=64, slope=0.2)    # groups of 16, 8 and 4 output columns, capped
DEFAULT = dict(n_scales=3, base_channels=16, n_layers=4, s=4, max_channels=1024, slope=0.2)


def layer_shapes(cfg):
    """(c_in, c_out, taps, stride, padding, groups) of the n_layers + 3 convolutions of one scale."""
    s, c = cfg["s"], cfg["base_channels"]
    shapes = [(1, c, 15, 1, 7, 1)]
    for _ in range(cfg["n_layers"]):
        cn = min(c * s, cfg["max_channels"])
        shapes.append((c, cn, 10 * s + 1, s, 5 * s, c // 4))
        c = cn
    c2 = min(2 * c, cfg["max_channels"])
    return shapes + [(c, c2, 5, 1, 2, 1), (c2, 1, 3, 1, 1, 1)]


def min_samples(cfg):
    return 8 << (cfg["n_scales"] - 1)


def map_lengths(cfg, n):
    """[scale][map] -> length, for a row of n samples."""
    out = []
    for k in range(cfg["n_scales"]):
        L, lens = n >> k, []
        for _ci, _co, _k, stride, _p, _g in layer_shapes(cfg):
            if stride > 1:
                L = (L - 1) // stride + 1
            lens.append(L)
        out.append(lens)
    return out


def param_names(cfg):
    return [f"scales.{k}.layers.{i}.{w}" for k in range(cfg["n_scales"]) for i in range(cfg["n_layers"] + 3) for w in ("weight", "bias")]


def random_state(cfg, seed, gain=1.0):
    """N(0, gain^2 / fan_in) weights and N(0, 0.1^2) biases, float64."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in range(cfg["n_scales"]):
        for i, (ci, co, kk, _s, _p, gr) in enumerate(layer_shapes(cfg)):
            fan = (ci // gr) * kk
            sd[f"scales.{k}.layers.{i}.weight"] = torch.randn(co, ci // gr, kk, generator=g, dtype=torch.float64) * gain * fan ** -0.5
            sd[f"scales.{k}.layers.{i}.bias"] = torch.randn(co, generator=g, dtype=torch.float64) * 0.1
    return sd


def random_wav(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g, dtype=torch.float64) * 0.5


def discriminator(sd, wav, cfg, masks=None):
    """wav [B, n] -> [scale][map] tensors [B, C, L]: post-activation features, then the score.  ``masks``: None, or [scale][map]
    tensors (the score's entry unused) that replace lrelu(x) by x * masks[k][i]."""
    out, x = [], wav[:, None, :]
    shapes = layer_shapes(cfg)
    for k in range(cfg["n_scales"]):
        if k > 0:
            x = F.avg_pool1d(x, 4, stride=2, padding=1, count_include_pad=False)
        maps, h = [], x
        for i, (_ci, _co, _k, stride, pad, groups) in enumerate(shapes):
            w, b = sd[f"scales.{k}.layers.{i}.weight"], sd[f"scales.{k}.layers.{i}.bias"]
            if i == 0:
                h = F.conv1d(F.pad(h, (7, 7), mode="reflect"), w, b)
            else:
                h = F.conv1d(h, w, b, stride=stride, padding=pad, groups=groups)
            if i < len(shapes) - 1:
                h = F.leaky_relu(h, cfg["slope"]) if masks is None else h * masks[k][i]
            maps.append(h)
        out.append(maps)
    return out


def run(sd, wav, lengths, cfg, G=None, masks=None, dtype=torch.float64):
    """Forward (and, with cotangents G [scale][map] of full [B, C, L_max] shape, backward) in ``dtype``, every row alone at its own
    length (``lengths`` None: all rows at n).  -> (maps zero-filled behind the lengths, {name: gradient} with "wav" among the names;
    parameter gradients are summed over rows; None without G)."""
    sd = {k: v.to(dtype).clone().requires_grad_(G is not None) for k, v in sd.items()}
    B, n = wav.shape
    lengths = [n] * B if lengths is None else list(lengths)
    full = map_lengths(cfg, n)
    shapes = layer_shapes(cfg)
    maps_all = [[torch.zeros(B, shapes[i][1], full[k][i], dtype=dtype) for i in range(len(shapes))] for k in range(cfg["n_scales"])]
    d_wav = torch.zeros(B, n, dtype=dtype)
    for b, nb in enumerate(lengths):
        x = wav[b:b + 1, :nb].to(dtype).clone().requires_grad_(G is not None)
        own = map_lengths(cfg, nb)
        mk = None if masks is None else [[m[b:b + 1, :, :own[k][i]].to(dtype) for i, m in enumerate(ms)] for k, ms in enumerate(masks)]
        maps = discriminator(sd, x, cfg, mk)
        loss = 0.0
        for k, ms in enumerate(maps):
            for i, m in enumerate(ms):
                assert m.shape[2] == own[k][i], (k, i, m.shape, own[k][i])
                maps_all[k][i][b:b + 1, :, :m.shape[2]] = m.detach()
                if G is not None and G[k][i] is not None:
                    loss = loss + (m * G[k][i][b:b + 1, :, :m.shape[2]].to(dtype)).sum()
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


def near_ties(ref, cfg, lengths=None):
    """How many non-score map values of the float64 forward (inside the rows) lie within FACTOR x that map's float32 error of 0: where
    float32 arithmetic in another order may take the other side of a LeakyReLU.  lrelu keeps the sign and shrinks negative values, so
    a pre-activation that close to 0 is a map value that close to 0 (on the negative side the test is the stricter by 1 / slope)."""
    count = 0
    for k, ms in enumerate(ref["maps"]):
        for i, m in enumerate(ms[:-1]):
            close = m.abs() <= FACTOR * ref["map_err"][k][i]
            B, _, L = m.shape
            for b in range(B):
                nb = L if lengths is None else map_lengths(cfg, lengths[b])[k][i]
                close[b, :, nb:] = False
            count += int(close.sum())
    return count


def masks_from_maps(maps, slope):
    """maps [scale][map] (any dtype) -> the masks that pin every LeakyReLU to the side ``y > 0`` decides."""
    one, low = torch.tensor(1.0, dtype=torch.float64), torch.tensor(slope, dtype=torch.float64)
    return [[torch.where(m.cpu() > 0, one, low) for m in ms] for ms in maps]


def random_cotangents(cfg, B, n, seed, only=None):
    """[scale][map] float64 cotangents of the full shapes; ``only``: a set of (scale, map) that get one, the others are None."""
    g = torch.Generator().manual_seed(seed)
    full, shapes = map_lengths(cfg, n), layer_shapes(cfg)
    out = []
    for k in range(cfg["n_scales"]):
        row = []
        for i in range(len(shapes)):
            t = torch.randn(B, shapes[i][1], full[k][i], generator=g, dtype=torch.float64)
            row.append(t if only is None or (k, i) in only else None)
        out.append(row)
    return out


def tie_free_case(sd, cfg, B, n, lengths, G, seeds=range(1, 9)):
    """The first ``random_wav`` seed among ``seeds`` whose float64 forward has no near-tie -> (seed, wav, reference)."""
    for seed in seeds:
        wav = random_wav(B, n, seed)
        ref = reference(sd, wav, lengths, cfg, G)
        if near_ties(ref, cfg, lengths) == 0:
            return seed, wav, ref
    raise AssertionError(f"no tie-free waveform among seeds {list(seeds)} for {B} x {n}")
