"""The multi-resolution spectrogram discriminator of include/genvox_amd.h ("Multi-resolution spectrogram discriminator") restated with
torch's own ``F.pad(mode="reflect")``, ``torch.stft(center=False)`` and ``F.conv2d``, for the tests of the device's forward and backward.
It imports nothing from genvox_amd.  Everything is computed in the dtype asked for; every row is run alone at its own length.

The maps are returned as [B, C, W, F] - frames in front of bins, the device's order; the convolutions themselves run on torch's
[B, C, F, W] with the published kernels (3, 9) / (3, 3).

Gradients come from autograd of ``loss = sum over the maps of sum(map * G_map)`` for cotangents G supplied from outside.  Every
``lrelu(x)`` can be *pinned*: replaced by ``x * m`` with ``m`` in {1, slope} supplied from outside, one mask per non-score map, so that
float64 and the device differentiate the same piecewise-linear function (tests/melgan_disc_ref64.py has the reasoning).

Bounds: per tensor, FACTOR = 8 times max(the largest |float32 restatement - float64|, one ulp of the tensor's largest value).

The magnitude's gradient d_mag (re, im) / mag is ill-conditioned at small magnitudes, so gradient cases use noise of scale 0.3 and
``well_conditioned_case`` takes the first seed whose float32 restatement of d_wav is finite and none of whose bin magnitudes is below
FACTOR times the spectrogram's own float32 error.

The two configs:
  DEFAULT  the published shape: resolutions (1024, 120, 600), (2048, 240, 1200), (512, 50, 240), 32 channels, rectangular window.  The
           C -> C layers run on the matrix kernels' 128-position x 32-channel tile.
  HANN     one resolution (512, 64, 256), 64 channels, periodic Hann window: the matrix kernels' 64 x 64 tile, two k blocks per bin."""
import torch
import torch.nn.functional as F

FACTOR = 8.0
ULP = 2.0 ** -23
MAPS = 6

DEFAULT = dict(resolutions=((1024, 120, 600), (2048, 240, 1200), (512, 50, 240)), channels=32, slope=0.1, window="rectangular")
HANN = dict(resolutions=((512, 64, 256),), channels=64, slope=0.1, window="hann")


def layer_shapes(cfg):
    """(c_in, c_out, (taps in frequency, taps in time), stride in time), the score last."""
    C = cfg["channels"]
    return [(1, C, (3, 9), 1), (C, C, (3, 9), 2), (C, C, (3, 9), 2), (C, C, (3, 9), 2), (C, C, (3, 3), 1), (C, 1, (3, 3), 1)]


def min_samples(cfg):
    return max((n_fft - hop) // 2 + 1 for n_fft, hop, _w in cfg["resolutions"])


def parameter_count(cfg):
    return len(cfg["resolutions"]) * sum(co * ci * kf * kt + co for ci, co, (kf, kt), _s in layer_shapes(cfg))


def layer_name(j, i):
    return f"discriminators.{j}.conv_post" if i == MAPS - 1 else f"discriminators.{j}.convs.{i}"


def frames(n, res):
    n_fft, hop, _w = res
    p = (n_fft - hop) // 2
    return 1 + (n + 2 * p - n_fft) // hop


def map_widths(cfg, n):
    """[resolution][map] -> frames, for a row of n samples."""
    out = []
    for res in cfg["resolutions"]:
        w, ws = frames(n, res), []
        for _ci, _co, _k, stride in layer_shapes(cfg):
            if stride > 1:
                w = (w - 1) // stride + 1
            ws.append(w)
        out.append(ws)
    return out


def bins(res):
    return res[0] // 2 + 1


def random_state(cfg, seed, gain=1.0):
    """N(0, gain^2 / fan_in) weights [out, in, 3, kt] and N(0, 0.1^2) biases, float64."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for j in range(len(cfg["resolutions"])):
        for i, (ci, co, (kf, kt), _s) in enumerate(layer_shapes(cfg)):
            sd[layer_name(j, i) + ".weight"] = torch.randn(co, ci, kf, kt, generator=g, dtype=torch.float64) * gain * (ci * kf * kt) ** -0.5
            sd[layer_name(j, i) + ".bias"] = torch.randn(co, generator=g, dtype=torch.float64) * 0.1
    return sd


def random_wav(B, n, seed, silent=()):
    """Noise of scale 0.3; the rows named in ``silent`` are all zeros."""
    g = torch.Generator().manual_seed(seed)
    wav = torch.randn(B, n, generator=g, dtype=torch.float64) * 0.3
    for b in silent:
        wav[b] = 0.0
    return wav


def window_of(cfg, res, dtype):
    win = res[2]
    return torch.ones(win, dtype=dtype) if cfg["window"] == "rectangular" else torch.hann_window(win, periodic=True, dtype=dtype)


def spectrogram(x, cfg, res):
    """x [B, n] -> magnitudes [B, F, W], as the published code: reflection by (n_fft - hop) // 2, no centring, the 2-norm of (re, im)."""
    n_fft, hop, win = res
    p = (n_fft - hop) // 2
    x = F.pad(x[:, None, :], (p, p), mode="reflect")[:, 0, :]
    X = torch.stft(x, n_fft, hop_length=hop, win_length=win, window=window_of(cfg, res, x.dtype), center=False, return_complex=True)
    return torch.linalg.vector_norm(torch.view_as_real(X), dim=-1)


def discriminator(sd, wav, cfg, masks=None):
    """wav [B, n] -> ([resolution][map] tensors [B, C, W, F]: post-activation features, then the score; [resolution] magnitudes
    [B, W, F]).  ``masks``: None, or [resolution][map] tensors [B, C, W, F] (the score's entry unused) that replace lrelu(x) by
    x * masks[j][i]."""
    out, mags, shapes = [], [], layer_shapes(cfg)
    for j, res in enumerate(cfg["resolutions"]):
        mag = spectrogram(wav, cfg, res)
        mags.append(mag.transpose(1, 2))
        maps, h = [], mag[:, None]
        for i, (_ci, _co, (kf, kt), stride) in enumerate(shapes):
            h = F.conv2d(h, sd[layer_name(j, i) + ".weight"], sd[layer_name(j, i) + ".bias"], stride=(1, stride), padding=(kf // 2, kt // 2))
            if i < MAPS - 1:
                h = F.leaky_relu(h, cfg["slope"]) if masks is None else h * masks[j][i].transpose(2, 3)
            maps.append(h.transpose(2, 3))
        out.append(maps)
    return out, mags


def run(sd, wav, lengths, cfg, G=None, masks=None, dtype=torch.float64):
    """Forward (and, with cotangents G [resolution][map] of full [B, C, W_max, F] shape, backward) in ``dtype``, every row alone at its
    own length.  -> (maps zero-filled behind the widths, [resolution] magnitudes [B, W_max, F] likewise, {name: gradient} with "wav"
    among the names; None without G)."""
    sd = {k: v.to(dtype).clone().requires_grad_(G is not None) for k, v in sd.items()}
    B, n = wav.shape
    lengths = [n] * B if lengths is None else list(lengths)
    full, shapes = map_widths(cfg, n), layer_shapes(cfg)
    maps_all = [[torch.zeros(B, shapes[i][1], full[j][i], bins(res), dtype=dtype) for i in range(MAPS)] for j, res in enumerate(cfg["resolutions"])]
    mags_all = [torch.zeros(B, frames(n, res), bins(res), dtype=dtype) for res in cfg["resolutions"]]
    d_wav = torch.zeros(B, n, dtype=dtype)
    for b, nb in enumerate(lengths):
        x = wav[b:b + 1, :nb].to(dtype).clone().requires_grad_(G is not None)
        own = map_widths(cfg, nb)
        mk = None if masks is None else [[m[b:b + 1, :, :own[j][i]].to(dtype) for i, m in enumerate(ms)] for j, ms in enumerate(masks)]
        maps, mags = discriminator(sd, x, cfg, mk)
        loss = 0.0
        for j, ms in enumerate(maps):
            mags_all[j][b:b + 1, :mags[j].shape[1]] = mags[j].detach()
            for i, m in enumerate(ms):
                assert m.shape[2] == own[j][i], (j, i, m.shape, own[j][i])
                maps_all[j][i][b:b + 1, :, :m.shape[2]] = m.detach()
                if G is not None and G[j][i] is not None:
                    loss = loss + (m * G[j][i][b:b + 1, :, :m.shape[2]].to(dtype)).sum()
        if G is not None:
            loss.backward()
            d_wav[b, :nb] = x.grad[0]
    if G is None:
        return maps_all, mags_all, None
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
    grads["wav"] = d_wav
    return maps_all, mags_all, grads


def tol_of(a32, a64):
    err = (a32.double() - a64).abs().max().item() if a64.numel() else 0.0
    return err, FACTOR * max(err, ULP * (a64.abs().max().item() if a64.numel() else 0.0))


def reference(sd, wav, lengths, cfg, G=None, masks=None):
    """-> dict(maps, mags, grads: float64;  map_err, map_tol: [resolution][map] the float32 restatement's error and the bound of every
    map;  mag_err: [resolution] the same error of the magnitudes;  grad_err, grad_tol: per gradient tensor)."""
    m64, s64, g64 = run(sd, wav, lengths, cfg, G, masks, torch.float64)
    sd32 = {k: v.float() for k, v in sd.items()}
    m32, s32, g32 = run(sd32, wav.float(), lengths, cfg, None if G is None else [[None if g is None else g.float() for g in gs] for gs in G],
                        None if masks is None else [[m.float() for m in ms] for ms in masks], torch.float32)
    pairs = [[tol_of(a, b) for a, b in zip(r32, r64)] for r32, r64 in zip(m32, m64)]
    ref = dict(maps=m64, mags=s64, map_err=[[p[0] for p in ps] for ps in pairs], map_tol=[[p[1] for p in ps] for ps in pairs], grads=g64,
               mag_err=[tol_of(a, b)[0] for a, b in zip(s32, s64)])
    if G is not None:
        both = {k: tol_of(g32[k], g64[k]) for k in g64}
        ref["grad_err"] = {k: v[0] for k, v in both.items()}
        ref["grad_tol"] = {k: v[1] for k, v in both.items()}
    return ref


def masks_from_maps(maps, slope):
    """maps [resolution][map] (any dtype) -> the masks that pin every LeakyReLU to the side ``y > 0`` decides."""
    one, low = torch.tensor(1.0, dtype=torch.float64), torch.tensor(slope, dtype=torch.float64)
    return [[torch.where(m.cpu() > 0, one, low) for m in ms] for ms in maps]


def random_cotangents(cfg, B, n, seed, only=None):
    """[resolution][map] float64 cotangents of the full shapes; ``only``: a set of (resolution, map) that get one, the others are None."""
    g = torch.Generator().manual_seed(seed)
    full, shapes = map_widths(cfg, n), layer_shapes(cfg)
    out = []
    for j, res in enumerate(cfg["resolutions"]):
        row = []
        for i in range(MAPS):
            t = torch.randn(B, shapes[i][1], full[j][i], bins(res), generator=g, dtype=torch.float64)
            row.append(t if only is None or (j, i) in only else None)
        out.append(row)
    return out


def well_conditioned(ref, cfg, B, n, lengths, silent=()):
    """The float32 restatement's error of d_wav is finite, and no bin magnitude of a sounding row is below FACTOR x the float32 error of
    its resolution's magnitudes."""
    if "grad_err" in ref and not ref["grad_err"]["wav"] < float("inf"):
        return False
    for j, res in enumerate(cfg["resolutions"]):
        for b in range(B):
            if b in silent:
                continue
            w = frames(n if lengths is None else lengths[b], res)
            if w > 0 and ref["mags"][j][b, :w].min().item() < FACTOR * ref["mag_err"][j]:
                return False
    return True


def well_conditioned_case(sd, cfg, B, n, lengths, G, silent=(), seeds=range(1, 9)):
    """The first ``random_wav`` seed among ``seeds`` whose unpinned reference is ``well_conditioned`` -> (seed, wav, reference)."""
    for seed in seeds:
        wav = random_wav(B, n, seed, silent)
        ref = reference(sd, wav, lengths, cfg, G)
        if well_conditioned(ref, cfg, B, n, lengths, silent):
            return seed, wav, ref
    raise AssertionError(f"no well-conditioned waveform among seeds {list(seeds)} for {B} x {n}")
