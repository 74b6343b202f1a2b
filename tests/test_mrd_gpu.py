"""GPU: gvx_mrd_forward and gvx_mrd_backward (csrc/mrd.hip) through the C ABI against the float64 restatement in tests/mrd_ref64.py -
every map of every resolution, every parameter gradient and d_wav, tensor by tensor - and the module on top of them.  Features,
workspace, gradients and padded inputs all start as NaN; buffers have exactly their stated sizes, with a sentinel behind them that must
survive.

Tolerance.  Per tensor, e is the largest |float32 restatement - float64| (a number of the reference alone); the device may differ from
float64 by at most 8 x max(e, 2^-23 x the tensor's largest value).  Every F is 2^k + 1, so the frequency axis always has a one-bin
tail: bins 0 and F - 1 are asserted apart from the bins between them.

LeakyReLU ties.  The backward reads its masks off the device's own maps.  Every decision that differs from float64's is asserted to be a
near-tie (the float64 value within its map's bound of 0), and the float64 gradient is taken with the restatement pinned to the device's
decisions.

Conditioning.  d_mag (re, im) / mag is ill-conditioned at small magnitudes: every case is noise of scale 0.3, the first seed of 1 .. 8
whose float32 restatement of d_wav is finite and none of whose bin magnitudes is below 8 x the spectrogram's float32 error
(mrd_ref64.well_conditioned_case; silent rows, which are all zeros on purpose, apart).

Lengths: tests/mrd_cases.py says what LENGTHS holds and tests/test_mrd_cpu.py checks it.  The weight gradients' pieces are
GVX_MRD_PIECE_FRAMES = 16 output frames of one row: at B = 1, DEFAULT's n = 1920 / 2040 (HANN's 1024 / 1088) give the first layer's VALU
weight gradient exactly one piece / one piece plus one frame, and n = 1550 / 1650 (1984 / 2112) give layer 1's matrix weight gradient
the same; at B = 3 every row has its own pieces."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from genvox_amd import _lib
from tests import mrd_cases as MC
from tests import mrd_ref64 as MR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 64   # floats behind every exactly-sized buffer
CFGS = MC.CFGS
RAGGED = dict(DEFAULT=(3250, 905, 2040), HANN=(4160, 225, 2112))   # (n_max, the least row, a middle row)


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    torch.cuda.empty_cache()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _guarded(n_bytes):
    """A NaN-filled float32 buffer of n_bytes plus a sentinel run behind it."""
    assert n_bytes % 4 == 0
    return torch.full((n_bytes // 4 + SENTINEL,), NAN, dtype=torch.float32, device=DEV)


def _sentinel_intact(buf):
    return bool(torch.isnan(buf[-SENTINEL:]).all())


def dims_of(cfg):
    res = cfg["resolutions"]
    n_fft, hop, win = ((C.c_int32 * 8)(*[r[k] for r in res]) for k in range(3))
    return _lib.gvx_mrd_dims(len(res), n_fft, hop, win, cfg["channels"], ("rectangular", "hann").index(cfg["window"]), cfg["slope"])


class DiscNet:
    """A handle driven through the C ABI alone."""

    def __init__(self, cfg, sd):
        self.cfg, self.lib = cfg, _lib.load()
        self.dims = dims_of(cfg)
        self.shapes = {k: tuple(v.shape) for k, v in sd.items()}
        self.weights = {k: v.to(DEV, torch.float32).contiguous() for k, v in sd.items()}
        table = (_lib.gvx_weight_desc * len(self.weights))()
        for i, (k, v) in enumerate(self.weights.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
        self.blob = torch.full((self.lib.gvx_mrd_blob_floats(C.byref(self.dims)),), NAN, dtype=torch.float32, device=DEV)
        _lib.check(self.lib.gvx_mrd_pack_weights_device(C.byref(self.dims), table, len(self.weights), self.blob.data_ptr(), stream()))
        h = C.c_void_p()
        _lib.check(self.lib.gvx_mrd_create(C.byref(self.dims), C.byref(h)))
        self.h = h.value
        _lib.check(self.lib.gvx_mrd_bind(self.h, self.blob.data_ptr()))

    def __del__(self):
        self.lib.gvx_mrd_destroy(self.h)

    def views(self, buf, B, n):
        """[resolution][map] views [B, C, W, F] of a features-shaped float32 buffer."""
        e = (_lib.gvx_mrd_entry * 48)()
        count = self.lib.gvx_mrd_layout(C.byref(self.dims), B, n, e, 48)
        assert count == MR.MAPS * len(self.cfg["resolutions"])
        flat = []
        for i in range(count):
            x = e[i]
            assert x.byte_offset % 256 == 0 and x.bins == MR.bins(self.cfg["resolutions"][i // MR.MAPS])
            flat.append(buf[x.byte_offset // 4: x.byte_offset // 4 + B * x.channels * x.frames * x.bins].as_strided(
                (B, x.channels, x.frames, x.bins), (x.stride_b, x.stride_c, x.stride_w, x.stride_f)))
        return [flat[j * MR.MAPS:(j + 1) * MR.MAPS] for j in range(len(self.cfg["resolutions"]))]

    def forward(self, wav, lens=None):
        """-> (the features buffer, its maps as [resolution][map] views)."""
        B, n = wav.shape
        fb, wb = self.lib.gvx_mrd_features_bytes(C.byref(self.dims), B, n), self.lib.gvx_mrd_workspace_bytes(C.byref(self.dims), B, n, 0)
        feats, ws = _guarded(fb), _guarded(wb)
        _lib.check(self.lib.gvx_mrd_forward(self.h, wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, n, feats.data_ptr(), fb,
                                            ws.data_ptr(), wb, stream()))
        torch.cuda.synchronize()
        assert _sentinel_intact(feats) and _sentinel_intact(ws), "the forward wrote behind its features buffer or its workspace"
        return feats, self.views(feats, B, n)

    def cotangent_buffer(self, G, B, n, lens):
        """d_features: NaN everywhere, G (or 0 where a map has no cotangent) inside every row's own frames."""
        buf = _guarded(self.lib.gvx_mrd_features_bytes(C.byref(self.dims), B, n))
        for j, sub in enumerate(self.views(buf, B, n)):
            for i, view in enumerate(sub):
                for b in range(B):
                    W = MR.map_widths(self.cfg, n if lens is None else lens[b])[j][i]
                    view[b, :, :W] = 0.0 if G[j][i] is None else G[j][i][b, :, :W].to(DEV, torch.float32)
        return buf

    def backward(self, wav, lens, feats, d_feats, want_params=True, want_wav=True):
        B, n = wav.shape
        grads = {k: torch.full(s, NAN, dtype=torch.float32, device=DEV) for k, s in self.shapes.items()} if want_params else {}
        table = (_lib.gvx_weight_desc * max(len(grads), 1))()
        for i, (k, g) in enumerate(grads.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), g.data_ptr(), g.numel())
        d_wav = torch.full((B, n), NAN, dtype=torch.float32, device=DEV) if want_wav else None
        wb = self.lib.gvx_mrd_workspace_bytes(C.byref(self.dims), B, n, 1)
        ws = _guarded(wb)
        _lib.check(self.lib.gvx_mrd_backward(self.h, wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, n, feats.data_ptr(),
                                             d_feats.data_ptr(), table if grads else None, len(grads), d_wav.data_ptr() if want_wav else None,
                                             ws.data_ptr(), wb, stream()))
        torch.cuda.synchronize()
        assert _sentinel_intact(ws), "the backward wrote behind its workspace"
        if want_wav:
            grads["wav"] = d_wav
        return grads


@functools.lru_cache(maxsize=None)
def _net(name):
    cfg = CFGS[name]
    sd = MR.random_state(cfg, seed=11)
    return cfg, sd, DiscNet(cfg, sd)


def _poisoned(wav, lens):
    wav = wav.clone()
    if lens is not None:
        for b, nb in enumerate(lens):
            wav[b, nb:] = NAN
    return wav.to(DEV, torch.float32)


@functools.lru_cache(maxsize=None)
def _case(name, B, n, lens, only, silent):
    """(wav, cotangents, the unpinned float64 reference): computed once, shared, never changed."""
    cfg, sd, _ = _net(name)
    G = MR.random_cotangents(cfg, B, n, 1000 * B + n, only)
    seed, wav, ref = MR.well_conditioned_case(sd, cfg, B, n, lens, G, silent)
    print(f"{name} {B} x {n}: waveform seed {seed}")
    return wav, G, ref


def _check_forward(name, B, n, lens=None, only=None, silent=()):
    cfg, sd, net = _net(name)
    wav, G, ref = _case(name, B, n, lens, only, silent)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(_poisoned(wav, lens), lens_d)
    worst = 0.0
    for j, sub in enumerate(maps):
        for i, got in enumerate(sub):
            got = got.double().cpu()
            want, tol = ref["maps"][j][i], ref["map_tol"][j][i]
            assert got.shape == want.shape
            for b in range(B):
                W = MR.map_widths(cfg, n if lens is None else lens[b])[j][i]
                assert not got[b, :, W:].any() and not torch.isnan(got[b]).any(), f"{name} {B} x {n}: map ({j}, {i}) row {b} is not exact zeros behind {W}"
                diff = (got[b, :, :W] - want[b, :, :W]).abs()
                what = f"{name} {B} x {n} {lens}: map ({j}, {i}) row {b}"
                for part, d in (("bin 0", diff[..., 0].max().item()), ("the last bin", diff[..., -1].max().item()), ("the bins between", diff[..., 1:-1].max().item())):
                    worst = max(worst, d / tol)
                    assert d <= tol, f"{what}, {part}: {d:.3e} from float64, above the bound {tol:.3e} (float32 restatement {ref['map_err'][j][i]:.3e})"
    print(f"{name} {B} x {n} {lens}: largest forward error {worst:.3f} of its bound")
    return wav, G, ref, feats, maps


def _check_backward(name, B, n, lens=None, only=None, silent=()):
    """Gradients against float64 pinned to the device's LeakyReLU decisions -> (wav, lens, feats, d_feats, grads, largest share of a bound)."""
    cfg, sd, net = _net(name)
    wav, G, free, feats, maps = _check_forward(name, B, n, lens, only, silent)
    flips = 0
    for j, sub in enumerate(maps):
        for i, got in enumerate(sub[:-1]):
            want = free["maps"][j][i]
            differ = (got.cpu() > 0) != (want > 0)
            flips += int(differ.sum())
            assert (want[differ].abs() <= free["map_tol"][j][i]).all(), f"map ({j}, {i}): a sign differs from float64 away from 0"
    ref = MR.reference(sd, wav, lens, cfg, G, MR.masks_from_maps(maps, cfg["slope"]))
    assert ref["grad_err"]["wav"] < float("inf")
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    wav_d = _poisoned(wav, lens)
    d_feats = net.cotangent_buffer(G, B, n, lens)
    grads = net.backward(wav_d, lens_d, feats, d_feats)
    what, worst = f"{name} {B} x {n} {lens or ''} cotangents {sorted(only) if only else 'on all maps'} ({flips} LeakyReLU decisions differ)", 0.0
    for key, want in ref["grads"].items():
        g = grads[key].double().cpu()
        assert g.shape == want.shape and not torch.isnan(g).any(), f"{what}: {key} holds NaN or has the wrong shape"
        d, tol = (g - want).abs().max().item(), ref["grad_tol"][key]
        print(f"  d {key}: {d:.3e} of {tol:.3e}")
        assert d <= tol, f"{what}: d {key} differs from float64 by {d:.3e}, above the bound {tol:.3e} (float32 restatement: {ref['grad_err'][key]:.3e})"
        worst = max(worst, d / tol if tol > 0.0 else 0.0)   # a bound of 0: a gradient no cotangent reaches, exact zeros on both sides
    for b in range(B):
        nb = n if lens is None else lens[b]
        assert not grads["wav"][b, nb:].any(), f"{what}: d_wav row {b} is not exact zeros behind {nb}"
    print(f"{what}: largest gradient error {worst:.3f} of its bound")
    return wav_d, lens_d, feats, d_feats, grads, worst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,n", [(name, n) for name in ("DEFAULT", "HANN") for n in MC.LENGTHS[name]])
def test_forward_and_backward(name, n, B):
    """Every map, then every gradient with cotangents on all maps."""
    _check_backward(name, B, n)


@pytest.mark.parametrize("name", ["DEFAULT", "HANN"])
def test_ragged_rows_partial_calls_and_repeats(name):
    """A ragged B = 3, the shortest legal row and a middle one beside the longest: rows are their one-row runs bit for bit, forward and
    d_wav; the d_wav-only and the parameters-only call give the full call's bits; so does a second call."""
    cfg, sd, net = _net(name)
    lens = RAGGED[name]
    assert lens[1] == MR.min_samples(cfg)
    wav_d, lens_d, feats, d_feats, full, _ = _check_backward(name, 3, lens[0], lens)
    maps = net.views(feats, 3, lens[0])
    feats2, maps2 = net.forward(wav_d, lens_d)
    assert torch.equal(feats2[:-SENTINEL].view(torch.int32), feats[:-SENTINEL].view(torch.int32)), f"{name}: two forward calls differ"
    again = net.backward(wav_d, lens_d, feats, d_feats)
    dx_only = net.backward(wav_d, lens_d, feats, d_feats, want_params=False)
    dw_only = net.backward(wav_d, lens_d, feats, d_feats, want_wav=False)
    assert set(dx_only) == {"wav"} and set(dw_only) == set(sd)
    for k, v in full.items():
        assert torch.equal(again[k], v), f"{name}: d {k} differs between two calls"
        other = dx_only if k == "wav" else dw_only
        assert torch.equal(other[k], v), f"{name}: d {k} of a partial call differs from the full call"
    G_views = net.views(d_feats, 3, lens[0])
    for b, nb in enumerate(lens):
        one = wav_d[b:b + 1, :nb].contiguous()
        f1, m1 = net.forward(one)
        for j in range(len(cfg["resolutions"])):
            for i, m in enumerate(m1[j]):
                assert torch.equal(maps[j][i][b, :, :m.shape[2]], m[0]), f"{name}: row {b} of {nb} samples, map ({j}, {i}) differs from its one-row run"
        d1 = net.cotangent_buffer([[g[b:b + 1, :, :m.shape[2]].cpu() for g, m in zip(gs, ms)] for gs, ms in zip(G_views, m1)], 1, nb, None)
        alone = net.backward(one, None, f1, d1, want_params=False)
        assert torch.equal(alone["wav"][0], full["wav"][b, :nb]), f"{name}: d_wav of row {b} differs from its one-row run"


@pytest.mark.parametrize("name,only", [("DEFAULT", "scores"), ("DEFAULT", "first"), ("HANN", "scores"), ("HANN", "first")])
def test_backward_single_cotangents(name, only):
    """A cotangent on the scores alone, and one on map 0 of one resolution alone: the other maps have none."""
    cfg = CFGS[name]
    which = {(j, MR.MAPS - 1) for j in range(len(cfg["resolutions"]))} if only == "scores" else {(len(cfg["resolutions"]) - 1, 0)}
    _check_backward(name, 2, 1650, only=frozenset(which))


@pytest.mark.parametrize("name", ["DEFAULT", "HANN"])
def test_a_silent_row(name):
    """A row of zeros beside a sounding one: mag == 0 everywhere, so away from the zero padding its first map is the bias's image, bit for
    bit; every map and every gradient is within its bound, and d_wav of the silent row is exactly 0 (the magnitude passes no gradient
    where it is 0)."""
    cfg, sd, net = _net(name)
    wav_d, _, feats, _, grads, _ = _check_backward(name, 2, 2500, silent=(1,))
    assert not wav_d[1].any()
    assert not grads["wav"][1].any() and grads["wav"][0].any()
    maps = net.views(feats, 2, 2500)
    for j in range(len(cfg["resolutions"])):
        inner = maps[j][0][1, :, 4:-4, 1:-1]
        want = F.leaky_relu(net.weights[MR.layer_name(j, 0) + ".bias"], cfg["slope"])
        assert inner.numel() and torch.equal(inner, want[:, None, None].expand_as(inner))


@pytest.mark.parametrize("name", ["DEFAULT", "HANN"])
def test_a_row_below_min_samples_is_silent(name):
    """The host cannot see device lengths: a row below min_samples that reaches the kernels comes out as all-zero maps and an all-zero
    d_wav row, its neighbour as its one-row run, and nothing is written behind a buffer."""
    cfg, sd, net = _net(name)
    q = MR.min_samples(cfg)
    lens = (q + 300, q - 1)
    wav = _poisoned(MR.random_wav(2, lens[0], 7), lens)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(wav, lens_d)
    _, alone = net.forward(wav[:1].contiguous())
    for j, sub in enumerate(maps):
        for i, m in enumerate(sub):
            assert not m[1].any() and not torch.isnan(m).any(), f"{name}: map ({j}, {i}) of the short row is not exact zeros"
            assert torch.equal(m[0], alone[j][i][0])
    d_feats = _guarded(feats.numel() * 4 - SENTINEL * 4)
    for sub in net.views(d_feats, 2, lens[0]):
        for v in sub:
            v[0] = 1.0
    grads = net.backward(wav, lens_d, feats, d_feats)
    assert not grads["wav"][1].any() and not any(torch.isnan(g).any() for g in grads.values())


def test_bad_arguments_are_refused_before_a_launch():
    cfg, sd, net = _net("HANN")
    lib, wav = net.lib, torch.zeros(1, 400, device=DEV)
    fb, wb = lib.gvx_mrd_features_bytes(C.byref(net.dims), 1, 400), lib.gvx_mrd_workspace_bytes(C.byref(net.dims), 1, 400, 0)
    bw = lib.gvx_mrd_workspace_bytes(C.byref(net.dims), 1, 400, 1)
    feats, ws = _guarded(fb), _guarded(bw)
    assert lib.gvx_mrd_forward(net.h, wav.data_ptr(), None, 0, 400, feats.data_ptr(), fb, ws.data_ptr(), wb, stream()) != 0
    assert lib.gvx_mrd_forward(net.h, wav.data_ptr(), None, 1, 224, feats.data_ptr(), fb, ws.data_ptr(), wb, stream()) != 0
    assert lib.gvx_mrd_forward(net.h, wav.data_ptr(), None, 1, 400, feats.data_ptr(), fb - 256, ws.data_ptr(), wb, stream()) != 0
    assert lib.gvx_mrd_forward(net.h, wav.data_ptr(), None, 1, 400, feats.data_ptr(), fb, ws.data_ptr(), wb - 256, stream()) != 0
    assert lib.gvx_mrd_forward(net.h, wav.data_ptr(), None, 1, 400, feats.data_ptr(), fb, None, 0, stream()) != 0
    assert lib.gvx_mrd_backward(net.h, wav.data_ptr(), None, 1, 400, feats.data_ptr(), feats.data_ptr(), None, 0, None, ws.data_ptr(), bw, stream()) != 0
    assert lib.gvx_mrd_backward(net.h, wav.data_ptr(), None, 1, 400, feats.data_ptr(), feats.data_ptr(), None, 0, wav.data_ptr(), ws.data_ptr(), bw - 256, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(feats).all()) and bool(torch.isnan(ws).all()) and not wav.any(), "a refused call wrote to a buffer"


@pytest.mark.parametrize("name", ["DEFAULT", "HANN"])
def test_the_module_is_the_c_abi_with_autograd(name):
    """MultiResolutionDiscriminator: the maps are [B, C, W, F] views with the C ABI's bits; host and device lengths give the same result;
    backward() fills the parameters' and the waveform's gradients with the C ABI's bits; a row below min_samples raises ValueError."""
    from genvox_amd import MultiResolutionDiscriminator, MultiResolutionDiscriminatorConfig
    cfg, sd, net = _net(name)
    model = MultiResolutionDiscriminator(MultiResolutionDiscriminatorConfig(resolutions=cfg["resolutions"], channels=cfg["channels"],
                                                                           leaky_slope=cfg["slope"], window=cfg["window"])).to(DEV)
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    lens = RAGGED[name]
    wav, G, _ = _case(name, 3, lens[0], lens, None, ())
    wav_d = _poisoned(wav, lens)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(wav_d, lens_d)
    with torch.no_grad():
        plain = model(wav_d, list(lens))
    x = wav_d.clone().requires_grad_(True)
    out = model(x, lens_d)
    assert model.map_lengths(lens) == [[[MR.map_widths(cfg, n)[j][i] for n in lens] for i in range(MR.MAPS)] for j in range(len(cfg["resolutions"]))]
    for j, sub in enumerate(maps):
        for i, m in enumerate(sub):
            assert out[j][i].shape == m.shape == plain[j][i].shape and m.shape[2] == MR.map_widths(cfg, lens[0])[j][i] and m.shape[3] == MR.bins(cfg["resolutions"][j])
            assert torch.equal(out[j][i], m) and torch.equal(plain[j][i], m), f"{name}: map ({j}, {i}) of the module differs from the C ABI's"
    loss = sum((m[b, :, :MR.map_widths(cfg, nb)[j][i]] * G[j][i][b, :, :MR.map_widths(cfg, nb)[j][i]].to(DEV, torch.float32)).sum()
               for j, sub in enumerate(out) for i, m in enumerate(sub) for b, nb in enumerate(lens))
    loss.backward()
    want = net.backward(wav_d, lens_d, feats, net.cotangent_buffer(G, 3, lens[0], lens))
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, want[k]), f"{name}: d {k} of the module differs from the C ABI's"
    assert torch.equal(x.grad, want["wav"])
    short = (lens[0], MR.min_samples(cfg) - 1, lens[2])
    with pytest.raises(ValueError, match="reflection"):
        model(wav_d, short)
    with pytest.raises(ValueError, match="reflection"):
        model(wav_d[:, :MR.min_samples(cfg) - 1].contiguous())
