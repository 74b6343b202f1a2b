"""GPU: gvx_hifigan_mpd_forward and gvx_hifigan_mpd_backward (csrc/hifigan_disc.hip) through the C ABI alone against the float64
restatement in tests/hifigan_disc_ref64.py - every map of every period, every parameter gradient and d_wav, tensor by tensor.
Features, workspace, gradients and padded inputs all start as NaN; buffers have exactly their stated sizes, with a sentinel behind them
that must survive.

Tolerance.  Per tensor, e is the largest |float32 restatement - float64| (a number of the reference alone); the device may differ from
float64 by at most 8 x max(e, 2^-23 x the tensor's largest value).

LeakyReLU ties.  The backward reads its masks off the device's own maps.  Every decision that differs from float64's is asserted to be a
near-tie (the float64 value within its map's bound of 0), and the float64 gradient is taken with the restatement pinned to the device's
decisions.

Tiles.  Every convolution kernel works in tiles of GVX_HIFIGAN_MPD_TILE = 64 positions (height, column) of one row: the forward
kernels over the positions H_i p of their output map; the data-gradient kernels over the positions of ONE stride phase of their input
map, ceil(H_{i-1} / 3) p - which for a strided layer is H_i p again, and for the last (stride 1) layer H_{i-1} p = H_i p.  So
``edge_lengths(cfg, j, i)`` - the two largest n at which map (j, i) still has at most 64 positions and the two smallest at which it has
more: an odd and an even count on each side - puts the first tile edge of the forward kernel that writes map i AND of the data gradient
that leaves layer i under test.  LENGTHS takes that edge for every map of the first period (the matrix kernels of MIXED's layers 2, 3
and 4; the score's wave-per-position kernel; the VALU kernels), and for map 0 of every period (the first layer's kernel, which absorbs
the reflection), besides
  - n = 30, 31, 29: n % p = 0, 1 (p - 1 reflected samples) and p - 1 (n = 29, for p = 3 and 5) for every period of both configs;
  - n = min_samples;
  - n = q, 2 q, 3 q, 4 q, 5 q for the largest period q: heights 1 .. 5 into the first strided layer, 1, 1, 1, 2, 2 out of it.
The ragged batches put the shortest legal row beside a row that has a second tile in every map of the first period, so the short rows'
second tiles lie wholly behind them.  The weight gradients' pieces are runs of multiples of 32 positions (pd_pieces); the same lengths
end their last run everywhere from 1 position to a full run."""
import ctypes as C
import functools

import pytest
import torch

from genvox_amd import _lib
from tests import hifigan_disc_ref64 as DR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
TILE = 64
SENTINEL = 64   # floats behind every exactly-sized buffer
CFGS = dict(TINY=DR.TINY, MIXED=DR.MIXED, DEFAULT=DR.DEFAULT)


def edge_lengths(cfg, j, i):
    n = DR.min_samples(cfg)
    while DR.map_heights(cfg, n)[j][i] * cfg["periods"][j] <= TILE:
        n += 1
    return (n - 2, n - 1, n, n + 1)


def lengths_of(cfg):
    q, out = DR.min_samples(cfg), set()
    for i in range(len(cfg["channels"]) + 1):
        out.update(edge_lengths(cfg, 0, i))
    for j in range(len(cfg["periods"])):
        out.update(edge_lengths(cfg, j, 0))
    out.update((29, 30, 31, q, 2 * q, 3 * q, 4 * q, 5 * q))
    return tuple(sorted(n for n in out if n >= q))


LENGTHS = {name: lengths_of(CFGS[name]) for name in ("TINY", "MIXED")}
LONGEST = {name: edge_lengths(CFGS[name], 0, len(CFGS[name]["channels"]))[3] for name in ("TINY", "MIXED")}


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    torch.cuda.empty_cache()


def test_the_tile_sizes_are_the_ones_the_lengths_were_chosen_for():
    header = open(__file__.replace("tests/test_hifigan_disc_gpu.py", "include/genvox_amd.h")).read()
    assert f"GVX_HIFIGAN_MPD_TILE = {TILE}" in header and "GVX_HIFIGAN_MPD_TILE_N = 64" in header and "GVX_HIFIGAN_MPD_TILE_N_WIDE = 128" in header and "GVX_HIFIGAN_MPD_MFMA_MULT = 32" in header
    internal = open(__file__.replace("tests/test_hifigan_disc_gpu.py", "genvox_amd/csrc/hifigan_disc_internal.h")).read()
    assert f"PD_TILE = {TILE};" in internal and "PD_WG_CHUNK = 32;" in internal


def test_the_lengths_hold_what_the_docstring_says():
    for name, cfg in (("TINY", DR.TINY), ("MIXED", DR.MIXED)):
        for i in range(len(cfg["channels"]) + 1):
            a, b, c, d = edge_lengths(cfg, 0, i)
            pos = [DR.map_heights(cfg, n)[0][i] * cfg["periods"][0] for n in (a, b, c, d)]
            assert pos[0] <= TILE and pos[1] <= TILE and pos[2] > TILE and pos[3] > TILE and {a, b, c, d} <= set(LENGTHS[name])
        q = DR.min_samples(cfg)
        jq = cfg["periods"].index(q)
        assert [DR.map_heights(cfg, m * q)[jq][0] for m in (1, 2, 3, 4, 5)] == [1, 1, 1, 2, 2]
        for p in cfg["periods"]:
            assert {n % p for n in LENGTHS[name]} >= {0, 1, p - 1}


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _guarded(n_bytes):
    """A NaN-filled float32 buffer of n_bytes plus a sentinel run behind it."""
    assert n_bytes % 4 == 0
    return torch.full((n_bytes // 4 + SENTINEL,), NAN, dtype=torch.float32, device=DEV)


def _sentinel_intact(buf):
    return bool(torch.isnan(buf[-SENTINEL:]).all())


def dims_of(cfg):
    periods, channels = (C.c_int32 * 8)(*cfg["periods"]), (C.c_int32 * 8)(*cfg["channels"])
    return _lib.gvx_hifigan_mpd_dims(len(cfg["periods"]), periods, len(cfg["channels"]), channels, cfg["kernel_size"], cfg["stride"], cfg["slope"])


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
        self.blob = torch.full((self.lib.gvx_hifigan_mpd_blob_floats(C.byref(self.dims)),), NAN, dtype=torch.float32, device=DEV)
        _lib.check(self.lib.gvx_hifigan_mpd_pack_weights_device(C.byref(self.dims), table, len(self.weights), self.blob.data_ptr(), stream()))
        h = C.c_void_p()
        _lib.check(self.lib.gvx_hifigan_mpd_create(C.byref(self.dims), C.byref(h)))
        self.h = h.value
        _lib.check(self.lib.gvx_hifigan_mpd_bind(self.h, self.blob.data_ptr()))

    def __del__(self):
        self.lib.gvx_hifigan_mpd_destroy(self.h)

    def views(self, buf, B, n):
        """[period][map] views [B, C, H, p] of a features-shaped float32 buffer."""
        e = (_lib.gvx_hifigan_mpd_entry * 80)()
        count = self.lib.gvx_hifigan_mpd_layout(C.byref(self.dims), B, n, e, 80)
        per = len(self.cfg["channels"]) + 1
        assert count == per * len(self.cfg["periods"])
        flat = []
        for i in range(count):
            x = e[i]
            assert x.byte_offset % 256 == 0 and x.period == self.cfg["periods"][i // per]
            flat.append(buf[x.byte_offset // 4: x.byte_offset // 4 + B * x.channels * x.height * x.period].as_strided(
                (B, x.channels, x.height, x.period), (x.stride_b, x.stride_c, x.stride_h, x.stride_p)))
        return [flat[j * per:(j + 1) * per] for j in range(len(self.cfg["periods"]))]

    def forward(self, wav, lens=None):
        """-> (the features buffer, its maps as [period][map] views)."""
        B, n = wav.shape
        fb, wb = self.lib.gvx_hifigan_mpd_features_bytes(C.byref(self.dims), B, n), self.lib.gvx_hifigan_mpd_workspace_bytes(C.byref(self.dims), B, n, 0)
        feats, ws = _guarded(fb), _guarded(wb)
        _lib.check(self.lib.gvx_hifigan_mpd_forward(self.h, wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, n, feats.data_ptr(), fb,
                                                    ws.data_ptr(), wb, stream()))
        torch.cuda.synchronize()
        assert _sentinel_intact(feats) and _sentinel_intact(ws), "the forward wrote behind its features buffer or its workspace"
        return feats, self.views(feats, B, n)

    def cotangent_buffer(self, G, B, n, lens):
        """d_features: NaN everywhere, G (or 0 where a map has no cotangent) inside every row's own heights."""
        buf = _guarded(self.lib.gvx_hifigan_mpd_features_bytes(C.byref(self.dims), B, n))
        for j, period in enumerate(self.views(buf, B, n)):
            for i, view in enumerate(period):
                for b in range(B):
                    H = DR.map_heights(self.cfg, n if lens is None else lens[b])[j][i]
                    view[b, :, :H] = 0.0 if G[j][i] is None else G[j][i][b, :, :H].to(DEV, torch.float32)
        return buf

    def backward(self, wav, lens, feats, d_feats, want_params=True, want_wav=True):
        B, n = wav.shape
        grads = {k: torch.full(s, NAN, dtype=torch.float32, device=DEV) for k, s in self.shapes.items()} if want_params else {}
        table = (_lib.gvx_weight_desc * max(len(grads), 1))()
        for i, (k, g) in enumerate(grads.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), g.data_ptr(), g.numel())
        d_wav = torch.full((B, n), NAN, dtype=torch.float32, device=DEV) if want_wav else None
        wb = self.lib.gvx_hifigan_mpd_workspace_bytes(C.byref(self.dims), B, n, 1)
        ws = _guarded(wb)
        _lib.check(self.lib.gvx_hifigan_mpd_backward(self.h, wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, n, feats.data_ptr(),
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
    sd = DR.random_state(cfg, seed=11)
    return cfg, sd, DiscNet(cfg, sd)


def _poisoned(wav, lens):
    wav = wav.clone()
    if lens is not None:
        for b, nb in enumerate(lens):
            wav[b, nb:] = NAN
    return wav.to(DEV, torch.float32)


@functools.lru_cache(maxsize=None)
def _forward_case(name, B, n, lens):
    """(wav, float64 reference of the forward): computed once, shared, never changed."""
    cfg, sd, _ = _net(name)
    wav = DR.random_wav(B, n, seed=100 * B + n)
    return wav, DR.reference(sd, wav, lens, cfg)


def _check_forward(name, B, n, lens=None):
    cfg, sd, net = _net(name)
    wav, ref = _forward_case(name, B, n, lens)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(_poisoned(wav, lens), lens_d)
    worst = 0.0
    for j, period in enumerate(maps):
        for i, got in enumerate(period):
            got = got.double().cpu()
            assert got.shape == ref["maps"][j][i].shape
            for b in range(B):
                H = DR.map_heights(cfg, n if lens is None else lens[b])[j][i]
                assert not got[b, :, H:].any() and not torch.isnan(got[b]).any(), f"{name} {B} x {n}: map ({j}, {i}) row {b} is not exact zeros behind {H}"
                d, tol = (got[b, :, :H] - ref["maps"][j][i][b, :, :H]).abs().max().item(), ref["map_tol"][j][i]
                worst = max(worst, d / tol)
                assert d <= tol, f"{name} {B} x {n} {lens}: map ({j}, {i}) row {b}: {d:.3e} from float64, above the bound {tol:.3e} (float32 restatement {ref['map_err'][j][i]:.3e})"
    print(f"{name} {B} x {n} {lens}: largest forward error {worst:.3f} of its bound")
    return wav, ref, feats, maps


def _check_backward(name, B, n, lens=None, only=None, seed=5):
    """Gradients against float64 pinned to the device's LeakyReLU decisions -> (wav, lens, feats, d_feats, grads, largest share of a bound)."""
    cfg, sd, net = _net(name)
    wav, free, feats, maps = _check_forward(name, B, n, lens)
    flips = 0
    for j, period in enumerate(maps):
        for i, got in enumerate(period[:-1]):
            want = free["maps"][j][i]
            differ = (got.cpu() > 0) != (want > 0)
            flips += int(differ.sum())
            assert (want[differ].abs() <= free["map_tol"][j][i]).all(), f"map ({j}, {i}): a sign differs from float64 away from 0"
    G = DR.random_cotangents(cfg, B, n, seed, only)
    ref = DR.reference(sd, wav, lens, cfg, G, DR.masks_from_maps(maps, cfg["slope"]))
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


@pytest.mark.parametrize("name,n", [(name, n) for name in ("TINY", "MIXED") for n in LENGTHS[name]])
def test_forward_and_backward_one_row(name, n):
    """B = 1: every map, then every gradient with cotangents on all maps."""
    _check_backward(name, 1, n)


@pytest.mark.parametrize("name", ["TINY", "MIXED"])
def test_ragged_rows_partial_calls_and_repeats(name):
    """A ragged B = 3, the shortest legal row beside the longest: rows are their one-row runs bit for bit, forward and d_wav; the d_wav-only
    and the parameters-only call give the full call's bits; so does a second call."""
    cfg, sd, net = _net(name)
    lens = (LONGEST[name], DR.min_samples(cfg), LONGEST[name] // 2 + 1)
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
        for j in range(len(cfg["periods"])):
            for i, m in enumerate(m1[j]):
                assert torch.equal(maps[j][i][b, :, :m.shape[2]], m[0]), f"{name}: row {b} of {nb} samples, map ({j}, {i}) differs from its one-row run"
        d1 = net.cotangent_buffer([[g[b:b + 1, :, :m.shape[2]].cpu() for g, m in zip(gs, ms)] for gs, ms in zip(G_views, m1)], 1, nb, None)
        alone = net.backward(one, None, f1, d1, want_params=False)
        assert torch.equal(alone["wav"][0], full["wav"][b, :nb]), f"{name}: d_wav of row {b} differs from its one-row run"


@pytest.mark.parametrize("name,only", [("MIXED", "scores"), ("MIXED", "middle"), ("TINY", "scores"), ("TINY", "middle")])
def test_backward_single_cotangents(name, only):
    """A cotangent on the scores alone, and one on a single middle map: the other maps have none."""
    cfg = CFGS[name]
    last = len(cfg["channels"])
    which = {(j, last) for j in range(len(cfg["periods"]))} if only == "scores" else {(1, 2)}
    _check_backward(name, 2, 200, only=frozenset(which))


def test_default_shape():
    """The published shape once, B = 2 and ragged, at most 2 x 2048 samples: the 128 -> 512, 512 -> 1024 and 1024 -> 1024 matrix layers."""
    _, _, _, _, _, worst = _check_backward("DEFAULT", 2, 2048, (2048, 1531))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["TINY", "MIXED"])
def test_a_row_below_min_samples_is_silent(name):
    """The host cannot see device lengths: a row shorter than the largest period that reaches the kernels comes out as all-zero maps and
    an all-zero d_wav row, its neighbour as its one-row run, and nothing is written behind a buffer."""
    cfg, sd, net = _net(name)
    q = DR.min_samples(cfg)
    lens = (70, q - 1)
    wav = _poisoned(DR.random_wav(2, 70, 7), lens)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(wav, lens_d)
    _, alone = net.forward(wav[:1].contiguous())
    for j, period in enumerate(maps):
        for i, m in enumerate(period):
            assert not m[1].any() and not torch.isnan(m).any(), f"{name}: map ({j}, {i}) of the short row is not exact zeros"
            assert torch.equal(m[0], alone[j][i][0])
    d_feats = _guarded(feats.numel() * 4 - SENTINEL * 4)
    for period in net.views(d_feats, 2, 70):
        for v in period:
            v[0] = 1.0
    grads = net.backward(wav, lens_d, feats, d_feats)
    assert not grads["wav"][1].any() and not any(torch.isnan(g).any() for g in grads.values())


def test_bad_arguments_are_refused_before_a_launch():
    cfg, sd, net = _net("TINY")
    lib, wav = net.lib, torch.zeros(1, 64, device=DEV)
    fb = lib.gvx_hifigan_mpd_features_bytes(C.byref(net.dims), 1, 64)
    feats, ws = _guarded(fb), _guarded(256)
    assert lib.gvx_hifigan_mpd_forward(net.h, wav.data_ptr(), None, 0, 64, feats.data_ptr(), fb, ws.data_ptr(), 256, stream()) != 0
    assert lib.gvx_hifigan_mpd_forward(net.h, wav.data_ptr(), None, 1, 2, feats.data_ptr(), fb, ws.data_ptr(), 256, stream()) != 0
    assert lib.gvx_hifigan_mpd_forward(net.h, wav.data_ptr(), None, 1, 64, feats.data_ptr(), fb - 256, ws.data_ptr(), 256, stream()) != 0
    assert lib.gvx_hifigan_mpd_forward(net.h, wav.data_ptr(), None, 1, 64, feats.data_ptr(), fb, None, 0, stream()) != 0
    assert lib.gvx_hifigan_mpd_backward(net.h, wav.data_ptr(), None, 1, 64, feats.data_ptr(), feats.data_ptr(), None, 0, None, ws.data_ptr(), 256, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(feats).all()), "a refused call wrote to the features buffer"
